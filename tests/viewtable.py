"""What the view tables (tests/test_views_gpu.py, tests/test_warp_views_gpu.py) share: the device side of tests/viewcheck.py, the name of the kernel a call ran
(mi355cv_lastKernel, with a marker so that a hook that names none shows as such), the norm-relative comparison of the ops' own suites, the content of a source
image, one row of a table, and the "op -> kernel per layout" table each module prints from its fixture's teardown."""
import numpy as np
import torch

import orc as O
import viewcheck as vc


class Device:
    @staticmethod
    def put(a):
        return torch.from_numpy(a).cuda()

    @staticmethod
    def get(t):
        return t.cpu().numpy()


UNNAMED = "(unnamed)"
_MARK = {}


def mark(cv):
    """mi355cv_lastKernel keeps the last name any hook noted, and not every hook notes one: before each call of the table a tiny medianBlur with an aperture the
    table does not use leaves a name of its own there; if that name is still there after the call, the op named no kernel"""
    if "img" not in _MARK:
        _MARK["img"] = torch.zeros((3, 3), dtype=torch.uint8, device="cuda")
    cv.medianBlur(_MARK["img"], 11)
    _MARK["name"] = _raw_kernel()
    assert "K=11" in _MARK["name"], _MARK["name"]


def _raw_kernel():
    from opencv_amd import _lib
    return _lib.lib.mi355cv_lastKernel().decode()


def last_kernel():
    k = _raw_kernel()
    return UNNAMED if k == _MARK.get("name") else k


def short(kernel):
    """the kernel's name without its launch geometry"""
    for cut in (" grid=", " blocks="):
        kernel = kernel.split(cut)[0]
    return kernel


def marked(cv, call):
    def run(s, d, *inputs):
        mark(cv)
        return call(cv, s, d, *inputs)
    return run


def rel(tol, abs_tol=None):
    """the norm-relative comparison of the existing suites (orc.rel_err), optionally with their absolute bound"""
    def compare(got, want):
        if got.shape != want.shape or got.dtype != want.dtype:
            return False, None, " (shape / dtype)"
        r = O.rel_err(got, want)
        a = float(np.abs(got.astype(np.float64) - want).max()) if got.size else 0.0
        ok = r <= tol and (abs_tol is None or a <= abs_tol) and not np.isnan(got).any()
        return ok, None, ": rel_err %.3g (<= %g), max abs %.3g" % (r, tol, a)
    return compare


def img(dtype, cn, w, h, seed=0, **kw):
    return vc.content(dtype, (h, w, cn) if cn > 1 else (h, w), seed * 1000 + w * 3 + h, **kw)


class Op:
    """one row of a table.  source(w, h) -> image; oracle(image) -> expected array (None: no image output); call(cv, src_view, dst_view) -> return value;
    compare as in viewcheck; kernel(w, h) -> substring mi355cv_lastKernel must hold on layout A (None: the op's own suite asserts none); extra(rv, image):
    checks of the return value"""

    def __init__(self, name, source, oracle, call, shapes, compare=vc.exact, kernel=None, extra=None):
        self.name, self.source, self.oracle, self.call, self.shapes, self.compare, self.kernel, self.extra = name, source, oracle, call, shapes, compare, kernel, extra


def print_kernel_table(kernels, forms):
    """kernels: (op, layout or form) -> set of kernel names"""
    print("\nop -> kernel named by mi355cv_lastKernel per layout (launch geometry cut; '= A': the same set as the control; %s: the hook names none)" % UNNAMED)
    for name in sorted({k[0] for k in kernels}):
        first, cells = None, []
        for lay in forms:
            if (name, lay) not in kernels:
                continue
            names = " | ".join(sorted(kernels[(name, lay)]))
            cells.append("%s: %s" % (lay, "= " + first[0] if first and names == first[1] else names))
            first = first or (lay, names)
        print("%-36s %s" % (name, "   ".join(cells)))
