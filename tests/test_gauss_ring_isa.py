"""The rolling Gaussian kernel's row-load ring, checked on the compiler's own gfx950 assembly (CPU only: hipcc cross-compiles without a GPU).

k_binomial_roll2<..., RING = true> (gauss_variant 6, smooth.hip) is meant to keep KS rows of loads in flight per wave.  Whether it does is decided by the
`s_waitcnt vmcnt(N)` the compiler places, and small edits to the loop's control flow have silently turned them into full drains before (a tail guard in
the unrolled group: vmcnt(0) once per KS rows).  With one channel a row is two loads (16 bytes + one side dword), so a wait that leaves the KS - 1 newer
rows in flight is vmcnt(2 (KS - 1)); tools/ring_isa.py prints the whole picture."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ring_isa  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(ring_isa.HIPCC) and shutil.which("hipcc") is None, reason="no hipcc")


@pytest.fixture(scope="module")
def asm():
    return ring_isa.compile_asm()


def _kernel(asm, targs):
    sym, ev = ring_isa.events(asm, ring_isa.mangled("k_binomial_roll2", targs))
    return ev, ring_isa.resources(asm, sym)


@pytest.mark.parametrize("ks", [5, 3])
def test_row_loop_never_drains_the_ring(asm, ks):
    ev, _ = _kernel(asm, "%d,1,true,false,4,true,true" % ks)
    waits = ring_isa.loop_waits(ev)
    assert waits, "no vmcnt wait inside a loop: the row loop was not found"
    assert sum(1 for k, _, _, lp in ev if k == "load" and lp) == 2 * ks      # the loop is the unrolled group of KS rows, each refilling its slot
    assert min(waits) >= 2 * (ks - 1), sorted(set(waits))


def test_prologue_issues_every_starting_row_before_it_waits(asm):
    ks = 5
    ev, _ = _kernel(asm, "5,1,true,false,4,true,true")
    assert ring_isa.loads_before_first_wait(ev) == 2 * (2 * ks - 1)            # KS - 1 prologue rows and KS ring rows, all batched
    first_loop = next(i for i, e in enumerate(ev) if e[3])
    assert not any(e[3] for e in ev[:first_loop] if e[0] == "load")
    # the waits between those loads and the loop are the prologue rows', oldest first, each leaving every newer row in flight
    pre = [a for k, a, _, _ in ev[:first_loop] if k == "wait"]
    assert pre[:ks - 1] == [2 * (2 * ks - 1) - 2 * (i + 1) for i in range(ks - 1)], pre


def test_headline_instance_keeps_five_waves_per_simd(asm):
    _, res = _kernel(asm, "5,1,true,false,4,true,true")
    assert res["vgpr"] <= 96 and res["scratch"] == 0, res
