"""Builds and loads the host emulations of tests/hostemu (TEST INFRASTRUCTURE, never imported by opencv_amd): the *_math.h lines of opencv_amd/csrc compiled by g++ into
one shared library per emulation.  One compile line and one staleness rule, for every test that holds an emulation against its restatement."""
import ctypes
import glob
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opencv_amd", "csrc")
EMU_DIR = os.path.join(ROOT, "tests", "hostemu")


def load(source, library, flags=()):
    """tests/hostemu/<source> as tests/hostemu/<library>, loaded.  `flags` are the ones that differ between emulations (floating-point contraction, warnings).

    The library is rebuilt when it is missing or older than its source or than ANY header (*.h, *.inc) of opencv_amd/csrc: an over-approximation that rebuilds a
    one-second library too often and in exchange keeps no list of headers that could go stale.  It is written under a temporary name and renamed, so that another
    test process never loads a half-written file."""
    src, out = os.path.join(EMU_DIR, source), os.path.join(EMU_DIR, library)
    deps = [src] + glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.inc"))
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        tmp = os.path.join(EMU_DIR, "tmp%d_%s" % (os.getpid(), library))
        try:
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", *flags, "-I" + CSRC, src, "-o", tmp])
            os.replace(tmp, out)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
    return ctypes.CDLL(out)
