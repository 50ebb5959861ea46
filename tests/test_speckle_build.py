"""The tile kernel of opencv_amd/csrc/speckle.hip keeps a lane's four pixels, the four of the row above and three planes of bits in registers, with unrolled loops over
small arrays; a compiler that moved any of them to scratch memory would turn the bit work into memory accesses.  The compiler decides that, so the build is checked:
every k_spk_* kernel in the built object must report no spilled registers and no scratch, and the set of kernels is the expected one.  CPU test: reads the code object's
metadata, no GPU."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
# per depth (CV_8U, CV_16S) the kernels that read the image; the two counting kernels read the parents only
TYPED = ("k_spk_init", "k_spk_link", "k_spk_tile", "k_spk_vseam", "k_spk_hseam", "k_spk_erase")
UNTYPED = ("k_spk_count", "k_spk_count_runs")


def test_no_speckle_kernel_spills_or_uses_scratch():
    obj = os.path.join(ROOT, "opencv_amd", "csrc", "build", "speckle.o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")):
        pytest.skip("no built object / no llvm tools here")
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "speckle.co")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    kernels = [b for b in notes.split("- .agpr_count:")[1:] if "k_spk_" in b]
    names = [re.search(r"\.name:\s+(\S+)", b).group(1) for b in kernels]
    base = sorted(re.search(r"(k_spk_[a-z_]+?)(?:I[hs])?E", n).group(1) for n in names)
    assert base == sorted(TYPED * 2 + UNTYPED), names
    for b, name in zip(kernels, names):
        print(name, {f: int(re.search(r"\.%s:\s+(\d+)" % f, b).group(1)) for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size")})
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1)) == 0, name
        assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", b).group(1)) == 0, name
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)) == 0, name
        if "k_spk_tile" in name:
            assert int(re.search(r"\.vgpr_count:\s+(\d+)", b).group(1)) <= 64, name              # eight waves per SIMD stay possible
            assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", b).group(1)) <= 20 * 1024, name     # and eight tiles per CU in 160 KiB of LDS
