"""The kernels of opencv_amd/csrc/bfmatch.hip hold a query's descriptor and its k best keys in small arrays indexed by unrolled loops; a compiler that moved either to
scratch memory would turn every XOR / popcount and every insertion into a memory access.  The compiler decides that, so the build is checked: every k_bf* kernel in the
built object must report no spilled registers and no scratch.  CPU test: reads the code object's metadata, no GPU."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
KERNELS = ("k_bf_hamming", "k_bf_generic", "k_bf_merge", "k_bf_intersect", "k_bf_radius", "k_bf_scan", "k_bf_radius_sort")


def test_no_bfmatch_kernel_spills_or_uses_scratch():
    obj = os.path.join(ROOT, "opencv_amd", "csrc", "build", "bfmatch.o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")):
        pytest.skip("no built object / no llvm tools here")
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "bfmatch.co")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    kernels = [b for b in notes.split("- .agpr_count:")[1:] if "k_bf_" in b]
    names = [re.search(r"\.name:\s+(\S+)", b).group(1) for b in kernels]
    for k in KERNELS:
        assert any(k in n for n in names), (k, names)
    # k_bf_hamming: rows of 8 / 16 dwords x lists of 1, 2, 4, 8; k_bf_generic: lists of 1, 2, 4, 8; k_bf_radius: count and fill
    assert len(kernels) == 8 + 4 + 2 + 4, names
    for b, name in zip(kernels, names):
        print(name, {f: int(re.search(r"\.%s:\s+(\d+)" % f, b).group(1)) for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size")})
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1)) == 0, name
        assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", b).group(1)) == 0, name
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", b).group(1)) <= 128, name      # four waves per SIMD stay possible: the kernels are bound by the vector ALU, not by latency
