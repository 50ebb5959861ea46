"""The tile kernel of opencv_amd/csrc/nlmeans.hip keeps a wave's 16 rows of weight sums and estimates and the last T rows of squared differences in arrays indexed by
an unrolled walk.  A compiler that moved any of them to scratch memory would turn every offset of the search window into memory traffic.  The compiler decides that, so
the build is checked: every k_nlm_* kernel in the built object must report no spilled registers and no scratch.  The accumulators grow with the channel count, so the
tile kernels are held to the step of the register file that their channel count was designed for: 128 VGPRs for one channel (four waves per SIMD), 168 for two (three
waves), 256 for three (two waves), 512 for four (one wave per SIMD, which a workgroup of four waves still fits).  CPU test: reads the code object's metadata, no GPU."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
VGPR_STEP = {1: 128, 2: 168, 3: 256, 4: 512}
# k_nlm_plain<CN>, k_nlm_tile<CN, TH>: CN = 1 .. 4, TH = 0 .. 4
KERNELS = tuple("k_nlm_plainILi%dE" % cn for cn in range(1, 5)) + tuple("k_nlm_tileILi%dELi%dE" % (cn, th) for cn in range(1, 5) for th in range(5))


def test_no_nlmeans_kernel_spills_or_uses_scratch():
    obj = os.path.join(ROOT, "opencv_amd", "csrc", "build", "nlmeans.o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")):
        pytest.skip("no built object / no llvm tools here")
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "nlmeans.co")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    kernels = [b for b in notes.split("- .agpr_count:")[1:] if "k_nlm_" in b]
    names = [re.search(r"\.name:\s+(\S+)", b).group(1) for b in kernels]
    for k in KERNELS:
        assert any(k in n for n in names), (k, names)
    assert len(kernels) == len(KERNELS), names
    for b, name in zip(kernels, names):
        print(name, {f: int(re.search(r"\.%s:\s+(\d+)" % f, b).group(1)) for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size")})
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1)) == 0, name
        assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", b).group(1)) == 0, name
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)) == 0, name
        m = re.search(r"k_nlm_tileILi(\d)E", name)
        if m:
            assert int(re.search(r"\.vgpr_count:\s+(\d+)", b).group(1)) <= VGPR_STEP[int(m.group(1))], name
