"""The fast kernel of opencv_amd/csrc/stereobm.hip holds a lane's 16 running sums and its 16 SADs in small arrays indexed by unrolled loops; a compiler that moved either
to scratch memory would turn every byte difference into a memory access.  The compiler decides that, so the build is checked: every k_sbm* kernel in the built object must
report no spilled registers and no scratch, and the fast cost kernel at most 128 VGPRs.  CPU test: reads the code object's metadata, no GPU."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
KERNELS = ("k_sbm_prefilter", "k_sbm_fill", "k_sbm_cost_generic", "k_sbm_cost_roll", "k_sbm_lr_vote", "k_sbm_lr_apply", "k_sbm_to32f")


def test_no_stereobm_kernel_spills_or_uses_scratch():
    obj = os.path.join(ROOT, "opencv_amd", "csrc", "build", "stereobm.o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")):
        pytest.skip("no built object / no llvm tools here")
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "stereobm.co")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    kernels = [b for b in notes.split("- .agpr_count:")[1:] if "k_sbm_" in b]
    names = [re.search(r"\.name:\s+(\S+)", b).group(1) for b in kernels]
    for k in KERNELS:
        assert any(k in n for n in names), (k, names)
    assert len(kernels) == len(KERNELS), names
    for b, name in zip(kernels, names):
        print(name, {f: int(re.search(r"\.%s:\s+(\d+)" % f, b).group(1)) for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size")})
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1)) == 0, name
        assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", b).group(1)) == 0, name
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)) == 0, name
        if "k_sbm_cost_roll" in name:
            assert int(re.search(r"\.vgpr_count:\s+(\d+)", b).group(1)) <= 128, name          # four waves per SIMD stay possible
