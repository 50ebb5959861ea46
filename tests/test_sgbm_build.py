"""The kernels of opencv_amd/csrc/sgbm.hip keep their state in small arrays indexed by unrolled loops: the cost kernel a lane's 16 running sums, the fast path kernel
the previous step's costs and two blocks of loaded vectors.  A compiler that moved any of them to scratch memory would turn the dependent chain of a path into memory
accesses.  The compiler decides that, so the build is checked: every k_sgbm_* kernel in the built object must report no spilled registers and no scratch, the cost kernel
at most 128 VGPRs (its workgroup is up to 1024 lanes) and the fast path kernels at most 128.  CPU test: reads the code object's metadata, no GPU."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
KERNELS = ("k_sgbm_prefilter", "k_sgbm_fill", "k_sgbm_cost", "k_sgbm_path_plain", "k_sgbm_path_fastILi16ELi1E", "k_sgbm_path_fastILi32ELi1E", "k_sgbm_path_fastILi64ELi1E",
           "k_sgbm_path_fastILi64ELi2E", "k_sgbm_path_fastILi64ELi4E", "k_sgbm_decide", "k_sgbm_lr_vote", "k_sgbm_lr_apply", "k_sgbm_store")


def test_no_sgbm_kernel_spills_or_uses_scratch():
    obj = os.path.join(ROOT, "opencv_amd", "csrc", "build", "sgbm.o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")):
        pytest.skip("no built object / no llvm tools here")
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "sgbm.co")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    kernels = [b for b in notes.split("- .agpr_count:")[1:] if "k_sgbm_" in b]
    names = [re.search(r"\.name:\s+(\S+)", b).group(1) for b in kernels]
    for k in KERNELS:
        assert any(k in n for n in names), (k, names)
    assert len(kernels) == len(KERNELS), names
    for b, name in zip(kernels, names):
        print(name, {f: int(re.search(r"\.%s:\s+(\d+)" % f, b).group(1)) for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size")})
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1)) == 0, name
        assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", b).group(1)) == 0, name
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)) == 0, name
        if "k_sgbm_cost" in name or "k_sgbm_path_fast" in name:
            assert int(re.search(r"\.vgpr_count:\s+(\d+)", b).group(1)) <= 128, name
