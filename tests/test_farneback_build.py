"""The kernels of opencv_amd/csrc/farneback.hip hold their taps in kernel arguments indexed by loop counters and their per-pixel sums in small arrays; a compiler that
moved either to scratch memory would turn every tap into a memory access.  The compiler decides that, so the build is checked: every k_fb_* kernel in the built object
must report no spilled registers and no scratch.  CPU test: reads the code object's metadata, no GPU."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
KERNELS = ("k_fb_smooth3", "k_fb_smooth_h", "k_fb_smooth_v", "k_fb_resize", "k_fb_polyexp", "k_fb_update_matrices", "k_fb_update_flow")


def test_no_farneback_kernel_spills_or_uses_scratch():
    obj = os.path.join(ROOT, "opencv_amd", "csrc", "build", "farneback.o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")):
        pytest.skip("no built object / no llvm tools here")
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "farneback.co")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    kernels = [b for b in notes.split("- .agpr_count:")[1:] if "k_fb_" in b]
    names = [re.search(r"\.name:\s+(\S+)", b).group(1) for b in kernels]
    for k in KERNELS:
        assert any(k in n for n in names), (k, names)
    assert len(kernels) == 8, names                                          # k_fb_resize has two instantiations
    for b, name in zip(kernels, names):
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1)) == 0, name
        assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", b).group(1)) == 0, name
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", b).group(1)) <= 64, name       # eight waves per SIMD stay possible
