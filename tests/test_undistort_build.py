"""k_undist8_tile of opencv_amd/csrc/undistort.hip keeps the fixed-point coordinates of a lane's 16 (one channel) or 8 (3 / 4 channels) pixels in registers with
compile-time indices, across the frames of a batch.  A compiler that moved them to scratch memory, or that kept every pixel's derived offsets and weights alive across the
frame loop (it did: 506 VGPRs and spilled SGPRs before the coordinates went behind an empty asm and the arguments into HBM), would cost the kernel its occupancy.  The
compiler decides that, so the build is checked: every k_undist* and k_reproject* kernel in the built object must report no spilled registers and no scratch, and the tile
kernels stay within 128 VGPRs, the step of the register file the design chose: four waves per SIMD, which the default LDS allotment of 24 KiB (six workgroups of four
waves per CU) can use up.  CPU test: reads the code object's metadata, no GPU."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
TILE_VGPR_STEP = 128
KERNELS = ("k_undist_map", "k_reproject3d") + tuple("k_undist8_tileILi%dE" % cn for cn in (1, 3, 4))


def test_no_undistort_kernel_spills_or_uses_scratch():
    obj = os.path.join(ROOT, "opencv_amd", "csrc", "build", "undistort.o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")):
        pytest.skip("no built object / no llvm tools here")
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "undistort.co")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    kernels = [b for b in notes.split("- .agpr_count:")[1:] if "k_undist" in b or "k_reproject" in b]
    names = [re.search(r"\.name:\s+(\S+)", b).group(1) for b in kernels]
    for k in KERNELS:
        assert any(k in n for n in names), (k, names)
    assert len(kernels) == len(KERNELS), names
    for b, name in zip(kernels, names):
        print(name, {f: int(re.search(r"\.%s:\s+(\d+)" % f, b).group(1)) for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size")})
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", b).group(1)) == 0, name
        assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", b).group(1)) == 0, name
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", b).group(1)) == 0, name
        if "k_undist8_tile" in name:
            assert int(re.search(r"\.vgpr_count:\s+(\d+)", b).group(1)) <= TILE_VGPR_STEP, name
