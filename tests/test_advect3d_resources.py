"""The 3D advection tile kernels and the 3D clamp-bounds reduction compile without scratch and without VGPR spills (CPU: hipcc cross-compiles for gfx950).  build_lib
refuses such a build too; this test states it on its own and checks that the remark parser sees every guarded instantiation."""
import os
import subprocess

from fluidnet_cxx_amd import build


def test_advect3d_tile_kernels_use_no_scratch(tmp_path):
    unit = "fnx_advect.hip"
    kernels, _ = build.SCRATCH_FREE[unit]
    assert "-Rpass-analysis=kernel-resource-usage" in build.HIP_UNITS[unit]
    cmd = ([build.HIPCC] + build.COMMON + build.HIP_UNITS[unit] +
           ["--cuda-device-only", "-c", os.path.join(build.CSRC, unit), "-o", str(tmp_path / "advect.o")])
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    for kernel in kernels:
        bad, seen = build._scratch_users(p.stdout, kernel)
        assert seen >= 1, f"no resource-usage remark for {kernel}"
        assert not bad, f"{kernel} uses scratch / spills VGPRs: {bad}"
    # the instantiations a step launches: forward (density + velocity, both sample_outside modes) and the fused backward march
    assert build._scratch_users(p.stdout, "advect3d_fwd_tile_kernel")[1] == 6
    assert build._scratch_users(p.stdout, "advect3d_bwd_tile_kernel")[1] == 2
    # the clamp-bounds reduction of the per-cell path and of the passive scalars (fnx_scalars.hip): both sample_outside modes
    assert "box_minmax_kernel" in kernels and build._scratch_users(p.stdout, "box_minmax_kernel")[1] == 2


def test_scratch_parser_flags_a_spill():
    remarks = ("remark: x.h:1:0: Function Name: _ZN12_GLOBAL__N_124advect3d_bwd_tile_kernelILb0EEEv8GridDims [-Rpass-analysis]\n"
               "remark: x.h:1:0:     VGPRs: 256 [-Rpass-analysis]\n"
               "remark: x.h:1:0:     ScratchSize [bytes/lane]: 92 [-Rpass-analysis]\n"
               "remark: x.h:1:0:     VGPRs Spill: 24 [-Rpass-analysis]\n")
    bad, seen = build._scratch_users(remarks, "advect3d_bwd_tile_kernel")
    assert seen == 1 and bad == [("_ZN12_GLOBAL__N_124advect3d_bwd_tile_kernelILb0EEEv8GridDims", 92, 24)]
