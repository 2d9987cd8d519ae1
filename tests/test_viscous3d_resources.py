"""The 3D addViscosity march compiles without scratch and without VGPR spills, and in few enough registers for the occupancy DESIGN.md
section 22 counts on (CPU: hipcc cross-compiles for gfx950).  build_lib refuses a spilling build too; this test states it on its own
and adds the register budget: a block is 8 waves, a CU holds 32, so four blocks a CU -- 8 waves a SIMD -- need the allocation
(VGPRs rounded up to a multiple of 8) to stay within 512 / 8 = 64 registers, and 4 x 21120 bytes of LDS within the CU's 160 KiB."""
import os
import re
import subprocess

from fluidnet_cxx_amd import build

UNIT, KERNEL = "fnx_viscous.hip", "add_viscosity3d_kernel"
WAVES_PER_SIMD = 8


def _usage(remarks, kernel, what):
    m = re.search(r"Function Name: \S*" + re.escape(kernel) + r"\S*.*?" + re.escape(what) + r": (\d+)", remarks, re.S)
    assert m, f"no '{what}' remark for {kernel}"
    return int(m.group(1))


def test_add_viscosity3d_uses_no_scratch_and_few_registers(tmp_path):
    kernels, _ = build.SCRATCH_FREE[UNIT]
    assert KERNEL in kernels
    assert "-Rpass-analysis=kernel-resource-usage" in build.HIP_UNITS[UNIT] and "-ffp-contract=off" in build.HIP_UNITS[UNIT]
    cmd = ([build.HIPCC] + build.COMMON + build.HIP_UNITS[UNIT] +
           ["--cuda-device-only", "-c", os.path.join(build.CSRC, UNIT), "-o", str(tmp_path / "viscous.o")])
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    bad, seen = build._scratch_users(p.stdout, KERNEL)
    assert seen == 1, f"expected one resource-usage remark for {KERNEL}, saw {seen}"
    assert not bad, f"{KERNEL} uses scratch / spills VGPRs: {bad}"
    vgprs, lds = _usage(p.stdout, KERNEL, "VGPRs"), _usage(p.stdout, KERNEL, "LDS Size [bytes/block]")
    alloc = (vgprs + 7) // 8 * 8
    print(f"{KERNEL}: {vgprs} VGPRs (allocation {alloc}), {lds} bytes of LDS a block")
    assert min(8, 512 // alloc) >= WAVES_PER_SIMD, f"{vgprs} VGPRs allow {512 // alloc} waves a SIMD, section 22 counts on {WAVES_PER_SIMD}"
    assert 4 * lds <= 160 * 1024
    # the stick kernel is one thread per cell: no scratch either (a runtime-indexed axis would show up here)
    bad, seen = build._scratch_users(p.stdout, "set_wall_bcs_stick3d_kernel")
    assert seen == 1 and not bad, bad
