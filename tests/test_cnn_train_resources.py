"""The weight-gradient kernels of the training unit compile for gfx950 without scratch and without VGPR spills, in both dimensions
(CPU: hipcc cross-compiles).  The MFMA kernel keeps nine 32x32 accumulators (144 registers) across its march over the pixel tiles (in 3D:
of one z tap) and must leave room for two workgroups per CU; the plain kernel slices the 125 taps of a 5x5x5 layer by dz so that its 25
fp64 accumulators stay in registers.  build_lib refuses a spilling build too; these tests state it on their own, per instantiation, and
pin the register budget."""
import os
import re
import subprocess

import pytest

from fluidnet_cxx_amd import build

UNIT = "fnx_cnn_train.hip"
MFMA, PLAIN = "wgrad_mfma_kernel", "wgrad_small_kernel"
# the mangled template arguments: IS3D of the MFMA kernel, <K, IS3D> of the plain one
MFMA_INSTANCES = {"2D": "ILb0EE", "3D": "ILb1EE"}
PLAIN_INSTANCES = {f"K = {k}, {dim}": f"ILi{k}ELb{b}EE" for k in (1, 3, 5) for dim, b in (("2D", 0), ("3D", 1))}


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    assert UNIT in build.HIP_UNITS and "-Rpass-analysis=kernel-resource-usage" in build.HIP_UNITS[UNIT]
    cmd = ([build.HIPCC] + build.COMMON + build.HIP_UNITS[UNIT] +
           ["--cuda-device-only", "-c", os.path.join(build.CSRC, UNIT), "-o", str(tmp_path_factory.mktemp("train") / "train.o")])
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    return p.stdout


def resources(remarks, kernel, args):
    """(function, VGPRs, AGPRs, LDS bytes) of the one instantiation of `kernel` whose mangled name carries `args`"""
    found = re.findall(r"Function Name: (\S*\d" + kernel + args + r"\S*).*?VGPRs: (\d+).*?AGPRs: (\d+).*?LDS Size \[bytes/block\]: (\d+)",
                       remarks, re.S)
    assert len(found) == 1, f"one resource-usage remark for {kernel}<{args}> expected, {len(found)} found"
    return (found[0][0],) + tuple(int(v) for v in found[0][1:])


def test_scratch_free_lists():
    kernels, _ = build.SCRATCH_FREE[UNIT]
    assert kernels == [MFMA, PLAIN]
    assert "fnx_cnn_train3d.hip" not in build.HIP_UNITS and "fnx_cnn_train3d.hip" not in build.SCRATCH_FREE
    assert "fnx_scenes3d.hip" not in build.HIP_UNITS and "fnx_scenes3d.hip" not in build.SCRATCH_FREE


def test_wgrad_mfma_kernel_uses_no_scratch(remarks):
    bad, seen = build._scratch_users(remarks, MFMA)
    assert seen == len(MFMA_INSTANCES), f"a remark per instantiation (2D, 3D) of {MFMA} expected, {seen} found"
    assert not bad, f"{MFMA} uses scratch / spills VGPRs: {bad}"
    for args in MFMA_INSTANCES.values():
        resources(remarks, MFMA, args)             # (each instantiation by name; its budget: test_mfma_kernel_fits_two_workgroups_per_cu)


def test_weight_gradient_kernels_use_no_scratch(remarks):
    bad, seen = build._scratch_users(remarks, PLAIN)
    assert seen == len(PLAIN_INSTANCES), f"a remark per instantiation (K = 1, 3, 5 in 2D and 3D) of {PLAIN} expected, {seen} found"
    assert not bad, f"{PLAIN} uses scratch / spills VGPRs: {bad}"
    for what, args in PLAIN_INSTANCES.items():
        _, vgprs, agprs, _ = resources(remarks, PLAIN, args)
        print(f"\n{PLAIN}<{what}>: {vgprs} VGPRs, {agprs} AGPRs")
    assert "wgrad3_mfma_kernel" not in remarks and "wgrad_dz_mfma_kernel" not in remarks and "wgrad3d_small_kernel" not in remarks


def test_mfma_kernel_fits_two_workgroups_per_cu(remarks):
    for dim, args in MFMA_INSTANCES.items():
        name, vgprs, agprs, lds = resources(remarks, MFMA, args)
        print(f"\n{MFMA}<{dim}>: {vgprs} VGPRs, {agprs} AGPRs, {lds} B LDS")
        # two 4-wave workgroups per CU: 256 registers per lane (VGPRs + AGPRs of the unified file), half of the 160 KiB LDS
        assert vgprs + agprs <= 256 and lds <= 80 * 1024, name
