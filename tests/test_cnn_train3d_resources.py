"""The weight-gradient kernels of the 3D training unit compile for gfx950 without scratch and without VGPR spills (CPU: hipcc
cross-compiles).  The MFMA kernel keeps nine 32x32 accumulators (144 registers) across its march over the pixel tiles of one z tap and
must leave room for two workgroups per CU; the plain kernel slices the 125 taps of a 5x5x5 layer by dz so that its 25 fp64 accumulators
stay in registers.  The 2D unit's list is as it was."""
import os
import re
import subprocess

import pytest

from fluidnet_cxx_amd import build

UNIT = "fnx_cnn_train3d.hip"
MFMA, PLAIN = "wgrad_dz_mfma_kernel", "wgrad3d_small_kernel"


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    assert UNIT in build.HIP_UNITS and "-Rpass-analysis=kernel-resource-usage" in build.HIP_UNITS[UNIT]
    cmd = ([build.HIPCC] + build.COMMON + build.HIP_UNITS[UNIT] +
           ["--cuda-device-only", "-c", os.path.join(build.CSRC, UNIT), "-o", str(tmp_path_factory.mktemp("t3d") / "train3d.o")])
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    return p.stdout


def test_scratch_free_lists():
    kernels, _ = build.SCRATCH_FREE[UNIT]
    assert kernels == [MFMA, PLAIN]
    assert "wgrad3_mfma_kernel" not in MFMA and "wgrad3_mfma_kernel" not in PLAIN
    assert build.SCRATCH_FREE["fnx_cnn_train.hip"][0] == ["wgrad3_mfma_kernel"]


def test_weight_gradient_kernels_use_no_scratch(remarks):
    bad, seen = build._scratch_users(remarks, MFMA)
    assert seen == 1, f"one resource-usage remark for {MFMA} expected, {seen} found"
    assert not bad, f"{MFMA} uses scratch / spills VGPRs: {bad}"
    bad, seen = build._scratch_users(remarks, PLAIN)
    assert seen == 3, f"a remark per instantiation (K = 1, 3, 5) of {PLAIN} expected, {seen} found"
    assert not bad, f"{PLAIN} uses scratch / spills VGPRs: {bad}"
    assert "wgrad3_mfma_kernel" not in remarks


def test_mfma_kernel_fits_two_workgroups_per_cu(remarks):
    m = re.search(r"Function Name: \S*" + MFMA + r"\S*.*?VGPRs: (\d+).*?AGPRs: (\d+).*?LDS Size \[bytes/block\]: (\d+)", remarks, re.S)
    assert m, "resource remark format"
    vgprs, agprs, lds = (int(v) for v in m.groups())
    print(f"\n{MFMA}: {vgprs} VGPRs, {agprs} AGPRs, {lds} B LDS")
    # two 4-wave workgroups per CU: 256 registers per lane (VGPRs + AGPRs of the unified file), half of the 160 KiB LDS
    assert vgprs + agprs <= 256 and lds <= 80 * 1024
    for k in re.finditer(r"Function Name: (\S*" + PLAIN + r"\S*).*?VGPRs: (\d+).*?AGPRs: (\d+)", remarks, re.S):
        print(f"{k.group(1)}: {k.group(2)} VGPRs, {k.group(3)} AGPRs")
