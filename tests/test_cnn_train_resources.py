"""The MFMA weight-gradient kernel compiles for gfx950 without scratch and without VGPR spills (CPU: hipcc cross-compiles).  Its nine
32x32 accumulators (144 registers) live across the whole march over the pixel tiles; build_lib refuses a spilling build too, this
test states it on its own and pins the register budget that lets two workgroups share a CU."""
import os
import re
import subprocess

from fluidnet_cxx_amd import build


def test_wgrad_mfma_kernel_uses_no_scratch(tmp_path):
    unit = "fnx_cnn_train.hip"
    assert unit in build.HIP_UNITS and "-Rpass-analysis=kernel-resource-usage" in build.HIP_UNITS[unit]
    kernels, _ = build.SCRATCH_FREE[unit]
    assert kernels == ["wgrad3_mfma_kernel"]
    cmd = ([build.HIPCC] + build.COMMON + build.HIP_UNITS[unit] +
           ["--cuda-device-only", "-c", os.path.join(build.CSRC, unit), "-o", str(tmp_path / "train.o")])
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    bad, seen = build._scratch_users(p.stdout, "wgrad3_mfma_kernel")
    assert seen == 1, "no resource-usage remark for wgrad3_mfma_kernel"
    assert not bad, f"wgrad3_mfma_kernel uses scratch / spills VGPRs: {bad}"
    m = re.search(r"Function Name: \S*wgrad3_mfma_kernel\S*.*?VGPRs: (\d+).*?AGPRs: (\d+).*?LDS Size \[bytes/block\]: (\d+)", p.stdout, re.S)
    assert m, "resource remark format"
    vgprs, agprs, lds = (int(v) for v in m.groups())
    print(f"\nwgrad3_mfma_kernel: {vgprs} VGPRs, {agprs} AGPRs, {lds} B LDS")
    # two 4-wave workgroups per CU: 256 registers per lane (VGPRs + AGPRs of the unified file), half of the 160 KiB LDS
    assert vgprs + agprs <= 256 and lds <= 80 * 1024
