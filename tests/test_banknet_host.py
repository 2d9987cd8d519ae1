"""The reference's 'FluidNet' bank model without a GPU: the float64 model of tests/banknet_reference.py against what the reference's own
modules computed (tests/golden/banknet.npz), the conditions under which the GPU tests' tolerances mean something, the host behaviour
of FluidNet(mconf) with model='FluidNet', the refusals the C ABI makes before any launch, and the kernels' resources."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from banknet_reference import GOLDEN_SHAPES, SHAPES, bank_input, banknet_forward64, propagating_bank_weights
from fluidnet_cxx_amd import build
from util import FnxGrid, assert_close_rel

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "banknet.npz")
MCONF = dict(model="FluidNet", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True, normalizeInputChan="UDiv",
             normalizeInputThreshold=1e-5, inputDim=2, is3D=False)
NAMES = {"conv1.weight": (16, 2, 3, 3), "conv1.bias": (16,), "convBank.block.0.weight": (16, 16, 3, 3), "convBank.block.0.bias": (16,),
         "convBank.block.2.weight": (16, 16, 3, 3), "convBank.block.2.bias": (16,), "conv2.weight": (16, 16, 1, 1), "conv2.bias": (16,),
         "conv3.weight": (8, 16, 1, 1), "conv3.bias": (8,), "convOut.weight": (1, 8, 1, 1), "convOut.bias": (1,)}


def _header():
    return open(os.path.join(os.path.dirname(build.HERE), "include", "fluidnet_hip.h")).read()


def test_float64_model_vs_reference_net():
    """The model against the reference's own float32 modules at the four golden shapes, 1e-5 |ref|max (torch's float32 forward is
    2.8e-7 to 4.6e-7 |ref|max from a float64 one at these shapes)."""
    g = np.load(GOLDEN)
    w = propagating_bank_weights()
    for i, shape in enumerate(GOLDEN_SHAPES):
        x, ref = g[f"fwd{i}_net_x"], g[f"fwd{i}_net_p"]
        assert x.shape == (shape[0], 2) + shape[1:] and ref.shape == (shape[0], 1) + shape[1:]
        got = banknet_forward64(w, x).numpy()
        print(f"{shape}: {np.abs(got - ref).max() / np.abs(ref).max():.2e} |ref|max")
        assert_close_rel(got, ref, 1e-5, f"float64 model vs the reference's net at {shape}")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_level_reaches_the_output(shape):
    """Under the propagating weights, at every shape of the GPU tests: dropping any one level moves the output by at least 5 % of
    |ref|max, and the output varies about its mean by at least 40 % of |ref|max -- a kernel that loses a level, or a halo, cannot
    hide inside 1e-5.  (Default-scale weights: 0.6 to 2.8 % variation, the output is its bias; they set no tolerance here.)"""
    w = propagating_bank_weights()
    x = bank_input(*shape, boxes=shape[1] >= 16)
    ref = banknet_forward64(w, x).numpy()
    scale = np.abs(ref).max()
    for drop in range(3):
        moved = np.abs(banknet_forward64(w, x, drop=drop).numpy() - ref).max() / scale
        print(f"{shape}: without level {drop} the output moves by {moved:.3f} |ref|max")
        assert moved >= 0.05, (shape, drop, moved)
    var = np.abs(ref - ref.mean()).max() / scale
    print(f"{shape}: variation about the mean {var:.3f} |ref|max")
    assert var >= 0.40, (shape, var)


def test_fresh_net_names_shapes_and_round_trip():
    from fluidnet_cxx_amd import FluidNet
    from fluidnet_cxx_amd.weights import banknet_layers, make_banknet_weights, make_scalenet_weights
    net = FluidNet(MCONF, dropout=False)
    assert net.is_bank and not net.is3D
    sd = net.state_dict()
    assert list(sd) == list(NAMES) and {k: tuple(v.shape) for k, v in sd.items()} == NAMES
    assert sum(v.numel() for v in sd.values()) == 5361
    assert [L["name"] for L in banknet_layers()] == ["conv1", "convBank.block.0", "convBank.block.2", "conv2", "conv3", "convOut"]
    fresh = make_banknet_weights(0)
    assert all(np.array_equal(sd[k].numpy(), fresh[k]) for k in NAMES)
    # the hash streams do not collide with ScaleNet's (2 per layer from 0, in 2D and in 3D)
    from fluidnet_cxx_amd import weights
    assert weights._BANKNET_STREAM0 >= 2 * max(len(weights.scalenet_layers(2, 2)), len(weights.scalenet_layers(2, 3)))
    want = weights.hash_uniform(288, weights._BANKNET_STREAM0, 0) * np.float32(1 / np.sqrt(18))
    assert np.array_equal(fresh["conv1.weight"].ravel(), want)
    # a reference checkpoint always carries multiScale.* and scale.*: accepted and kept verbatim
    w = propagating_bank_weights(3)
    ck = {k: torch.from_numpy(v) for k, v in w.items()}
    ck.update({k: torch.from_numpy(v) for k, v in make_scalenet_weights(1).items()})
    net.load_state_dict(ck)
    back = net.state_dict()
    assert set(back) == set(ck) and all(torch.equal(back[k], ck[k]) for k in ck)
    net2 = FluidNet(MCONF)
    net2.load_state_dict(back)
    assert all(torch.equal(net2.state_dict()[k], ck[k]) for k in ck)
    # a ScaleNet model is what it was
    sn = FluidNet(dict(MCONF, model="ScaleNet"))
    assert not sn.is_bank and all(k.startswith("multiScale.") for k in sn.state_dict())
    assert not FluidNet({k: v for k, v in MCONF.items() if k != "model"}).is_bank


def test_strict_loading():
    from fluidnet_cxx_amd import FluidNet
    net = FluidNet(MCONF)
    w = {k: torch.from_numpy(v) for k, v in propagating_bank_weights().items()}
    missing = {k: v for k, v in w.items() if k != "conv3.bias"}
    with pytest.raises(RuntimeError, match=r'Error\(s\) in loading state_dict for FluidNet:\n\tMissing key\(s\) in state_dict: "conv3.bias"\.'):
        net.load_state_dict(missing)
    with pytest.raises(RuntimeError, match=r'Missing key\(s\)'):
        net.load_state_dict(missing, strict=False)
    extra = dict(w, **{"deconv1.weight": torch.zeros(1)})
    with pytest.raises(RuntimeError, match=r'Unexpected key\(s\) in state_dict: "deconv1.weight"\.'):
        net.load_state_dict(extra)
    net.load_state_dict(extra, strict=False)
    assert "deconv1.weight" not in net.state_dict()
    bad = dict(w, **{"conv2.weight": torch.zeros(16, 16, 3, 3)})
    with pytest.raises(RuntimeError, match=r"size mismatch for conv2.weight: copying a param with shape \(16, 16, 3, 3\) from checkpoint, "
                                           r"the shape in current model is \(16, 16, 1, 1\)\."):
        net.load_state_dict(bad)
    # a ScaleNet checkpoint alone is not a bank checkpoint
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    with pytest.raises(RuntimeError, match=r'Missing key\(s\) in state_dict: "conv1.weight"'):
        net.load_state_dict({k: torch.from_numpy(v) for k, v in make_scalenet_weights(0).items()})


def test_the_bank_blob_cannot_reach_the_native_step_or_the_trainers():
    from fluidnet_cxx_amd import FluidNet, FluidNetTrain, FluidNetTrain3D
    net = FluidNet(MCONF)
    for what in (lambda: net.packed_for("cuda"), lambda: net.packed, lambda: net.multiScale):
        with pytest.raises(RuntimeError, match="bank model"):
            what()
    with pytest.raises(RuntimeError, match="ScaleNet model"):
        FluidNet(dict(MCONF, model="ScaleNet")).bank
    with pytest.raises(AssertionError, match="2D only"):
        FluidNet(dict(MCONF, is3D=True))
    with pytest.raises(AssertionError, match="'ScaleNet' or 'FluidNet'"):
        FluidNet(dict(MCONF, model="BankNet"))
    with pytest.raises(ValueError, match="ScaleNet"):
        FluidNetTrain(MCONF)
    with pytest.raises(ValueError, match="ScaleNet"):
        FluidNetTrain3D(dict(MCONF, is3D=True))
    with pytest.raises(AssertionError, match="inference-only"):
        net.train()


def test_abi_version_and_symbols():
    build.build_all()
    hdr = _header()
    assert int(re.search(r"#define FNX_ABI_VERSION (\d+)", hdr).group(1)) >= 30
    lib = ctypes.CDLL(build.LIB)
    assert lib.fnx_abi_version() == int(re.search(r"#define FNX_ABI_VERSION (\d+)", hdr).group(1))
    for name in ("fnx_banknet_weight_floats", "fnx_banknet_packed_bytes", "fnx_banknet_pack", "fnx_banknet_ws_bytes", "fnx_banknet_forward",
                 "fnx_fluidnet_bank_forward"):
        assert hasattr(lib, name) and re.search(r"\b" + name + r"\(", hdr), name
    lib.fnx_banknet_weight_floats.restype = lib.fnx_banknet_packed_bytes.restype = lib.fnx_banknet_ws_bytes.restype = ctypes.c_size_t
    lib.fnx_banknet_ws_bytes.argtypes = [ctypes.POINTER(FnxGrid), ctypes.c_int]
    assert lib.fnx_banknet_weight_floats() == 5361
    assert lib.fnx_banknet_packed_bytes() >= 5361 * 4 and lib.fnx_banknet_packed_bytes() % 256 == 0
    g = FnxGrid(B=3, D=1, H=36, W=68)
    net_ws = lib.fnx_banknet_ws_bytes(ctypes.byref(g), 0)
    # the two coarser banks' results: 16 channels at 1/4 and 1/16 of the cells = 20 bytes per full-resolution cell
    assert 3 * 36 * 68 * 20 <= net_ws <= 3 * 36 * 68 * 20 + 512
    assert lib.fnx_banknet_ws_bytes(ctypes.byref(g), 1) >= net_ws + 3 * 36 * 68 * 4 * 4
    assert lib.fnx_banknet_ws_bytes(None, 0) == 0


def test_refusals_before_any_launch():
    """fnx_banknet_forward and fnx_fluidnet_bank_forward on dummy host pointers that nothing may read: NULL, a 3D grid, the bf16 modes,
    an unknown mode, H % 4, W % 4 and a short workspace, each with its code and its own text."""
    build.build_all()
    lib = ctypes.CDLL(build.LIB)
    lib.fnx_last_error.restype = ctypes.c_char_p
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    G = ctypes.POINTER(FnxGrid)
    lib.fnx_banknet_forward.argtypes = [G, vp, vp, vp, ci, vp, sz, vp]
    lib.fnx_fluidnet_bank_forward.argtypes = [G, vp, vp, ctypes.c_float, vp, vp, ci, vp, sz, vp]
    lib.fnx_banknet_pack.argtypes = [vp, vp, vp]
    lib.fnx_banknet_ws_bytes.restype = sz
    lib.fnx_banknet_ws_bytes.argtypes = [G, ci]
    a = ctypes.cast(ctypes.create_string_buffer(64), vp).value
    modes = {k: int(v) for k, v in re.findall(r"(FNX_PRECISION_\w+) = (\d+)", _header())}
    EINVAL, EWORKSPACE = 1, [int(v) for v in re.findall(r"FNX_EWORKSPACE = (\d+)", _header())][0]
    big = 1 << 40

    def net(g, mode=0, x=a, ws_bytes=big):
        return lib.fnx_banknet_forward(ctypes.byref(g), a, x, a, mode, a, ws_bytes, None), lib.fnx_last_error().decode()

    def whole(g, mode=0, x=a, ws_bytes=big):
        return lib.fnx_fluidnet_bank_forward(ctypes.byref(g), a, x, 1e-5, a, a, mode, a, ws_bytes, None), lib.fnx_last_error().decode()

    ok = dict(B=1, D=1, H=16, W=24)
    for call, fn in ((net, "fnx_banknet_forward"), (whole, "fnx_fluidnet_bank_forward")):
        assert call(FnxGrid(**ok), x=None) == (EINVAL, f"{fn}: null argument")
        rc, msg = call(FnxGrid(B=1, D=8, H=16, W=24, is3D=1))
        assert rc == EINVAL and "2D only" in msg and msg.startswith(fn), msg
        for m in ("FNX_PRECISION_BF16X6", "FNX_PRECISION_BF16X3"):
            rc, msg = call(FnxGrid(**ok), mode=modes[m])
            assert rc == EINVAL and "fp32 arithmetic only" in msg and "bf16" in msg, msg
        rc, msg = call(FnxGrid(**ok), mode=99)
        assert rc == EINVAL and "unknown precision_mode 99" in msg, msg
        rc, msg = call(FnxGrid(B=1, D=1, H=18, W=24))
        assert rc == EINVAL and "H = 18 must be a positive multiple of 4" in msg, msg
        rc, msg = call(FnxGrid(B=1, D=1, H=16, W=26))
        assert rc == EINVAL and "W = 26 must be a positive multiple of 4" in msg, msg
        need = lib.fnx_banknet_ws_bytes(ctypes.byref(FnxGrid(**ok)), int(call is whole))
        rc, msg = call(FnxGrid(**ok), ws_bytes=need - 1)
        assert rc == EWORKSPACE and f"workspace of {need - 1} bytes is too small" in msg, msg
        # every fp32 mode is taken (the next refusal, the workspace, is reached)
        for m in ("FNX_PRECISION_FP32", "FNX_PRECISION_FP32_DIRECT", "FNX_PRECISION_FP32_F4", "FNX_PRECISION_FP32_F2"):
            assert call(FnxGrid(**ok), mode=modes[m], ws_bytes=0)[0] == EWORKSPACE
    assert lib.fnx_banknet_pack(None, a, None) == EINVAL and lib.fnx_last_error().decode() == "fnx_banknet_pack: null argument"
    # the whole forward's workspace and its refusal word for word, as recorded before the three nets' whole forwards became one body
    assert whole(FnxGrid(**ok), ws_bytes=30463) == (EWORKSPACE, "fnx_fluidnet_bank_forward: workspace of 30463 bytes is too small (30464 needed)")
    assert lib.fnx_banknet_ws_bytes(ctypes.byref(FnxGrid(**ok)), 1) == 30464


def test_bank_kernels_use_no_scratch(tmp_path):
    """The three instantiations of banknet_level_kernel compile for gfx950 without scratch or VGPR spills (build_lib refuses such a build
    too), within a static 64 KiB of LDS -- at least two workgroups of four waves per CU -- and within the registers of as many waves per
    SIMD as that LDS admits."""
    unit = "fnx_banknet.hip"
    kernels, _ = build.SCRATCH_FREE[unit]
    assert kernels == ["banknet_level_kernel"] and "-Rpass-analysis=kernel-resource-usage" in build.HIP_UNITS[unit]
    cmd = ([build.HIPCC] + build.COMMON + build.HIP_UNITS[unit] +
           ["--cuda-device-only", "-c", os.path.join(build.CSRC, unit), "-o", str(tmp_path / "banknet.o")])
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    bad, seen = build._scratch_users(p.stdout, "banknet_level_kernel")
    assert seen == 3, f"one resource-usage remark per level, saw {seen}"
    assert not bad, f"banknet_level_kernel uses scratch / spills VGPRs: {bad}"
    found = re.findall(r"Function Name: \S*banknet_level_kernel\S*.*?VGPRs: (\d+).*?AGPRs: (\d+).*?LDS Size \[bytes/block\]: (\d+)", p.stdout, re.S)
    assert len(found) == 3, "resource remark format"
    for vgprs, agprs, lds in found:
        print(f"\nbanknet_level_kernel: {vgprs} VGPRs, {agprs} AGPRs, {lds} B LDS")
        # a workgroup is one wave per SIMD; LDS admits 160 KiB / lds of them per CU (at least two), and the registers must admit as many
        groups = 160 * 1024 // int(lds)
        assert int(lds) <= 64 * 1024 and groups >= 2
        assert ((int(vgprs) + 7) // 8 * 8 + (int(agprs) + 7) // 8 * 8) * min(groups, 8) <= 512, "registers, not LDS, would limit the occupancy"
