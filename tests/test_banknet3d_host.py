"""The Conv3d bank net ('FluidNet3D') without a GPU: the float64 model of tests/banknet3d_reference.py against torch's own float32
modules, the conditions under which the GPU tests' tolerance means something, the host behaviour of FluidNet(mconf) with
model='FluidNet3D', the refusals the C ABI makes before any launch, the workspace, the launch plan and the kernels' resources."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from banknet3d_reference import SHAPES3D, bank3d_input, banknet3d_forward64, propagating_bank3d_weights
from fluidnet_cxx_amd import build
from util import FnxGrid

MCONF = dict(model="FluidNet3D", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True, normalizeInputChan="UDiv",
             normalizeInputThreshold=1e-5, inputDim=3, is3D=True)
NAMES = {"conv1.weight": (16, 2, 3, 3, 3), "conv1.bias": (16,), "convBank.block.0.weight": (16, 16, 3, 3, 3), "convBank.block.0.bias": (16,),
         "convBank.block.2.weight": (16, 16, 3, 3, 3), "convBank.block.2.bias": (16,), "conv2.weight": (16, 16, 1, 1, 1), "conv2.bias": (16,),
         "conv3.weight": (8, 16, 1, 1, 1), "conv3.bias": (8,), "convOut.weight": (1, 8, 1, 1, 1), "convOut.bias": (1,)}
IDS = ["x".join(map(str, s)) for s in SHAPES3D]


def _header():
    return open(os.path.join(os.path.dirname(build.HERE), "include", "fluidnet_hip.h")).read()


@pytest.fixture(scope="module")
def refs():
    """(x, float64 p) per shape, computed once"""
    w = propagating_bank3d_weights()
    out = {}
    for s in SHAPES3D:
        x = bank3d_input(*s)
        out[s] = (x, banknet3d_forward64(w, x).numpy())
    return out


def torch_float32_net(w, x):
    """the net from torch's own float32 modules (nn.Conv3d, nn.AvgPool3d, F.interpolate(nearest)), the way model.py builds its 2D net"""
    import torch.nn as nn
    import torch.nn.functional as F

    def conv(name, cin, cout, k):
        m = nn.Conv3d(cin, cout, k, padding=k // 2)
        with torch.no_grad():
            m.weight.copy_(torch.from_numpy(w[name + ".weight"]))
            m.bias.copy_(torch.from_numpy(w[name + ".bias"]))
        return m

    conv1, cb0, cb2 = conv("conv1", 2, 16, 3), conv("convBank.block.0", 16, 16, 3), conv("convBank.block.2", 16, 16, 3)
    conv2, conv3, convOut = conv("conv2", 16, 16, 1), conv("conv3", 16, 8, 1), conv("convOut", 8, 1, 1)
    bank = nn.Sequential(cb0, nn.ReLU(), cb2, nn.ReLU())
    with torch.no_grad():
        t = torch.from_numpy(x)
        a = F.relu(conv1(t))
        size = tuple(a.shape[2:])
        t = bank(a) + F.interpolate(bank(nn.AvgPool3d(2)(a)), size=size, mode="nearest") + F.interpolate(bank(nn.AvgPool3d(4)(a)), size=size,
                                                                                                       mode="nearest")
        t = F.relu(conv2(t))
        t = F.relu(conv2(t))
        t = F.relu(conv3(t))
        return convOut(t).numpy()


@pytest.mark.parametrize("shape", SHAPES3D, ids=IDS)
def test_float64_model_vs_torch_float32_modules(refs, shape):
    """1e-5 |ref|max; torch's float32 forward sits 5e-7 to 1.4e-6 |ref|max from the float64 model at these shapes"""
    x, ref = refs[shape]
    got = torch_float32_net(propagating_bank3d_weights(), x)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"{shape}: {err:.2e} |ref|max")
    assert ref.shape == (shape[0], 1) + shape[1:] and err <= 1e-5, (shape, err)


@pytest.mark.parametrize("shape", SHAPES3D, ids=IDS)
def test_every_level_reaches_the_output(refs, shape):
    """Under the propagating weights, at every shape of the GPU tests: dropping any one level moves the output by at least 5 % of
    |ref|max and the output varies about its mean by at least 50 % of |ref|max -- a kernel that loses a level, or a halo, cannot hide
    inside 1e-5.  (Default-scale weights: the output is its bias to within 1.6 %; they set no tolerance here.)"""
    w = propagating_bank3d_weights()
    x, ref = refs[shape]
    scale = np.abs(ref).max()
    for drop in range(3):
        moved = np.abs(banknet3d_forward64(w, x, drop=drop).numpy() - ref).max() / scale
        print(f"{shape}: without level {drop} the output moves by {moved:.3f} |ref|max")
        assert moved >= 0.05, (shape, drop, moved)
    var = np.abs(ref - ref.mean()).max() / scale
    print(f"{shape}: variation about the mean {var:.3f} |ref|max")
    assert var >= 0.50, (shape, var)


def test_fresh_net_names_shapes_and_round_trip():
    from fluidnet_cxx_amd import BankNet, BankNet3D, FluidNet, weights
    from fluidnet_cxx_amd.weights import banknet3d_layers, make_banknet3d_weights, make_scalenet_weights
    assert BankNet3D is not BankNet
    net = FluidNet(MCONF, dropout=False)
    assert net.is_bank and net.is3D
    sd = net.state_dict()
    assert list(sd) == list(NAMES) and {k: tuple(v.shape) for k, v in sd.items()} == NAMES
    assert sum(v.numel() for v in sd.values()) == 15153
    assert [L["name"] for L in banknet3d_layers()] == ["conv1", "convBank.block.0", "convBank.block.2", "conv2", "conv3", "convOut"]
    fresh = make_banknet3d_weights(0)
    assert all(np.array_equal(sd[k].numpy(), fresh[k]) for k in NAMES)
    # hash streams of its own: 1100 .. 1111, torch's default bound
    assert weights._BANKNET3D_STREAM0 == 1100 and weights._BANKNET_STREAM0 + 12 <= weights._BANKNET3D_STREAM0
    assert np.array_equal(fresh["conv1.weight"].ravel(), weights.hash_uniform(864, 1100, 0) * np.float32(1 / np.sqrt(54)))
    assert np.array_equal(fresh["convOut.bias"], weights.hash_uniform(1, 1111, 0) * np.float32(1 / np.sqrt(8)))
    half = make_banknet3d_weights(0, gain=0.5)
    assert np.allclose(half["conv2.weight"], 0.5 * fresh["conv2.weight"], rtol=1e-6, atol=0)
    # multiScale.* and scale.* are accepted and kept verbatim
    ck = {k: torch.from_numpy(v) for k, v in propagating_bank3d_weights(3).items()}
    ck.update({k: torch.from_numpy(v) for k, v in make_scalenet_weights(1, ndim=3).items()})
    ck["scale.weight"] = torch.ones(1)
    net.load_state_dict(ck)
    back = net.state_dict()
    assert set(back) == set(ck) and all(torch.equal(back[k], ck[k]) for k in ck)


def test_strict_loading():
    from fluidnet_cxx_amd import FluidNet
    from fluidnet_cxx_amd.weights import make_banknet_weights, make_scalenet_weights
    net = FluidNet(MCONF)
    w = {k: torch.from_numpy(v) for k, v in propagating_bank3d_weights().items()}
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
    # a 2D bank checkpoint: torch's size-mismatch wording
    with pytest.raises(RuntimeError, match=r"size mismatch for conv1.weight: copying a param with shape \(16, 2, 3, 3\) from checkpoint, "
                                           r"the shape in current model is \(16, 2, 3, 3, 3\)\."):
        net.load_state_dict({k: torch.from_numpy(v) for k, v in make_banknet_weights(0).items()})
    # and the other way round
    with pytest.raises(RuntimeError, match=r"size mismatch for conv1.weight"):
        FluidNet(dict(MCONF, model="FluidNet", is3D=False, inputDim=2)).load_state_dict(w)
    with pytest.raises(RuntimeError, match=r'Missing key\(s\) in state_dict: "conv1.weight"'):
        net.load_state_dict({k: torch.from_numpy(v) for k, v in make_scalenet_weights(0, ndim=3).items()})


def test_python_refusals():
    from fluidnet_cxx_amd import FluidNet, FluidNetBankTrain, FluidNetTrain, FluidNetTrain3D
    from fluidnet_cxx_amd.training3d import train3d
    net = FluidNet(MCONF)
    for what in (lambda: net.packed_for("cuda"), lambda: net.packed, lambda: net.multiScale):
        with pytest.raises(RuntimeError, match="bank model"):
            what()
    with pytest.raises(AssertionError, match="3D only"):
        FluidNet(dict(MCONF, is3D=False))
    with pytest.raises(AssertionError, match="3D only"):
        FluidNet({k: v for k, v in MCONF.items() if k != "is3D"})
    # 'FluidNet' stays what the reference defines, and the message for an unknown model names the new one after the old phrase
    with pytest.raises(AssertionError, match="2D only"):
        FluidNet(dict(MCONF, model="FluidNet"))
    with pytest.raises(AssertionError, match="'ScaleNet' or 'FluidNet' .*'FluidNet3D'"):
        FluidNet(dict(MCONF, model="BankNet"))
    for make in (lambda: FluidNetTrain3D(MCONF), lambda: FluidNetBankTrain(MCONF), lambda: FluidNetTrain(dict(MCONF, is3D=False)),
                 lambda: FluidNetBankTrain(dict(MCONF, is3D=False)), lambda: train3d(MCONF, dict(res=16, batch=1))):
        with pytest.raises(ValueError, match="training the 'FluidNet3D' model is not built"):
            make()
    with pytest.raises(AssertionError, match="inference-only"):
        net.train()


def _lib():
    build.build_all()
    lib = ctypes.CDLL(build.LIB)
    lib.fnx_last_error.restype = ctypes.c_char_p
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    G = ctypes.POINTER(FnxGrid)
    lib.fnx_banknet3d_weight_floats.restype = lib.fnx_banknet3d_packed_bytes.restype = lib.fnx_banknet3d_ws_bytes.restype = sz
    lib.fnx_banknet3d_ws_bytes.argtypes = [G, ci]
    lib.fnx_banknet3d_forward.argtypes = [G, vp, vp, vp, ci, vp, sz, vp]
    lib.fnx_fluidnet_bank3d_forward.argtypes = [G, vp, vp, ctypes.c_float, vp, vp, ci, vp, sz, vp]
    lib.fnx_banknet3d_pack.argtypes = [vp, vp, vp]
    lib.fnx_banknet3d_launch_plan.argtypes = [G, ci, ctypes.POINTER(ci * 6)]
    return lib


def test_abi_version_symbols_and_workspace():
    lib = _lib()
    hdr = _header()
    assert int(re.search(r"#define FNX_ABI_VERSION (\d+)", hdr).group(1)) >= 32
    assert lib.fnx_abi_version() == int(re.search(r"#define FNX_ABI_VERSION (\d+)", hdr).group(1))
    for name in ("fnx_banknet3d_weight_floats", "fnx_banknet3d_packed_bytes", "fnx_banknet3d_pack", "fnx_banknet3d_ws_bytes",
                 "fnx_banknet3d_forward", "fnx_fluidnet_bank3d_forward", "fnx_banknet3d_launch_plan"):
        assert hasattr(lib, name) and re.search(r"\b" + name + r"\(", hdr), name
    assert lib.fnx_banknet3d_weight_floats() == 15153 == 880 + 6928 + 6928 + 272 + 136 + 9
    assert lib.fnx_banknet3d_packed_bytes() >= 15153 * 4 and lib.fnx_banknet3d_packed_bytes() % 256 == 0
    for B, D, H, W in ((3, 8, 36, 68), (1, 4, 4, 4), (2, 64, 64, 64)):
        g = FnxGrid(B=B, D=D, H=H, W=W, is3D=1)
        cells = B * D * H * W
        net_ws = lib.fnx_banknet3d_ws_bytes(ctypes.byref(g), 0)
        # relu(conv1) and block.0's output at full resolution (2 x 64 B a cell), three 16-channel tensors at 1/8 of the cells (3 x 8 B) and
        # three at 1/64 (3 x 1 B): 155 bytes per full-resolution cell, each of the eight tensors rounded up to 256 bytes
        assert cells * 155 <= net_ws <= cells * 155 + 8 * 255, (B, D, H, W, net_ws)
        whole = lib.fnx_banknet3d_ws_bytes(ctypes.byref(g), 1)
        # + the flags copy, the divergence and the two-channel input (16 B a cell), 1024 pairs of fp64 partial sums and a scale a sample
        assert net_ws + cells * 16 + 16388 * B <= whole <= net_ws + cells * 16 + 16388 * B + 5 * 255, (whole, net_ws)
    assert lib.fnx_banknet3d_ws_bytes(None, 0) == 0
    assert lib.fnx_banknet3d_ws_bytes(ctypes.byref(FnxGrid(B=1, D=1, H=16, W=16)), 0) == 0


def test_refusals_before_any_launch():
    """fnx_banknet3d_forward and fnx_fluidnet_bank3d_forward on dummy host pointers that nothing may read: NULL, a grid that is not 3D,
    D, H or W no multiple of 4, the bf16 modes, an unknown mode and a short workspace, each with its code, its own text and the
    function's name in front."""
    lib = _lib()
    vp = ctypes.c_void_p
    a = ctypes.cast(ctypes.create_string_buffer(64), vp).value
    modes = {k: int(v) for k, v in re.findall(r"(FNX_PRECISION_\w+) = (\d+)", _header())}
    EINVAL, EWORKSPACE = 1, [int(v) for v in re.findall(r"FNX_EWORKSPACE = (\d+)", _header())][0]
    big = 1 << 44

    def net(g, mode=0, x=a, ws_bytes=big):
        return lib.fnx_banknet3d_forward(ctypes.byref(g), a, x, a, mode, a, ws_bytes, None), lib.fnx_last_error().decode()

    def whole(g, mode=0, x=a, ws_bytes=big):
        return lib.fnx_fluidnet_bank3d_forward(ctypes.byref(g), a, x, 1e-5, a, a, mode, a, ws_bytes, None), lib.fnx_last_error().decode()

    ok = dict(B=1, D=8, H=16, W=24, is3D=1)
    for call, fn in ((net, "fnx_banknet3d_forward"), (whole, "fnx_fluidnet_bank3d_forward")):
        assert call(FnxGrid(**ok), x=None) == (EINVAL, f"{fn}: null argument")
        for bad in (dict(ok, is3D=0), dict(ok, D=1, is3D=0), dict(ok, D=1), dict(ok, D=3)):
            rc, msg = call(FnxGrid(**bad))
            assert rc == EINVAL and "3D only" in msg and msg.startswith(fn + ": "), msg
        for axis, v in (("D", 6), ("H", 18), ("W", 26), ("D", 10)):
            rc, msg = call(FnxGrid(**dict(ok, **{axis: v})))
            assert rc == EINVAL and f"{axis} = {v} must be a positive multiple of 4" in msg and msg.startswith(fn + ": "), msg
        rc, msg = call(FnxGrid(**dict(ok, W=0)))
        assert rc == EINVAL and "W = 0 must be a positive multiple of 4" in msg, msg
        for m in ("FNX_PRECISION_BF16X6", "FNX_PRECISION_BF16X3"):
            rc, msg = call(FnxGrid(**ok), mode=modes[m])
            assert rc == EINVAL and "fp32 arithmetic only" in msg and "bf16" in msg and msg.startswith(fn + ": "), msg
        rc, msg = call(FnxGrid(**ok), mode=99)
        assert rc == EINVAL and "unknown precision_mode 99" in msg and msg.startswith(fn + ": "), msg
        need = lib.fnx_banknet3d_ws_bytes(ctypes.byref(FnxGrid(**ok)), int(call is whole))
        rc, msg = call(FnxGrid(**ok), ws_bytes=need - 1)
        assert rc == EWORKSPACE and f"workspace of {need - 1} bytes is too small" in msg and msg.startswith(fn + ": "), msg
        # every fp32 mode is taken (the next refusal, the workspace, is reached)
        for m in ("FNX_PRECISION_FP32", "FNX_PRECISION_FP32_DIRECT", "FNX_PRECISION_FP32_F4", "FNX_PRECISION_FP32_F2"):
            assert call(FnxGrid(**ok), mode=modes[m], ws_bytes=0)[0] == EWORKSPACE
    assert lib.fnx_banknet3d_pack(None, a, None) == EINVAL and lib.fnx_last_error().decode() == "fnx_banknet3d_pack: null argument"
    # the whole forward's workspace and its refusal word for word, as recorded before the three nets' whole forwards became one body
    assert whole(FnxGrid(**ok), ws_bytes=541951) == (EWORKSPACE,
                                                     "fnx_fluidnet_bank3d_forward: workspace of 541951 bytes is too small (541952 needed)")
    assert lib.fnx_banknet3d_ws_bytes(ctypes.byref(FnxGrid(**ok)), 1) == 541952


def test_launch_plan_covers_every_cell_once():
    """The plan of the 16 -> 16 convolution, a host function of (B, D, H, W): at each level of each grid, the (y, x) tiles and the z
    chunks cover every cell exactly once, no chunk is empty, and the plan's grid stays within a launch's limits.  The test shapes, cubes
    and grids whose extents are no multiple of the tile."""
    lib = _lib()
    grids = list(SHAPES3D) + [(1, 64, 64, 64), (4, 64, 64, 64), (1, 128, 128, 128), (1, 256, 256, 256), (1, 8, 124, 244), (1, 36, 4, 32),
                              (7, 12, 8, 60), (1, 4, 4, 4096)]
    split = False
    for B, D, H, W in grids:
        for level in (1, 2, 4):
            plan = (ctypes.c_int * 6)()
            assert lib.fnx_banknet3d_launch_plan(ctypes.byref(FnxGrid(B=B, D=D, H=H, W=W, is3D=1)), level, ctypes.byref(plan)) == 0
            tx, ty, chunks, chunk, th, tw = list(plan)
            d, h, w = D // level, H // level, W // level
            assert tx >= 1 and ty >= 1 and chunks >= 1 and chunk >= 1 and ty * chunks <= 65535 and B <= 65535
            assert chunks == 1 or chunk >= 4, "a chunk loads two planes more than it computes"
            seen = np.zeros((d, h, w), np.int32)
            for c in range(chunks):
                z0, z1 = c * chunk, min(d, (c + 1) * chunk)
                assert z0 < z1, ("an empty chunk", (B, D, H, W), level, list(plan))
                for i in range(ty):
                    for j in range(tx):
                        seen[z0:z1, i * th:(i + 1) * th, j * tw:(j + 1) * tw] += 1
            assert (seen == 1).all(), ((B, D, H, W), level, list(plan))
            split |= chunks > 1
    assert split
    bad = (ctypes.c_int * 6)()
    assert lib.fnx_banknet3d_launch_plan(ctypes.byref(FnxGrid(B=1, D=8, H=8, W=8, is3D=1)), 3, ctypes.byref(bad)) == 1
    assert lib.fnx_banknet3d_launch_plan(ctypes.byref(FnxGrid(B=1, D=8, H=8, W=10, is3D=1)), 1, ctypes.byref(bad)) == 1


def test_bank3d_kernels_use_no_scratch(tmp_path):
    """bank3d_conv1_kernel and the two instantiations of bank3d_conv_kernel compile for gfx950 without scratch or VGPR spills (build_lib
    refuses such a build too), within a static 64 KiB of LDS, and both LDS and registers admit two workgroups (two waves a SIMD) per CU."""
    unit = "fnx_banknet3d.hip"
    kernels, _ = build.SCRATCH_FREE[unit]
    assert kernels == ["bank3d_conv1_kernel", "bank3d_conv_kernel"] and "-Rpass-analysis=kernel-resource-usage" in build.HIP_UNITS[unit]
    cmd = ([build.HIPCC] + build.COMMON + build.HIP_UNITS[unit] +
           ["--cuda-device-only", "-c", os.path.join(build.CSRC, unit), "-o", str(tmp_path / "banknet3d.o")])
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    for kernel, n in (("bank3d_conv1_kernel", 1), ("bank3d_conv_kernel", 2)):
        bad, seen = build._scratch_users(p.stdout, kernel)
        assert seen == n, f"{kernel}: {n} resource-usage remark(s) expected, saw {seen}"
        assert not bad, f"{kernel} uses scratch / spills VGPRs: {bad}"
        found = re.findall(r"Function Name: \S*" + kernel + r"\S*.*?VGPRs: (\d+).*?AGPRs: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?"
                           r"LDS Size \[bytes/block\]: (\d+)", p.stdout, re.S)
        assert len(found) == n, "resource remark format"
        for vgprs, agprs, waves, lds in found:
            print(f"\n{kernel}: {vgprs} VGPRs, {agprs} AGPRs, {waves} waves a SIMD, {lds} B LDS")
            # a workgroup is one wave per SIMD.  The AGPRs follow the VGPRs at a multiple of 4 in the 512 registers a SIMD lane has, and
            # a wave's share is a multiple of 8
            assert int(lds) <= 64 * 1024 and 2 * int(lds) <= 160 * 1024
            assert (((int(vgprs) + 3) // 4 * 4 + int(agprs)) + 7) // 8 * 8 * 2 <= 512 and int(waves) >= 2, "fewer than two waves a SIMD"
