"""Training of the 'FluidNet' bank model without a GPU: the ABI's version and symbols, the tape layout, the refusals the new entry points
make before any launch, the new unit's resources, the conditions under which the GPU tests' bounds mean something (every level and
both applications of conv2 carry a share of the shared tensors' gradients), and the host behaviour of FluidNetBankTrain and train()."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import banknet_grad_reference as BG
from banknet_reference import SHAPES, bank_input, propagating_bank_weights
from fluidnet_cxx_amd import build
from util import FnxGrid

MCONF = dict(model="FluidNet", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True, normalizeInputChan="UDiv",
             normalizeInputThreshold=1e-5, inputDim=2, is3D=False)
EINVAL = 1
NEW_SYMBOLS = ["fnx_banknet_tape_entries", "fnx_banknet_tape_layout", "fnx_banknet_packed_t_bytes", "fnx_banknet_pack_t",
               "fnx_banknet_backward_ws_bytes", "fnx_banknet_forward_train", "fnx_banknet_backward", "fnx_fluidnet_bank_train_ws_bytes",
               "fnx_fluidnet_bank_forward_train", "fnx_fluidnet_bank_backward"]


class TapeEntry(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 8), ("offset", ctypes.c_size_t), ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int)]


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(build.LIB)
    lib.fnx_last_error.restype = ctypes.c_char_p
    for fn in ("fnx_banknet_tape_layout", "fnx_banknet_packed_t_bytes", "fnx_banknet_backward_ws_bytes", "fnx_fluidnet_bank_train_ws_bytes"):
        getattr(lib, fn).restype = ctypes.c_size_t
    return lib


def _header():
    return open(os.path.join(os.path.dirname(build.HERE), "include", "fluidnet_hip.h")).read()


def test_abi_version_and_symbols(lib):
    hdr = _header()
    version = int(re.search(r"#define FNX_ABI_VERSION (\d+)", hdr).group(1))
    assert version >= 31 and lib.fnx_abi_version() == version
    for fn in NEW_SYMBOLS:
        assert hasattr(lib, fn) and re.search(r"\b" + fn + r"\(", hdr), fn
    assert "HSA_XNACK" not in hdr


def test_tape_layout(lib):
    B, H, W = 3, 36, 68
    g = FnxGrid(B=B, D=1, H=H, W=W)
    n = lib.fnx_banknet_tape_entries()
    e = (TapeEntry * n)()
    total = lib.fnx_banknet_tape_layout(ctypes.byref(g), e)
    assert total == lib.fnx_banknet_tape_layout(ctypes.byref(g), None)
    got = [(t.name.decode(), t.C, t.H, t.W) for t in e]
    want = [("a", 16, H, W), ("h1", 16, H, W), ("b1", 16, H, W), ("a2", 16, H // 2, W // 2), ("h2", 16, H // 2, W // 2),
            ("b2", 16, H // 2, W // 2), ("a4", 16, H // 4, W // 4), ("h4", 16, H // 4, W // 4), ("b4", 16, H // 4, W // 4),
            ("t", 16, H, W), ("c2a", 16, H, W), ("c2b", 16, H, W), ("c3", 8, H, W), ("x", 2, H, W)]
    assert got == want and [t[0] for t in want] == BG.TAPE_NAMES
    end = 0
    for t in e:
        assert t.offset >= end and t.offset % 64 == 0, t.name       # no overlap, in order
        end = t.offset + B * t.C * t.H * t.W
    assert end <= total < end + 64
    # 16 (1 + 2 + 3/4 + 3/16) + 16 * 3 + 8 + 2 = 121 floats per full-resolution cell
    assert sum(B * t.C * t.H * t.W for t in e) == 121 * B * H * W
    # a function of (B, H, W) alone; grids without a layout
    e2 = (TapeEntry * n)()
    assert lib.fnx_banknet_tape_layout(ctypes.byref(FnxGrid(B=B, D=1, H=H, W=W)), e2) == total
    assert [(t.name, t.offset) for t in e2] == [(t.name, t.offset) for t in e]
    for bad in (FnxGrid(B=1, D=1, H=18, W=24), FnxGrid(B=1, D=4, H=16, W=24, is3D=1), FnxGrid(B=0, D=1, H=16, W=24)):
        assert lib.fnx_banknet_tape_layout(ctypes.byref(bad), None) == 0


def test_refusals_before_any_launch(lib):
    """null arguments, 3D, bf16 modes, an unknown mode, H or W no multiple of 4 and a short workspace, on dummy host pointers: nothing
    reaches the device"""
    hdr = _header()
    modes = {k: int(v) for k, v in re.findall(r"(FNX_PRECISION_\w+) = (\d+)", hdr)}
    EWORKSPACE = [int(v) for v in re.findall(r"FNX_EWORKSPACE = (\d+)", hdr)][0]
    a = ctypes.c_void_p(64)                # never dereferenced
    f = ctypes.c_float(1e-5)
    size = ctypes.c_size_t

    def fwd(g, mode=0, x=a, ws_bytes=0):
        return lib.fnx_banknet_forward_train(ctypes.byref(g), a, x, a, a, mode, None)

    def bwd(g, mode=0, x=a, ws_bytes=1 << 40):
        return lib.fnx_banknet_backward(ctypes.byref(g), a, x, a, a, a, mode, a, size(ws_bytes), None)

    def ffwd(g, mode=0, x=a, ws_bytes=1 << 40):
        return lib.fnx_fluidnet_bank_forward_train(ctypes.byref(g), a, x, f, a, a, a, a, a, mode, a, size(ws_bytes), None)

    def fbwd(g, mode=0, x=a, ws_bytes=1 << 40):
        return lib.fnx_fluidnet_bank_backward(ctypes.byref(g), a, x, a, a, a, a, a, mode, a, size(ws_bytes), None)

    ok = dict(B=1, D=1, H=16, W=24)
    sizes = {bwd: lib.fnx_banknet_backward_ws_bytes, ffwd: lib.fnx_fluidnet_bank_train_ws_bytes, fbwd: lib.fnx_fluidnet_bank_train_ws_bytes}
    for call, fn in ((fwd, "fnx_banknet_forward_train"), (bwd, "fnx_banknet_backward"), (ffwd, "fnx_fluidnet_bank_forward_train"),
                     (fbwd, "fnx_fluidnet_bank_backward")):
        def msg_of(rc):
            return rc, lib.fnx_last_error().decode()
        assert msg_of(call(FnxGrid(**ok), x=None)) == (EINVAL, f"{fn}: null argument")
        rc, msg = msg_of(call(FnxGrid(B=1, D=8, H=16, W=24, is3D=1)))
        assert rc == EINVAL and "2D only" in msg and msg.startswith(fn), msg
        for m in ("FNX_PRECISION_BF16X6", "FNX_PRECISION_BF16X3"):
            rc, msg = msg_of(call(FnxGrid(**ok), mode=modes[m]))
            assert rc == EINVAL and "fp32 arithmetic only" in msg and "bf16" in msg, msg
        rc, msg = msg_of(call(FnxGrid(**ok), mode=99))
        assert rc == EINVAL and "unknown precision_mode 99" in msg and msg.startswith(fn), msg
        rc, msg = msg_of(call(FnxGrid(B=1, D=1, H=18, W=24)))
        assert rc == EINVAL and "H = 18 must be a positive multiple of 4" in msg, msg
        rc, msg = msg_of(call(FnxGrid(B=1, D=1, H=16, W=26)))
        assert rc == EINVAL and "W = 26 must be a positive multiple of 4" in msg, msg
        if call in sizes:
            need = sizes[call](ctypes.byref(FnxGrid(**ok)))
            assert need > 0
            rc, msg = msg_of(call(FnxGrid(**ok), ws_bytes=need - 1))
            assert rc == EWORKSPACE and f"workspace of {need - 1} bytes is too small" in msg, msg
            for m in ("FNX_PRECISION_FP32", "FNX_PRECISION_FP32_DIRECT", "FNX_PRECISION_FP32_F4", "FNX_PRECISION_FP32_F2"):
                assert call(FnxGrid(**ok), mode=modes[m], ws_bytes=0) == EWORKSPACE
    assert lib.fnx_banknet_pack_t(None, a, None) == EINVAL and lib.fnx_last_error().decode() == "fnx_banknet_pack_t: null argument"
    # one workspace size serves the FluidNet-level forward and backward, and it grows with the grid
    g1, g2 = FnxGrid(**ok), FnxGrid(B=2, D=1, H=32, W=24)
    assert lib.fnx_fluidnet_bank_train_ws_bytes(ctypes.byref(g2)) > lib.fnx_fluidnet_bank_train_ws_bytes(ctypes.byref(g1)) > \
        lib.fnx_banknet_backward_ws_bytes(ctypes.byref(g1))
    # the sizes themselves at two grids, as recorded before the four nets' training wrappers became one body
    for shape, train_ws in (((3, 1, 36, 68), 3068672), ((64, 1, 4, 4), 4026368)):
        assert lib.fnx_fluidnet_bank_train_ws_bytes(ctypes.byref(FnxGrid(*shape))) == train_ws, shape
    assert lib.fnx_banknet_backward_ws_bytes(ctypes.byref(FnxGrid(3, 1, 36, 68))) == 2892032


def test_train_kernels_resources(tmp_path):
    """The new unit compiles for gfx950 without scratch or VGPR spills (build_lib refuses such a build too) and within a static 64 KiB of
    LDS; a kernel that uses LDS stays within the registers of as many workgroups (of one wave per SIMD) as that LDS admits per CU -- the
    rule of test_bank_kernels_use_no_scratch -- and at least two; the one kernel without LDS (conv1's plain sums, 76 accumulators a
    lane), which no LDS limits, within the registers of two workgroups per CU too.  The inference unit keeps its figures."""
    unit = "fnx_banknet_train.hip"
    kernels, _ = build.SCRATCH_FREE[unit]
    assert set(kernels) == {"banknet_level_tape_kernel", "bank_tail_bwd_kernel", "bank_level_bwd_kernel", "bank_conv1_bwd_kernel"}
    assert "-Rpass-analysis=kernel-resource-usage" in build.HIP_UNITS[unit]
    cmd = ([build.HIPCC] + build.COMMON + build.HIP_UNITS[unit] +
           ["--cuda-device-only", "-c", os.path.join(build.CSRC, unit), "-o", str(tmp_path / "banknet_train.o")])
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    want = {"banknet_level_tape_kernel": 3, "bank_tail_bwd_kernel": 1, "bank_level_bwd_kernel": 3, "bank_conv1_bwd_kernel": 1,
            "bank_reduce_kernel": 1, "banknet_pack_t_kernel": 1}
    for kernel, count in want.items():
        bad, seen = build._scratch_users(p.stdout, kernel)
        assert seen == count, f"{kernel}: {seen} resource-usage remarks, expected {count}"
        assert not bad, f"{kernel} uses scratch / spills VGPRs: {bad}"
        found = re.findall(r"Function Name: \S*" + kernel + r"\S*.*?VGPRs: (\d+).*?AGPRs: (\d+).*?LDS Size \[bytes/block\]: (\d+)", p.stdout, re.S)
        assert len(found) == count, "resource remark format"
        for vgprs, agprs, lds in found:
            print(f"\n{kernel}: {vgprs} VGPRs, {agprs} AGPRs, {lds} B LDS")
            regs = (int(vgprs) + 7) // 8 * 8 + (int(agprs) + 7) // 8 * 8
            assert int(lds) <= 64 * 1024
            groups = 160 * 1024 // int(lds) if int(lds) else 2
            assert groups >= 2
            assert regs * min(groups, 8) <= 512, "registers, not LDS, would limit the occupancy"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_use_of_a_shared_tensor_carries_gradient(shape):
    """Under the propagating weights and the GPU tests' loss, in float64: every level carries at least 0.2 of the max of each summed
    bank gradient and each application of conv2 at least 0.41 of conv2's, so a dropped level or application cannot hide under the GPU
    tests' bounds (8 x e32, some 1e-5); and between a quarter and 0.6 of every ReLU layer is active.  A use's share is
    max|g - g without that use| / max|g|, the gradient without a use taken with that use's weights detached: 0.21 (the quarter level
    of block.0's weight at 2x8x12) to 0.29 for the levels and 0.46 to 0.75 for conv2 at these shapes."""
    B, H, W = shape
    w = propagating_bank_weights(0)
    x = bank_input(B, H, W, boxes=H >= 16)
    wp = np.random.default_rng(7).standard_normal((B, 1, H, W)).astype(np.float32)
    full, _, masks = BG.gradients(w, x, wp)
    for level in range(3):
        rest, _, _ = BG.gradients(w, x, wp, drop_level=level)
        for name in BG.BANK_TENSORS:
            share = np.abs(full[name] - rest[name]).max() / np.abs(full[name]).max()
            print(f"{shape}: level {level} carries {share:.3f} of max|{name} gradient|")
            assert share >= 0.2, (shape, level, name, share)
    for app in range(2):
        rest, _, _ = BG.gradients(w, x, wp, drop_conv2=app)
        for name in ("conv2.weight", "conv2.bias"):
            share = np.abs(full[name] - rest[name]).max() / np.abs(full[name]).max()
            print(f"{shape}: application {app} carries {share:.3f} of max|{name} gradient|")
            assert share >= 0.41, (shape, app, name, share)
    if B * H * W >= 256:                     # (a 4 x 4 grid has a quarter level of one cell)
        for name, m in masks.items():
            print(f"{shape}: {name} active {m.mean():.2f}")
            assert 0.2 <= m.mean() <= 0.8, (shape, name, m.mean())


def test_module_names_round_trip_and_strict_loading():
    from fluidnet_cxx_amd import FluidNet, FluidNetBankTrain
    from fluidnet_cxx_amd.weights import make_banknet_weights, make_scalenet_weights
    net = FluidNetBankTrain(MCONF)
    assert isinstance(net, torch.nn.Module) and net.is_bank and not net.is3D
    assert [k for k, _ in net.named_parameters()] == BG.PARAM_NAMES == list(net.state_dict())
    fresh = make_banknet_weights(0)
    assert all(np.array_equal(net.state_dict()[k].numpy(), fresh[k]) for k in fresh)
    # both ways with FluidNet(bank mconf), keeping multiScale.* / scale.*
    ck = {k: torch.from_numpy(v) for k, v in propagating_bank_weights(3).items()}
    ck.update({k: torch.from_numpy(v) for k, v in make_scalenet_weights(1).items()})
    inf = FluidNet(MCONF)
    inf.load_state_dict(ck)
    net.load_state_dict(inf.state_dict())
    back = net.state_dict()
    assert set(back) == set(ck) and all(torch.equal(back[k], ck[k]) for k in ck)
    inf2 = FluidNet(MCONF)
    inf2.load_state_dict(back)
    assert all(torch.equal(inf2.state_dict()[k], ck[k]) for k in ck)
    # strict on the twelve tensors
    with pytest.raises(RuntimeError, match=r'Missing key\(s\) in state_dict: "conv3.bias"'):
        net.load_state_dict({k: v for k, v in ck.items() if k != "conv3.bias"})
    with pytest.raises(RuntimeError, match=r'Unexpected key\(s\) in state_dict: "deconv1.weight"'):
        net.load_state_dict(dict(ck, **{"deconv1.weight": torch.zeros(1)}))
    with pytest.raises(RuntimeError, match=r"size mismatch for conv2.weight"):
        net.load_state_dict(dict(ck, **{"conv2.weight": torch.zeros(16, 16, 3, 3)}))
    with pytest.raises(RuntimeError, match=r'Missing key\(s\)'):
        net.load_state_dict({k: torch.from_numpy(v) for k, v in make_scalenet_weights(0).items()})
    for what in (lambda: net.packed_for("cuda"), lambda: net.packed):
        with pytest.raises(RuntimeError, match="bank model"):
            what()


def test_kaiming_init_is_seeded_and_touches_the_six_weights():
    from fluidnet_cxx_amd import FluidNetBankTrain
    from fluidnet_cxx_amd.training import kaiming_init
    fresh = FluidNetBankTrain(MCONF).state_dict()
    a, b, c = (kaiming_init(FluidNetBankTrain(MCONF), s).state_dict() for s in (5, 5, 6))
    for k in fresh:
        assert torch.equal(a[k], b[k]), k
        if k.endswith(".weight"):
            assert not torch.equal(a[k], fresh[k]) and not torch.equal(a[k], c[k]), k
        else:
            assert torch.equal(a[k], fresh[k]), k
    assert sum(k.endswith(".weight") for k in fresh) == 6


def test_out_of_scope_constructions_raise():
    from fluidnet_cxx_amd import FluidNet, FluidNetBankTrain, FluidNetTrain
    with pytest.raises(ValueError, match="2D only"):
        FluidNetBankTrain(dict(MCONF, is3D=True))
    with pytest.raises(ValueError, match="dropout"):
        FluidNetBankTrain(MCONF, dropout=True)
    with pytest.raises(ValueError, match="inputChannels"):
        FluidNetBankTrain(dict(MCONF, inputChannels=dict(div=True, pDiv=True, UDiv=False)))
    with pytest.raises(ValueError, match="fp32 arithmetic only"):
        FluidNetBankTrain(dict(MCONF, precisionMode="bf16x6"))
    with pytest.raises(ValueError, match="must be 'FluidNet'"):
        FluidNetBankTrain(dict(MCONF, model="ScaleNet"))
    # what the existing tests pin stays
    with pytest.raises(ValueError, match="only the ScaleNet variant is accelerated"):
        FluidNetTrain(MCONF)
    with pytest.raises(AssertionError, match="inference-only"):
        FluidNet(MCONF).train()
    net = FluidNetBankTrain(MCONF).train()
    with pytest.raises(RuntimeError, match="requires_grad"):
        net(torch.zeros(1, 5, 1, 8, 8, requires_grad=True))
    with pytest.raises(RuntimeError, match="requires_grad"):
        net.bank(torch.zeros(1, 2, 8, 8, requires_grad=True))


def test_train_picks_the_bank_net_and_train3d_refuses_it():
    """train() with a bank mconf on device='cpu' gets past the construction of the net and fails where the ScaleNet run fails there"""
    from fluidnet_cxx_amd import training, training3d
    tconf = dict(res=16, batch=1, iters=1, seed=1, sceneLength=4, stride=1, evalEvery=0, evalBatches=0, saveEvery=0)
    assert training._DIM_BANK.net.__name__ == "FluidNetBankTrain" and training._DIM.net.__name__ == "FluidNetTrain"
    seen = []
    for model in ("ScaleNet", "FluidNet"):
        with pytest.raises(Exception) as err:
            training.train(dict(model=model), tconf, device="cpu")
        assert not isinstance(err.value, ValueError) or "variant" not in str(err.value), err.value
        seen.append((type(err.value), str(err.value)))
    assert seen[0] == seen[1], seen
    with pytest.raises(ValueError, match="only the ScaleNet variant is accelerated"):
        training3d.train3d(dict(model="FluidNet", is3D=True), dict(tconf, D=16), device="cpu")
