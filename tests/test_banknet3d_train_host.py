"""Training of the Conv3d bank net without a GPU: the ABI's version and symbols, the tape layout, the refusals the new entry points make
before any launch, the backward's launch plan, the new unit's resources, the conditions under which the GPU tests' bounds mean something
(every level and both applications of conv2 carry a share of the shared tensors' gradients), and the host behaviour of
FluidNetBankTrain3D and train_bank3d()."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import banknet3d_grad_reference as BG
from banknet3d_reference import SHAPES3D, bank3d_input, propagating_bank3d_weights
from fluidnet_cxx_amd import build
from util import FnxGrid

MCONF = dict(model="FluidNet3D", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True, normalizeInputChan="UDiv",
             normalizeInputThreshold=1e-5, inputDim=3, is3D=True)
EINVAL = 1
NEW_SYMBOLS = ["fnx_banknet3d_tape_entries", "fnx_banknet3d_tape_layout", "fnx_banknet3d_packed_t_bytes", "fnx_banknet3d_pack_t",
               "fnx_banknet3d_backward_ws_bytes", "fnx_banknet3d_backward_plan", "fnx_banknet3d_forward_train", "fnx_banknet3d_backward",
               "fnx_fluidnet_bank3d_train_ws_bytes", "fnx_fluidnet_bank3d_forward_train", "fnx_fluidnet_bank3d_backward"]


class TapeEntry3D(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 8), ("offset", ctypes.c_size_t), ("C", ctypes.c_int), ("D", ctypes.c_int), ("H", ctypes.c_int),
                ("W", ctypes.c_int)]


class BwdLaunch(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 16), ("level", ctypes.c_int), ("items", ctypes.c_longlong), ("workgroups", ctypes.c_int),
                ("cap", ctypes.c_int), ("partial_floats", ctypes.c_int), ("partial_offset", ctypes.c_size_t), ("dims", ctypes.c_int * 4)]


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(build.LIB)
    lib.fnx_last_error.restype = ctypes.c_char_p
    for fn in ("fnx_banknet3d_tape_layout", "fnx_banknet3d_packed_t_bytes", "fnx_banknet3d_backward_ws_bytes",
               "fnx_fluidnet_bank3d_train_ws_bytes"):
        getattr(lib, fn).restype = ctypes.c_size_t
    return lib


def _header():
    return open(os.path.join(os.path.dirname(build.HERE), "include", "fluidnet_hip.h")).read()


def _id(s):
    return "x".join(map(str, s))


def test_abi_version_and_symbols(lib):
    hdr = _header()
    version = int(re.search(r"#define FNX_ABI_VERSION (\d+)", hdr).group(1))
    assert version >= 34 and lib.fnx_abi_version() == version
    assert len(NEW_SYMBOLS) == 11
    for fn in NEW_SYMBOLS:
        assert hasattr(lib, fn) and re.search(r"\b" + fn + r"\(", hdr), fn
    assert "HSA_XNACK" not in hdr


@pytest.mark.parametrize("shape", [(3, 8, 36, 68), (1, 4, 4, 4)], ids=_id)
def test_tape_layout(lib, shape):
    B, D, H, W = shape
    g = FnxGrid(B=B, D=D, H=H, W=W, is3D=1)
    n = lib.fnx_banknet3d_tape_entries()
    assert n == 14
    e = (TapeEntry3D * n)()
    total = lib.fnx_banknet3d_tape_layout(ctypes.byref(g), e)
    assert total == lib.fnx_banknet3d_tape_layout(ctypes.byref(g), None)
    got = [(t.name.decode(), t.C, t.D, t.H, t.W) for t in e]
    full, half, quarter = (D, H, W), (D // 2, H // 2, W // 2), (D // 4, H // 4, W // 4)
    want = [("a", 16) + full, ("h1", 16) + full, ("b1", 16) + full, ("a2", 16) + half, ("h2", 16) + half, ("b2", 16) + half,
            ("a4", 16) + quarter, ("h4", 16) + quarter, ("b4", 16) + quarter, ("t", 16) + full, ("c2a", 16) + full, ("c2b", 16) + full,
            ("c3", 8) + full, ("x", 2) + full]
    assert got == want and [t[0] for t in want] == BG.TAPE_NAMES
    end = 0
    for t in e:
        assert t.offset >= end and t.offset % 64 == 0, t.name       # no overlap, in order
        end = t.offset + B * t.C * t.D * t.H * t.W
    assert end <= total < end + 64
    # 16 x 6 + 8 + 2 = 106 floats a full-resolution voxel, 48 a half- and 48 a quarter-resolution one: 112.75 a full-resolution voxel
    assert sum(B * t.C * t.D * t.H * t.W for t in e) * 4 == 451 * B * D * H * W
    # a function of (B, D, H, W) alone; grids without a layout
    e2 = (TapeEntry3D * n)()
    assert lib.fnx_banknet3d_tape_layout(ctypes.byref(FnxGrid(B=B, D=D, H=H, W=W, is3D=1)), e2) == total
    assert [(t.name, t.offset) for t in e2] == [(t.name, t.offset) for t in e]
    for bad in (FnxGrid(B=1, D=8, H=18, W=24, is3D=1), FnxGrid(B=1, D=6, H=16, W=24, is3D=1), FnxGrid(B=1, D=1, H=16, W=24),
                FnxGrid(B=0, D=8, H=16, W=24, is3D=1)):
        assert lib.fnx_banknet3d_tape_layout(ctypes.byref(bad), None) == 0


def test_refusals_before_any_launch(lib):
    """null arguments, 2D, the bf16 modes, an unknown mode, D, H or W no multiple of 4 and a short workspace, on dummy host pointers:
    nothing reaches the device"""
    hdr = _header()
    modes = {k: int(v) for k, v in re.findall(r"(FNX_PRECISION_\w+) = (\d+)", hdr)}
    EWORKSPACE = [int(v) for v in re.findall(r"FNX_EWORKSPACE = (\d+)", hdr)][0]
    a = ctypes.c_void_p(64)                # never dereferenced
    f = ctypes.c_float(1e-5)
    size = ctypes.c_size_t

    def fwd(g, mode=0, x=a, ws_bytes=0):
        return lib.fnx_banknet3d_forward_train(ctypes.byref(g), a, x, a, a, mode, None)

    def bwd(g, mode=0, x=a, ws_bytes=1 << 40):
        return lib.fnx_banknet3d_backward(ctypes.byref(g), a, x, a, a, a, mode, a, size(ws_bytes), None)

    def ffwd(g, mode=0, x=a, ws_bytes=1 << 40):
        return lib.fnx_fluidnet_bank3d_forward_train(ctypes.byref(g), a, x, f, a, a, a, a, a, mode, a, size(ws_bytes), None)

    def fbwd(g, mode=0, x=a, ws_bytes=1 << 40):
        return lib.fnx_fluidnet_bank3d_backward(ctypes.byref(g), a, x, a, a, a, a, a, mode, a, size(ws_bytes), None)

    ok = dict(B=1, D=8, H=16, W=24, is3D=1)
    sizes = {bwd: lib.fnx_banknet3d_backward_ws_bytes, ffwd: lib.fnx_fluidnet_bank3d_train_ws_bytes,
             fbwd: lib.fnx_fluidnet_bank3d_train_ws_bytes}
    for call, fn in ((fwd, "fnx_banknet3d_forward_train"), (bwd, "fnx_banknet3d_backward"), (ffwd, "fnx_fluidnet_bank3d_forward_train"),
                     (fbwd, "fnx_fluidnet_bank3d_backward")):
        def msg_of(rc):
            return rc, lib.fnx_last_error().decode()
        assert msg_of(call(FnxGrid(**ok), x=None)) == (EINVAL, f"{fn}: null argument")
        for flat in (FnxGrid(B=1, D=1, H=16, W=24), FnxGrid(B=1, D=8, H=16, W=24, is3D=0)):
            rc, msg = msg_of(call(flat))
            assert rc == EINVAL and "3D only" in msg and msg.startswith(fn), msg
        for m in ("FNX_PRECISION_BF16X6", "FNX_PRECISION_BF16X3"):
            rc, msg = msg_of(call(FnxGrid(**ok), mode=modes[m]))
            assert rc == EINVAL and "fp32 arithmetic only" in msg and "bf16" in msg, msg
        rc, msg = msg_of(call(FnxGrid(**ok), mode=99))
        assert rc == EINVAL and "unknown precision_mode 99" in msg and msg.startswith(fn), msg
        for axis, grid in (("D = 6", dict(ok, D=6)), ("H = 18", dict(ok, H=18)), ("W = 26", dict(ok, W=26))):
            rc, msg = msg_of(call(FnxGrid(**grid)))
            assert rc == EINVAL and f"{axis} must be a positive multiple of 4" in msg, msg
        if call in sizes:
            need = sizes[call](ctypes.byref(FnxGrid(**ok)))
            assert need > 0
            rc, msg = msg_of(call(FnxGrid(**ok), ws_bytes=need - 1))
            assert rc == EWORKSPACE and f"workspace of {need - 1} bytes is too small" in msg, msg
            for m in ("FNX_PRECISION_FP32", "FNX_PRECISION_FP32_DIRECT", "FNX_PRECISION_FP32_F4", "FNX_PRECISION_FP32_F2"):
                assert call(FnxGrid(**ok), mode=modes[m], ws_bytes=0) == EWORKSPACE
    assert lib.fnx_banknet3d_pack_t(None, a, None) == EINVAL and lib.fnx_last_error().decode() == "fnx_banknet3d_pack_t: null argument"
    # grids without a size
    for bad in (FnxGrid(B=1, D=1, H=16, W=24), FnxGrid(B=0, D=8, H=16, W=24, is3D=1), FnxGrid(B=1, D=8, H=2, W=24, is3D=1)):
        assert lib.fnx_banknet3d_backward_ws_bytes(ctypes.byref(bad)) == 0
        assert lib.fnx_fluidnet_bank3d_train_ws_bytes(ctypes.byref(bad)) == 0
        assert lib.fnx_banknet3d_tape_layout(ctypes.byref(bad), None) == 0
    # one workspace size serves the FluidNet-level forward and backward, and it grows with the grid
    g1, g2 = FnxGrid(**ok), FnxGrid(B=2, D=8, H=32, W=24, is3D=1)
    assert lib.fnx_fluidnet_bank3d_train_ws_bytes(ctypes.byref(g2)) > lib.fnx_fluidnet_bank3d_train_ws_bytes(ctypes.byref(g1)) > \
        lib.fnx_banknet3d_backward_ws_bytes(ctypes.byref(g1))
    # the sizes themselves at two grids, as recorded before the four nets' training wrappers became one body
    for shape, train_ws in (((2, 8, 12, 20), 2088448), ((1, 4, 4, 4), 186112)):
        assert lib.fnx_fluidnet_bank3d_train_ws_bytes(ctypes.byref(FnxGrid(*shape, is3D=1))) == train_ws, shape
    assert lib.fnx_banknet3d_backward_ws_bytes(ctypes.byref(FnxGrid(2, 8, 12, 20, is3D=1))) == 1965568


PLAN_GRIDS = [(1, 4, 4, 4), (2, 8, 12, 20), (1, 12, 20, 36), (2, 4, 36, 68), (1, 20, 12, 132), (2, 32, 64, 64), (3, 16, 40, 72),
              (1, 64, 64, 64), (5, 8, 8, 260), (1, 128, 128, 128), (2, 128, 64, 256), (1, 4, 256, 256), (1, 256, 256, 256)]


@pytest.mark.parametrize("shape", PLAN_GRIDS, ids=_id)
def test_backward_plan_covers_every_item_once(lib, shape):
    """fnx_banknet3d_backward_plan: every item of every launch with partial sums is owned by exactly one workgroup (item i by workgroup
    i mod n), no launch has more workgroups than its cap, the items of a launch cover the cells of its level exactly once, and the
    partial buffers lie inside the reported workspace without overlapping each other or the gradient tensors in front of them"""
    B, D, H, W = shape
    g = FnxGrid(B=B, D=D, H=H, W=W, is3D=1)
    n = lib.fnx_banknet3d_backward_launches()
    assert n == 8
    L = (BwdLaunch * n)()
    assert lib.fnx_banknet3d_backward_plan(ctypes.byref(g), L) == 0
    L2 = (BwdLaunch * n)()
    assert lib.fnx_banknet3d_backward_plan(ctypes.byref(FnxGrid(B=B, D=D, H=H, W=W, is3D=1)), L2) == 0
    assert bytes(L) == bytes(L2), "a function of (B, D, H, W) alone"
    ws = lib.fnx_banknet3d_backward_ws_bytes(ctypes.byref(g))
    assert [(t.name.decode(), t.level) for t in L] == [("tail", 1), ("wgrad.2", 4), ("wgrad.0", 4), ("wgrad.2", 2), ("wgrad.0", 2),
                                                       ("wgrad.2", 1), ("wgrad.0", 1), ("conv1", 1)]
    # the gradient tensors of the three levels lie in front of the partial sums: 2 x 16 channels x 4 bytes a cell of each level
    cells = D * H * W
    spans = [(0, 2 * 16 * 4 * B * (cells + cells // 8 + cells // 64))]
    for t in L:
        assert t.items >= 1 and t.workgroups == min(t.items, t.cap) and t.workgroups <= t.cap <= 512, t.name
        owners = np.arange(t.items) % t.workgroups             # item i on workgroup i mod n
        assert np.array_equal(np.unique(owners), np.arange(t.workgroups)), "no idle workgroup writes an unset partial"
        if t.name.startswith(b"wgrad"):
            d, h, w = D // t.level, H // t.level, W // t.level
            tx, ty, chunks, chunk = t.dims
            assert t.items == B * tx * ty * chunks
            # tiles of 4 x 36 cells and chunks of `chunk` planes cover the level once: the last tile and chunk start inside it
            assert (tx - 1) * 36 < w <= tx * 36 and (ty - 1) * 4 < h <= ty * 4 and (chunks - 1) * chunk < d <= chunks * chunk
            assert t.partial_floats == 27 * 256 + 16
        else:
            ups, unit = t.dims[0], t.dims[1]
            assert unit == 64 and (ups - 1) * 64 < cells <= ups * 64 and t.items == B * ups
            assert t.partial_floats == (816 if t.name == b"tail" else 880)
        spans.append((t.partial_offset, t.partial_offset + 4 * t.workgroups * t.partial_floats))
    spans.sort()
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 <= b0, (spans,)
    assert spans[-1][1] <= ws
    if shape == (2, 32, 64, 64):              # what tests/test_banknet3d_train_gpu.py says of this shape
        assert all(t.items > t.workgroups for t in L if t.level == 1)


def test_backward_plan_refusals(lib):
    L = (BwdLaunch * 8)()
    for bad in (FnxGrid(B=1, D=1, H=16, W=24), FnxGrid(B=1, D=6, H=16, W=24, is3D=1), FnxGrid(B=0, D=8, H=16, W=24, is3D=1)):
        assert lib.fnx_banknet3d_backward_plan(ctypes.byref(bad), L) == EINVAL
    assert lib.fnx_banknet3d_backward_plan(ctypes.byref(FnxGrid(B=1, D=8, H=16, W=24, is3D=1)), None) == EINVAL


def test_train3d_kernels_resources(tmp_path):
    """The new unit compiles for gfx950 without scratch or VGPR spills (build_lib refuses such a build too) and within a static 64 KiB of
    LDS.  A kernel of this unit's own stays within the registers of as many workgroups (of one wave per SIMD) as its LDS admits per CU
    -- the rule of test_train_kernels_resources -- and at least two.  The three instantiations of the forward's convolution body
    (fnx_banknet3d_tile.h: the taping tail, the two input-gradient epilogues) are held to the budget that
    test_bank3d_kernels_use_no_scratch pins for that body: its 53 248 bytes of LDS would admit three workgroups, its 108 weight operands
    a lane admit two, which is the occupancy the body is built for (two waves a SIMD); so both LDS and registers must admit two."""
    unit = "fnx_banknet3d_train.hip"
    kernels, _ = build.SCRATCH_FREE[unit]
    assert set(kernels) == {"bank3d_tail_tape_kernel", "bank3d_conv_bwd_kernel", "bank3d_wgrad_kernel", "bank3d_conv1_bwd_kernel"}
    assert "-Rpass-analysis=kernel-resource-usage" in build.HIP_UNITS[unit]
    cmd = ([build.HIPCC] + build.COMMON + build.HIP_UNITS[unit] +
           ["--cuda-device-only", "-c", os.path.join(build.CSRC, unit), "-o", str(tmp_path / "banknet3d_train.o")])
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    want = {"bank3d_tail_tape_kernel": 1, "bank3d_pool_bwd_kernel": 1, "bank3d_conv_bwd_kernel": 2, "bank3d_wgrad_kernel": 1,
            "bank3d_conv1_bwd_kernel": 1, "bank3d_reduce_kernel": 1, "bank3d_pack_t_kernel": 1}
    body = {"bank3d_tail_tape_kernel", "bank3d_conv_bwd_kernel"}
    for kernel, count in want.items():
        bad, seen = build._scratch_users(p.stdout, kernel)
        assert seen == count, f"{kernel}: {seen} resource-usage remarks, expected {count}"
        assert not bad, f"{kernel} uses scratch / spills VGPRs: {bad}"
        found = re.findall(r"Function Name: \S*" + kernel + r"\S*.*?VGPRs: (\d+).*?AGPRs: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?"
                           r"LDS Size \[bytes/block\]: (\d+)", p.stdout, re.S)
        assert len(found) == count, "resource remark format"
        for vgprs, agprs, waves, lds in found:
            print(f"\n{kernel}: {vgprs} VGPRs, {agprs} AGPRs, {waves} waves a SIMD, {lds} B LDS")
            assert int(lds) <= 64 * 1024
            groups = 160 * 1024 // int(lds) if int(lds) else 2
            assert groups >= 2 and int(waves) >= 2
            if kernel in body:
                assert int(lds) == 53248 and (((int(vgprs) + 3) // 4 * 4 + int(agprs)) + 7) // 8 * 8 * 2 <= 512, "fewer than two waves a SIMD"
            else:
                regs = (int(vgprs) + 7) // 8 * 8 + (int(agprs) + 7) // 8 * 8
                assert regs * min(groups, 8) <= 512, "registers, not LDS, would limit the occupancy"


@pytest.mark.parametrize("shape", SHAPES3D, ids=_id)
def test_every_use_of_a_shared_tensor_carries_gradient(shape):
    """Under the propagating weights and the GPU tests' loss, in float64: every level carries at least 0.1 of the max of each summed bank
    gradient and each application of conv2 at least 0.4 of conv2's, so a dropped level or application cannot hide under the GPU tests'
    bounds (8 x e32, some 1e-5); and between 0.2 and 0.8 of every ReLU layer is active.  A use's share is
    max|g - g without that use| / max|g|, the gradient without a use taken with that use's weights detached."""
    w = propagating_bank3d_weights(0)
    x = bank3d_input(*shape)
    wp = np.random.default_rng(7).standard_normal((shape[0], 1) + shape[1:]).astype(np.float32)
    full, _, masks = BG.gradients(w, x, wp)
    for level in range(3):
        rest, _, _ = BG.gradients(w, x, wp, drop_level=level)
        for name in BG.BANK_TENSORS:
            share = np.abs(full[name] - rest[name]).max() / np.abs(full[name]).max()
            print(f"{shape}: level {level} carries {share:.3f} of max|{name} gradient|")
            assert share >= 0.1, (shape, level, name, share)
    for app in range(2):
        rest, _, _ = BG.gradients(w, x, wp, drop_conv2=app)
        for name in ("conv2.weight", "conv2.bias"):
            share = np.abs(full[name] - rest[name]).max() / np.abs(full[name]).max()
            print(f"{shape}: application {app} carries {share:.3f} of max|{name} gradient|")
            assert share >= 0.4, (shape, app, name, share)
    for name, m in masks.items():
        print(f"{shape}: {name} active {m.mean():.2f}")
        assert 0.2 <= m.mean() <= 0.8, (shape, name, m.mean())


def test_module_names_round_trip_and_strict_loading():
    from fluidnet_cxx_amd import FluidNet, FluidNetBankTrain3D
    from fluidnet_cxx_amd.weights import make_banknet_weights, make_scalenet_weights
    net = FluidNetBankTrain3D(MCONF)
    assert isinstance(net, torch.nn.Module) and net.is_bank and net.is3D
    assert [k for k, _ in net.named_parameters()] == BG.PARAM_NAMES == list(net.state_dict())
    fresh = make_banknet_weights(0, ndim=3)
    assert all(net.state_dict()[k].dim() == (5 if k.endswith(".weight") else 1) for k in fresh)
    assert all(np.array_equal(net.state_dict()[k].numpy(), fresh[k]) for k in fresh)
    # both ways with FluidNet(bank mconf), keeping multiScale.* / scale.*
    ck = {k: torch.from_numpy(v) for k, v in propagating_bank3d_weights(3).items()}
    ck.update({k: torch.from_numpy(v) for k, v in make_scalenet_weights(1, ndim=3).items()})
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
        net.load_state_dict(dict(ck, **{"conv2.weight": torch.zeros(16, 16, 3, 3, 3)}))
    with pytest.raises(RuntimeError, match=r"size mismatch for conv1.weight"):            # a 2D bank checkpoint
        net.load_state_dict({k: torch.from_numpy(v) for k, v in make_banknet_weights(0).items()})
    with pytest.raises(RuntimeError, match=r'Missing key\(s\)'):
        net.load_state_dict({k: torch.from_numpy(v) for k, v in make_scalenet_weights(0, ndim=3).items()})
    for what in (lambda: net.packed_for("cuda"), lambda: net.packed):
        with pytest.raises(RuntimeError, match="bank model"):
            what()


def test_kaiming_init_is_seeded_and_touches_the_six_weights():
    from fluidnet_cxx_amd import FluidNetBankTrain3D
    from fluidnet_cxx_amd.training import kaiming_init
    fresh = FluidNetBankTrain3D(MCONF).state_dict()
    a, b, c = (kaiming_init(FluidNetBankTrain3D(MCONF), s).state_dict() for s in (5, 5, 6))
    for k in fresh:
        assert torch.equal(a[k], b[k]), k
        if k.endswith(".weight"):
            assert not torch.equal(a[k], fresh[k]) and not torch.equal(a[k], c[k]), k
        else:
            assert torch.equal(a[k], fresh[k]), k
    assert sum(k.endswith(".weight") for k in fresh) == 6


def test_out_of_scope_constructions_raise():
    from fluidnet_cxx_amd import FluidNet, FluidNetBankTrain, FluidNetBankTrain3D, FluidNetTrain3D
    with pytest.raises(ValueError, match="3D only"):
        FluidNetBankTrain3D(dict(MCONF, is3D=False))
    with pytest.raises(ValueError, match="dropout"):
        FluidNetBankTrain3D(MCONF, dropout=True)
    with pytest.raises(ValueError, match="inputChannels"):
        FluidNetBankTrain3D(dict(MCONF, inputChannels=dict(div=True, pDiv=True, UDiv=False)))
    with pytest.raises(ValueError, match="fp32 arithmetic only"):
        FluidNetBankTrain3D(dict(MCONF, precisionMode="bf16x6"))
    with pytest.raises(ValueError, match="must be 'FluidNet3D'"):
        FluidNetBankTrain3D(dict(MCONF, model="FluidNet"))
    with pytest.raises(ValueError, match="must be 'FluidNet3D'"):
        FluidNetBankTrain3D(dict(MCONF, model="ScaleNet"))
    # the classes that do not train this model keep saying so, and now point to the one that does
    for cls in (FluidNetTrain3D, FluidNetBankTrain):
        with pytest.raises(ValueError, match="training the 'FluidNet3D' model is not built.*FluidNetBankTrain3D"):
            cls(MCONF)
    with pytest.raises(AssertionError, match="inference-only"):
        FluidNet(MCONF).train()
    net = FluidNetBankTrain3D(MCONF).train()
    with pytest.raises(RuntimeError, match="requires_grad"):
        net(torch.zeros(1, 6, 8, 8, 8, requires_grad=True))
    with pytest.raises(RuntimeError, match="requires_grad"):
        net.bank(torch.zeros(1, 2, 8, 8, 8, requires_grad=True))


def test_train_bank3d_picks_the_bank_net():
    """train_bank3d() on device='cpu' gets past the construction of the net and fails where train3d with the ScaleNet fails there;
    train3d keeps refusing the model and names train_bank3d"""
    from fluidnet_cxx_amd import training3d
    tconf = dict(res=16, batch=1, iters=1, seed=1, sceneLength=4, stride=1, evalEvery=0, evalBatches=0, saveEvery=0)
    assert training3d._DIM3_BANK.net.__name__ == "FluidNetBankTrain3D" and training3d._DIM3.net.__name__ == "FluidNetTrain3D"
    seen = []
    for run, mconf in ((training3d.train3d, dict(model="ScaleNet")), (training3d.train_bank3d, None),
                       (training3d.train_bank3d, dict(model="FluidNet3D"))):
        with pytest.raises(Exception) as err:
            run(mconf, tconf, device="cpu")
        assert not isinstance(err.value, ValueError), err.value
        seen.append((type(err.value), str(err.value)))
    assert seen[0] == seen[1] == seen[2], seen
    with pytest.raises(ValueError, match="training the 'FluidNet3D' model is not built.*train_bank3d"):
        training3d.train3d(dict(model="FluidNet3D"), tconf, device="cpu")
    with pytest.raises(ValueError, match="must be 'FluidNet3D'"):
        training3d.train_bank3d(dict(model="ScaleNet"), tconf, device="cpu")
    with pytest.raises(ValueError, match="3D only"):
        training3d.train_bank3d(dict(is3D=False), tconf, device="cpu")
