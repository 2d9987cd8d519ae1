"""Host-side surface of 3D CNN training (no GPU): the new C ABI symbols and their version, the tape layout against a numpy statement
of it, every refusal of the C ABI on host pointers with its own text, and FluidNetTrain3D's construction, checkpoint exchange with
FluidNet and out-of-scope configurations."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from fluidnet_cxx_amd import build
from fluidnet_cxx_amd.weights import make_scalenet_weights, scalenet_layers
from util import TRAIN_BANNED, FnxGrid as _FnxGrid

MCONF = dict(model="ScaleNet", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True,
             normalizeInputChan="UDiv", normalizeInputThreshold=1e-5, is3D=True, inputDim=3)
SHAPES = [(2, 6, 10, 37), (1, 9, 14, 70), (1, 4, 4, 4)]
NAMES = ["xq", "y0", "y1", "y2", "y3", "in2", "y4", "y5", "y6", "y7", "y8", "y9", "in1"] + [f"y{l}" for l in range(10, 16)]
SYMBOLS = ["fnx_multiscale3d_tape_layout", "fnx_scalenet3d_packed_t_bytes", "fnx_scalenet3d_pack_t", "fnx_multiscale3d_backward_ws_bytes",
           "fnx_multiscale3d_forward_train", "fnx_multiscale3d_backward", "fnx_multiscale3d_backward_plain",
           "fnx_fluidnet3d_train_ws_bytes", "fnx_fluidnet3d_forward_train", "fnx_fluidnet3d_backward"]


@pytest.fixture(scope="module")
def built():
    build.build_all()
    return build


class _Entry(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 8), ("offset", ctypes.c_size_t)] + [(n, ctypes.c_int) for n in ("C", "D", "H", "W")]


@pytest.fixture(scope="module")
def lib(built):
    lib = ctypes.CDLL(built.LIB)
    lib.fnx_last_error.restype = ctypes.c_char_p
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    G = ctypes.POINTER(_FnxGrid)
    for f in ("fnx_multiscale3d_tape_layout", "fnx_scalenet3d_packed_t_bytes", "fnx_multiscale3d_backward_ws_bytes",
              "fnx_fluidnet3d_train_ws_bytes", "fnx_scalenet_packed_bytes"):
        getattr(lib, f).restype = sz
    lib.fnx_multiscale3d_tape_layout.argtypes = [G, ctypes.POINTER(_Entry)]
    lib.fnx_multiscale3d_backward_ws_bytes.argtypes = [G]
    lib.fnx_fluidnet3d_train_ws_bytes.argtypes = [G]
    lib.fnx_scalenet3d_pack_t.argtypes = [vp, vp, vp]
    lib.fnx_multiscale3d_forward_train.argtypes = [G, vp, sz, vp, vp, vp, ci, vp]
    lib.fnx_multiscale3d_backward.argtypes = [G, vp, sz, vp, vp, vp, ci, vp, sz, vp]
    lib.fnx_multiscale3d_backward_plain.argtypes = [G, vp, sz, vp, vp, vp, ci, vp, sz, vp]
    lib.fnx_fluidnet3d_forward_train.argtypes = [G, vp, sz, vp, ctypes.c_float, vp, vp, vp, vp, vp, ci, vp, sz, vp]
    lib.fnx_fluidnet3d_backward.argtypes = [G, vp, sz, vp, vp, vp, vp, vp, vp, ci, vp, sz, vp]
    return lib


def _header():
    return open(os.path.join(os.path.dirname(build.HERE), "include", "fluidnet_hip.h")).read()


def test_symbols_and_abi_version(lib):
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert re.search(r"\b" + s + r"\(", _header()), f"{s} is not declared in the header"
    ver = int(re.search(r"#define FNX_ABI_VERSION (\d+)", _header()).group(1))
    assert ver >= 25 and lib.fnx_abi_version() == ver
    from fluidnet_cxx_amd._ext import ext
    for f in ("multiscale3d_tape_layout", "scalenet3d_pack_t", "multiscale3d_forward_train", "multiscale3d_backward",
              "multiscale3d_backward_plain", "fluidnet3d_forward_train", "fluidnet3d_backward"):
        assert callable(getattr(ext, f)), f


def _numpy_layout(B, D, H, W):
    """xq, y0..y3 at int(n * 0.25); in2, y4..y9 at int(n * 0.5); in1, y10..y15 at full size; every entry a contiguous (B,C,D,H,W) on a
    64-float boundary; 1024 floats of slack behind the last"""
    L = scalenet_layers(2, 3)
    q = [int(n * 0.25) for n in (D, H, W)]
    h = [int(n * 0.5) for n in (D, H, W)]
    chans = [(2, q)] + [(L[l]["cout"], q) for l in range(4)] + [(3, h)] + [(L[l]["cout"], h) for l in range(4, 10)] + \
            [(3, [D, H, W])] + [(L[l]["cout"], [D, H, W]) for l in range(10, 16)]
    out, off = [], 0
    for name, (C, d) in zip(NAMES, chans):
        out.append((name, off, C, d[0], d[1], d[2]))
        off = (off + B * C * int(np.prod(d)) + 63) // 64 * 64
    return out, off + 1024


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tape_layout_is_the_numpy_statement(lib, shape):
    B, D, H, W = shape
    e = (_Entry * 19)()
    floats = lib.fnx_multiscale3d_tape_layout(ctypes.byref(_FnxGrid(B=B, D=D, H=H, W=W, is3D=1)), e)
    got = [(t.name.decode(), t.offset, t.C, t.D, t.H, t.W) for t in e]
    want, total = _numpy_layout(B, D, H, W)
    assert got == want and floats == total
    from fluidnet_cxx_amd._ext import ext
    assert [tuple(t) for t in ext.multiscale3d_tape_layout(B, D, H, W)] == want
    # a function of the grid alone
    assert lib.fnx_multiscale3d_tape_layout(ctypes.byref(_FnxGrid(B=B, D=D, H=H, W=W, is3D=1)), None) == total
    if shape == (2, 6, 10, 37):
        assert [tuple(t[3:]) for t in got if t[0] in ("xq", "in2")] == [(1, 2, 9), (3, 5, 18)]
    assert sum(t[2] for t in got if (t[3], t[4], t[5]) == (D, H, W)) == 331            # floats per full-resolution voxel


def test_entry_points_check_before_the_device(lib):
    """every refusal with its own message, before anything reads a pointer (host memory here)"""
    hdr = _header()
    einval = int(re.search(r"FNX_EINVAL = (\d+)", hdr).group(1))
    ework = int(re.search(r"FNX_EWORKSPACE = (\d+)", hdr).group(1))
    modes = dict(re.findall(r"(FNX_PRECISION_\w+) = (\d+)", hdr))
    buf = ctypes.create_string_buffer(64)
    a = ctypes.cast(buf, ctypes.c_void_p)
    fwd, bwd = lib.fnx_scalenet_packed_bytes(1), lib.fnx_scalenet3d_packed_t_bytes()
    assert fwd != bwd and fwd > 0 and bwd > 0

    def calls(g, mode, a=a, fwd=fwd, bwd=bwd):
        r = ctypes.byref(g)
        return {"fnx_multiscale3d_forward_train": lambda: lib.fnx_multiscale3d_forward_train(r, a, fwd, a, a, a, mode, None),
                "fnx_multiscale3d_backward": lambda: lib.fnx_multiscale3d_backward(r, a, bwd, a, a, a, mode, a, 0, None),
                "fnx_multiscale3d_backward_plain": lambda: lib.fnx_multiscale3d_backward_plain(r, a, bwd, a, a, a, mode, a, 0, None),
                "fnx_fluidnet3d_forward_train": lambda: lib.fnx_fluidnet3d_forward_train(r, a, fwd, a, 1e-3, a, a, a, a, a, mode, a, 0, None),
                "fnx_fluidnet3d_backward": lambda: lib.fnx_fluidnet3d_backward(r, a, bwd, a, a, a, a, a, a, mode, a, 0, None)}

    def refused(g, mode, text, code=einval, **kw):
        for name, call in calls(g, mode, **kw).items():
            assert call() == code, (name, text)
            assert text in lib.fnx_last_error().decode(), (name, text, lib.fnx_last_error().decode())

    ok = dict(B=1, D=8, H=16, W=16, is3D=1)
    refused(_FnxGrid(**ok), 0, "null argument", a=None)
    refused(_FnxGrid(B=1, D=1, H=16, W=16), 0, "3D only")                          # a 2D grid
    refused(_FnxGrid(B=1, D=8, H=16, W=16, is3D=0), 0, "3D only")
    refused(_FnxGrid(B=1, D=3, H=16, W=16, is3D=1), 0, "3D only")                  # too few planes for the three scales
    refused(_FnxGrid(B=1, D=8, H=3, W=16, is3D=1), 0, "at least 4 cells per axis")
    refused(_FnxGrid(B=1, D=8, H=16, W=2, is3D=1), 0, "at least 4 cells per axis")
    for m in ("FNX_PRECISION_BF16X6", "FNX_PRECISION_BF16X3"):
        refused(_FnxGrid(**ok), int(modes[m]), "fp32 arithmetic only")
    refused(_FnxGrid(**ok), 99, "precision_mode 99")
    refused(_FnxGrid(k_begin=2, k_end=6, **ok), 0, "compute window")
    refused(_FnxGrid(z_offset=8, D_global=32, **ok), 0, "z-slab view")
    refused(_FnxGrid(B=1, D=512, H=512, W=512, is3D=1), 0, "beyond the training kernels' ranges")
    refused(_FnxGrid(B=4096, D=32, H=16, W=16, is3D=1), 0, "beyond the training kernels' ranges")
    refused(_FnxGrid(B=16383, D=4, H=16000, W=260, is3D=1), 0, "pixel tiles")           # within the other ranges; 2.4e9 tiles
    refused(_FnxGrid(B=0, D=8, H=16, W=16, is3D=1), 0, "batch size")
    refused(_FnxGrid(**ok), 0, "swapped", fwd=bwd, bwd=fwd)
    refused(_FnxGrid(**ok), 0, "the weight image has 5 bytes", fwd=5, bwd=5)
    # everything in order but the workspace (the forward of the net alone takes none)
    for name, call in calls(_FnxGrid(**ok), 0).items():
        if name != "fnx_multiscale3d_forward_train":
            assert call() == ework and "too small" in lib.fnx_last_error().decode(), name
    assert lib.fnx_scalenet3d_pack_t(None, a, None) == einval and "null argument" in lib.fnx_last_error().decode()
    for f in (lib.fnx_multiscale3d_backward_ws_bytes, lib.fnx_fluidnet3d_train_ws_bytes):
        assert f(ctypes.byref(_FnxGrid(B=1, D=1, H=16, W=16))) == 0 and "3D only" in lib.fnx_last_error().decode()
        assert f(ctypes.byref(_FnxGrid(**ok))) > 0
    assert lib.fnx_multiscale3d_tape_layout(ctypes.byref(_FnxGrid(B=1, D=1, H=16, W=16)), None) == 0
    assert "3D only" in lib.fnx_last_error().decode()


def test_parameters_carry_the_reference_names_in_conv3d_shapes(built):
    import inspect
    from fluidnet_cxx_amd import FluidNetTrain3D
    sig = inspect.signature(FluidNetTrain3D.__init__)
    assert list(sig.parameters) == ["self", "mconf", "dropout"] and sig.parameters["dropout"].default is False
    net = FluidNetTrain3D(MCONF)
    assert isinstance(net, torch.nn.Module) and net.training and net.is3D
    want = make_scalenet_weights(0, ndim=3)
    named = dict(net.named_parameters())
    assert list(named) == [L["name"] + sfx for L in scalenet_layers(2, 3) for sfx in (".weight", ".bias")] and len(named) == 34
    for k, v in want.items():
        assert tuple(named[k].shape) == v.shape and named[k].requires_grad and np.array_equal(named[k].detach().numpy(), v), k
    assert named["multiScale.convN_4.encode.0.weight"].shape == (32, 2, 3, 3, 3)
    assert named["multiScale.convN_1.encode.10.weight"].shape == (8, 32, 5, 5, 5)
    assert callable(net.packed_for) and net.precision_mode == "fp32"


def test_checkpoints_go_both_ways_with_the_3d_fluidnet(built):
    from fluidnet_cxx_amd import FluidNet, FluidNetTrain3D
    w = make_scalenet_weights(3, ndim=3)
    sd = {k: torch.from_numpy(v) for k, v in w.items()}
    sd["conv1.weight"] = torch.zeros(16, 2, 3, 3, 3)             # a reference checkpoint's unused parameters are kept
    inf = FluidNet(MCONF, dropout=False)
    inf.load_state_dict(sd)
    net = FluidNetTrain3D(MCONF)
    net.load_state_dict(inf.state_dict())                      # FluidNet -> FluidNetTrain3D
    out = net.state_dict()
    assert set(out) == set(sd) and all(torch.equal(out[k], sd[k]) for k in sd)
    with torch.no_grad():
        net.multiScale.final.bias += 1.0
    back = FluidNet(MCONF, dropout=False)
    back.load_state_dict(net.state_dict())                     # and back
    got = back.state_dict()
    assert torch.equal(got["multiScale.final.bias"], sd["multiScale.final.bias"] + 1.0)
    assert all(torch.equal(got[k], sd[k]) for k in sd if k != "multiScale.final.bias")
    # a 2D checkpoint does not fit
    with pytest.raises(RuntimeError, match="size mismatch"):
        net.load_state_dict({k: torch.from_numpy(v) for k, v in make_scalenet_weights(0).items()})
    bad = dict(sd); del bad["multiScale.final.bias"]
    with pytest.raises(RuntimeError, match="Missing key"):
        net.load_state_dict(bad)


def test_out_of_scope_configurations_raise(built):
    from fluidnet_cxx_amd import FluidNetTrain3D
    with pytest.raises(ValueError, match="3D net only"):
        FluidNetTrain3D(dict(MCONF, is3D=False))
    with pytest.raises(ValueError, match="3D net only"):
        FluidNetTrain3D({k: v for k, v in MCONF.items() if k != "is3D"})
    for mode in ("bf16x6", "bf16x3"):
        with pytest.raises(ValueError, match="fp32 arithmetic only"):
            FluidNetTrain3D(dict(MCONF, precisionMode=mode))
    with pytest.raises(ValueError, match="dropout"):
        FluidNetTrain3D(MCONF, dropout=True)
    with pytest.raises(ValueError, match="ScaleNet"):
        FluidNetTrain3D(dict(MCONF, model="FluidNet"))
    for mode in ("fp32", "fp32_f2", "fp32_f4", "fp32_direct"):
        assert FluidNetTrain3D(dict(MCONF, precisionMode=mode)).precision_mode == mode


def test_train3d_py_has_no_torch_arithmetic():
    """as tests/test_cnn_train_host.py states it for train.py: the gradients come from the kernels"""
    txt = open(os.path.join(os.path.dirname(build.HERE), "fluidnet_cxx_amd", "train3d.py")).read()
    code = "\n".join(l.split("#")[0] for l in txt.splitlines())
    assert not TRAIN_BANNED.search(code), TRAIN_BANNED.search(code).group(0)
