"""Host-side surface of FluidNetTrain (no GPU: the weights are only packed on the first forward): the reference's parameter names,
shapes and count, checkpoint exchange with FluidNet both ways, the out-of-scope configurations, and FluidNet.train() as it was."""
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
             normalizeInputChan="UDiv", normalizeInputThreshold=1e-5, is3D=False, inputDim=2)


@pytest.fixture(scope="module")
def built():
    build.build_all()
    return build


def test_parameters_carry_the_reference_names_and_shapes(built):
    import inspect
    from fluidnet_cxx_amd import FluidNetTrain
    sig = inspect.signature(FluidNetTrain.__init__)
    assert list(sig.parameters) == ["self", "mconf", "dropout"] and sig.parameters["dropout"].default is False
    net = FluidNetTrain(MCONF, dropout=False)
    assert isinstance(net, torch.nn.Module) and net.training
    want = make_scalenet_weights(0)
    named = dict(net.named_parameters())
    assert list(named) == [L["name"] + sfx for L in scalenet_layers() for sfx in (".weight", ".bias")]
    assert len(named) == 34 and sum(p.numel() for p in net.parameters()) == 418643
    for k, v in want.items():
        assert tuple(named[k].shape) == v.shape and named[k].requires_grad and np.array_equal(named[k].detach().numpy(), v), k
    assert net.eval() is net and not net.training and net.train() is net and net.training
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    for p in net.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    assert np.allclose(named["multiScale.final.bias"].detach().numpy(), want["multiScale.final.bias"] - 0.1)
    net.zero_grad()
    assert all(p.grad is None for p in net.parameters())


def test_checkpoints_go_both_ways(built):
    from fluidnet_cxx_amd import FluidNet, FluidNetTrain
    w = make_scalenet_weights(3)
    sd = {k: torch.from_numpy(v) for k, v in w.items()}
    # a reference checkpoint also carries the parameters of the layers its ScaleNet forward never reads
    sd["conv1.weight"] = torch.zeros(16, 2, 3, 3); sd["conv1.bias"] = torch.zeros(16)
    sd["convBank.encode.0.weight"] = torch.zeros(16, 16, 3, 3)
    inf = FluidNet(MCONF, dropout=False)
    inf.load_state_dict(sd)
    net = FluidNetTrain(MCONF)
    net.load_state_dict(inf.state_dict())                      # FluidNet -> FluidNetTrain
    out = net.state_dict()
    assert set(out) == set(sd) and all(torch.equal(out[k], sd[k]) for k in sd)
    with torch.no_grad():
        net.multiScale.final.bias += 1.0
    back = FluidNet(MCONF, dropout=False)
    back.load_state_dict(net.state_dict())                     # and back
    got = back.state_dict()
    assert torch.equal(got["multiScale.final.bias"], sd["multiScale.final.bias"] + 1.0)
    assert all(torch.equal(got[k], sd[k]) for k in sd if k != "multiScale.final.bias")
    bad = dict(sd); del bad["multiScale.final.bias"]
    with pytest.raises(RuntimeError, match="Missing key"):
        net.load_state_dict(bad)
    bad = dict(sd); bad["somethingElse.weight"] = torch.zeros(1)
    with pytest.raises(RuntimeError, match="Unexpected key"):
        net.load_state_dict(bad)
    net.load_state_dict(bad, strict=False)
    bad = dict(sd); bad["multiScale.final.weight"] = torch.zeros(2, 8, 1, 1)
    with pytest.raises(RuntimeError, match="size mismatch"):
        net.load_state_dict(bad)


def test_kept_keys_survive_a_parent_module(built):
    """a parent's state_dict() passes its own destination to the child and ignores the return value"""
    from fluidnet_cxx_amd import FluidNetTrain
    net = FluidNetTrain(MCONF)
    sd = dict(net.state_dict())
    sd["conv1.weight"] = torch.zeros(16, 2, 3, 3)
    net.load_state_dict(sd)
    parent = torch.nn.Module()
    parent.add_module("net", net)
    out = parent.state_dict()
    assert set(out) == {"net." + k for k in sd} and torch.equal(out["net.conv1.weight"], sd["conv1.weight"])
    assert set(net.state_dict(prefix="x.")) == {"x." + k for k in sd}


def test_the_surface_simulate_uses(built):
    """simulate(..., net, 'convnet') and the z-slab driver ask a net for packed_for(device) and precision_mode, as they ask FluidNet"""
    from fluidnet_cxx_amd import FluidNet, FluidNetTrain
    net = FluidNetTrain(dict(MCONF, precisionMode="fp32_f2"))
    assert callable(net.packed_for) and callable(FluidNet(MCONF, dropout=False).packed_for)
    assert net.precision_mode == "fp32_f2"


def test_nets_copy_and_pickle_and_an_old_api_record_loads(built):
    """FluidNet, FluidNetTrain and FluidNetBankTrain survive copy.deepcopy and a pickle round trip with their parameters and the entry
    points they name (the tables of names live at module level, not on the instances), and an _Api pickled before the bank net existed,
    whose state has no `bank`, still names the ScaleNet's entry points."""
    import copy
    import pickle
    from fluidnet_cxx_amd import FluidNet, FluidNetBankTrain, FluidNetTrain, train
    from fluidnet_cxx_amd._ext import ext
    bank = dict(MCONF, model="FluidNet")
    for cls, mconf, forward in ((FluidNet, MCONF, None), (FluidNet, bank, None), (FluidNetTrain, MCONF, ext.fluidnet_forward_train),
                                (FluidNetBankTrain, bank, ext.fluidnet_bank_forward_train)):
        net = cls(mconf)
        for twin in (copy.deepcopy(net), pickle.loads(pickle.dumps(net))):
            assert type(twin) is cls and twin.mconf == mconf
            sd, want = twin.state_dict(), net.state_dict()
            assert list(sd) == list(want) and all(torch.equal(sd[k], want[k]) for k in want)
            if forward is not None:
                assert (twin._api.ndim, twin._api.nc, twin._api.bank) == (2, 2, cls is FluidNetBankTrain)
                assert twin._api.fluidnet_forward_train == forward
    old = train._Api.__new__(train._Api)
    old.__dict__.update(ndim=3, nc=3)                      # (the state of an _Api of the 3D trainer from before the bank net)
    old = pickle.loads(pickle.dumps(old))
    assert old.bank is False and "bank" not in old.__dict__
    assert old.fluidnet_backward == ext.fluidnet3d_backward and old.multiscale_forward_train == ext.multiscale3d_forward_train


def test_out_of_scope_configurations_raise(built):
    from fluidnet_cxx_amd import FluidNet, FluidNetTrain
    with pytest.raises(ValueError, match="2D only"):
        FluidNetTrain(dict(MCONF, is3D=True))
    for mode in ("bf16x6", "bf16x3"):
        with pytest.raises(ValueError, match="fp32 arithmetic only"):
            FluidNetTrain(dict(MCONF, precisionMode=mode))
    with pytest.raises(ValueError, match="dropout"):
        FluidNetTrain(MCONF, dropout=True)
    for mode in ("fp32", "fp32_f2", "fp32_f4", "fp32_direct"):
        assert FluidNetTrain(dict(MCONF, precisionMode=mode)).precision_mode == mode
    with pytest.raises(AssertionError):
        FluidNet(MCONF, dropout=False).train()                 # the inference class keeps refusing


def test_train_py_has_no_torch_arithmetic():
    """as tests/test_abi.py states it for the operator surface: the gradients come from the kernels"""
    txt = open(os.path.join(os.path.dirname(build.HERE), "fluidnet_cxx_amd", "train.py")).read()
    code = "\n".join(l.split("#")[0] for l in txt.splitlines())
    assert not TRAIN_BANNED.search(code), TRAIN_BANNED.search(code).group(0)


def test_training_entry_points_check_before_the_device(built):
    """3D grids and the bf16 modes are refused with their own message, before anything reads a pointer (host memory here)."""
    lib = ctypes.CDLL(built.LIB)
    lib.fnx_last_error.restype = ctypes.c_char_p
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    G = ctypes.POINTER(_FnxGrid)
    lib.fnx_multiscale_forward_train.argtypes = [G, vp, vp, vp, vp, ci, vp]
    lib.fnx_multiscale_backward.argtypes = [G, vp, vp, vp, vp, ci, vp, sz, vp]
    lib.fnx_multiscale_backward_plain.argtypes = [G, vp, vp, vp, vp, ci, vp, sz, vp]
    lib.fnx_fluidnet_forward_train.argtypes = [G, vp, vp, ctypes.c_float, vp, vp, vp, vp, vp, ci, vp, sz, vp]
    lib.fnx_fluidnet_backward.argtypes = [G, vp, vp, vp, vp, vp, vp, vp, ci, vp, sz, vp]
    hdr = open(os.path.join(os.path.dirname(build.HERE), "include", "fluidnet_hip.h")).read()
    einval = int(re.search(r"FNX_EINVAL = (\d+)", hdr).group(1))
    modes = dict(re.findall(r"(FNX_PRECISION_\w+) = (\d+)", hdr))
    buf = ctypes.create_string_buffer(64)
    a = ctypes.cast(buf, vp)

    def calls(g, mode):
        r = ctypes.byref(g)
        return {"fnx_multiscale_forward_train": lambda: lib.fnx_multiscale_forward_train(r, a, a, a, a, mode, None),
                "fnx_multiscale_backward": lambda: lib.fnx_multiscale_backward(r, a, a, a, a, mode, a, 0, None),
                "fnx_multiscale_backward_plain": lambda: lib.fnx_multiscale_backward_plain(r, a, a, a, a, mode, a, 0, None),
                "fnx_fluidnet_forward_train": lambda: lib.fnx_fluidnet_forward_train(r, a, a, 1e-3, a, a, a, a, a, mode, a, 0, None),
                "fnx_fluidnet_backward": lambda: lib.fnx_fluidnet_backward(r, a, a, a, a, a, a, a, mode, a, 0, None)}
    for name, call in calls(_FnxGrid(B=1, D=8, H=16, W=16, is3D=1), 0).items():
        assert call() == einval, name
        assert "2D only" in lib.fnx_last_error().decode(), name
    for m in ("FNX_PRECISION_BF16X6", "FNX_PRECISION_BF16X3"):
        for name, call in calls(_FnxGrid(B=1, D=1, H=16, W=16), int(modes[m])).items():
            assert call() == einval, (name, m)
            assert "fp32 arithmetic only" in lib.fnx_last_error().decode(), (name, m)
    for name, call in calls(_FnxGrid(B=1, D=1, H=16, W=16), 99).items():
        assert call() == einval, name
        assert "precision_mode 99" in lib.fnx_last_error().decode(), name


def test_tape_layout_is_a_function_of_the_grid(built):
    from fluidnet_cxx_amd._ext import ext
    B, H, W = 3, 199, 215
    lay = ext.multiscale_tape_layout(B, H, W)
    assert [e[0] for e in lay] == ["xq", "y0", "y1", "y2", "y3", "in2", "y4", "y5", "y6", "y7", "y8", "y9", "in1"] + [f"y{l}" for l in range(10, 16)]
    L = scalenet_layers()
    end = 0
    for name, off, C, h, w in lay:
        assert off >= end and off % 64 == 0, name
        end = off + B * C * h * w
        if name.startswith("y"):
            l = int(name[1:])
            assert C == L[l]["cout"]
            assert (h, w) == ((int(H * 0.25), int(W * 0.25)) if l < 4 else (int(H * 0.5), int(W * 0.5)) if l < 10 else (H, W)), name
    assert dict((e[0], e[2]) for e in lay)["xq"] == 2 and dict((e[0], e[2]) for e in lay)["in1"] == 3
    assert sum(e[2] for e in lay if e[3] == H) == 331            # floats per full-resolution pixel
    assert ext.multiscale_tape_layout(B, H, W) == lay
