"""Host-side surface of the training loop (no GPU): the new C entry points refuse bad calls before they touch the device (host pointers
here, as in tests/test_cnn_train_host.py), the ABI version, the seeded initialisation and the checkpoint's way into FluidNet."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from fluidnet_cxx_amd import build

REPO = os.path.dirname(build.HERE)
MCONF = dict(model="ScaleNet", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True,
             normalizeInputChan="UDiv", normalizeInputThreshold=1e-5, is3D=False, inputDim=2)


@pytest.fixture(scope="module")
def built():
    build.build_all()
    return build


class _FnxGrid(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("B", "D", "H", "W", "is3D", "ref_quirks", "z_offset", "D_global", "k_begin", "k_end")]


class _FnxSceneParams(ctypes.Structure):
    _fields_ = [("seed", ctypes.c_uint), ("n_min", ctypes.c_int), ("n_max", ctypes.c_int), ("centre_min", ctypes.c_float),
                ("centre_max", ctypes.c_float), ("size_min", ctypes.c_float), ("size_max", ctypes.c_float), ("octaves", ctypes.c_int),
                ("wavelength", ctypes.c_float), ("amplitude", ctypes.c_float), ("density_scale", ctypes.c_float)]


def _params(**kw):
    d = dict(seed=1, n_min=0, n_max=4, centre_min=-0.3, centre_max=0.3, size_min=0.03, size_max=0.12, octaves=4, wavelength=32.0,
             amplitude=8.0, density_scale=1.0)
    d.update(kw)
    return _FnxSceneParams(**d)


@pytest.fixture(scope="module")
def lib(built):
    lib = ctypes.CDLL(built.LIB)
    lib.fnx_last_error.restype = ctypes.c_char_p
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    G, P = ctypes.POINTER(_FnxGrid), ctypes.POINTER(_FnxSceneParams)
    lib.fnx_scene_obstacles.argtypes = [G, P, vp, vp, vp]
    lib.fnx_scene_turbulence.argtypes = [G, P, vp, vp, vp, vp]
    lib.fnx_train_loss.argtypes = [G, vp, vp, vp, vp, ctypes.POINTER(ctypes.c_float), vp, vp, vp, vp, vp, sz, vp]
    lib.fnx_train_loss_ws_bytes.argtypes = [G]
    lib.fnx_train_loss_ws_bytes.restype = sz
    return lib


def _einval():
    hdr = open(os.path.join(REPO, "include", "fluidnet_hip.h")).read()
    return int(re.search(r"FNX_EINVAL = (\d+)", hdr).group(1)), hdr


def test_abi_version_is_the_headers(lib):
    _, hdr = _einval()
    want = int(re.search(r"#define FNX_ABI_VERSION (\d+)", hdr).group(1))
    lib.fnx_abi_version.restype = ctypes.c_int
    assert lib.fnx_abi_version() == want and want >= 23


def test_new_entry_points_refuse_before_the_device(lib):
    """null, 3D, a grid below 4 cells, n_max over the cap, inverted ranges, pressure lambdas without a target: each with its own message,
    on host memory that nothing may read"""
    einval, hdr = _einval()
    cap = int(re.search(r"#define FNX_SCENE_MAX_PRIMITIVES (\d+)", hdr).group(1))
    buf = ctypes.create_string_buffer(64)
    a = ctypes.cast(buf, ctypes.c_void_p)
    lam0 = (ctypes.c_float * 4)(0.0, 1.0, 0.0, 0.0)
    lam1 = (ctypes.c_float * 4)(1.0, 1.0, 0.0, 0.0)
    lam2 = (ctypes.c_float * 4)(0.0, 1.0, 0.5, 0.0)
    ok = _FnxGrid(B=1, D=1, H=16, W=16)
    prm = _params()

    def calls(g, p=prm, lam=lam0, tgt=a):
        r, q = ctypes.byref(g), ctypes.byref(p)
        return {"fnx_scene_obstacles": lambda: lib.fnx_scene_obstacles(r, q, a, a, None),
                "fnx_scene_turbulence": lambda: lib.fnx_scene_turbulence(r, q, a, a, a, None),
                "fnx_train_loss": lambda: lib.fnx_train_loss(r, a, a, a, tgt, lam, a, a, a, a, a, 1 << 20, None)}

    def refused(call, text, what):
        assert call() == einval, what
        assert text in lib.fnx_last_error().decode(), (what, lib.fnx_last_error().decode())

    for name, call in calls(_FnxGrid(B=1, D=8, H=16, W=16, is3D=1)).items():
        refused(call, "2D only", name)
    for name, call in calls(_FnxGrid(B=1, D=2, H=16, W=16, is3D=0)).items():
        refused(call, "2D only", name)
    for g in (_FnxGrid(B=1, D=1, H=3, W=16), _FnxGrid(B=1, D=1, H=16, W=2)):
        for name, call in calls(g).items():
            refused(call, "at least 4 cells", name)
    # null arguments
    r, q = ctypes.byref(ok), ctypes.byref(prm)
    refused(lambda: lib.fnx_scene_obstacles(r, q, None, a, None), "null argument", "obstacles ids")
    refused(lambda: lib.fnx_scene_obstacles(r, q, a, None, None), "null argument", "obstacles flags")
    refused(lambda: lib.fnx_scene_obstacles(r, None, a, a, None), "null argument", "obstacles params")
    refused(lambda: lib.fnx_scene_obstacles(None, q, a, a, None), "null argument", "obstacles grid")
    refused(lambda: lib.fnx_scene_turbulence(r, q, None, a, a, None), "null argument", "turbulence ids")
    refused(lambda: lib.fnx_scene_turbulence(r, q, a, None, a, None), "null argument", "turbulence U")
    refused(lambda: lib.fnx_train_loss(r, None, a, a, a, lam0, a, a, a, a, a, 1 << 20, None), "null argument", "loss out_p")
    refused(lambda: lib.fnx_train_loss(r, a, None, a, a, lam0, a, a, a, a, a, 1 << 20, None), "null argument", "loss out_U")
    refused(lambda: lib.fnx_train_loss(r, a, a, None, a, lam0, a, a, a, a, a, 1 << 20, None), "null argument", "loss flags")
    refused(lambda: lib.fnx_train_loss(r, a, a, a, a, lam0, None, a, a, a, a, 1 << 20, None), "null argument", "loss upstream")
    refused(lambda: lib.fnx_train_loss(r, a, a, a, a, lam0, a, a, a, None, a, 1 << 20, None), "null argument", "loss grad_U")
    refused(lambda: lib.fnx_train_loss(r, a, a, a, a, lam0, a, None, None, None, a, 1 << 20, None), "null argument", "loss no output")
    refused(lambda: lib.fnx_train_loss(r, a, a, a, a, lam0, a, a, a, a, None, 0, None), "null argument", "loss workspace")
    # the cap and the ranges
    refused(calls(ok, _params(n_max=cap + 1))["fnx_scene_obstacles"], f"cap of {cap}", "n_max")
    refused(calls(ok, _params(n_min=3, n_max=2))["fnx_scene_obstacles"], "inverted range", "n range")
    refused(calls(ok, _params(n_min=-1))["fnx_scene_obstacles"], "inverted range", "negative n_min")
    refused(calls(ok, _params(centre_min=0.2, centre_max=0.1))["fnx_scene_obstacles"], "inverted range", "centre range")
    refused(calls(ok, _params(size_min=0.2, size_max=0.1))["fnx_scene_obstacles"], "inverted range", "size range")
    refused(calls(ok, _params(octaves=0))["fnx_scene_turbulence"], "octaves", "octaves 0")
    refused(calls(ok, _params(octaves=9))["fnx_scene_turbulence"], "octaves", "octaves 9")
    refused(calls(ok, _params(octaves=4, wavelength=4.0))["fnx_scene_turbulence"], "wavelength", "wavelength")
    # pressure lambdas with a null target
    for lam in (lam1, lam2):
        refused(calls(ok, lam=lam, tgt=None)["fnx_train_loss"], "target_p is null", "p lambda without target")
    assert lib.fnx_train_loss_ws_bytes(ctypes.byref(_FnxGrid(B=1, D=8, H=16, W=16, is3D=1))) == 0
    assert lib.fnx_train_loss_ws_bytes(ctypes.byref(_FnxGrid(B=3, D=1, H=37, W=130))) == 3 * 10 * 3 * 4 * 8


def test_python_surface_refuses_3d(built):
    from fluidnet_cxx_amd import training
    with pytest.raises(ValueError, match="2D only"):
        training.SceneSampler(MCONF, 2, 16, 16, 0, device="cpu", depth=8)
    with pytest.raises(ValueError, match="2D only"):
        training.SceneSampler(dict(MCONF, is3D=True), 2, 16, 16, 0, device="cpu")
    with pytest.raises(ValueError, match="2D only"):
        training.train(dict(MCONF, is3D=True), dict(res=16, batch=1, iters=1), device="cpu")
    with pytest.raises(ValueError, match="2D only"):
        training.fluidnet_loss(torch.zeros(1, 1, 4, 8, 8), torch.zeros(1, 3, 4, 8, 8), torch.ones(1, 1, 4, 8, 8), None, (0, 1, 0, 0))
    with pytest.raises(RuntimeError, match="GPU"):          # no CPU path: the kernel is the loss
        training.fluidnet_loss(torch.zeros(1, 1, 1, 8, 8), torch.zeros(1, 2, 1, 8, 8), torch.ones(1, 1, 1, 8, 8), None, (0, 1, 0, 0))


def test_training_py_keeps_the_arithmetic_in_the_kernels():
    """the rule of tests/test_abi.py for the operator surface: no torch compute op stands in for a kernel, and torch's global generator
    is not used"""
    banned = re.compile(r"torch\.where\(|F\.conv|functional\.conv|interpolate\(|torch\.nn\.functional|\.conv[123]d\(|autograd\.grad\(|"
                        r"torch\.rand|torch\.randn|torch\.normal|manual_seed\(\s*\)|\.mean\(|\.abs\(|\.pow\(|\*\* ?2\)\.")
    txt = open(os.path.join(REPO, "fluidnet_cxx_amd", "training.py")).read()
    txt = re.sub(r'""".*?"""', "", txt, flags=re.S)
    code = "\n".join(l.split("#")[0] for l in txt.splitlines())
    assert not banned.search(code), banned.search(code).group(0)


def test_kaiming_initialisation_is_seeded(built):
    from fluidnet_cxx_amd import FluidNetTrain
    from fluidnet_cxx_amd.training import kaiming_init
    torch.manual_seed(123)
    a = kaiming_init(FluidNetTrain(MCONF), 5).state_dict()
    torch.manual_seed(321)                                   # the global generator plays no part
    b = kaiming_init(FluidNetTrain(MCONF), 5).state_dict()
    c = kaiming_init(FluidNetTrain(MCONF), 6).state_dict()
    plain = FluidNetTrain(MCONF).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    for k in a:
        if k.endswith(".weight"):
            assert not torch.equal(a[k], c[k]) and not torch.equal(a[k], plain[k]), k
            fan_in = a[k][0].numel()
            bound = float(np.sqrt(6.0 / fan_in))             # kaiming_uniform_: gain sqrt(2), bound gain sqrt(3 / fan_in)
            assert float(a[k].abs().max()) <= bound and float(a[k].abs().max()) > 0.5 * bound, k
        else:
            assert torch.equal(a[k], plain[k]), k            # init_weights touches the weights only


def test_checkpoint_round_trip_into_fluidnet(built, tmp_path):
    """the checkpoint's keys, through torch.save / torch.load, into FluidNet and FluidNetTrain"""
    from fluidnet_cxx_amd import FluidNet, FluidNetTrain
    from fluidnet_cxx_amd.training import MCONF_DEFAULTS, kaiming_init
    mconf = dict(MCONF_DEFAULTS)
    net = kaiming_init(FluidNetTrain(mconf), 9)
    opt = torch.optim.Adam(net.parameters(), lr=mconf["lr"])
    for p in net.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    f = tmp_path / "ck.pth"
    torch.save(dict(state_dict={k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, optimizer=opt.state_dict(), mconf=mconf,
                    it=1), str(f))
    ck = torch.load(str(f), map_location="cpu", weights_only=False)
    assert {"state_dict", "optimizer", "mconf", "it"} <= set(ck) and ck["it"] == 1
    inf = FluidNet(ck["mconf"], dropout=False)
    inf.load_state_dict(ck["state_dict"])
    got = inf.state_dict()
    want = net.state_dict()
    assert set(got) == set(want) and all(torch.equal(got[k], want[k].detach()) for k in want)
    again = FluidNetTrain(ck["mconf"])
    again.load_state_dict(ck["state_dict"])
    opt2 = torch.optim.Adam(again.parameters(), lr=mconf["lr"])
    opt2.load_state_dict(ck["optimizer"])
    assert all(torch.equal(a, b) for a, b in zip(again.parameters(), net.parameters()))
    assert opt2.state_dict()["state"][0]["step"] == opt.state_dict()["state"][0]["step"]
