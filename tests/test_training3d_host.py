"""Host-side surface of the 3D training loop (no GPU): the ABI-26 entry points refuse bad calls before they touch the device (host
pointers here, as in tests/test_training_host.py), the workspace size, the Python surface's refusals, the banned-pattern scan of the
3D module and the shared bases, the checkpoint's way into FluidNet and FluidNetTrain3D, and the two drivers' argument parsing."""
import ctypes
import importlib.util
import os
import re

import pytest
import torch

from fluidnet_cxx_amd import build

REPO = os.path.dirname(build.HERE)
MCONF3 = dict(model="ScaleNet", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True,
              normalizeInputChan="UDiv", normalizeInputThreshold=1e-5, is3D=True, inputDim=3)


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
    d = dict(seed=1, n_min=0, n_max=4, centre_min=-0.3, centre_max=0.3, size_min=0.03, size_max=0.12, octaves=3, wavelength=16.0,
             amplitude=4.0, density_scale=1.0)
    d.update(kw)
    return _FnxSceneParams(**d)


@pytest.fixture(scope="module")
def lib(built):
    lib = ctypes.CDLL(built.LIB)
    lib.fnx_last_error.restype = ctypes.c_char_p
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    G, P = ctypes.POINTER(_FnxGrid), ctypes.POINTER(_FnxSceneParams)
    lib.fnx_scene_obstacles3d.argtypes = [G, P, vp, vp, vp]
    lib.fnx_scene_turbulence3d.argtypes = [G, P, vp, vp, vp, vp]
    lib.fnx_train_loss3d.argtypes = [G, vp, vp, vp, vp, ctypes.POINTER(ctypes.c_float), vp, vp, vp, vp, vp, sz, vp]
    lib.fnx_train_loss3d_ws_bytes.argtypes = [G]
    lib.fnx_train_loss3d_ws_bytes.restype = sz
    return lib


def _header():
    return open(os.path.join(REPO, "include", "fluidnet_hip.h")).read()


def _code(kind):
    return int(re.search(rf"{kind} = (\d+)", _header()).group(1))


def test_abi_version_and_symbols(lib):
    want = int(re.search(r"#define FNX_ABI_VERSION (\d+)", _header()).group(1))
    lib.fnx_abi_version.restype = ctypes.c_int
    assert want >= 26 and lib.fnx_abi_version() == want
    for name in ("fnx_scene_obstacles3d", "fnx_scene_turbulence3d", "fnx_train_loss3d", "fnx_train_loss3d_ws_bytes"):
        assert hasattr(lib, name) and re.search(rf"\b{name}\(", _header()), name


def test_entry_points_refuse_before_the_device(lib):
    """a 2D grid, an axis below 4 cells, null arguments, a grid beyond the lattice addressing or the launch dimensions, the caps and
    inverted ranges, pressure lambdas without a target, a small workspace: each with its own text, on host memory nothing may read"""
    einval, ews = _code("FNX_EINVAL"), _code("FNX_EWORKSPACE")
    cap = int(re.search(r"#define FNX_SCENE_MAX_PRIMITIVES (\d+)", _header()).group(1))
    buf = ctypes.create_string_buffer(64)
    a = ctypes.cast(buf, ctypes.c_void_p)
    lam0 = (ctypes.c_float * 4)(0.0, 1.0, 0.0, 0.0)
    lam1 = (ctypes.c_float * 4)(1.0, 1.0, 0.0, 0.0)
    lam2 = (ctypes.c_float * 4)(0.0, 1.0, 0.5, 0.0)
    ok = _FnxGrid(B=1, D=8, H=16, W=16, is3D=1)
    prm = _params()

    def calls(g, p=prm, lam=lam0, tgt=a, ws=1 << 20):
        r, q = ctypes.byref(g), ctypes.byref(p)
        return {"fnx_scene_obstacles3d": lambda: lib.fnx_scene_obstacles3d(r, q, a, a, None),
                "fnx_scene_turbulence3d": lambda: lib.fnx_scene_turbulence3d(r, q, a, a, a, None),
                "fnx_train_loss3d": lambda: lib.fnx_train_loss3d(r, a, a, a, tgt, lam, a, a, a, a, a, ws, None)}

    def refused(call, text, what, code=einval):
        assert call() == code, what
        assert text in lib.fnx_last_error().decode(), (what, lib.fnx_last_error().decode())

    for g in (_FnxGrid(B=1, D=1, H=16, W=16, is3D=0), _FnxGrid(B=1, D=8, H=16, W=16, is3D=0), _FnxGrid(B=1, D=3, H=16, W=16, is3D=1)):
        for name, call in calls(g).items():
            refused(call, "3D only", name)
    for g in (_FnxGrid(B=1, D=8, H=3, W=16, is3D=1), _FnxGrid(B=1, D=8, H=16, W=2, is3D=1)):
        for name, call in calls(g).items():
            refused(call, "at least 4 cells per axis", name)
    # beyond the lattice addressing (16 bits along x and y), the launch dimension (B * D) and the cells of a sample
    for g, text in ((_FnxGrid(B=1, D=8, H=16, W=32769, is3D=1), "<= 32768"), (_FnxGrid(B=1, D=8, H=32769, W=16, is3D=1), "<= 32768"),
                    (_FnxGrid(B=1, D=32769, H=16, W=16, is3D=1), "<= 32768"), (_FnxGrid(B=8192, D=8, H=16, W=16, is3D=1), "B * D <= 65535"),
                    (_FnxGrid(B=1, D=2048, H=1024, W=1024, is3D=1), "< 2^31")):
        for name, call in calls(g).items():
            refused(call, text, name)
    # null arguments
    r, q = ctypes.byref(ok), ctypes.byref(prm)
    refused(lambda: lib.fnx_scene_obstacles3d(r, q, None, a, None), "null argument", "obstacles ids")
    refused(lambda: lib.fnx_scene_obstacles3d(r, q, a, None, None), "null argument", "obstacles flags")
    refused(lambda: lib.fnx_scene_obstacles3d(r, None, a, a, None), "null argument", "obstacles params")
    refused(lambda: lib.fnx_scene_obstacles3d(None, q, a, a, None), "null argument", "obstacles grid")
    refused(lambda: lib.fnx_scene_turbulence3d(r, q, None, a, a, None), "null argument", "turbulence ids")
    refused(lambda: lib.fnx_scene_turbulence3d(r, q, a, None, a, None), "null argument", "turbulence U")
    refused(lambda: lib.fnx_train_loss3d(r, None, a, a, a, lam0, a, a, a, a, a, 1 << 20, None), "null argument", "loss out_p")
    refused(lambda: lib.fnx_train_loss3d(r, a, None, a, a, lam0, a, a, a, a, a, 1 << 20, None), "null argument", "loss out_U")
    refused(lambda: lib.fnx_train_loss3d(r, a, a, None, a, lam0, a, a, a, a, a, 1 << 20, None), "null argument", "loss flags")
    refused(lambda: lib.fnx_train_loss3d(r, a, a, a, a, lam0, None, a, a, a, a, 1 << 20, None), "null argument", "loss upstream")
    refused(lambda: lib.fnx_train_loss3d(r, a, a, a, a, lam0, a, a, a, None, a, 1 << 20, None), "null argument", "loss grad_U")
    refused(lambda: lib.fnx_train_loss3d(r, a, a, a, a, lam0, a, None, None, None, a, 1 << 20, None), "null argument", "loss no output")
    refused(lambda: lib.fnx_train_loss3d(r, a, a, a, a, lam0, a, a, a, a, None, 0, None), "null argument", "loss workspace")
    # the cap and the ranges, as in 2D
    refused(calls(ok, _params(n_max=cap + 1))["fnx_scene_obstacles3d"], f"cap of {cap}", "n_max")
    refused(calls(ok, _params(n_min=3, n_max=2))["fnx_scene_obstacles3d"], "inverted range", "n range")
    refused(calls(ok, _params(n_min=-1))["fnx_scene_obstacles3d"], "inverted range", "negative n_min")
    refused(calls(ok, _params(centre_min=0.2, centre_max=0.1))["fnx_scene_obstacles3d"], "inverted range", "centre range")
    refused(calls(ok, _params(size_min=0.2, size_max=0.1))["fnx_scene_obstacles3d"], "inverted range", "size range")
    refused(calls(ok, _params(octaves=0))["fnx_scene_turbulence3d"], "octaves", "octaves 0")
    refused(calls(ok, _params(octaves=9))["fnx_scene_turbulence3d"], "octaves", "octaves 9")
    refused(calls(ok, _params(octaves=4, wavelength=4.0))["fnx_scene_turbulence3d"], "wavelength", "wavelength")
    for lam in (lam1, lam2):
        refused(calls(ok, lam=lam, tgt=None)["fnx_train_loss3d"], "target_p is null", "p lambda without target")
    # the workspace: one fp64 quadruple per workgroup of 64 x 4 cells of a plane
    assert lib.fnx_train_loss3d_ws_bytes(ctypes.byref(_FnxGrid(B=3, D=1, H=37, W=130))) == 0
    assert lib.fnx_train_loss3d_ws_bytes(ctypes.byref(_FnxGrid(B=3, D=5, H=37, W=130, is3D=0))) == 0
    odd = _FnxGrid(B=3, D=5, H=37, W=130, is3D=1)
    need = 3 * 5 * 10 * 3 * 4 * 8
    assert lib.fnx_train_loss3d_ws_bytes(ctypes.byref(odd)) == need
    refused(calls(odd, ws=need - 1)["fnx_train_loss3d"], "too small", "workspace one byte short", code=ews)


def test_python_surface_refuses_2d(built):
    from fluidnet_cxx_amd import training3d
    with pytest.raises(ValueError, match="3D only"):
        training3d.SceneSampler3D(dict(MCONF3, is3D=False), 2, 8, 16, 16, 0, device="cpu")
    with pytest.raises(ValueError, match="3D only"):
        training3d.SceneSampler3D(MCONF3, 2, 1, 16, 16, 0, device="cpu")
    with pytest.raises(ValueError, match="3D only"):
        training3d.train3d(dict(MCONF3, is3D=False), dict(res=16, batch=1, iters=1), device="cpu")
    with pytest.raises(ValueError, match="3D only"):
        training3d.train3d(MCONF3, dict(res=16, D=1, batch=1, iters=1), device="cpu")
    with pytest.raises(ValueError, match="3D only"):
        training3d.fluidnet_loss3d(torch.zeros(1, 1, 1, 8, 8), torch.zeros(1, 2, 1, 8, 8), torch.ones(1, 1, 1, 8, 8), None, (0, 1, 0, 0))
    with pytest.raises(RuntimeError, match="GPU"):          # no CPU path: the kernel is the loss
        training3d.fluidnet_loss3d(torch.zeros(1, 1, 4, 8, 8), torch.zeros(1, 3, 4, 8, 8), torch.ones(1, 1, 4, 8, 8), None, (0, 1, 0, 0))
    assert training3d.MCONF3D_DEFAULTS == dict(__import__("fluidnet_cxx_amd.training", fromlist=["x"]).MCONF_DEFAULTS, is3D=True, inputDim=3)
    assert {"res", "batch", "iters", "seed"} <= set(training3d.TCONF3D_DEFAULTS) and {"octaves", "wavelength", "n_max"} <= set(training3d.SCENE3D_DEFAULTS)


def test_training3d_py_keeps_the_arithmetic_in_the_kernels():
    """the rule of tests/test_training_host.py for the 3D module and for training.py, which holds the bases both loops share"""
    banned = re.compile(r"torch\.where\(|F\.conv|functional\.conv|interpolate\(|torch\.nn\.functional|\.conv[123]d\(|autograd\.grad\(|"
                        r"torch\.rand|torch\.randn|torch\.normal|manual_seed\(\s*\)|\.mean\(|\.abs\(|\.pow\(|\*\* ?2\)\.")
    for name in ("training3d.py", "training.py"):
        txt = open(os.path.join(REPO, "fluidnet_cxx_amd", name)).read()
        txt = re.sub(r'""".*?"""', "", txt, flags=re.S)
        code = "\n".join(l.split("#")[0] for l in txt.splitlines())
        assert not banned.search(code), (name, banned.search(code).group(0))
    src = open(os.path.join(REPO, "fluidnet_cxx_amd", "training3d.py")).read()
    assert "_SceneSamplerBase" in src and "_train(" in src            # the 3D loop is the shared one, not a copy


def test_checkpoint_round_trip_into_fluidnet_3d(built, tmp_path):
    """the checkpoint's keys, through torch.save / torch.load, into FluidNet (is3D) and FluidNetTrain3D"""
    from fluidnet_cxx_amd import FluidNet, FluidNetTrain3D
    from fluidnet_cxx_amd.training import kaiming_init
    from fluidnet_cxx_amd.training3d import MCONF3D_DEFAULTS
    mconf = dict(MCONF3D_DEFAULTS)
    net = kaiming_init(FluidNetTrain3D(mconf), 9)
    opt = torch.optim.Adam(net.parameters(), lr=mconf["lr"])
    for p in net.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    f = tmp_path / "ck3d.pth"
    torch.save(dict(state_dict={k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, optimizer=opt.state_dict(), mconf=mconf,
                    it=1), str(f))
    ck = torch.load(str(f), map_location="cpu", weights_only=False)
    assert {"state_dict", "optimizer", "mconf", "it"} <= set(ck) and ck["it"] == 1 and ck["mconf"]["is3D"]
    inf = FluidNet(ck["mconf"], dropout=False)
    inf.load_state_dict(ck["state_dict"])
    got, want = inf.state_dict(), net.state_dict()
    assert set(got) == set(want) and all(torch.equal(got[k], want[k].detach()) for k in want)
    assert any(v.dim() == 5 for v in got.values())                   # Conv3d shapes
    again = FluidNetTrain3D(ck["mconf"])
    again.load_state_dict(ck["state_dict"])
    opt2 = torch.optim.Adam(again.parameters(), lr=mconf["lr"])
    opt2.load_state_dict(ck["optimizer"])
    assert all(torch.equal(a, b) for a, b in zip(again.parameters(), net.parameters()))
    assert opt2.state_dict()["state"][0]["step"] == opt.state_dict()["state"][0]["step"]


def _example(name):
    spec = importlib.util.spec_from_file_location(f"example_{name}", os.path.join(REPO, "examples", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plume_driver_takes_3d_weights(built, capsys):
    plume = _example("plume")
    a = plume.parse_args(["--depth", "8", "--method", "convnet", "--weights3d", "w.pth"])
    assert a.depth == 8 and a.method == "convnet" and a.weights3d == "w.pth" and a.weights is None
    for argv in (["--depth", "8", "--method", "convnet"], ["--method", "convnet", "--weights3d", "w.pth"],
                 ["--depth", "8", "--method", "jacobi", "--weights3d", "w.pth"], ["--depth", "8", "--method", "convnet", "--weights", "w.pth"]):
        with pytest.raises(SystemExit):
            plume.parse_args(argv)
    assert "--weights3d" in capsys.readouterr().err


def test_train_driver_parses_depth(built):
    train = _example("train")
    a = train.parse_args(["--depth", "16"])
    assert a.depth == 16 and a.res == 64 and a.batch == 4
    b = train.parse_args([])
    assert b.depth is None and b.res == 128 and b.batch == 64
    assert train.parse_args(["--depth", "16", "--res", "32", "--batch", "2"]).res == 32
    with pytest.raises(SystemExit):
        train.parse_args(["--depth", "3"])
