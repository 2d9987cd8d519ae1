"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol the header
declares, the torch extension exposes the reference's entry points, and the product path fails loudly
(no CPU fallback) when handed CPU tensors."""
import ctypes
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    from fluidnet_cxx_amd import build
    build.build_all()
    return build


def test_header_symbols_exported(built):
    hdr = open(os.path.join(REPO, "include", "fluidnet_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = sorted(set(re.findall(r"\b(fnx_[a-z_0-9]+)\s*\(", hdr)))
    assert len(names) >= 18, names
    lib = ctypes.CDLL(built.LIB)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/fluidnet_hip.h but not exported"
    lib.fnx_abi_version.restype = ctypes.c_int
    m = re.search(r"#define FNX_ABI_VERSION (\d+)", open(os.path.join(REPO, "include", "fluidnet_hip.h")).read())
    assert lib.fnx_abi_version() == int(m.group(1))


def test_no_oracle_in_product(built):
    """The shipped library must not link or reference the oracle."""
    import subprocess
    out = subprocess.check_output(["readelf", "-d", built.LIB]).decode() + subprocess.check_output(["readelf", "-d", built.EXT]).decode()
    assert "oracle" not in out
    for root, _, files in os.walk(os.path.join(REPO, "fluidnet_cxx_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(root, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt and "ora_" not in txt, f


def test_no_torch_arithmetic_in_the_operator_surface(built):
    """The operators and the step are the extension's kernels: no torch compute op (where / conv / interpolate / elementwise arithmetic on
    fields) may stand in for one in the Python surface.  (Allocation, views, copies, the generators' index arithmetic and the autograd
    glue are plumbing.)"""
    import re
    banned = re.compile(r"torch\.where\(|F\.conv|functional\.conv|interpolate\(|torch\.nn\.functional|\.conv[123]d\(")
    for f in ("fluid/ops.py", "_simulate.py", "model.py"):
        txt = open(os.path.join(REPO, "fluidnet_cxx_amd", f)).read()
        code = "\n".join(l.split("#")[0] for l in txt.splitlines())
        assert not banned.search(code), (f, banned.search(code).group(0))


def test_no_environment_switches_in_product(built):
    """Kernel selection is a function of the arguments alone: the library reads no environment variable (round 2 had ~18
    getenv switches selecting variants once per process -- hidden process-global state in a library whose contract says
    'no globals'), and its dynamic symbol table does not import getenv."""
    import subprocess
    for root, _, files in os.walk(os.path.join(REPO, "fluidnet_cxx_amd", "csrc")):
        for f in files:
            assert "getenv" not in open(os.path.join(root, f)).read(), f
    syms = subprocess.check_output(["nm", "-D", "--undefined-only", built.LIB]).decode()
    assert "getenv" not in syms


def test_extension_entry_points(built):
    from fluidnet_cxx_amd._ext import ext
    # the reference's pybind names (pytorch/lib/fluid/cpp/fluids_init.cpp:1009-1014)
    for n in ("advect_scalar", "advect_vel", "solve_linear_system"):
        assert hasattr(ext, n)
    for n in ("velocity_divergence", "velocity_update_", "add_buoyancy_", "set_wall_bcs_", "set_const_vals_",
              "flags_to_occupancy", "empty_domain_", "fluidnet_forward", "simulate_step_", "create_cylinder_", "create_box2d_",
              "get_centered"):
        assert hasattr(ext, n)
    # no mutable module state (the reference is re-entrant): quirk mode / slab view / window are per-call (ext.Geom)
    for n in ("set_ref_quirks", "set_slab", "set_window"):
        assert not hasattr(ext, n), n
    g = ext.Geom(ref_quirks=True, z_offset=2, D_global=9, k_begin=1, k_end=3)
    assert (g.ref_quirks, g.z_offset, g.D_global, g.k_begin, g.k_end) == (True, 2, 9, 1, 3)


def test_python_surface_matches_reference(built):
    import inspect
    from fluidnet_cxx_amd import fluid
    def positional(sig):          # the reference's parameters; keyword-only extras: `geom` (per-call 3D options), `plan` (kernel family of the advections)
        extra = [n for n, p in sig.parameters.items() if p.kind is p.KEYWORD_ONLY]
        assert extra in ([], ["geom"], ["geom", "plan"]), extra
        return [n for n, p in sig.parameters.items() if p.kind is not p.KEYWORD_ONLY]
    sig = inspect.signature(fluid.advectScalar)
    assert positional(sig) == ["dt", "src", "U", "flags", "method", "boundary_width", "sample_outside_fluid", "maccormack_strength"]
    assert sig.parameters["maccormack_strength"].default == 0.75 and sig.parameters["method"].default == "maccormackFluidNet"
    sig = inspect.signature(fluid.advectVelocity)
    assert positional(sig) == ["dt", "orig", "U", "flags", "method", "boundary_width", "maccormack_strength"]
    sig = inspect.signature(fluid.solveLinearSystemJacobi)
    assert positional(sig) == ["flags", "div", "is_3d", "p_tol", "max_iter", "verbose"]
    assert sig.parameters["p_tol"].default == 1e-5 and sig.parameters["max_iter"].default == 1000
    # every name the reference's lib/fluid/__init__.py:1-14 re-exports is there
    for n in ("CellType", "getDx", "getCentered", "setWallBcs", "setWallBcsStick", "flagsToOccupancy", "velocityDivergence",
              "velocityUpdate", "addBuoyancy", "addGravity", "addViscosity", "createCylinder", "createBox2D", "emptyDomain",
              "createPlumeBCs", "createRayleighTaylorBCs", "correctScalar", "advectScalar", "advectVelocity",
              "solveLinearSystemJacobi"):
        assert hasattr(fluid, n), n
    assert int(fluid.CellType.TypeFluid) == 1 and int(fluid.CellType.TypeObstacle) == 2 and int(fluid.CellType.TypeEmpty) == 4


def test_cpu_tensors_fail_loudly(built):
    from fluidnet_cxx_amd import fluid
    U = torch.zeros(1, 2, 1, 8, 8); flags = torch.ones(1, 1, 1, 8, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        fluid.velocityDivergence(U, flags)
    with pytest.raises(RuntimeError, match="GPU"):
        fluid.advectScalar(0.1, flags.clone(), U, flags)
    with pytest.raises(AssertionError):
        fluid.advectScalar(0.1, flags.clone(), U, flags, method="semiLagrange")
    with pytest.raises(AssertionError):
        fluid.velocityDivergence(U[0], flags)


class _FnxGrid(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("B", "D", "H", "W", "is3D", "ref_quirks", "z_offset", "D_global", "k_begin", "k_end")]


def test_cnn_entry_points_reject_an_unknown_precision_mode(built):
    """The three CNN entry points check the precision mode before they touch the device, and their message names all six modes."""
    lib = ctypes.CDLL(built.LIB)
    lib.fnx_last_error.restype = ctypes.c_char_p
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    lib.fnx_multiscale_forward.argtypes = [ctypes.POINTER(_FnxGrid), vp, vp, vp, ctypes.c_int, vp, sz, vp]
    lib.fnx_multiscale_forward_crop.argtypes = [ctypes.POINTER(_FnxGrid), vp, vp, vp, ctypes.c_int, vp, vp, sz, vp]
    lib.fnx_fluidnet_forward.argtypes = [ctypes.POINTER(_FnxGrid), vp, vp, ctypes.c_float, vp, vp, ctypes.c_int, vp, sz, vp]
    hdr = open(os.path.join(REPO, "include", "fluidnet_hip.h")).read()
    einval = int(re.search(r"FNX_EINVAL = (\d+)", hdr).group(1))
    g = _FnxGrid(B=1, D=1, H=16, W=16)
    buf = ctypes.create_string_buffer(64)                       # host memory: nothing may read it
    trim = (ctypes.c_int * 4)(0, 0, 0, 0)
    a = ctypes.cast(buf, vp)
    for mode in (-1, 6, 99):
        calls = {"fnx_multiscale_forward": lambda: lib.fnx_multiscale_forward(ctypes.byref(g), a, a, a, mode, a, 0, None),
                 "fnx_multiscale_forward_crop": lambda: lib.fnx_multiscale_forward_crop(ctypes.byref(g), a, a, a, mode,
                                                                                        ctypes.cast(trim, vp), a, 0, None),
                 "fnx_fluidnet_forward": lambda: lib.fnx_fluidnet_forward(ctypes.byref(g), a, a, 1e-3, a, a, mode, a, 0, None)}
        for name, call in calls.items():
            assert call() == einval, (name, mode)
            msg = lib.fnx_last_error().decode()
            assert f"precision_mode {mode}" in msg and "_FP32_F2" in msg and "_FP32_F4" in msg, (name, msg)


def test_weights_deterministic_and_param_count():
    from fluidnet_cxx_amd.weights import make_scalenet_weights, scalenet_layers
    w1, w2 = make_scalenet_weights(0), make_scalenet_weights(0)
    assert all((w1[k] == w2[k]).all() for k in w1)
    assert sum(v.size for v in w1.values()) == 418643          # reference MultiScaleNet parameter count
    assert len(scalenet_layers()) == 17
    w3 = make_scalenet_weights(1)
    assert not (w1["multiScale.final.weight"] == w3["multiScale.final.weight"]).all()
    assert abs(float(w1["multiScale.convN_1.encode.2.weight"].mean())) < 1e-2


def test_restart_file_round_trip(tmp_path):
    """The reference drivers' checkpoint format ({'batch_dict', 'it'} via torch.save, plume.py:168-175,423-424)."""
    import torch
    from fluidnet_cxx_amd import load_restart, save_restart
    from util import plume_state
    st = {k: torch.from_numpy(v) for k, v in plume_state(16).items()}
    st["U"] += 0.25
    f = tmp_path / "restart.pth"
    save_restart(str(f), st, 17)
    raw = torch.load(str(f), weights_only=False)                      # what the reference's restart branch sees
    assert set(raw) == {"batch_dict", "it"} and raw["it"] == 17 and torch.equal(raw["batch_dict"]["U"], st["U"])
    bd, it = load_restart(str(f), torch.device("cpu"))
    assert it == 17 and all(torch.equal(bd[k], st[k]) for k in st)
    torch.save({"batch_dict": {k: v.double() if k == "density" else v for k, v in st.items()}, "it": 3}, str(f))
    bd, it = load_restart(str(f), torch.device("cpu"))                # a foreign file: dtype normalised
    assert it == 3 and bd["density"].dtype == torch.float32 and bd["density"].is_contiguous()


MCONF = dict(model="ScaleNet", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True,
             normalizeInputChan="UDiv", normalizeInputThreshold=1e-5, is3D=False, inputDim=2)


def test_fluidnet_constructor_and_state_dict_like_reference(built):
    """The reference drivers build the net as FluidNet(mconf, dropout=False), then .cuda(), .load_state_dict(state
    ['state_dict']), .eval() (plume.py:119-123; model.py:45).  Host-side behaviour of that surface (no GPU needed: the
    weights are only repacked on the first forward)."""
    import inspect
    from fluidnet_cxx_amd import FluidNet
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    sig = inspect.signature(FluidNet.__init__)
    assert list(sig.parameters) == ["self", "mconf", "dropout"] and sig.parameters["dropout"].default is True
    net = FluidNet(MCONF, dropout=False)
    assert net.eval() is net and net.is3D is False
    w = make_scalenet_weights(3)
    # a reference checkpoint also carries the parameters of the layers its ScaleNet forward never reads
    sd = {k: torch.from_numpy(v) for k, v in w.items()}
    sd["conv1.weight"] = torch.zeros(16, 2, 3, 3); sd["conv1.bias"] = torch.zeros(16)
    sd["convBank.encode.0.weight"] = torch.zeros(16, 16, 3, 3)
    net.load_state_dict(sd)
    out = net.state_dict()
    assert set(out) == set(sd)
    assert all(torch.equal(out[k], sd[k]) for k in sd)
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
    with pytest.raises(AssertionError):
        net.train()
