"""Vorticity confinement on the GPU: the fused tile kernels against the float32 model of tests/vorticity_reference.py bit for bit,
and the stage in simulate() -- fused step, operator path and a step assembled by hand."""
import numpy as np
import pytest
import torch

import vorticity_reference as VR
from util import PLUME_CFG, assert_bitexact, make_flags, plume_state

pytestmark = pytest.mark.gpu
AMP = 0.5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    from fluidnet_cxx_amd._ext import ext
    return ext


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def N(t):
    return t.cpu().numpy()


def _flags(B, D, H, W):
    """tests/util.py's boxes and empties (where the grid has room) plus the model's own box and patch of empty cells"""
    f = VR.case_flags(B, D, H, W)
    g = make_flags(B, D, H, W, boxes=True, empties=H >= 12 and W >= 12)
    f[g == 2.0] = 2.0
    f[(g == 4.0) & (f == 1.0)] = 4.0
    return f


def _check(ext, dev, U, f, what):
    tU, tf = T(U, dev), T(f, dev)
    got = ext.add_vorticity_confinement(tU, tf, AMP, None)
    again = ext.add_vorticity_confinement(tU, tf, AMP, None)
    assert_bitexact(N(tU), U, f"{what}: U_in after the call"); assert_bitexact(N(tf), f, f"{what}: flags after the call")
    want = VR.confine(U, f, AMP)
    assert (want != U).any() or min(U.shape[3:]) < 5
    assert_bitexact(N(got), want, what)
    assert_bitexact(N(again), N(got), f"{what}: second call")
    return got


# 2D: (B, D, H, W); 3 x 3 has one interior cell; 199 x 215 has partial tiles in both axes
@pytest.mark.parametrize("shape", [(2, 1, 40, 48), (2, 1, 37, 53), (3, 1, 199, 215), (1, 1, 3, 3)])
def test_operator_2d_bitexact(dev, ext, shape):
    B, D, H, W = shape
    U = VR.sine_field((B, 2, D, H, W), seed=H)
    _check(ext, dev, U, _flags(B, D, H, W), f"2D {shape}")


# 3D: (1, 3, 13, 18) has one interior plane; 70 x 100 partial tiles; D = 11, 20 one chunk of the march
@pytest.mark.parametrize("shape", [(2, 20, 24, 28), (1, 9, 14, 22), (1, 3, 13, 18), (3, 11, 70, 100), (1, 70, 13, 61)])
def test_operator_3d_bitexact(dev, ext, shape):
    B, D, H, W = shape
    U = VR.sine_field((B, 3, D, H, W), seed=D + H)
    _check(ext, dev, U, _flags(B, D, H, W), f"3D {shape}")


def _big_field(shape, seed):
    """three separable sine modes per component plus 5 % white noise, built by broadcasting (cheap at 16.7 M cells)"""
    B, nc, D, H, W = shape
    rng = np.random.default_rng(seed)
    U = (0.05 * rng.standard_normal(shape, dtype=np.float32))
    ax = [np.arange(n, dtype=np.float32) for n in (D, H, W)]
    for a in range(nc):
        for _ in range(3):
            k = rng.integers(2, 12, 3) * 2 * np.pi / np.array([max(D, 2), H, W])
            ph = rng.uniform(0, 2 * np.pi, 3)
            s = [np.sin(k[q] * ax[q] + ph[q]).astype(np.float32) for q in range(3)]
            U[:, a] += np.float32(rng.uniform(0.3, 1.0)) * (s[0][:, None, None] * s[1][None, :, None] * s[2][None, None, :])
    return U


def test_operator_1024_squared_whole_field(dev, ext):
    shape = (1, 2, 1, 1024, 1024)
    _check(ext, dev, _big_field(shape, 1), _flags(1, 1, 1024, 1024), "1024^2")


def test_operator_256_cubed_whole_field(dev, ext):
    """the whole field against the model, so every first, last and partial tile position and every chunk of the march is in it"""
    shape = (1, 3, 256, 256, 256)
    _check(ext, dev, _big_field(shape, 2), _flags(1, 256, 256, 256), "256^3")


def test_amplitude_zero_copies_and_python_operator(dev, ext):
    from fluidnet_cxx_amd import fluid
    for shape in ((2, 2, 1, 40, 48), (2, 3, 12, 24, 28)):
        B, nc, D, H, W = shape
        U = VR.sine_field(shape, seed=5); U[0, 0, 0, 5, 5] = -0.0
        f = _flags(B, D, H, W)
        assert_bitexact(N(ext.add_vorticity_confinement(T(U, dev), T(f, dev), 0.0, None)), U, "amp 0")
        tU = T(U, dev)
        r = fluid.addVorticityConfinement(tU, T(f, dev), AMP)
        assert r is tU
        assert_bitexact(N(tU), VR.confine(U, f, AMP), "fluid.addVorticityConfinement (in place)")
    with pytest.raises(RuntimeError, match="compute window or z-slab"):
        fluid.addVorticityConfinement(T(U, dev), T(f, dev), AMP, geom=ext.Geom(k_begin=2, k_end=6))
    with pytest.raises(RuntimeError, match="compute window or z-slab"):
        fluid.addVorticityConfinement(T(U, dev), T(f, dev), AMP, geom=ext.Geom(z_offset=2, D_global=40))


# ---- the stage in simulate()
def _state(D, dev):
    """a plume with boxes and empty cells in the way and a rough velocity field, so that the confinement has something to act on"""
    H, W = (40, 72) if D > 1 else (72, 136)
    st = plume_state(W, D)
    st = {k: np.ascontiguousarray(v[:, :, :, :H]) for k, v in st.items()}
    st["flags"] = make_flags(1, D, H, W, boxes=True, empties=True)
    rng = np.random.default_rng(3)
    st["U"] = (st["U"] + rng.standard_normal(st["U"].shape).astype(np.float32) * np.float32(0.5)).astype(np.float32)
    st["density"] = rng.random(st["density"].shape).astype(np.float32)
    return {k: T(v, dev) for k, v in st.items()}


def _run(cfg, D, dev, method, fused, net=None, steps=3):
    from fluidnet_cxx_amd import _simulate, simulate
    _simulate.release_workspaces()
    bd = _state(D, dev)
    for _ in range(steps):
        simulate(cfg, bd, net, method, fused=fused)
    _simulate.release_workspaces()
    return {k: N(bd[k]) for k in ("U", "density", "p")}


@pytest.mark.parametrize("D", [1, 12])
@pytest.mark.parametrize("method", ["jacobi", "pcg"])
def test_simulate_fused_and_operator_path_same_bits(dev, D, method):
    cfg = dict(PLUME_CFG, jacobiIter=9, pcgTol=0.0, pcgIter=8, vorticityConfinementAmp=AMP)
    a = _run(cfg, D, dev, method, True)
    b = _run(cfg, D, dev, method, False)
    off = _run(dict(cfg, vorticityConfinementAmp=0), D, dev, method, True)
    for k in ("U", "density", "p"):
        assert_bitexact(a[k], b[k], f"{method} D={D}: fused vs operator path, {k}")
    assert np.isfinite(a["U"]).all()
    assert (a["U"] != off["U"]).mean() > 0.2, "the confinement changes the step"
    # amplitude 0 and the key absent are the same step
    none = _run({k: v for k, v in cfg.items() if k != "vorticityConfinementAmp"}, D, dev, method, True)
    for k in ("U", "density", "p"):
        assert_bitexact(off[k], none[k], f"{method} D={D}: amplitude 0 vs no key, {k}")


@pytest.mark.parametrize("D", [1, 12])
def test_simulate_with_optional_stages_and_periodic_patches(dev, D):
    """the cut stage next to gravity, the periodic patches and (2D) viscosity: fused and operator path agree in bits"""
    extra = {"gravityScale": 0.5, "correctScalar": True, "periodic-x": True, "periodic-y": True}
    if D == 1:
        extra["viscosity"] = 0.02
    cfg = dict(PLUME_CFG, jacobiIter=9, vorticityConfinementAmp=AMP, **extra)
    a, b = _run(cfg, D, dev, "jacobi", True), _run(cfg, D, dev, "jacobi", False)
    for k in ("U", "density", "p"):
        assert_bitexact(a[k], b[k], f"optional stages D={D}: fused vs operator path, {k}")


@pytest.mark.parametrize("D", [1, 12])
def test_simulate_convnet(dev, D):
    """The convnet step with the key positive, fused against the operator path.  Both paths are held to 1e-5 of |ref|max of one
    reference today (test_parity_gpu.py::test_sim64_convnet_vs_reference), so they may differ by 2e-5 of it; that bound holds here
    with and without the confinement."""
    from fluidnet_cxx_amd import FluidNet
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    is3d = D > 1
    cfg = dict(PLUME_CFG, model="ScaleNet", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True,
               normalizeInputChan="UDiv", is3D=is3d)
    net = FluidNet.from_weights(cfg, make_scalenet_weights(0, ndim=3 if is3d else 2), dev)
    res = {}
    for amp in (0, AMP):
        c = dict(cfg, vorticityConfinementAmp=amp)
        a, b = _run(c, D, dev, "convnet", True, net), _run(c, D, dev, "convnet", False, net)
        res[amp] = a
        for k in ("U", "density", "p"):
            scale = float(np.abs(b[k]).max())
            d = float(np.abs(a[k].astype(np.float64) - b[k]).max())
            print(f"\nconvnet D={D} amp={amp}: {k} fused vs operator path max |d| = {d:.3e} = {d / scale:.2e} of |{k}|max")
            assert d <= 2e-5 * scale, (k, amp, d, scale)
    assert (res[0]["U"] != res[AMP]["U"]).mean() > 0.2


@pytest.mark.parametrize("D", [1, 12])
def test_step_assembled_by_hand(dev, D):
    """the operators in simulate()'s order with addVorticityConfinement between addGravity and setWallBcs: the bits of fused=False"""
    from fluidnet_cxx_amd import fluid
    cfg = dict(PLUME_CFG, jacobiIter=9, gravityScale=0.5, vorticityConfinementAmp=AMP)
    want = _run(cfg, D, dev, "jacobi", False)
    bd = _state(D, dev)
    dt, is3d = cfg["dt"], D > 1
    g = [cfg["gravityVec"][a] for a in "xyz"]
    for _ in range(3):
        p, U, flags = bd["p"], bd["U"], bd["flags"]
        density = fluid.advectScalar(dt, bd["density"], U, flags, method="maccormackFluidNet", boundary_width=1,
                                     sample_outside_fluid=cfg["sampleOutsideFluid"], maccormack_strength=cfg["maccormackStrength"])
        U = fluid.advectVelocity(dt=dt, orig=U, U=U, flags=flags, method="maccormackFluidNet", boundary_width=1,
                                 maccormack_strength=cfg["maccormackStrength"])
        fluid.setConstVals(bd, p, U, flags, density)
        U = fluid.addBuoyancy(U, flags, density, (torch.tensor(g, dtype=torch.float32) * (-cfg["buoyancyScale"])).tolist(),
                              cfg["operatingDensity"], dt)
        U = fluid.addGravity(U, flags, (torch.tensor(g, dtype=torch.float32) * (-cfg["gravityScale"])).tolist(), dt)
        U = fluid.addVorticityConfinement(U, flags, AMP)
        U = fluid.setWallBcs(U, flags)
        fluid.setConstVals(bd, p, U, flags, density)
        div = fluid.velocityDivergence(U, flags)
        p, _ = fluid.solveLinearSystemJacobi(flags=flags, div=div, is_3d=is3d, p_tol=cfg["pTol"], max_iter=cfg["jacobiIter"])
        fluid.velocityUpdate(pressure=p, U=U, flags=flags)
        U = fluid.setWallBcs(U, flags)
        fluid.setConstVals(bd, p, U, flags, density)
        bd["U"], bd["density"], bd["p"] = U, density, p
    for k in ("U", "density", "p"):
        assert_bitexact(N(bd[k]), want[k], f"hand-assembled step D={D}: {k}")


@pytest.mark.parametrize("D", [1, 12])
def test_step_with_confinement_is_graph_capturable(dev, D):
    from fluidnet_cxx_amd import _simulate, simulate
    _simulate.release_workspaces()
    cfg = dict(PLUME_CFG, jacobiIter=9, vorticityConfinementAmp=AMP)
    a, b = _state(D, dev), _state(D, dev)
    for _ in range(2):
        simulate(cfg, a, None, "jacobi")
        simulate(cfg, b, None, "jacobi", static_flags=0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        simulate(cfg, a, None, "jacobi")
    for _ in range(3):
        g.replay()
        simulate(cfg, b, None, "jacobi", static_flags=0)
    torch.cuda.synchronize()
    for k in ("U", "density", "p"):
        assert torch.equal(a[k], b[k]), k
    _simulate.release_workspaces()


def test_step_refuses_a_window_with_the_key(dev, ext):
    """ext.simulate_step_ refuses a compute window with the key positive, as it does for 'pcg'"""
    bd = {k: T(v, dev) for k, v in plume_state(16, D=8).items()}
    with pytest.raises(RuntimeError, match="compute window or z-slab"):
        ext.simulate_step_(bd["p"], bd["U"], bd["flags"], bd["density"], None, None, None, None, None, 0.1, 0.6, False, 0.25,
                           [0.0, -1.0, 0.0], 0.0, 0.0, 1, "jacobi", 1e-5, None, 0, ext.Geom(k_begin=2, k_end=6),
                           vorticity_confinement=0.5)
