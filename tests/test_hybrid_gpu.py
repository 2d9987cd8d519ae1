"""simulate(..., 'hybrid') -- the converged solve started from the net's pressure -- and 'pcg' started from the previous step's
pressure (mconf['pcgWarmStart']) on the GPU: the fused step against the operator path bit for bit, the cold step's bits where the guess
is rejected, the divergence the projection leaves, graph capture, and training.hybrid_iterations."""
import numpy as np
import pytest
import torch

import poisson_reference as PR
from util import PLUME_CFG, plume_state

pytestmark = pytest.mark.gpu

CFG = dict(PLUME_CFG, pcgTol=1e-5, pcgIter=60)
KEYS = ("U", "density", "p")


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


def make_net(D, dev, zero=False):
    """FluidNet with its deterministic default weights (or every weight and bias zero)"""
    from fluidnet_cxx_amd import FluidNet
    net = FluidNet(dict(CFG, is3D=D > 1, inputDim=3 if D > 1 else 2), dropout=False)
    if zero:
        net.load_state_dict({k: torch.zeros_like(v) for k, v in net.state_dict().items()})
    return net.to(dev).eval()


def run_plume(dev, res, D, method, net, cfg=CFG, steps=4, obstacle=True, **kw):
    from fluidnet_cxx_amd import simulate
    bd = {k: T(v, dev) for k, v in plume_state(res, D=D).items()}
    for step in range(steps):
        if obstacle and step == 2:                          # an obstacle inserted in place between steps
            bd["flags"][:, :, :, 20:24, 14:18] = 2.0
        simulate(cfg, bd, net, method, **kw)
    return {k: bd[k].cpu().numpy() for k in KEYS}


def same_bits(a, b, what=""):
    for k in KEYS:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), (what, k)


# ---- 6. fused, fused again, operator path, fresh workspaces --------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 12])
def test_hybrid_fused_unfused_repeatable(dev, ext, D):
    from fluidnet_cxx_amd import _simulate, simulate
    res = 40
    net = make_net(D, dev)
    runs = []
    for fused in (True, True, False):
        _simulate.release_workspaces()
        runs.append(run_plume(dev, res, D, "hybrid", net, fused=fused))
    assert np.abs(runs[0]["p"]).max() > 0 and np.isfinite(runs[0]["U"]).all()
    same_bits(runs[0], runs[1], "fused twice")
    same_bits(runs[0], runs[2], "fused / operator path")
    # an explicit fresh workspace each step (no reuse) gives the same bits as the automatic mode with its in-place obstacle
    bd = {k: T(v, dev) for k, v in plume_state(res, D=D).items()}
    for step in range(4):
        if step == 2:
            bd["flags"][:, :, :, 20:24, 14:18] = 2.0
        ws = torch.empty(ext.step_workspace_bytes(1, D, res, res, D > 1), dtype=torch.uint8, device=dev)
        simulate(CFG, bd, net, "hybrid", workspace=ws, static_flags=0)
    same_bits(runs[0], {k: bd[k].cpu().numpy() for k in KEYS}, "fresh workspaces")
    # the guess is used: the step is not the cold one
    cold = run_plume(dev, res, D, "pcg", None)
    assert not np.array_equal(runs[0]["p"].view(np.int32), cold["p"].view(np.int32))
    _simulate.release_workspaces()


# ---- 7. a zero net: the guess is rejected, the step is the 'pcg' step ------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 12])
@pytest.mark.parametrize("fused", [True, False])
def test_zero_net_is_the_pcg_step(dev, D, fused):
    from fluidnet_cxx_amd import _simulate
    _simulate.release_workspaces()
    hyb = run_plume(dev, 40, D, "hybrid", make_net(D, dev, zero=True), fused=fused)
    _simulate.release_workspaces()
    pcg = run_plume(dev, 40, D, "pcg", None, fused=fused)
    same_bits(hyb, pcg)
    _simulate.release_workspaces()


# ---- 8. / 9. what the projection leaves -----------------------------------------------------------------------------------------------
def divergence_norm(flags, is3d):
    f = flags.cpu().numpy()
    A, a = PR.matrix(f[0, 0], is3d)
    act = a.reshape(f.shape[2:])[None, None]
    sing = PR.is_singular(A, a)

    def norm(div):
        d = np.where(act, div.cpu().numpy().astype(np.float64), 0.0)
        if sing:
            d = np.where(act, d - d[act].mean(), 0.0)
        return np.linalg.norm(d)
    return norm


def staged(fluid, cfg, bd):
    """the stages of simulate()'s operator path in front of the projection (the plume configuration: advection, setConstVals, buoyancy,
    setWallBcs, setConstVals) on copies: the fields the projection starts from"""
    p, U, flags = bd["p"].clone(), bd["U"].clone(), bd["flags"]
    tmp = dict(bd)
    dt = cfg["dt"]
    rho = fluid.advectScalar(dt, bd["density"], U, flags, method="maccormackFluidNet", boundary_width=1,
                             sample_outside_fluid=cfg["sampleOutsideFluid"], maccormack_strength=cfg["maccormackStrength"])
    U = fluid.advectVelocity(dt=dt, orig=U, U=U, flags=flags, method="maccormackFluidNet", boundary_width=1,
                             maccormack_strength=cfg["maccormackStrength"])
    fluid.setConstVals(tmp, p, U, flags, rho)
    g = cfg["gravityVec"]
    U = fluid.addBuoyancy(U, flags, rho, [-cfg["buoyancyScale"] * g[a] for a in ("x", "y", "z")], cfg["operatingDensity"], dt)
    U = fluid.setWallBcs(U, flags)
    fluid.setConstVals(tmp, p, U, flags, rho)
    return dict(U=U, flags=flags)


def remaining_divergence(fluid, bd, is3d, norm, p0):
    """(what solveLinearSystemPCG(p0=p0), velocityUpdate and setWallBcs leave of the divergence of setWallBcs(U), iterations, p)"""
    from fluidnet_cxx_amd._ext import ext
    U = bd["U"].clone()
    fluid.setWallBcs(U, bd["flags"])
    div0 = fluid.velocityDivergence(U, bd["flags"])
    p, _, iters = ext.solve_linear_system_pcg(bd["flags"], div0, is3d, 1e-5, 100, False, None, p0=p0)
    fluid.velocityUpdate(p, U, bd["flags"])
    fluid.setWallBcs(U, bd["flags"])
    return norm(fluid.velocityDivergence(U, bd["flags"])) / norm(div0), iters, p


@pytest.mark.parametrize("D", [1, 24])
def test_hybrid_projection_removes_divergence(dev, D):
    from fluidnet_cxx_amd import fluid, simulate
    res, is3d = 64, D > 1
    bd = {k: T(v, dev) for k, v in plume_state(res, D=D).items()}
    for _ in range(3):
        simulate(PLUME_CFG, bd, None, "jacobi")
    net = make_net(D, dev)
    U0 = bd["U"].clone()
    fluid.setWallBcs(U0, bd["flags"])
    p0, _ = net(torch.cat((bd["p"], U0, bd["flags"], bd["density"]), 1))
    norm = divergence_norm(bd["flags"], is3d)
    left, iters, _ = remaining_divergence(fluid, bd, is3d, norm, p0)
    _, cold, _ = remaining_divergence(fluid, bd, is3d, norm, None)
    print(f"remaining divergence from the net's pressure: {left:.3e} after {iters} iterations (cold: {cold})")
    assert left <= 2e-5, left


@pytest.mark.parametrize("D", [1, 12])
def test_temporal_warm_start(dev, D):
    from fluidnet_cxx_amd import _simulate, fluid, simulate
    res, is3d = 40, D > 1
    warm_cfg = dict(CFG, pcgWarmStart=True)
    _simulate.release_workspaces()
    # the first step from p = 0 is the cold step
    first_cold = run_plume(dev, res, D, "pcg", None, steps=1)
    first_warm = run_plume(dev, res, D, "pcg", None, cfg=warm_cfg, steps=1)
    same_bits(first_cold, first_warm, "first step")
    runs = [run_plume(dev, res, D, "pcg", None, cfg=warm_cfg, fused=fused) for fused in (True, False)]
    same_bits(runs[0], runs[1], "fused / operator path")
    assert not np.array_equal(runs[0]["p"].view(np.int32), run_plume(dev, res, D, "pcg", None)["p"].view(np.int32)), "the guess is used"
    # every step's projection, at the operator level: the bound of the cold solve, and the two iteration counts
    bd = {k: T(v, dev) for k, v in plume_state(res, D=D).items()}
    counts = []
    for step in range(4):
        if step == 2:
            bd["flags"][:, :, :, 20:24, 14:18] = 2.0
        before = staged(fluid, warm_cfg, bd)
        norm = divergence_norm(bd["flags"], is3d)
        left, warm, _ = remaining_divergence(fluid, before, is3d, norm, bd["p"])
        _, cold, _ = remaining_divergence(fluid, before, is3d, norm, None)
        counts.append((cold[0], warm[0]))
        assert left <= 2e-5, (step, left)
        simulate(warm_cfg, bd, None, "pcg")
    print(f"D = {D}: (cold, warm) iterations per step: {counts}")
    _simulate.release_workspaces()


# ---- 10. graph capture ----------------------------------------------------------------------------------------------------------------
def test_hybrid_step_is_graph_capturable(dev):
    from fluidnet_cxx_amd import _simulate, simulate
    _simulate.release_workspaces()
    cfg = dict(PLUME_CFG, pcgTol=0.0, pcgIter=6)
    res = 48
    net = make_net(1, dev)
    a = {k: T(v, dev) for k, v in plume_state(res).items()}
    b = {k: T(v, dev) for k, v in plume_state(res).items()}
    for _ in range(2):
        simulate(cfg, a, net, "hybrid")
        simulate(cfg, b, net, "hybrid", static_flags=0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        simulate(cfg, a, net, "hybrid")
    for _ in range(3):
        g.replay()
        simulate(cfg, b, net, "hybrid", static_flags=0)
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    _simulate.release_workspaces()


# ---- 11. the figure of merit for trained nets -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(32, 32), (16, 16, 16)])
def test_hybrid_iterations(dev, dims):
    from fluidnet_cxx_amd import FluidNet, training, training3d
    B, is3d = 2, len(dims) == 3
    if is3d:
        mconf = dict(training3d.MCONF3D_DEFAULTS)
        sampler = training3d.SceneSampler3D(mconf, B, dims[0], dims[1], dims[2], 5, dev)
    else:
        mconf = dict(training.MCONF_DEFAULTS)
        sampler = training.SceneSampler(mconf, B, dims[0], dims[1], 5, dev)
    batches = [sampler.next() for _ in range(2)]
    net = FluidNet(mconf, dropout=False).to(dev).eval()
    cold, warm = training.hybrid_iterations(net, batches)
    print(f"{dims}: cold {cold}, warm {warm}")
    assert isinstance(cold, list) and isinstance(warm, list) and len(cold) == len(warm) == B * len(batches)
    assert all(isinstance(n, int) and 0 < n <= 100 for n in cold) and all(isinstance(n, int) and 0 <= n <= 100 for n in warm)
    zero = FluidNet(mconf, dropout=False)
    zero.load_state_dict({k: torch.zeros_like(v) for k, v in zero.state_dict().items()})
    cold0, warm0 = training.hybrid_iterations(zero.to(dev).eval(), batches, tol=1e-5, max_iter=100)
    assert cold0 == cold and warm0 == cold
