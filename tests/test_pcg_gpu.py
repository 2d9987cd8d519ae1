"""The converged pressure solve (fnx_pcg: multigrid-preconditioned CG) on the GPU against the float64 model of its operator
(tests/poisson_reference.py), and its place in simulate()."""
import numpy as np
import pytest
import torch

import poisson_reference as PR
from test_poisson_operator import case_flags
from util import PLUME_CFG, make_flags, plume_state

pytestmark = pytest.mark.gpu


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


def geom(ext, quirks):
    return ext.Geom(ref_quirks=True) if quirks else None


def active(f, is3d, quirks=False):
    return np.stack([PR.matrix(f[b, 0], is3d, quirks)[1].reshape(f.shape[2:]) for b in range(f.shape[0])])[:, None]


CASES = [((2, 1, 13, 17), False), ((2, 1, 24, 20), False), ((2, 9, 11, 7), False), ((2, 10, 12, 14), False),
         ((2, 9, 11, 7), True)]


@pytest.mark.parametrize("shape,quirks", CASES)
def test_poisson_apply_matches_model(dev, ext, shape, quirks):
    B, D, H, W = shape
    is3d = D > 1
    f = case_flags(B, D, H, W, seed=D * 100 + H)
    p = np.random.default_rng(1).standard_normal(f.shape).astype(np.float32)
    got = ext.poisson_apply(T(f, dev), T(p, dev), is3d, geom(ext, quirks)).cpu().numpy()
    want = PR.apply(f, np.where(active(f, is3d, quirks), p, 0.0), is3d, quirks)
    scale = float(np.abs(want).max())
    assert np.abs(got - want).max() <= 1e-6 * scale


# 66 x 66 (4356 cells) is above the one-workgroup limit of 4096: its finest level runs the multi-launch path (smooth / restrict /
# prolong launches, then the float4 coarse levels)
@pytest.mark.parametrize("shape,quirks", [((1, 1, 13, 17), False), ((1, 1, 12, 12), False), ((1, 7, 9, 11), False),
                                          ((1, 7, 9, 11), True), ((1, 1, 66, 66), False)])
def test_preconditioner_is_symmetric_positive_definite(dev, ext, shape, quirks):
    """M^-1 from pcg_precondition applied to the unit vectors of the active cells: symmetric and positive definite on the range of
    A (mean-zero vectors where the system is singular)."""
    B, D, H, W = shape
    is3d = D > 1
    f = case_flags(B, D, H, W, seed=11)
    A, act = PR.matrix(f[0, 0], is3d, quirks)
    ia = np.nonzero(act)[0]
    n = ia.size
    E = np.zeros((n, D * H * W), np.float32)
    E[np.arange(n), ia] = 1.0
    fl = T(np.broadcast_to(f, (n,) + f.shape[1:]), dev)
    Z = ext.pcg_precondition(fl, T(E.reshape((n, 1, D, H, W)), dev), is3d, geom(ext, quirks)).cpu().numpy()
    M = Z.reshape(n, -1)[:, ia].astype(np.float64).T
    assert np.abs(M - M.T).max() <= 1e-5 * np.abs(M).max()
    Ms = 0.5 * (M + M.T)
    if PR.is_singular(A, act):
        Q = np.eye(n) - 1.0 / n
        ev = np.linalg.eigvalsh(Q @ Ms @ Q)[1:]           # drop the null direction the projection adds
    else:
        ev = np.linalg.eigvalsh(Ms)
    assert ev.min() > 0, ev[:4]


@pytest.mark.parametrize("shape,quirks", [((1, 1, 13, 17), False), ((1, 1, 130, 130), False), ((1, 40, 40, 40), False),
                                          ((1, 40, 40, 40), True)])
def test_vcycle_matches_float64_model(dev, ext, shape, quirks):
    """one V-cycle against the float64 model of the same cycle.  130^2 and 40^3 need two levels above the one-workgroup limit (4096
    cells), so the multi-launch path runs on the level-0 code AND on a float4 Galerkin level"""
    B, D, H, W = shape
    is3d = D > 1
    f = case_flags(B, D, H, W, seed=13)
    r = np.random.default_rng(3).standard_normal(f.shape).astype(np.float32)
    z = ext.pcg_precondition(T(f, dev), T(r, dev), is3d, geom(ext, quirks)).cpu().numpy()
    want = PR.vcycle(f[0, 0], r[0, 0], is3d, quirks)
    d = np.abs(z[0, 0] - want).max()
    assert d <= 1e-4 * np.abs(want).max(), (d, np.abs(want).max())


@pytest.mark.parametrize("shape,quirks", [((2, 1, 96, 64), False), ((2, 40, 32, 24), False), ((2, 40, 32, 24), True)])
def test_solve_accuracy_against_model(dev, ext, shape, quirks):
    B, D, H, W = shape
    is3d = D > 1
    f = make_flags(B, D, H, W, boxes=True, empties=True)  # obstacles that seal no pocket: one fluid region per sample
    # sample 0: an open (non-obstacle) bottom row, Dirichlet contacts all along it; sample 1: a closed box (singular)
    f[0, 0, :, 0, 1:W - 1] = 1.0
    rng = np.random.default_rng(2)
    div = rng.standard_normal(f.shape).astype(np.float32)
    tol = 1e-5
    p, res, iters = ext.solve_linear_system_pcg(T(f, dev), T(div, dev), is3d, tol, 200, False, geom(ext, quirks))
    p = p.cpu().numpy().astype(np.float64)
    bproj = PR.project(f, div, is3d, quirks)
    pstar = PR.solve(f, div, is3d, quirks)
    act = active(f, is3d, quirks)
    assert not np.any(np.where(act, 0.0, p)), "p must be 0 off the active cells"
    assert float(res) <= tol and max(iters) <= 200, (float(res), iters)
    for b in range(B):
        r = bproj[b] - PR.apply(f[b:b + 1], p[b:b + 1], is3d, quirks)[0]
        A, a = PR.matrix(f[b, 0], is3d, quirks)
        if PR.is_singular(A, a):
            r = np.where(act[b], r - r[act[b]].mean(), 0.0)
        rel = np.linalg.norm(r) / np.linalg.norm(bproj[b])
        # 3D: <= 3e-5.  2D: the open-bottom-row sample's float64 residual of the fp32 p measured 4.2e-5 at a recurrence tolerance of
        # 1e-5 AND of 2e-6 -- a floor of the fp32 p (its rounding), not of the stopping test
        assert rel <= (3e-5 if is3d else 5e-5), (b, rel, iters)
        e = (p[b] - pstar[b]).ravel()
        if PR.is_singular(A, a):
            e = np.where(act[b].ravel(), e - e[act[b].ravel()].mean(), 0.0)
        en = np.sqrt(e @ (A @ e)) / np.sqrt(pstar[b].ravel() @ (A @ pstar[b].ravel()))
        assert en <= 1e-2, (b, en)


def test_zero_rhs_and_sealed_pocket(dev, ext):
    """div = 0 returns exact zeros; a fluid pocket sealed inside obstacles (a second null vector) stops unconverged with finite output"""
    B, D, H, W = 2, 1, 40, 48
    f = make_flags(B, D, H, W, boxes=False)
    f[1, 0, 0, 10:20, 10:20] = 2.0
    f[1, 0, 0, 12:18, 12:18] = 1.0                         # the pocket: fluid cells enclosed by obstacles
    rng = np.random.default_rng(4)
    div = rng.standard_normal(f.shape).astype(np.float32)
    div[0] = 0.0
    p, res, iters = ext.solve_linear_system_pcg(T(f, dev), T(div, dev), False, 1e-5, 40, False, None)
    p = p.cpu().numpy()
    assert not np.any(p[0]) and iters[0] == 0
    assert np.isfinite(p[1]).all()
    assert 0 < iters[1] <= 40 and float(res) > 1e-5, (iters, float(res))   # stopped (max_iter or diverging) unconverged


def _plume_dev(res, D, dev, steps, method="jacobi"):
    from fluidnet_cxx_amd import simulate
    st = plume_state(res, D=D)
    bd = {k: T(v, dev) for k, v in st.items()}
    for _ in range(steps):
        simulate(PLUME_CFG, bd, None, method)
    return bd


@pytest.mark.parametrize("res,D,bound", [(128, 1, 20), (1024, 1, 20), (128, 128, 30), (256, 256, 30)])
def test_iteration_counts_on_plume_states(dev, ext, res, D, bound):
    from fluidnet_cxx_amd import fluid
    bd = _plume_dev(res, D, dev, 4)
    is3d = D > 1
    div = fluid.velocityDivergence(bd["U"], bd["flags"])
    p, r, iters = ext.solve_linear_system_pcg(bd["flags"], div, is3d, 1e-5, 100, False, None)
    msg = f"PCG iterations to 1e-5 at {res}^{3 if is3d else 2}: {iters} (recurrence residual {float(r):.2e})"
    if not is3d:
        # the float64 residual of the fp32 p, on the projected div (the plume box is closed: singular), against what storing p in
        # fp32 alone costs: |A| |p| u (u = 2^-24) bounds A times the rounding error of p componentwise.  The plume's source is
        # concentrated, so |p| is ~1e4 |div| at 1024^2 and that floor is far above 1e-5
        f = bd["flags"].cpu().numpy()
        pn = p.cpu().numpy().astype(np.float64)
        b = PR.project(f, div.cpu().numpy(), False)
        act = active(f, False)
        rt = b - PR.apply(f, pn, False)
        rt = np.where(act, rt - rt[act].mean(), 0.0)
        A, _ = PR.matrix(f[0, 0], False)
        floor = 2.0 ** -24 * np.linalg.norm(abs(A) @ np.abs(pn[0, 0]).ravel()) / np.linalg.norm(b)
        true = np.linalg.norm(rt) / np.linalg.norm(b)
        msg += f", float64 residual {true:.2e} (fp32 rounding floor of p {floor:.2e})"
    print(msg)
    assert iters[0] <= bound and float(r) <= 1e-5, msg
    if not is3d:
        assert true <= 1e-5 + 8 * floor, msg


@pytest.mark.parametrize("D", [1, 24])
def test_projection_removes_divergence(dev, ext, D):
    from fluidnet_cxx_amd import fluid
    res = 64
    bd = _plume_dev(res, D, dev, 3)
    is3d = D > 1
    U0 = bd["U"].clone()
    fluid.setWallBcs(U0, bd["flags"])
    div0 = fluid.velocityDivergence(U0, bd["flags"])
    f = bd["flags"].cpu().numpy()
    act = active(f, is3d)
    A, a = PR.matrix(f[0, 0], is3d)
    sing = PR.is_singular(A, a)

    def norm(div):
        d = div.cpu().numpy().astype(np.float64)
        d = np.where(act, d, 0.0)
        if sing:
            d = np.where(act, d - d[act].mean(), 0.0)
        return np.linalg.norm(d)

    out = {}
    for name, solve in (("pcg", lambda d: fluid.solveLinearSystemPCG(bd["flags"], d, is3d, 1e-5, 100)),
                        ("jacobi28", lambda d: fluid.solveLinearSystemJacobi(bd["flags"], d, is3d, 0.0, 28))):
        U = U0.clone()
        p, _ = solve(div0)
        fluid.velocityUpdate(p, U, bd["flags"])
        fluid.setWallBcs(U, bd["flags"])
        out[name] = norm(fluid.velocityDivergence(U, bd["flags"])) / norm(div0)
    print("remaining divergence:", out)
    assert out["pcg"] <= 2e-5, out
    assert out["jacobi28"] >= 100 * out["pcg"], out


@pytest.mark.parametrize("D", [1, 12])
def test_simulate_pcg_fused_unfused_repeatable(dev, ext, D):
    from fluidnet_cxx_amd import _simulate, simulate
    cfg = dict(PLUME_CFG, pcgTol=1e-5, pcgIter=60)
    res = 40
    runs = []
    for fused in (True, True, False):
        _simulate.release_workspaces()
        st = plume_state(res, D=D)
        bd = {k: T(v, dev) for k, v in st.items()}
        for step in range(4):
            if step == 2:                                  # an obstacle inserted in place between steps
                bd["flags"][:, :, :, 20:24, 14:18] = 2.0
            simulate(cfg, bd, None, "pcg", fused=fused)
        runs.append({k: bd[k].cpu().numpy() for k in ("U", "density", "p")})
    for k in ("U", "density", "p"):
        assert np.array_equal(runs[0][k].view(np.int32), runs[1][k].view(np.int32)), k
        assert np.array_equal(runs[0][k].view(np.int32), runs[2][k].view(np.int32)), k
    # an explicit fresh workspace each step (no reuse) gives the same bits as the automatic mode with its in-place obstacle
    st = plume_state(res, D=D)
    bd = {k: T(v, dev) for k, v in st.items()}
    for step in range(4):
        if step == 2:
            bd["flags"][:, :, :, 20:24, 14:18] = 2.0
        ws = torch.empty(ext.step_workspace_bytes(1, D, res, res, D > 1), dtype=torch.uint8, device=dev)
        simulate(cfg, bd, None, "pcg", workspace=ws, static_flags=0)
    for k in ("U", "density", "p"):
        assert np.array_equal(runs[0][k].view(np.int32), bd[k].cpu().numpy().view(np.int32)), k
    _simulate.release_workspaces()


def test_pcg_step_is_graph_capturable(dev):
    from fluidnet_cxx_amd import _simulate, simulate
    _simulate.release_workspaces()
    cfg = dict(PLUME_CFG, pcgTol=0.0, pcgIter=12)
    res = 48
    a = {k: T(v, dev) for k, v in plume_state(res).items()}
    b = {k: T(v, dev) for k, v in plume_state(res).items()}
    for _ in range(2):
        simulate(cfg, a, None, "pcg")
        simulate(cfg, b, None, "pcg", static_flags=0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        simulate(cfg, a, None, "pcg")
    for _ in range(3):
        g.replay()
        simulate(cfg, b, None, "pcg", static_flags=0)
    torch.cuda.synchronize()
    for k in ("U", "density", "p"):
        assert torch.equal(a[k], b[k]), k
    _simulate.release_workspaces()


def test_argument_errors(dev, ext):
    from fluidnet_cxx_amd import fluid
    f = T(make_flags(1, 8, 10, 12), dev)
    div = torch.zeros_like(f)
    with pytest.raises(RuntimeError, match="iteration"):
        ext.solve_linear_system_pcg(f, div, True, 1e-5, 0, False, None)
    with pytest.raises(RuntimeError, match="compute window|z-slab"):
        ext.solve_linear_system_pcg(f, div, True, 1e-5, 10, False, ext.Geom(k_begin=1, k_end=5))
    with pytest.raises(RuntimeError, match="mismatch"):
        ext.solve_linear_system_pcg(f, torch.zeros(1, 1, 8, 10, 11, device=dev), True, 1e-5, 10, False, None)
    with pytest.raises(AssertionError):
        fluid.solveLinearSystemPCG(f, torch.zeros(1, 8, 10, 12, device=dev), True)
    st = plume_state(16, D=8)
    bd = {k: T(v, dev) for k, v in st.items()}
    with pytest.raises(RuntimeError, match="compute window|z-slab"):
        ext.simulate_step_(bd["p"], bd["U"], bd["flags"], bd["density"], None, None, None, None, None, 0.1, 0.6, False, 0.25,
                           [0.0, -1.0, 0.0], 0.0, 0.0, 1, "pcg", 1e-5, None, 0, ext.Geom(k_begin=2, k_end=6))
    drv = ext.SlabDriver(1, 16, 16, 8, 0, 1, 5, 5)
    o, lo, hi, _ = drv.layout()
    D = o + lo + hi
    z = lambda c: torch.zeros(1, c, D, 16, 16, device=dev)
    fl = torch.ones(1, 1, D, 16, 16, device=dev)
    ws = torch.empty(drv.workspace_bytes(), dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="PCG"):
        drv.step(z(1), z(3), fl, z(1), None, None, None, None, 0.1, 0.6, False, 0.25, [0.0, -1.0, 0.0], 0.0, 0.0, 4, ws,
                 method="pcg")
