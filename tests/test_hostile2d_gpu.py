"""The 2D kernels on hostile geometries (tests/hostile2d_cases.py): Fluid and Empty cells on the domain border -- rays that leave the
domain (case 1 of the line trace) in the per-cell advection kernels, the LDS tile kernels (fast path and fallback lanes), the
advect_step pair and advect_scalars; the MacCormack correction on fluid border cells -- scattered Obstacle / Empty cells (every
adjacency in both axes) and samples of a batch whose flags differ (a kernel that indexed flags without the sample offset).

  a. the reference's goldens on the six 2 x 19 x 37 states (hostile2d.npz / hostile2d_hi.npz): every operator, bit for bit
  b. larger shapes that cross one, two and four 64-column tiles with partial tiles in x and y, against the oracle
  c. the temporally blocked Jacobi, jacobi_sweeps_ from zero and the residual
  d. the adjoints of divergence and velocityUpdate, and autograd through the native operators against the reference's autograd
  e. whole steps: the reference's goldens (hostile2d_sim.npz) fused and unfused in the four-argument automatic mode, vorticity
     confinement, passive scalars, 'pcg' / 'hybrid' / 'convnet', fluidnet_forward
  f. the PCG pieces against poisson_reference
test_hostile2d_reference.py (CPU) shows that the oracle has the reference's bits on all of it and that the states meet their conditions.
Everything is bit-exact except where a tolerance is written at the assert (the forms of the existing tests).
Tried on a scratch build: with the MacCormack correction of advectScalar skipped on border cells (per-cell kernel, 2D tile kernel and
advectScalars) 35 of the 62 tests of this file fail -- every golden, advection and whole-step case on an open state -- while the advection,
golden and plume tests of test_parity_gpu.py all still pass."""
import functools

import numpy as np
import pytest
import torch

import hostile2d_cases as HC
import poisson_reference as PR
import vorticity_reference as VR
from util import F2_CFG, PLUME_CFG, assert_bitexact, assert_close, assert_close_rel, plume_state

pytestmark = pytest.mark.gpu
MAC, EULER = "maccormackFluidNet", "eulerFluidNet"
LARGE_SHAPES = HC.LARGE_SHAPES
NET_CFG = dict(PLUME_CFG, model="ScaleNet", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True,
               normalizeInputChan="UDiv", is3D=False)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fl():
    from fluidnet_cxx_amd import fluid
    return fluid


@pytest.fixture(scope="module")
def ext():
    from fluidnet_cxx_amd._ext import ext
    return ext


def T(x, dev):
    return torch.from_numpy(np.array(x, np.float32)).to(dev)            # (a copy: the shared states are read-only)


def N(t):
    return t.detach().cpu().numpy()


def to_dev(st, dev):
    return {k: T(v, dev) for k, v in st.items()}


# ---- a. the reference's goldens ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HC.GOLDEN_STATES))
def test_ops_vs_reference_golden(fl, dev, golden, name):
    from test_parity_gpu import run_ops
    z = HC.golden_arrays(golden, name)
    dt = float(z["dt"])
    out = run_ops(fl, dev, z["flags"], z["U"], z["rho"], z["p"], dt, z["gravity"].tolist(), float(z["rho_star"]), False, z["orig"],
                  int(z["jacobi_iters"]))
    tf, tU = T(z["flags"], dev), T(z["U"], dev)
    assert float(z["viscosity"]) == 0.07       # what run_ops passes to addViscosity
    Uv = tU.clone(); fl.addViscosity(0.1, Uv, tf, 0.05); out["add_viscosity_dt0p1_nu0p05"] = N(Uv)     # the double product, rounded once
    Us = tU.clone(); assert fl.setWallBcsStick(Us, tf, T(z["flags_stick"], dev)) is None; out["set_wall_bcs_stick"] = N(Us)
    for k, v in out.items():
        if k.endswith("_res"):
            assert abs(v - float(z[k])) <= 1e-5 * max(1.0, float(z[k])), (k, v, float(z[k]))   # reduction order differs
        else:
            assert_bitexact(v, z[k], f"{name}:{k}")
    assert set(out) >= {"advect_vel_orig", "add_viscosity", "set_wall_bcs_stick", "jacobi_p", "jacobi1_p", "occupancy"}
    for b in range(z["flags"].shape[0]):       # the tolerance exit, sample by sample (the reference's B > 1 solve mixes samples)
        pj, _ = fl.solveLinearSystemJacobi(tf[b:b + 1].contiguous(), T(z["divergence"][b:b + 1], dev), False, float(z["jacobi_tol"][b]), 50)
        assert_bitexact(N(pj), z["jacobi_tol_p"][b:b + 1], f"{name}: jacobi p_tol early exit, sample {b}")


# ---- b. larger shapes against the oracle -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _advection_reference(case):
    """the oracle on one state, computed once and never modified"""
    from oracle import oracle as O
    O.build()
    s = HC.state(*case)
    dt, rho, U, f = s["dt"], s["rho"], s["U"], s["flags"]
    o = {}
    for m in (MAC, EULER):
        for so in (False, True):
            o["scalar", m, so] = O.advect_scalar(dt, rho, U, f, m, 1, so, 0.6)
        o["vel", m] = O.advect_vel(dt, U, U, f, m, 1, 0.6)
    o["vel_orig"] = O.advect_vel(dt, s["orig"], U, f, MAC, 1, 0.6)
    rng = np.random.default_rng(5)
    o["src3"] = np.concatenate([rho, rng.random(rho.shape).astype(np.float32), rng.standard_normal(rho.shape).astype(np.float32)], 1)
    for so in (False, True):
        o["scalars", so] = np.concatenate([O.advect_scalar(dt, o["src3"][:, c:c + 1], U, f, MAC, 1, so, 0.6) for c in range(3)], 1)
    for v in o.values():
        v.setflags(write=False)
    return o


@pytest.mark.parametrize("cfl", list(HC.CFLS.values()))
@pytest.mark.parametrize("kind", HC.KINDS)
@pytest.mark.parametrize("shape", LARGE_SHAPES)
def test_advection_vs_oracle(fl, ext, dev, shape, kind, cfl):
    case = (kind, *shape, cfl, HC.LARGE_SEED)
    s, want = HC.state(*case), _advection_reference(case)
    dt = s["dt"]
    tf, tU, trho = T(s["flags"], dev), T(s["U"], dev), T(s["rho"], dev)
    for so in (False, True):
        for plan in ("tiles", "cells", "auto"):
            r, u = ext.advect_step(dt, trho, tU, tf, so, 0.6, plan=plan)
            assert_bitexact(N(r), want["scalar", MAC, so], f"advect_step density so={so} plan={plan}")
            assert_bitexact(N(u), want["vel", MAC], f"advect_step U so={so} plan={plan}")
        for plan in ("tiles", "cells"):
            for m in (MAC, EULER):
                assert_bitexact(N(fl.advectScalar(dt, trho, tU, tf, m, 1, so, 0.6, plan=plan)), want["scalar", m, so], f"advectScalar {m} so={so} plan={plan}")
        assert_bitexact(N(fl.advectScalars(dt, T(want["src3"], dev), tU, tf, MAC, 1, so, 0.6)), want["scalars", so], f"advectScalars so={so}")
    for plan in ("tiles", "cells"):
        for m in (MAC, EULER):
            assert_bitexact(N(fl.advectVelocity(dt, tU, tU, tf, m, 1, 0.6, plan=plan)), want["vel", m], f"advectVelocity {m} plan={plan}")
        assert_bitexact(N(fl.advectVelocity(dt, T(s["orig"], dev), tU, tf, MAC, 1, 0.6, plan=plan)), want["vel_orig"], f"orig != U plan={plan}")
    assert_bitexact(N(tU), s["U"], "U unchanged"); assert_bitexact(N(trho), s["rho"], "rho unchanged"); assert_bitexact(N(tf), s["flags"], "flags unchanged")


@pytest.mark.parametrize("kind", HC.KINDS)
@pytest.mark.parametrize("shape", LARGE_SHAPES)
def test_one_signed_velocity_vs_oracle(fl, ext, dev, oracle, shape, kind):
    """|U| and -|U| at cfl 6.2: every forward trace goes towards one corner and every backward trace away from it, so the rays of a pass
    leave through the two sides that face one corner (test_conditions_one_signed_states counts them), and the tile loader's chunks hang
    over the tensors' ends there"""
    s = HC.state(kind, *shape, 6.2, HC.LARGE_SEED)
    dt, tf, trho = s["dt"], T(s["flags"], dev), T(s["rho"], dev)
    for sign in (-1.0, 1.0):
        Un = HC.one_signed(s["U"], sign)
        tUn = T(Un, dev)
        want_r = oracle.advect_scalar(dt, s["rho"], Un, s["flags"], MAC, 1, False, 0.6)
        want_u = oracle.advect_vel(dt, Un, Un, s["flags"], MAC, 1, 0.6)
        for plan in ("tiles", "cells"):
            r, u = ext.advect_step(dt, trho, tUn, tf, False, 0.6, plan=plan)
            assert_bitexact(N(r), want_r, f"advect_step density, sign {sign}, {plan}"); assert_bitexact(N(u), want_u, f"advect_step U, sign {sign}, {plan}")
            assert_bitexact(N(fl.advectScalar(dt, trho, tUn, tf, MAC, 1, False, 0.6, plan=plan)), want_r, f"advectScalar, sign {sign}, {plan}")
            assert_bitexact(N(fl.advectVelocity(dt, tUn, tUn, tf, MAC, 1, 0.6, plan=plan)), want_u, f"advectVelocity, sign {sign}, {plan}")


# ---- c. Jacobi ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["open4", "salt"])
def test_jacobi_sweep_counts(fl, ext, dev, oracle, kind):
    s = HC.state(kind, *HC.JACOBI_SHAPE, 0.6, HC.LARGE_SEED)
    B, H, W = HC.JACOBI_SHAPE
    flags = s["flags"]
    div = oracle.velocity_divergence(s["U"], flags)
    tf, td = T(flags, dev), T(div, dev)
    assert_bitexact(N(fl.velocityDivergence(T(s["U"], dev), tf)), div, "divergence")
    ws = torch.empty(ext.jacobi_workspace_bytes(B, 1, H, W, False), dtype=torch.uint8, device=dev)
    for n in (1, 2, 7, 8, 9, 28):
        po, ro, _ = oracle.jacobi(flags, div, False, 0.0, n)
        runs = [fl.solveLinearSystemJacobi(tf, td, False, 0.0, n) for _ in range(2)]
        for pj, res in runs:
            assert_bitexact(N(pj), po, f"jacobi {n} sweeps")
        assert float(runs[0][1]) == float(runs[1][1]), "the residual differs between two runs of the same solve"
        assert abs(float(runs[0][1]) - ro) <= 2e-6 * max(ro, 1e-30), (n, float(runs[0][1]), ro)
        p = torch.full((B, 1, 1, H, W), float("nan"), device=dev)
        ext.jacobi_sweeps_(tf, td, p, False, n, ws, False, from_zero=True)
        assert_bitexact(N(p), po, f"jacobi_sweeps_ from zero, {n} sweeps")


# ---- d. adjoints -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["open4", "salt"])
def test_adjoints_vs_oracle_and_dot_product(fl, ext, dev, oracle, kind):
    B, H, W = HC.ADJOINT_SHAPE
    flags_np = HC.state(kind, B, H, W, 0.6, HC.LARGE_SEED)["flags"]
    flags = T(flags_np, dev)
    rng = np.random.default_rng(8)
    gd = rng.standard_normal((B, 1, 1, H, W)).astype(np.float32)
    gu = rng.standard_normal((B, 2, 1, H, W)).astype(np.float32)
    a = N(ext.velocity_divergence_backward(T(gd, dev), flags, False, None))
    assert_bitexact(a, oracle.velocity_divergence_backward(gd, flags_np, False), "divergence adjoint")
    gU, gp = ext.velocity_update_backward(T(gu, dev), flags, None)
    oU, op = oracle.velocity_update_backward(gu, flags_np)
    assert_bitexact(N(gU), oU, "velocityUpdate adjoint (U)")
    assert_bitexact(N(gp), op, "velocityUpdate adjoint (p)")
    x = T(rng.standard_normal((B, 2, 1, H, W)), dev)
    Jx = fl.velocityDivergence(x, flags).double()
    lhs = float((Jx * T(gd, dev).double()).sum())
    rhs = float((x.double() * T(a, dev).double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), 1.0), (lhs, rhs)
    pr = T(rng.standard_normal((B, 1, 1, H, W)), dev)
    Ux = x.clone()
    fl.velocityUpdate(pr, Ux, flags)
    lhs = float((Ux.double() * T(gu, dev).double()).sum())
    rhs = float((x.double() * gU.double()).sum() + (pr.double() * gp.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), 1.0), (lhs, rhs)


@pytest.mark.parametrize("kind", ["open4", "salt"])
def test_autograd_vs_reference_autograd(fl, dev, golden, kind):
    z, tag = golden("hostile2d"), f"grad_{kind}"
    G = lambda k: T(z[f"{tag}_{k}"], dev)
    flags = G("flags")
    U0 = G("U").requires_grad_(True)
    p = G("p").requires_grad_(True)
    U = U0 * 1.0
    assert fl.velocityUpdate(pressure=p, U=U, flags=flags) is None
    U = fl.setWallBcs(U, flags)
    div = fl.velocityDivergence(U.contiguous(), flags)
    ((div * G("wd")).sum() + (U * G("wu")).sum()).backward()
    assert_bitexact(N(U), z[f"{tag}_U_out"], "U")
    assert_bitexact(N(div), z[f"{tag}_div"], "div")
    assert_close_rel(N(U0.grad), z[f"{tag}_grad_U"], 1e-6, "grad U")
    assert_close_rel(N(p.grad), z[f"{tag}_grad_p"], 1e-6, "grad p")


# ---- e. whole steps ----------------------------------------------------------------------------------------------------------
def _sim_state(kind):
    return HC.sim_state(kind, plume_state(HC.SIM_RES))


def _run(dev, kind, cfg, method, net=None, steps=4, fused=True, extra=None, keep=()):
    """`steps` steps in the four-argument automatic mode (the class map is built on step 2 and reused from step 3)"""
    from fluidnet_cxx_amd import _simulate, simulate
    _simulate.release_workspaces()
    bd = to_dev(dict(_sim_state(kind), **(extra or {})), dev)
    out = {}
    for it in range(1, steps + 1):
        simulate(cfg, bd, net, method, fused=fused)
        if it in keep or it == steps:
            out[it] = {k: N(bd[k]) for k in ("U", "density", "p") + (("scalars",) if "scalars" in bd else ())}
    _simulate.release_workspaces()
    return out


def _same_bits(a, b, what):
    for k in ("U", "density", "p"):
        assert_bitexact(a[k], b[k], f"{what}: {k}")


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("cfgname,extra", [("plain", {}), ("f2", F2_CFG)])
@pytest.mark.parametrize("kind", HC.SIM_KINDS)
def test_whole_steps_vs_reference(dev, golden, kind, cfgname, extra, fused):
    z = golden("hostile2d_sim")
    got = _run(dev, kind, dict(PLUME_CFG, **extra), "jacobi", fused=fused, keep=(1, 4))
    for it in (1, 4):
        for k in ("U", "density", "p"):
            assert_bitexact(got[it][k], z[f"{kind}_{cfgname}_{k}_{it}"], f"{kind} {cfgname} fused={fused}: {k} after {it} steps")


@pytest.mark.parametrize("kind", HC.SIM_KINDS)
def test_vorticity_confinement_on_open_borders(dev, ext, kind):
    st = _sim_state(kind)
    tU, tf = T(st["U"], dev), T(st["flags"], dev)
    want = VR.confine(st["U"], st["flags"], 0.3)
    assert (want != st["U"]).any()
    assert_bitexact(N(ext.add_vorticity_confinement(tU, tf, 0.3, None)), want, "addVorticityConfinement vs vorticity_reference")
    cfg = dict(PLUME_CFG, vorticityConfinementAmp=0.3)
    a, b = _run(dev, kind, cfg, "jacobi", fused=True), _run(dev, kind, cfg, "jacobi", fused=False)
    _same_bits(a[4], b[4], f"{kind}: confinement, fused vs operator path")
    assert np.isfinite(a[4]["U"]).all()


@pytest.mark.parametrize("kind", HC.SIM_KINDS)
def test_scalars_on_open_borders(dev, kind):
    """two channels, channel 0 a copy of the density with the density's BC arrays: it stays the density, the flow does not see the key"""
    st = _sim_state(kind)
    other = np.random.default_rng(2).random(st["density"].shape).astype(np.float32)
    extra = dict(scalars=np.concatenate([st["density"], other], 1), scalarsBC=np.concatenate([st["densityBC"], np.zeros_like(other)], 1),
                 scalarsBCInvMask=np.concatenate([st["densityBCInvMask"], np.ones_like(other)], 1))
    plain = _run(dev, kind, PLUME_CFG, "jacobi", fused=True)
    for fused in (True, False):
        got = _run(dev, kind, PLUME_CFG, "jacobi", fused=fused, extra=extra)
        _same_bits(got[4], plain[4], f"{kind} fused={fused}: with and without the key")
        assert_bitexact(got[4]["scalars"][:, 0:1], got[4]["density"], f"{kind} fused={fused}: channel 0 vs density")
        assert (got[4]["scalars"][:, 1:] != other).mean() > 0.2, "the other channel moved"


def _zero_net(dev):
    from fluidnet_cxx_amd import FluidNet
    net = FluidNet(dict(PLUME_CFG, pcgTol=1e-5, pcgIter=60, is3D=False, inputDim=2), dropout=False)
    net.load_state_dict({k: torch.zeros_like(v) for k, v in net.state_dict().items()})
    return net.to(dev).eval()


@pytest.mark.parametrize("kind", HC.SIM_KINDS)
def test_pcg_and_hybrid_on_open_borders(dev, kind):
    """'pcg' fused against the operator path, and 'hybrid' with a zero net (the guess is rejected) is the 'pcg' step: same bits"""
    cfg = dict(PLUME_CFG, pcgTol=1e-5, pcgIter=60)
    net = _zero_net(dev)
    pcg = {fused: _run(dev, kind, cfg, "pcg", fused=fused)[4] for fused in (True, False)}
    _same_bits(pcg[True], pcg[False], f"{kind}: pcg, fused vs operator path")
    assert np.isfinite(pcg[True]["U"]).all() and np.abs(pcg[True]["p"]).max() > 0
    for fused in (True, False):
        _same_bits(_run(dev, kind, cfg, "hybrid", net=net, fused=fused)[4], pcg[fused], f"{kind} fused={fused}: hybrid with a zero net vs pcg")


@pytest.mark.parametrize("kind", HC.SIM_KINDS)
def test_convnet_steps_vs_oracle(dev, oracle, kind):
    """four steps with seeded weights, fused and operator by operator, every step against the oracle at the 1e-5 of the existing
    convnet tests.  Measured: at most 1.9e-6 of max(1, |ref|max) (U after step 4 on open_all), density 1.0e-6, p 1.3e-7."""
    from fluidnet_cxx_amd import FluidNet
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    w = make_scalenet_weights(0)
    net = FluidNet.from_weights(NET_CFG, w, dev)
    blob = oracle.pack_weights(w)
    st = _sim_state(kind)
    want = {}
    for it in (1, 2, 3, 4):
        st = oracle.simulate_step(st, PLUME_CFG, "convnet", blob)
        want[it] = st
    for fused in (True, False):
        got = _run(dev, kind, NET_CFG, "convnet", net=net, steps=4, fused=fused, keep=(1, 2, 3, 4))
        for it in (1, 2, 3, 4):               # (the class map of the BC stages is built on step 2 and reused on steps 3 and 4)
            for k in ("U", "density", "p"):
                d = np.abs(got[it][k].astype(np.float64) - want[it][k]).max() / max(1.0, float(np.abs(want[it][k]).max()))
                print(f"{kind} fused={fused}: convnet {k} after {it} steps: {d:.2e} of max(1, |ref|max)")
                assert_close(got[it][k], want[it][k], 1e-5, f"{kind} fused={fused}: convnet {k} after {it} steps")


def test_fluidnet_forward_on_open_borders(dev, oracle):
    """Empty and Fluid border cells in the net's input (pack_div_kernel: the divergence and the obstacle channel)"""
    from fluidnet_cxx_amd import FluidNet
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    w = make_scalenet_weights(0)
    net = FluidNet.from_weights(NET_CFG, w, dev)
    s = HC.state("open4", *LARGE_SHAPES[0], 0.6, HC.LARGE_SEED)
    inp = np.concatenate([np.zeros_like(s["p"]), s["U"] * np.float32(0.5), s["flags"], s["rho"]], 1)
    p, U = net(T(inp, dev))
    po, Uo = oracle.fluidnet_forward(oracle.pack_weights(w), inp)
    assert_close_rel(N(p), po, 1e-5, "FluidNet p"); assert_close_rel(N(U), Uo, 1e-5, "FluidNet U")


# ---- f. PCG pieces -----------------------------------------------------------------------------------------------------------
def _active(f):
    return np.stack([PR.matrix(f[b, 0], False)[1].reshape(f.shape[2:]) for b in range(f.shape[0])])[:, None]


def _solvable(f):
    """poisson_reference's matrix of one sample is nonsingular on its active cells: is_singular() sees no null vector over the whole
    sample AND every connected region of active cells has a Dirichlet contact (a row with a positive sum) -- a region sealed in by
    scattered obstacles is a null vector of its own that is_singular() does not look for, and spsolve cannot take"""
    from scipy.sparse.csgraph import connected_components
    A, act = PR.matrix(f, False)
    if PR.is_singular(A, act):
        return False
    ia = np.nonzero(act)[0]
    n, lab = connected_components(A[ia][:, ia], directed=False)
    contact = np.asarray(A.sum(axis=1)).ravel()[ia] > 0.5
    return all(contact[lab == c].any() for c in range(n))


@pytest.mark.parametrize("kind", ["open4", "salt"])
def test_pcg_pieces_vs_model(dev, ext, kind):
    B, H, W = HC.ADJOINT_SHAPE
    f = np.array(HC.state(kind, B, H, W, 0.6, HC.LARGE_SEED)["flags"])
    rng = np.random.default_rng(1)
    p = rng.standard_normal(f.shape).astype(np.float32)
    got = N(ext.poisson_apply(T(f, dev), T(p, dev), False, None))
    want = PR.apply(f, np.where(_active(f), p, 0.0), False)
    assert np.abs(got - want).max() <= 1e-6 * float(np.abs(want).max())
    r = rng.standard_normal(f.shape).astype(np.float32)
    z = N(ext.pcg_precondition(T(f, dev), T(r, dev), False, None))
    for b in range(B):
        wz = PR.vcycle(f[b, 0], r[b, 0], False)
        d = np.abs(z[b, 0] - wz).max()
        assert d <= 1e-4 * np.abs(wz).max(), (b, d, np.abs(wz).max())


def test_pcg_solve_accuracy_on_open_borders(dev, ext):
    """the form of test_pcg_gpu.test_solve_accuracy_against_model on the samples whose system is solvable (_solvable)"""
    B, H, W = HC.ADJOINT_SHAPE
    checked = []
    for kind in ("open4", "salt"):
        f = np.array(HC.state(kind, B, H, W, 0.6, HC.LARGE_SEED)["flags"])
        div = np.random.default_rng(2).standard_normal(f.shape).astype(np.float32)
        tol = 1e-5
        p, res, iters = ext.solve_linear_system_pcg(T(f, dev), T(div, dev), False, tol, 200, False, None)
        p = N(p).astype(np.float64)
        act = _active(f)
        assert not np.any(np.where(act, 0.0, p)), "p must be 0 off the active cells"
        for b in range(B):
            if not _solvable(f[b, 0]):
                continue
            checked.append((kind, b))
            assert iters[b] <= 200
            bproj = PR.project(f[b:b + 1], div[b:b + 1], False)[0]
            pstar = PR.solve(f[b:b + 1], div[b:b + 1], False)[0]
            rr = bproj - PR.apply(f[b:b + 1], p[b:b + 1], False)[0]
            rel = np.linalg.norm(rr) / np.linalg.norm(bproj)
            assert rel <= 5e-5, (kind, b, rel, iters)
            A, _ = PR.matrix(f[b, 0], False)
            e = (p[b] - pstar).ravel()
            en = np.sqrt(e @ (A @ e)) / np.sqrt(pstar.ravel() @ (A @ pstar.ravel()))
            assert en <= 1e-2, (kind, b, en)
    # both open4 samples have Dirichlet contacts all along their sides; both salt samples are closed boxes (singular, with pockets)
    assert checked == [("open4", 0), ("open4", 1)], checked


# ---- the defect these goldens exposed: the viscous coefficient is the DOUBLE product of dt and viscosity, rounded once --------
@pytest.mark.parametrize("nu", [0.05, 0.007, 0.02])
def test_viscous_coefficient_is_the_double_product(fl, dev, oracle, nu):
    """dt = 0.1 with viscosity 0.05 or 0.007: the two floats' product is an ulp off the reference's (0.02, the goldens' value, is not).
    The operator, the step (which runs such a pair operator by operator) and the operator path have the oracle's bits."""
    from fluidnet_cxx_amd import _simulate
    s = HC.golden_state("open4_lo")
    Uv = T(s["U"], dev)
    fl.addViscosity(0.1, Uv, T(s["flags"], dev), nu)
    assert_bitexact(N(Uv), oracle.add_viscosity(0.1, s["U"], s["flags"], nu), f"addViscosity(0.1, ., ., {nu})")
    assert _simulate._step_has_the_viscous_coefficient(0.1, nu) == (nu == 0.02)
    cfg = dict(PLUME_CFG, jacobiIter=9, viscosity=nu)
    st = _sim_state("open_all")
    for _ in range(3):
        st = oracle.simulate_step(st, cfg, "jacobi")
    for fused in (True, False):
        got = _run(dev, "open_all", cfg, "jacobi", steps=3, fused=fused)[3]
        _same_bits(got, st, f"viscosity {nu} fused={fused}: 3 steps vs oracle")
