"""3D default mode (ref_quirks = 0) pinned to a float64 model whose axis is a loop variable (fluid_model_nd.py) -- CPU part.

  a. the model is pinned to the reference's own goldens: with two axes it reproduces ops_2d_a..d (every advection option,
     advect_vel_orig, addBuoyancy, addGravity, setWallBcs, divergence, velocityUpdate); with three axes the arrays of
     ops_3d_a / ops_3d_b that no quirk Q10-Q15 touches (advect_scalar_eulerFluidNet_1, add_gravity, divergence).  The oracle
     in default mode reproduces those three bit for bit.
  b. analytic checks of the model alone (U = 0; a uniform velocity shifts a linear field exactly).
  c. the oracle in default mode against the model on ALL cells of nine 3D states with a z plate, a z bar, single obstacle
     cells, Empty cells and an obstacle on the k = 1 plane, at max|U| dt = 0.6 and 3.1, every operator and one Jacobi step.
     Six have an all-obstacle border like every golden: there no ray can leave the domain and the ray / border intersection
     of the line trace (case 1, with Q8 / Q9) never runs -- the goldens do NOT pin it.  Three more (max|U| dt = 6.2) have
     four open faces so that it runs (test_states_reach_both_cases_of_the_line_trace counts the rays); there the model is
     the only pin.  The clamp fallback of case 1 (Q8) is reached by no state.
  d. the guard: the model in float32 against itself in float64 stays within the tolerances used everywhere else.

Comparison rule and tolerances: semantics3d_cases.py (bad cell = beyond tol x the field's magnitude; at most 1e-3 of the cells
of an array bad; tol = 4 x the measured float32-against-float64 figure of the model on that state, the FIGURE table there).
Measured figures (largest over the states; per state in FIGURE): advect_scalar 6.2e-6 (ops_2d_d, max|U| dt = 4.9; <= 4.1e-6 on
the 3D states), advect_vel 3.9e-6, step_p / step_U / step_density 2.5e-6 / 2.7e-6 / 4.0e-6, divergence 9.3e-8,
velocity_update 7.2e-8, add_buoyancy 5.2e-8, add_gravity 5.2e-8, set_wall_bcs 0; no state has a cell beyond JUMP.  So tol
ranges from 0 (setWallBcs) over ~3e-7 (stencils) to 1.0e-6 .. 2.5e-5 (advection, the step).  Observed here: the oracle is within
tol on every cell of every state (0 bad cells; worst 6.2e-6 on ops_2d_d, <= 4.1e-6 in 3D)."""
import numpy as np
import pytest

import fluid_model_nd as M
import semantics3d_cases as C
from util import assert_bitexact

QUIRK_FREE_3D = ("advect_scalar_eulerFluidNet_1", "add_gravity", "divergence")


@pytest.mark.parametrize("case", C.GOLDEN_2D)
def test_model_reproduces_2d_goldens(case):
    g = C.state(case)["golden"]
    assert set(g) == set(C.OPS)
    for op in C.OPS:
        C.check(g[op], case, op, "reference golden vs model")


@pytest.mark.parametrize("case", C.GOLDEN_3D)
def test_model_reproduces_quirk_free_3d_goldens(case):
    g = C.state(case)["golden"]
    for op in QUIRK_FREE_3D:
        C.check(g[op], case, op, "reference golden vs model")


@pytest.mark.parametrize("case", C.GOLDEN_3D)
def test_oracle_default_mode_bitexact_on_quirk_free_3d_goldens(oracle, case):
    """what the reference does pin in 3D: the z term of getCentered, the 3D line trace's unit stepping and obstacle back-off (not
    its border intersection: the goldens' border is all obstacle), trilinear sampling, the z terms of addGravity and divergence"""
    s = C.state(case)
    out = C.run_ops(C.OracleBackend(oracle), s)
    for op in QUIRK_FREE_3D:
        assert_bitexact(out[op], s["golden"][op], f"{case}:{op}, oracle in default mode")


@pytest.mark.parametrize("nd", [2, 3])
@pytest.mark.parametrize("method", C.METHODS)
def test_model_zero_velocity_returns_src(nd, method):
    s = C.state("large_lo" if nd == 3 else "ops_2d_b")
    got = M.advect_scalar(0.3, s["rho"], np.zeros_like(s["U"]), s["flags"], method, False, 0.8)
    sel = (s["flags"] == M.FLUID)
    sel[:, :, :, 0] = sel[:, :, :, -1] = sel[..., 0] = sel[..., -1] = False
    if nd == 3:
        sel[:, :, 0] = sel[:, :, -1] = False
    assert sel.sum() > 100 and np.array_equal(got[sel], s["rho"].astype(np.float64)[sel])


@pytest.mark.parametrize("nd", [2, 3])
@pytest.mark.parametrize("method", C.METHODS)
def test_model_uniform_velocity_shifts_linear_field(nd, method):
    """obstacle-free box, U constant, src linear in the cell centres: dst(x) = src(x - dt U) wherever the samples of the pass
    (and, for MacCormack, of the backward pass, which reads the zeroed border of the forward one) stay off the border cells"""
    D, H, W = (12 if nd == 3 else 1), 20, 16
    vel, grad, dt = (0.7, -1.3, 0.4)[:nd], (0.3, -0.2, 0.5)[:nd], 1.0
    flags = np.full((1, 1, D, H, W), M.FLUID, np.float32)
    k, j, i = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    ctr = (i + 0.5, j + 0.5, k + 0.5)[:nd]
    src = (1.0 + sum(g * c for g, c in zip(grad, ctr)))[None, None]
    U = np.stack([np.full((1, D, H, W), v) for v in vel], 1)
    got = M.advect_scalar(dt, src, U, flags, method, False, 0.9)
    want = (1.0 + sum(g * (c - dt * v) for g, c, v in zip(grad, ctr, vel)))[None, None]
    sel = np.ones(src.shape, bool)
    for a, idx in enumerate((i, j, k)[:nd]):
        m = 2 + 2 * int(np.ceil(abs(vel[a] * dt)))    # the backward pass reads forward values that far away
        sel &= ((idx >= m) & (idx <= (W, H, D)[a] - 1 - m))[None, None]
    assert sel.sum() >= (20 if nd == 3 else 12)
    assert np.abs(got - want)[sel].max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("name", list(C.OWN))
def test_oracle_default_mode_vs_model_all_cells(oracle, name):
    s = C.state(name)
    out = C.run_ops(C.OracleBackend(oracle), s)
    st = oracle.simulate_step(dict(p=np.zeros_like(s["rho"]), U=s["U"], flags=s["flags"], density=s["rho"]), C.step_cfg(name),
                              "jacobi")
    out.update(step_p=st["p"], step_U=st["U"], step_density=st["density"])
    for op in C.OPS + C.STEP_OUT:
        C.check(out[op], name, op, "oracle vs model")


@pytest.mark.parametrize("name", C.GOLDEN_2D + C.GOLDEN_3D + tuple(C.OWN) + C.HOSTILE_2D)
def test_model_precision_guard(name):
    """float32 model against float64 model: at most a quarter of the cap beyond tol"""
    m32 = C.model_outputs(name, np.float32)
    for op in C.model_outputs(name):
        C.check(m32[op], name, op, "model float32 vs float64", cap=C.CAP / 4)


@pytest.mark.parametrize("name", list(C.OWN))
def test_states_reach_both_cases_of_the_line_trace(name):
    """what the comparisons above can vouch for: behind an all-obstacle border no ray ever leaves the domain (a unit step ends in the
    wall cell first), so only the states with open faces run the ray / border intersection (case 1); every state above
    max|U| dt = 1 runs the obstacle back-off (case 2).  No 3D golden has an open face: in 3D case 1 is pinned by the model alone (in 2D
    the goldens of hostile2d_cases.py have open sides, test_hostile2d_reference.py)."""
    s = C.state(name)
    M.TRACE_STATS.update(border=0, blocked=0)
    M.advect_scalar(s["dt"], s["rho"], s["U"], s["flags"], "eulerFluidNet", False, 0.6)
    assert (M.TRACE_STATS["border"] >= 30) == (name in C.OPEN) and (M.TRACE_STATS["border"] > 0) == (name in C.OPEN), M.TRACE_STATS
    assert (M.TRACE_STATS["blocked"] >= 50) == (not name.endswith("_lo")), M.TRACE_STATS
