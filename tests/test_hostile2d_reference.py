"""The reference on hostile 2D geometries (tests/hostile2d_cases.py; goldens hostile2d.npz / hostile2d_hi.npz / hostile2d_sim.npz from
tools/make_golden.py --only hostile2d) -- CPU part: the oracle has the reference's bits on every stored array, the float64 model with
two axes reproduces the goldens within the rule of semantics3d_cases.check, the hand-chained oracle adjoints match the reference's
autograd, and the states do put in front of the code what they are meant to (the conditions).

No golden before these had a Fluid or Empty cell on the domain border (the ray / border intersection of the line trace, case 1, and the
MacCormack correction on fluid border cells), scattered cells, or samples of a batch with different flags.  The reference raised on no
option of any state.  Measured FIGURE rows of the six states (semantics3d_cases.FIGURE; tol = 4 x): advect_scalar 1.37e-6 (cfl 0.6) and
2.46e-6 .. 2.56e-6 (cfl 6.2), advect_vel 2.03e-6 .. 2.28e-6, divergence <= 9.55e-8, velocity_update <= 6.46e-8, add_buoyancy <= 3.86e-8,
add_gravity <= 2.66e-8, set_wall_bcs 0; no cell beyond JUMP (the guard over them: test_fluid_model_nd.test_model_precision_guard)."""
import numpy as np
import pytest

import hostile2d_cases as HC
import semantics3d_cases as C
from test_grad import _chain_oracle
from util import F2_CFG, PLUME_CFG, assert_bitexact, assert_close_rel, plume_state

STATES = list(HC.GOLDEN_STATES)
# every state of hostile2d_cases.state() that test_hostile2d_gpu.py uses, besides the golden ones: (kind, B, H, W, cfl, seed)
GPU_STATES = [(k, *shp, cfl, HC.LARGE_SEED) for shp in HC.LARGE_SHAPES for k in HC.KINDS for cfl in HC.CFLS.values()] + \
             [(k, *HC.JACOBI_SHAPE, 0.6, HC.LARGE_SEED) for k in ("open4", "salt")] + \
             [(k, *HC.ADJOINT_SHAPE, 0.6, HC.LARGE_SEED) for k in ("open4", "salt")]


Z = HC.golden_arrays


@pytest.mark.parametrize("name", STATES)
def test_golden_inputs_are_the_builders(golden, name):
    """the fixture's inputs are hostile2d_cases.golden_state(name), bit for bit (the builder is numpy only: the goldens pin it)"""
    z, s = Z(golden, name), HC.golden_state(name)
    for k in ("flags", "U", "rho", "p", "orig"):
        assert_bitexact(z[k], s[k], f"{name}:{k}")
    assert float(z["dt"]) == s["dt"] and z["gravity"].tolist() == [np.float32(g) for g in s["gravity"]] and float(z["rho_star"]) == np.float32(s["rho_star"])
    assert_bitexact(z["flags_stick"], HC.stick_flags(np.array(s["flags"]), HC.STICK_SEED), "flags_stick")
    assert set(z.files) >= set(C.OPS) | {"jacobi_p", "jacobi1_p", "jacobi_tol_p", "add_viscosity", "occupancy", "set_wall_bcs_stick"}, \
        "the reference raised on an option when the fixture was made"


@pytest.mark.parametrize("name", STATES)
def test_oracle_has_the_reference_bits(oracle, golden, name):
    z, O = Z(golden, name), oracle
    dt, flags, U, rho, p = float(z["dt"]), z["flags"], z["U"], z["rho"], z["p"]
    for meth in C.METHODS:
        for so in (0, 1):
            assert_bitexact(O.advect_scalar(dt, rho, U, flags, meth, 1, bool(so), 0.6), z[f"advect_scalar_{meth}_{so}"], f"advect_scalar {meth} so={so}")
        assert_bitexact(O.advect_vel(dt, U, U, flags, meth, 1, 0.6), z[f"advect_vel_{meth}"], f"advect_vel {meth}")
    assert_bitexact(O.advect_vel(dt, z["orig"], U, flags, "maccormackFluidNet", 1, 0.75), z["advect_vel_orig"], "advect_vel orig")
    assert_bitexact(O.velocity_divergence(U, flags), z["divergence"], "divergence")
    n = int(z["jacobi_iters"])
    assert n == 9
    pj, res, _ = O.jacobi(flags, z["divergence"], False, 0.0, n)
    assert_bitexact(pj, z["jacobi_p"], "jacobi")
    assert abs(res - float(z["jacobi_res"])) <= 1e-5 * max(1.0, float(z["jacobi_res"]))
    pj, res, _ = O.jacobi(flags, z["divergence"], False, 0.0, 1)
    assert_bitexact(pj, z["jacobi1_p"], "jacobi 1 sweep")
    assert abs(res - float(z["jacobi1_res"])) <= 1e-5 * max(1.0, float(z["jacobi1_res"]))
    for b in range(flags.shape[0]):            # the tolerance exit, sample by sample (the reference's B > 1 solve mixes samples)
        pj, _, it = O.jacobi(flags[b:b + 1], z["divergence"][b:b + 1], False, float(z["jacobi_tol"][b]), 50)
        assert_bitexact(pj, z["jacobi_tol_p"][b:b + 1], f"jacobi p_tol exit, sample {b}")
        assert it < 50
    assert_bitexact(O.velocity_update(p, U, flags), z["velocity_update"], "velocity_update")
    assert_bitexact(O.set_wall_bcs(U, flags), z["set_wall_bcs"], "set_wall_bcs")
    assert_bitexact(O.add_buoyancy(U, flags, rho, z["gravity"], float(z["rho_star"]), dt, False), z["add_buoyancy"], "add_buoyancy")
    assert_bitexact(O.flags_to_occupancy(flags), z["occupancy"], "occupancy")
    assert_bitexact(O.add_gravity(U, flags, z["gravity"], dt), z["add_gravity"], "add_gravity")
    assert_bitexact(O.add_viscosity(dt, U, flags, float(z["viscosity"])), z["add_viscosity"], "add_viscosity")
    # a pair whose product as two floats is an ulp off the reference's double product: 87 to 112 of the 2,812 values differ by one ulp when both are rounded first
    assert_bitexact(O.add_viscosity(0.1, U, flags, 0.05), z["add_viscosity_dt0p1_nu0p05"], "add_viscosity(0.1, ., ., 0.05)")
    out = O.set_wall_bcs_stick(U, flags, z["flags_stick"])
    assert_bitexact(out, z["set_wall_bcs_stick"], "set_wall_bcs_stick")
    assert (out != U).sum() > 100                 # (the case does exercise the operator)


@pytest.mark.parametrize("kind", HC.SIM_KINDS)
@pytest.mark.parametrize("cfgname,extra", [("plain", {}), ("f2", F2_CFG)])
def test_oracle_whole_steps_have_the_reference_bits(oracle, golden, kind, cfgname, extra):
    z = golden("hostile2d_sim")
    st = HC.sim_state(kind, plume_state(HC.SIM_RES))
    for k in ("flags", "U", "density", "p", "UBC", "UBCInvMask", "densityBC", "densityBCInvMask"):
        assert_bitexact(st[k], z[f"{kind}_in_{k}"], f"{kind}: input {k}")
    cfg = dict(PLUME_CFG, **extra)
    for it in range(1, 5):
        st = oracle.simulate_step(st, cfg, "jacobi")
        if it in (1, 4):
            for k in ("U", "density", "p"):
                assert_bitexact(st[k], z[f"{kind}_{cfgname}_{k}_{it}"], f"{kind} {cfgname}: {k} after {it} steps")


@pytest.mark.parametrize("name", C.HOSTILE_2D)
def test_model_reproduces_hostile_goldens(name):
    g = C.state(name)["golden"]
    assert set(g) == set(C.OPS)
    for op in C.OPS:
        C.check(g[op], name, op, "reference golden vs model")


@pytest.mark.parametrize("kind", ["open4", "salt"])
def test_oracle_adjoints_vs_reference_autograd(oracle, golden, kind):
    z, tag = golden("hostile2d"), f"grad_{kind}"
    flags = z[f"{tag}_flags"]
    assert_bitexact(flags, HC.golden_state(kind + "_lo")["flags"], "flags")
    U = oracle.set_wall_bcs(oracle.velocity_update(z[f"{tag}_p"], z[f"{tag}_U"], flags), flags)
    assert_bitexact(U, z[f"{tag}_U_out"], "U after velocityUpdate + setWallBcs")
    assert_bitexact(oracle.velocity_divergence(U, flags), z[f"{tag}_div"], "divergence")
    gU, gp = _chain_oracle(oracle, z, tag)
    assert_close_rel(gU, z[f"{tag}_grad_U"], 1e-6, "grad U")
    assert_close_rel(gp, z[f"{tag}_grad_p"], 1e-6, "grad p")


@pytest.mark.parametrize("name", STATES)
def test_conditions_golden_states(golden, name):
    s = HC.golden_state(name)
    HC.check_conditions(s)
    if s["kind"] != "salt":
        # the MacCormack correction runs on fluid border cells: the reference writes a nonzero value there, its Euler output there is 0
        z = Z(golden, name)
        fb = (s["flags"] == HC.FLUID) & HC.border_mask(s["flags"].shape)
        for so in (0, 1):
            assert (z[f"advect_scalar_maccormackFluidNet_{so}"][fb] != 0).sum() >= 100
            assert (z[f"advect_scalar_eulerFluidNet_{so}"][fb] == 0).all()


@pytest.mark.parametrize("case", GPU_STATES, ids=lambda c: "-".join(str(v) for v in c))
def test_conditions_gpu_states(oracle, case):
    s = HC.state(*case)
    HC.check_conditions(s)
    if s["kind"] != "salt":
        fb = (s["flags"] == HC.FLUID) & HC.border_mask(s["flags"].shape)
        mac = oracle.advect_scalar(s["dt"], s["rho"], s["U"], s["flags"], "maccormackFluidNet", 1, False, 0.6)
        assert (mac[fb] != 0).sum() >= 100


@pytest.mark.parametrize("sign", [-1.0, 1.0])
@pytest.mark.parametrize("kind", HC.KINDS)
@pytest.mark.parametrize("shape", HC.LARGE_SHAPES)
def test_conditions_one_signed_states(shape, kind, sign):
    """|U| and -|U| at cfl 6.2 (test_one_signed_velocity_vs_oracle): the same conditions, and every ray that leaves an open state does
    so on the two sides that face the corner its pass traces towards -- the forward pass towards (0, 0) for |U|, the backward pass away"""
    import fluid_model_nd as M
    s = HC.one_signed_state(HC.state(kind, *shape, 6.2, HC.LARGE_SEED), sign)
    HC.check_conditions(s)
    if kind != "salt":
        M.TRACE_STATS.update(border=0, blocked=0)
        M.advect_scalar(s["dt"], s["rho"], s["U"], s["flags"], "eulerFluidNet", False, 0.6)
        fwd = M.TRACE_STATS["border"]
        assert fwd >= 10, fwd
        # the forward pass of the field with the other sign traces the other way: its rays are the remaining ones of the MacCormack count
        o = HC.one_signed_state(s, -sign)
        M.TRACE_STATS.update(border=0, blocked=0)
        M.advect_scalar(o["dt"], o["rho"], o["U"], o["flags"], "eulerFluidNet", False, 0.6)
        assert M.TRACE_STATS["border"] >= 10


@pytest.mark.parametrize("kind", HC.SIM_KINDS)
def test_conditions_sim_states(golden, kind):
    """the whole-step states: Fluid and Empty cells on the border, which the MacCormack correction writes (the Euler pass leaves 0
    there).  No ray leaves the domain on them -- max|U| dt is about 1.2 at the start and 0.6 after the first projection, a ray from an
    interior cell centre needs more than 1.5 -- so what they add is the border cells in every stage of the step, not case 1 of the trace
    (the op-level states at cfl 6.2 have that)."""
    z = golden("hostile2d_sim")
    f = z[f"{kind}_in_flags"]
    bm = HC.border_mask(f.shape)
    assert ((f == HC.FLUID) & bm).sum() >= (120 if kind == "open_all" else 40) and ((f == HC.EMPTY) & bm).sum() >= 4
    fb = (f == HC.FLUID) & bm
    for cfgname in ("plain", "f2"):
        for it in (1, 4):
            assert (z[f"{kind}_{cfgname}_density_{it}"][fb] != 0).sum() >= 40


# (dt, viscosity) whose product as two floats is an ulp off the reference's double product rounded once; F2_CFG's pair is not one
OFF_PAIRS = [(0.1, 0.05), (0.1, 0.007), (1.5282496213912964, 0.07)]


@pytest.mark.parametrize("dt,nu", OFF_PAIRS + [(0.1, 0.02)])
def test_viscous_coefficient_is_the_double_product(oracle, dt, nu):
    """the reference multiplies dt and viscosity as Python doubles (viscosity.py:64; pinned by add_viscosity_dt0p1_nu0p05 of the goldens;
    a first draft of the cfl 6.2 states, dt = 1.5282496 with 0.07, exposed it).  The oracle against
    the numpy statement of the operator with that coefficient, and the step layer's test for the pairs the native step's two floats
    cannot express"""
    import viscous_model_nd as V
    from fluidnet_cxx_amd import _simulate
    s = HC.golden_state("salt_lo")
    f32 = lambda x: float(np.float32(x))
    differs = f32(f32(dt) * f32(nu)) != f32(dt * nu)
    assert differs == ((dt, nu) in OFF_PAIRS)
    assert _simulate._step_has_the_viscous_coefficient(dt, nu) == (not differs)
    assert_bitexact(oracle.add_viscosity(dt, s["U"], s["flags"], nu), V.add_viscosity(dt, s["U"], s["flags"], nu, 2, ref_quirks=True), "add_viscosity")
