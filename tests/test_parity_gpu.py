"""Parity of the HIP path (through the `fluidnet_cpp` extension == the C ABI) with
  (1) golden vectors captured from the reference, (2) the CPU oracle on seeded inputs (ragged sizes, B>1, 3D in
  both semantic modes), (3) size-independent properties at the benchmark sizes.
Integer-like fields (flags, occupancy) and every stencil/advection op are bit-exact; the Jacobi residual and
the CNN are fp32-tolerance statements (tolerances written at the assert)."""
import numpy as np
import pytest
import torch

from util import PLUME_CFG, assert_bitexact, assert_close, assert_close_rel, make_flags, plume_state, random_state

pytestmark = pytest.mark.gpu


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
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def run_ops(fl, dev, flags, U, rho, p, dt, gravity, rho_star, is3d, orig=None, jac_iters=7, geom=None):
    tf, tU, trho, tp = T(flags, dev), T(U, dev), T(rho, dev), T(p, dev)
    out = {}
    for meth in ("maccormackFluidNet", "eulerFluidNet"):
        for so in (0, 1):
            out[f"advect_scalar_{meth}_{so}"] = N(fl.advectScalar(dt, trho, tU, tf, meth, 1, bool(so), 0.6, geom=geom))
        out[f"advect_vel_{meth}"] = N(fl.advectVelocity(dt, tU, tU, tf, meth, 1, 0.6, geom=geom))
    if orig is not None:
        out["advect_vel_orig"] = N(fl.advectVelocity(dt, T(orig, dev), tU, tf, "maccormackFluidNet", 1, 0.75, geom=geom))
    div = fl.velocityDivergence(tU, tf, geom=geom)
    out["divergence"] = N(div)
    pj, res = fl.solveLinearSystemJacobi(tf, div, is3d, 0.0, jac_iters, geom=geom)
    out["jacobi_p"], out["jacobi_res"] = N(pj), float(res)
    pj, res = fl.solveLinearSystemJacobi(tf, div, is3d, 0.0, 1, geom=geom)
    out["jacobi1_p"], out["jacobi1_res"] = N(pj), float(res)
    Uu = tU.clone(); assert fl.velocityUpdate(tp, Uu, tf, geom=geom) is None; out["velocity_update"] = N(Uu)
    Uw = tU.clone(); r = fl.setWallBcs(Uw, tf, geom=geom); assert r is Uw; out["set_wall_bcs"] = N(Uw)
    Ub = tU.clone(); r = fl.addBuoyancy(Ub, tf, trho, gravity, rho_star, dt, geom=geom); assert r is Ub; out["add_buoyancy"] = N(Ub)
    out["occupancy"] = N(fl.flagsToOccupancy(tf))
    Ug = tU.clone(); r = fl.addGravity(Ug, tf, gravity, dt, geom=geom); assert r is Ug; out["add_gravity"] = N(Ug)
    if not is3d:
        Uv = tU.clone(); fl.addViscosity(dt, Uv, tf, 0.07); out["add_viscosity"] = N(Uv)
    # inputs untouched (reference: advect_* and solve_linear_system never write to inputs)
    assert_bitexact(N(tU), U, "U unchanged"); assert_bitexact(N(trho), rho, "rho unchanged"); assert_bitexact(N(tf), flags, "flags unchanged")
    return out


@pytest.mark.parametrize("case", ["ops_2d_a", "ops_2d_b", "ops_2d_c", "ops_2d_d", "ops_3d_a", "ops_3d_b"])
def test_ops_vs_reference_golden(fl, ext, dev, golden, case):
    z = golden(case)
    is3d = bool(z["is3d"])
    geom = ext.Geom(ref_quirks=is3d)  # 3D goldens are the reference's own (defective) 3D behaviour
    out = run_ops(fl, dev, z["flags"], z["U"], z["rho"], z["p"], float(z["dt"]), z["gravity"].tolist(), float(z["rho_star"]),
                  is3d, z["orig"], int(z["jacobi_iters"]), geom=geom)
    if "jacobi_tol" in z.files:
        tf, div = T(z["flags"], dev), T(z["divergence"], dev)
        pj, res = fl.solveLinearSystemJacobi(tf, div, is3d, float(z["jacobi_tol"]), 50, geom=geom)
        assert_bitexact(N(pj), z["jacobi_tol_p"], "jacobi p_tol early exit")
    for k, v in out.items():
        if k.endswith("_res"):
            assert abs(v - float(z[k])) <= 1e-5 * max(1.0, float(z[k])), (k, v, float(z[k]))   # reduction order differs
        elif k in z.files:
            if is3d and k in ("velocity_update", "set_wall_bcs"):
                continue                       # the reference's 3D branches of these two raise; no golden
            assert_bitexact(v, z[k], f"{case}:{k}")


SHAPES = [  # B, D, H, W, sigma, empties
    (1, 1, 17, 19, 3.0, False), (2, 1, 64, 64, 1.0, True), (1, 1, 65, 130, 8.0, False), (3, 1, 40, 257, 4.0, True),
    (1, 1, 200, 72, 20.0, False), (1, 5, 9, 11, 2.0, False), (2, 12, 20, 33, 6.0, False), (1, 16, 16, 70, 12.0, False),
]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("quirks", [False, True])
def test_ops_vs_oracle(fl, ext, dev, oracle, shape, quirks):
    B, D, H, W, sigma, empties = shape
    is3d = D > 1
    if quirks and not is3d:
        pytest.skip("quirks only change 3D")
    s = random_state(B, D, H, W, sigma, seed=B * 1000 + H, empties=empties)
    flags, U, rho, p = s["flags"], s["U"], s["rho"], s["p"]
    dt, grav, rstar = 0.17, [0.3, 0.25, -0.2], 0.05
    out = run_ops(fl, dev, flags, U, rho, p, dt, grav, rstar, is3d, jac_iters=11, geom=ext.Geom(ref_quirks=quirks))
    O = oracle
    for meth in ("maccormackFluidNet", "eulerFluidNet"):
        for so in (0, 1):
            assert_bitexact(out[f"advect_scalar_{meth}_{so}"], O.advect_scalar(dt, rho, U, flags, meth, 1, bool(so), 0.6, quirks), f"advect_scalar {meth} {so}")
        assert_bitexact(out[f"advect_vel_{meth}"], O.advect_vel(dt, U, U, flags, meth, 1, 0.6, quirks), f"advect_vel {meth}")
    div = O.velocity_divergence(U, flags)
    assert_bitexact(out["divergence"], div, "divergence")
    pj, res, _ = O.jacobi(flags, div, is3d, 0.0, 11, quirks)
    assert_bitexact(out["jacobi_p"], pj, "jacobi 11 sweeps"); assert abs(out["jacobi_res"] - res) <= 1e-5 * max(1.0, res)
    pj, res, _ = O.jacobi(flags, div, is3d, 0.0, 1, quirks)
    assert_bitexact(out["jacobi1_p"], pj, "jacobi 1 sweep")
    assert_bitexact(out["velocity_update"], O.velocity_update(p, U, flags), "velocity_update")
    assert_bitexact(out["set_wall_bcs"], O.set_wall_bcs(U, flags), "set_wall_bcs")
    assert_bitexact(out["add_buoyancy"], O.add_buoyancy(U, flags, rho, grav, rstar, dt, quirks), "add_buoyancy")
    assert_bitexact(out["occupancy"], O.flags_to_occupancy(flags), "occupancy")
    assert_bitexact(out["add_gravity"], O.add_gravity(U, flags, grav, dt), "add_gravity")
    if not is3d:
        assert_bitexact(out["add_viscosity"], O.add_viscosity(dt, U, flags, 0.07), "add_viscosity")


@pytest.mark.parametrize("iters", [1, 2, 7, 8, 9, 16, 28, 37, 100])
def test_jacobi_sweep_counts(fl, dev, oracle, iters):
    """The temporally blocked kernel for every split of max_iter into launches."""
    s = random_state(2, 1, 96, 150, 2.0, seed=iters)
    div = oracle.velocity_divergence(s["U"], s["flags"])
    pj, res = fl.solveLinearSystemJacobi(T(s["flags"], dev), T(div, dev), False, 0.0, iters)
    po, ro, _ = oracle.jacobi(s["flags"], div, False, 0.0, iters)
    assert_bitexact(N(pj), po, f"jacobi {iters}")
    assert abs(float(res) - ro) <= 1e-5 * max(1.0, ro)


@pytest.mark.parametrize("shape", [(1, 6, 8, 100), (1, 1, 8, 120)])
def test_jacobi_denormal_front(fl, dev, oracle, shape):
    """A point source far from the other end of a long domain: the pressure front decays by ~1/6 (1/4) per cell and
    runs through the fp32 denormal range.  The 3D kernel's fast exact /6 hands denormal quotients to the true
    division; both must match the CPU's IEEE division bit for bit."""
    B, D, H, W = shape
    is3d = D > 1
    flags = make_flags(B, D, H, W, boxes=False)
    div = np.zeros((B, 1, D, H, W), np.float32)
    div[0, 0, D // 2, H // 2, 2] = -0.37
    n = 95
    pg, _ = fl.solveLinearSystemJacobi(T(flags, dev), T(div, dev), is3d, 0.0, n)
    po, _, _ = oracle.jacobi(flags, div, is3d, 0.0, n)
    tiny = np.abs(po[po != 0]).min()
    assert tiny < 1.2e-38, f"the case does not reach the denormal range (min |p| = {tiny})"
    assert_bitexact(N(pg), po, "jacobi through the denormal range")


@pytest.mark.parametrize("shape,n", [((2, 1, 70, 130), 9), ((1, 12, 24, 66), 7), ((1, 1, 40, 90), 1), ((2, 6, 12, 70), 1)])
def test_jacobi_residual_value_and_reproducibility(fl, dev, oracle, shape, n):
    """solve_linear_system's second return value, max_b ||p_n - p_(n-1)||_2 (fluids_init.cpp:961-966): equal to the oracle's
    within fp32 rounding of a long sum, and -- summed in a fixed order, no atomics -- the same bits on every run; asking for
    it does not change the pressure (the last sweep runs as its own launch)."""
    B, D, H, W = shape
    is3d = D > 1
    s = random_state(B, D, H, W, 2.0, seed=17)
    div = oracle.velocity_divergence(s["U"], s["flags"])
    po, ro, _ = oracle.jacobi(s["flags"], div, is3d, 0.0, n)
    tf, td = T(s["flags"], dev), T(div, dev)
    runs = [fl.solveLinearSystemJacobi(tf, td, is3d, 0.0, n) for _ in range(4)]
    for p, r in runs:
        assert_bitexact(N(p), po, "pressure")
        assert float(r) == float(runs[0][1]), "the residual differs between two runs of the same solve"
    assert abs(float(runs[0][1]) - ro) <= 2e-6 * max(ro, 1e-30), (float(runs[0][1]), ro)


def test_jacobi_verbose_prints_every_sweep(fl, dev, oracle, capfd):
    """verbose=True (fluids_init.cpp:968-987): one "Jacobi iteration N: residual R" line per sweep and the termination line;
    the pressure is the non-verbose one."""
    s = random_state(1, 1, 24, 40, 2.0, seed=4)
    div = oracle.velocity_divergence(s["U"], s["flags"])
    tf, td = T(s["flags"], dev), T(div, dev)
    p0, r0 = fl.solveLinearSystemJacobi(tf, td, False, 0.0, 5)
    capfd.readouterr()
    p1, r1 = fl.solveLinearSystemJacobi(tf, td, False, 0.0, 5, verbose=True)
    out = capfd.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("Jacobi iteration")]
    assert [int(l.split()[2].rstrip(":")) for l in lines] == [1, 2, 3, 4, 5], out
    assert "Jacobi max iteration count (5) reached (terminating)" in out
    assert abs(float(lines[-1].split()[-1]) - float(r1)) <= 1e-5 * float(r1)
    assert_bitexact(N(p1), N(p0), "verbose pressure"); assert float(r0) == float(r1)
    _, ro, _ = oracle.jacobi(s["flags"], div, False, 0.0, 5)
    assert abs(float(r1) - ro) <= 2e-6 * ro


def test_jacobi_tolerance_exit(fl, dev, oracle):
    s = random_state(1, 1, 48, 80, 2.0, seed=3)
    div = oracle.velocity_divergence(s["U"], s["flags"])
    _, r5, _ = oracle.jacobi(s["flags"], div, False, 0.0, 5)
    _, r6, _ = oracle.jacobi(s["flags"], div, False, 0.0, 6)
    tol = 0.5 * (r5 + r6)
    po, ro, it = oracle.jacobi(s["flags"], div, False, tol, 100)
    pj, res = fl.solveLinearSystemJacobi(T(s["flags"], dev), T(div, dev), False, tol, 100)
    assert_bitexact(N(pj), po, "early exit pressure")
    with pytest.raises(RuntimeError, match="At least 1 iteration"):
        fl.solveLinearSystemJacobi(T(s["flags"], dev), T(div, dev), False, 0.0, 0)


def test_error_behaviour(fl, dev):
    U = torch.zeros(1, 2, 1, 8, 8, device=dev); flags = torch.ones(1, 1, 1, 8, 8, device=dev)
    with pytest.raises(RuntimeError, match="Advection method not supported"):
        from fluidnet_cxx_amd._ext import ext
        ext.advect_scalar(0.1, flags.clone(), U, flags, "semiLagrange", 1, False, 0.5)
    with pytest.raises(RuntimeError):
        fl.advectScalar(0.1, flags.clone(), U, flags, boundary_width=2)
    with pytest.raises(RuntimeError, match="contiguous"):
        fl.velocityDivergence(U.transpose(3, 4), flags) if False else fl.ops.ext.velocity_divergence(U.transpose(3, 4), flags)


def to_dev(st, dev):
    return {k: T(v, dev) for k, v in st.items()}


@pytest.mark.parametrize("fused", [True, False])
def test_plume128_simulation_vs_reference(dev, golden, fused):
    """Config C1 (128^2 plume, Jacobi-28): whole-step parity with the reference after 1, 5, 20 steps -- bit-exact."""
    from fluidnet_cxx_amd import simulate
    z = golden("plume128")
    bd = to_dev(plume_state(128), dev)
    for it in range(1, 21):
        simulate(PLUME_CFG, bd, None, "jacobi", fused=fused)
        if it in (1, 5, 20):
            for k in ("U", "density", "p"):
                assert_bitexact(N(bd[k]), z[f"{k}_{it}"], f"{k} after {it} steps (fused={fused})")


def test_generators_bitexact(fl, dev, golden):
    z = golden("generators")
    f3 = torch.zeros(2, 1, 6, 7, 8, device=dev); fl.emptyDomain(f3)
    assert_bitexact(N(f3), z["empty3d"], "emptyDomain 3D")
    for res in (16, 128):
        bd = dict(p=torch.zeros(1, 1, 1, res, res, device=dev), U=torch.zeros(1, 2, 1, res, res, device=dev),
                  flags=torch.zeros(1, 1, 1, res, res, device=dev), density=torch.zeros(1, 1, 1, res, res, device=dev))
        fl.emptyDomain(bd["flags"]); fl.createPlumeBCs(bd, 0.1, 2, 0.145)
        assert_bitexact(N(bd["flags"]), z[f"plume{res}_flags"], "flags")
        for k in ("UBC", "UBCInvMask", "densityBC", "densityBCInvMask"):
            assert_bitexact(N(bd[k]), z[f"plume{res}_{k}"], k)
    bd = dict(p=torch.zeros(1, 1, 1, 40, 32, device=dev), U=torch.zeros(1, 2, 1, 40, 32, device=dev),
              flags=torch.zeros(1, 1, 1, 40, 32, device=dev), density=torch.zeros(1, 1, 1, 40, 32, device=dev))
    fl.createRayleighTaylorBCs(bd, dict(perturbThickness=100, perturbAmplitude=0.01, height=0.5), -0.01, 0.01)
    assert_close(N(bd["density"]), z["rt_density"], 1e-6, "Rayleigh-Taylor density")


def test_geometry_and_centered_bitexact(fl, dev, golden, oracle):
    """createCylinder / createBox2D / getCentered as native kernels: the reference's flags and centred velocities (goldens),
    and the oracle on a larger 3D grid with off-grid centres and radii that are not fp32 numbers."""
    z = golden("generators")
    for tag, shape in (("cyl2d", (1, 1, 40, 32)), ("cyl3d", (1, 5, 24, 28))):
        bd = dict(flags=T(make_flags(*shape, boxes=False), dev))
        fl.createCylinder(bd, 15.5, 20.0, 6.3)
        assert_bitexact(N(bd["flags"]), z[tag + "_flags"], tag)
    bd = dict(flags=T(make_flags(1, 1, 20, 30, boxes=False), dev))
    fl.createBox2D(bd, 5, 9, 3, 6)
    want = make_flags(1, 1, 20, 30, boxes=False); want[0, 0, 0, 3:6, 5:9] = 2
    assert_bitexact(N(bd["flags"]), want, "box2d")
    f0 = make_flags(1, 7, 150, 131, boxes=True)
    for (cx, cy, r) in ((0.5 * 131, 0.5 * 150, 50), (40.3, 77.7, 12.1), (-3.0, 10.0, 9.9), (130.0, 149.0, 0.0)):
        bd = dict(flags=T(f0, dev)); fl.createCylinder(bd, cx, cy, r)
        assert_bitexact(N(bd["flags"]), oracle.create_cylinder(f0, cx, cy, r), f"cylinder {cx},{cy},{r}")
    for box in ((0.5 * 131, 0.7 * 131, 0.2 * 150, 0.7 * 150), (-5, 3.5, 140.2, 1000), (10, 10, 3, 9)):
        bd = dict(flags=T(f0, dev)); fl.createBox2D(bd, *box)
        assert_bitexact(N(bd["flags"]), oracle.create_box2d(f0, *box), f"box {box}")
    zg = golden("grid")
    for tag in ("2d", "3d"):
        assert_bitexact(N(fl.getCentered(T(zg[f"U_{tag}"], dev))), zg[f"centered_{tag}"], f"getCentered {tag}")
    rng = np.random.default_rng(5)
    for shape in ((2, 2, 1, 67, 130), (1, 3, 9, 33, 70)):
        U = rng.standard_normal(shape).astype(np.float32)
        assert_bitexact(N(fl.getCentered(T(U, dev))), oracle.get_centered(U), f"getCentered {shape}")


@pytest.mark.parametrize("shape", [(1, 40, 70, 130), (1, 40, 1040, 1030)])
def test_jacobi_pass_two_ranges(dev, ext, shape):
    """fnx_jacobi_pass2: two disjoint plane ranges in one launch == the two single-range calls, bit for bit (1 and 2 sweeps,
    from p and from zero; the second shape has more tiles than resident waves: the launcher then runs the ranges one
    after the other)."""
    B, D, H, W = shape
    rng = np.random.default_rng(4)
    flags = T(make_flags(B, D, H, W, boxes=True), dev)
    div = T(rng.standard_normal((B, 1, D, H, W)).astype(np.float32), dev)
    p = T(rng.standard_normal((B, 1, D, H, W)).astype(np.float32), dev)
    ws = torch.empty(ext.jacobi_workspace_bytes(B, D, H, W, True), dtype=torch.uint8, device=dev)
    first = True
    for n in (2, 1):
        for pin in (p, None):
            for (a, b, a2) in ((3, 17, 20), (2, 8, 30), (0, 5, 35)):
                one = torch.full_like(p, 7.0); two = torch.full_like(p, 7.0)
                ext.jacobi_pass_(flags, div, pin, one, n, a, b, ws, not first, a2); first = False
                ext.jacobi_pass_(flags, div, pin, two, n, a, b, ws, True)
                ext.jacobi_pass_(flags, div, pin, two, n, a2, a2 + b - a, ws, True)
                assert torch.equal(one, two), (n, pin is None, a, b, a2)
    with pytest.raises(RuntimeError, match="overlapping"):
        ext.jacobi_pass_(flags, div, p, torch.empty_like(p), 2, 3, 17, ws, True, 10)


@pytest.mark.parametrize("B", [1, 2])
def test_jacobi_pass_mirror_window_inside_and_across_the_range(dev, ext, B):
    """fnx_jacobi_pass_mirror with a mirror window that is NOT the launch's plane range (the z-slab driver always passes window ==
    range): a window inside the range, one that starts below it, one that ends above it, one wholly outside, and two ranges with a
    window each.  p_out is the plain two-sweep pass's, the mirror holds exactly the window's computed planes, and the canary floats
    around and inside the mirror (planes of the window the launch does not compute) are untouched -- the mirrored store is dropped
    by a wave-uniform plane test, not by the buffer range check (a plane below the window used to wrap the scalar offset)."""
    D, H, W = 40, 64, 120
    if not ext.jacobi_pass_mirror_ok(B, D, H, W, 22, True, 0):
        pytest.skip("this device holds fewer resident waves than the test grid has tiles")
    rng = np.random.default_rng(8)
    flags = T(make_flags(B, D, H, W, boxes=True), dev)
    div = T(rng.standard_normal((B, 1, D, H, W)).astype(np.float32), dev)
    p = T(rng.standard_normal((B, 1, D, H, W)).astype(np.float32), dev)
    ws = torch.empty(ext.jacobi_workspace_bytes(B, D, H, W, True), dtype=torch.uint8, device=dev)
    want = torch.full_like(p, 7.0)
    ext.jacobi_pass_(flags, div, p, want, 2, 0, D, ws, False)
    guard, CAN = 3 * H * W, 777.0

    def run(kb, ke, kf, n, kb2=-1, kf2=0):
        bufs = [torch.full((2 * guard + B * n * H * W,), CAN, device=dev) for _ in range(2 if kb2 >= 0 else 1)]
        mir = [b[guard:guard + B * n * H * W] for b in bufs]
        out = torch.full_like(p, 7.0)
        ext.jacobi_pass_mirror_(flags, div, p, out, kb, ke, ws, True, mir[0], kf, n, kb2, mir[1] if kb2 >= 0 else None, kf2)
        torch.cuda.synchronize()
        ranges = [(kb, ke, kf, 0)] + ([(kb2, kb2 + ke - kb, kf2, 1)] if kb2 >= 0 else [])
        inside = torch.zeros(D, dtype=torch.bool)
        for a, b_, f, q in ranges:
            inside[a:b_] = True
            assert torch.equal(out[:, :, a:b_], want[:, :, a:b_]), ("p_out", kb, ke, kf, n, q)
            assert bool((bufs[q][:guard] == CAN).all()) and bool((bufs[q][guard + B * n * H * W:] == CAN).all()), ("canary around the mirror", kb, ke, kf, n, q)
            m = mir[q].view(B, n, H, W)
            for i in range(n):
                k = f + i
                if a <= k < b_:
                    assert torch.equal(m[:, i], want[:, 0, k]), ("mirrored plane", k, kb, ke, kf, n, q)
                else:
                    assert bool((m[:, i] == CAN).all()), ("plane of the window outside the range must stay untouched", k, kb, ke, kf, n, q)
        assert bool((out[:, :, ~inside] == 7.0).all()), "planes outside the range untouched"

    run(8, 30, 12, 4)            # window inside the range
    run(8, 30, 8, 22)            # window == range (what the z-slab driver passes)
    run(8, 30, 5, 6)             # starts 3 planes below the range
    run(8, 30, 27, 6)            # ends 3 planes above it
    run(20, 30, 2, 5)            # wholly below: nothing mirrored
    run(3, 12, 30, 5)            # wholly above
    run(2, 12, 4, 3, 25, 22)     # two ranges, a window inside the first and one that starts below the second
    run(2, 12, 0, 4, 25, 33)     # ... one below the first range's start, one over the second's end


@pytest.mark.parametrize("shape,n", [((2, 12, 24, 70), 10), ((1, 9, 21, 66), 7), ((1, 1, 40, 90), 20), ((1, 5, 4, 10), 6), ((2, 3, 8, 130), 8)])
def test_jacobi_sweeps_from_zero_flag(dev, ext, fl, oracle, shape, n):
    """fnx_jacobi_sweeps_ex with the from-zero bit (what the z-slab drivers run on a single rank): p is not read -- it is
    handed over full of NaN -- and the result has the bits of the whole-solve entry point and of the oracle (3D with
    H % 4 == 0: the passes hand each other p in the row-quad layout; H % 4 != 0: in rows; 2D)."""
    B, D, H, W = shape
    is3d = D > 1
    s = random_state(B, D, H, W, 2.0, seed=n)
    div = oracle.velocity_divergence(s["U"], s["flags"])
    tf, td = T(s["flags"], dev), T(div, dev)
    p = torch.full((B, 1, D, H, W), float("nan"), device=dev)
    ws = torch.empty(ext.jacobi_workspace_bytes(B, D, H, W, is3d), dtype=torch.uint8, device=dev)
    ext.jacobi_sweeps_(tf, td, p, is3d, n, ws, False, from_zero=True)
    po, _, _ = oracle.jacobi(s["flags"], div, is3d, 0.0, n)
    assert_bitexact(N(p), po, f"jacobi_sweeps from zero {shape} n={n}")
    pj, _ = fl.solveLinearSystemJacobi(tf, td, is3d, 0.0, n)
    assert torch.equal(p, pj)
    ext.jacobi_sweeps_(tf, td, p, is3d, 4, ws, True)          # and 4 more sweeps from there (rows in, rows out)
    po4 = oracle.jacobi_sweeps(s["flags"], div, po, is3d, 4)
    assert_bitexact(N(p), po4, "4 more sweeps")


def test_jacobi_quad_handover_more_tiles_than_waves(dev, fl, oracle):
    """3D solve on planes with more 60x4 tiles than resident waves (the launcher then splits the (tile, plane) space evenly
    over the waves) and H % 4 == 0 (the passes hand each other p in the row-quad layout): bits of the oracle."""
    B, D, H, W = 1, 7, 1040, 1030
    rng = np.random.default_rng(11)
    flags = make_flags(B, D, H, W, boxes=True)
    div = rng.standard_normal((B, 1, D, H, W)).astype(np.float32)
    for n in (6, 5):
        pg, _ = fl.solveLinearSystemJacobi(T(flags, dev), T(div, dev), True, 0.0, n)
        po, _, _ = oracle.jacobi(flags, div, True, 0.0, n)
        assert_bitexact(N(pg), po, f"jacobi {n} sweeps on {D}x{H}x{W}")


def test_jacobi_pass_layout_chain_and_errors(dev, ext, oracle):
    """fnx_jacobi_pass_layout: a chain of two-sweep passes that hand each other p in the row-quad layout (first pass from
    zero, last pass writes rows) has the bits of the oracle; the layout is refused for one-sweep passes and for grids
    fnx_jacobi_quad_ok does not accept."""
    B, D, H, W = 2, 10, 16, 70
    rng = np.random.default_rng(21)
    flags = make_flags(B, D, H, W, boxes=True)
    div = rng.standard_normal((B, 1, D, H, W)).astype(np.float32)
    tf, td = T(flags, dev), T(div, dev)
    assert ext.jacobi_quad_ok(B, D, H, W) and not ext.jacobi_quad_ok(B, D, H + 1, W)
    ws = torch.empty(ext.jacobi_workspace_bytes(B, D, H, W, True), dtype=torch.uint8, device=dev)
    a = torch.full((B, 1, D, H, W), float("nan"), device=dev); b = torch.full_like(a, float("nan"))
    ext.jacobi_pass_(tf, td, None, a, 2, 0, 0, ws, False, layout=2)      # from zero, quad out
    ext.jacobi_pass_(tf, td, a, b, 2, 0, 0, ws, True, layout=3)          # quad in, quad out
    ext.jacobi_pass_(tf, td, b, a, 2, 0, 0, ws, True, layout=3)
    ext.jacobi_pass_(tf, td, a, b, 2, 0, 0, ws, True, layout=1)          # quad in, rows out
    po, _, _ = oracle.jacobi(flags, div, True, 0.0, 8)
    assert_bitexact(N(b), po, "four two-sweep passes through the row-quad layout")
    with pytest.raises(RuntimeError, match="row-quad"):
        ext.jacobi_pass_(tf, td, b, a, 1, 0, 0, ws, True, layout=1)
    H2 = H + 2
    f2 = T(make_flags(B, D, H2, W, boxes=False), dev); d2 = torch.zeros(B, 1, D, H2, W, device=dev)
    ws2 = torch.empty(ext.jacobi_workspace_bytes(B, D, H2, W, True), dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="row-quad"):
        ext.jacobi_pass_(f2, d2, None, torch.empty_like(d2), 2, 0, 0, ws2, False, layout=2)


def test_jacobi_pass_from_zero_respects_plane_range(dev, ext, oracle):
    """fnx_jacobi_pass with p_in = NULL ("p is 0 everywhere") and nsweeps 1 or 2 writes the planes [k_begin, k_end) only
    (the header's contract; the single-sweep from-zero kernel used to write every plane, which clobbered planes in
    flight in the slab driver's edge_first schedule with an odd sweep block)."""
    B, D, H, W = 2, 20, 24, 70
    rng = np.random.default_rng(9)
    flags = make_flags(B, D, H, W, boxes=True)
    div = rng.standard_normal((B, 1, D, H, W)).astype(np.float32)
    tf, td = T(flags, dev), T(div, dev)
    ws = torch.empty(ext.jacobi_workspace_bytes(B, D, H, W, True), dtype=torch.uint8, device=dev)
    first = True
    for n in (1, 2):
        full = oracle.jacobi_sweeps(flags, div, np.zeros_like(div), True, n)
        for (a, b, a2) in ((3, 9, -1), (0, 4, -1), (15, 20, -1), (2, 6, 12)):
            out = torch.full((B, 1, D, H, W), 7.0, device=dev)
            ext.jacobi_pass_(tf, td, None, out, n, a, b, ws, not first, a2); first = False
            got = N(out)
            want = np.full_like(got, 7.0)
            want[:, :, a:b] = full[:, :, a:b]
            if a2 >= 0:
                want[:, :, a2:a2 + b - a] = full[:, :, a2:a2 + b - a]
            assert_bitexact(got, want, f"from-zero pass n={n} planes [{a},{b}) + {a2}")


def test_extension_is_stateless(fl, ext, dev, oracle):
    """SURVEY 8b "no globals": quirk mode, slab view and compute window travel with the call (ext.Geom); a call with
    them leaves nothing behind for the next call, and the module exports no setters."""
    for name in ("set_ref_quirks", "set_slab", "set_window", "get_ref_quirks"):
        assert not hasattr(ext, name), name
    s = random_state(1, 10, 12, 20, 2.0, seed=5)
    tf, tU, trho = T(s["flags"], dev), T(s["U"], dev), T(s["rho"], dev)
    plain0 = N(fl.advectScalar(0.2, trho, tU, tf))
    quirk = N(fl.advectScalar(0.2, trho, tU, tf, geom=ext.Geom(ref_quirks=True)))
    win = torch.full_like(trho, 5.0)
    ext.advect_scalar(0.2, trho, tU, tf, "maccormackFluidNet", 1, False, 0.75, win, ext.Geom(k_begin=3, k_end=6))
    plain1 = N(fl.advectScalar(0.2, trho, tU, tf))
    assert_bitexact(plain0, plain1, "a geom call changed a later plain call")
    assert_bitexact(plain0, oracle.advect_scalar(0.2, s["rho"], s["U"], s["flags"], "maccormackFluidNet", 1, False, 0.75, False), "plain")
    assert_bitexact(quirk, oracle.advect_scalar(0.2, s["rho"], s["U"], s["flags"], "maccormackFluidNet", 1, False, 0.75, True), "quirks")
    w = N(win)
    assert_bitexact(w[:, :, 3:6], plain0[:, :, 3:6], "window planes")
    assert (w[:, :, :3] == 5.0).all() and (w[:, :, 6:] == 5.0).all(), "planes outside the window were written"


def _permute_state(s, grav, perm):
    """The same physical state with two axes exchanged: perm = "xz" or "yz".  Arrays are (B,C,D,H,W); the velocity
    channels (x,y,z) follow their axes (MAC faces move with them)."""
    ax = (0, 1, 4, 3, 2) if perm == "xz" else (0, 1, 3, 2, 4)
    ch = [2, 1, 0] if perm == "xz" else [0, 2, 1]
    t = lambda a: np.ascontiguousarray(np.transpose(a, ax))
    out = dict(flags=t(s["flags"]), rho=t(s["rho"]), p=t(s["p"]), U=t(s["U"][:, ch]))
    return out, [grav[c] for c in ch], (lambda a: t(a[:, ch]) if a.shape[1] == 3 else t(a))


@pytest.mark.parametrize("perm", ["xz", "yz"])
def test_3d_default_semantics_axis_symmetry(fl, dev, perm):
    """An oracle-independent check of the intended 3D semantics (ref_quirks=0: what bench.py and configs[3]/[4] run).
    The reference's 3D raises, so the default mode is otherwise pinned only to this repo's own CPU restatement, which
    shares its reading of the z rules with the kernels.  The x and y rules ARE pinned to the reference (2D goldens); a
    correct 3D extension treats z like them, so running an operator on the state with z exchanged with x (or y) must
    give the exchanged result.  Not bit-exact -- sums and interpolations nest the axes in a fixed order -- hence a
    rounding-level tolerance (2e-6 of the field's magnitude) on >= 99.9 % of the cells; a wrong offset, a missing z term
    or a misplaced face would move O(1) of them."""
    s = random_state(1, 14, 18, 22, 1.3, seed=77)
    grav = [0.3, 0.25, -0.2]
    sp, gravp, back = _permute_state(s, grav, perm)
    dt, rstar = 0.17, 0.05

    def run(st, g):
        tf, tU, trho, tp = T(st["flags"], dev), T(st["U"], dev), T(st["rho"], dev), T(st["p"], dev)
        o = {}
        o["advect_scalar"] = N(fl.advectScalar(dt, trho, tU, tf, "maccormackFluidNet", 1, False, 0.6))
        o["advect_scalar_outside"] = N(fl.advectScalar(dt, trho, tU, tf, "maccormackFluidNet", 1, True, 0.6))
        o["advect_scalar_euler"] = N(fl.advectScalar(dt, trho, tU, tf, "eulerFluidNet", 1, False, 0.6))
        o["advect_vel"] = N(fl.advectVelocity(dt, tU, tU, tf, "maccormackFluidNet", 1, 0.6))
        o["advect_vel_euler"] = N(fl.advectVelocity(dt, tU, tU, tf, "eulerFluidNet", 1, 0.6))
        div = fl.velocityDivergence(tU, tf)
        o["divergence"] = N(div)
        o["jacobi"] = N(fl.solveLinearSystemJacobi(tf, div, True, 0.0, 9)[0])
        Uu = tU.clone(); fl.velocityUpdate(tp, Uu, tf); o["velocity_update"] = N(Uu)
        Ub = tU.clone(); fl.addBuoyancy(Ub, tf, trho, g, rstar, dt); o["add_buoyancy"] = N(Ub)
        Ug = tU.clone(); fl.addGravity(Ug, tf, g, dt); o["add_gravity"] = N(Ug)
        Uw = tU.clone(); fl.setWallBcs(Uw, tf); o["set_wall_bcs"] = N(Uw)
        return o
    a, b = run(s, grav), run(sp, gravp)
    # Where the reference's rules are anisotropic BY CONSTRUCTION the exchange cannot hold and the cells are left out:
    #  * the fluid-aware interpolation of advectScalar pairs the corners y first, then x, then z (grid.cpp:118-269) and falls
    #    back corner by corner next to non-fluid cells, the line trace backs off along an axis-ordered box test, and a
    #    non-fluid cell of advectVel receives the reference's channel shuffle (fluids_init.cpp:413-416): the advection
    #    operators are compared on the cells whose 5x5x5 neighbourhood is fluid (CFL < 1 here);
    #  * setWallBcs at index 0: the x / y neighbour clamps to the cell itself, the z rule needs k > 0.
    fl3 = back(s["flags"]) == 1.0
    deep = fl3.copy()
    for ax in (2, 3, 4):                                  # separable erosion: the full 5x5x5 cube, diagonals included
        cur = deep.copy()
        for sh in (-2, -1, 1, 2):
            deep &= np.roll(cur, sh, axis=ax)
    deep[:, :, :2] = False; deep[:, :, -2:] = False; deep[:, :, :, :2] = False; deep[:, :, :, -2:] = False
    deep[..., :2] = False; deep[..., -2:] = False
    assert deep.mean() > 0.1
    for k in a:
        want, got = back(a[k]), b[k]                      # operator(exchanged state) vs exchanged(operator(state))
        sel = np.ones(want.shape, bool)
        if k.startswith("advect"):
            sel = np.broadcast_to(deep, want.shape)
        if k == "set_wall_bcs":
            sel = sel.copy(); sel[:, :, 0] = False; sel[:, :, :, 0] = False; sel[..., 0] = False
        scale = max(float(np.abs(want).max()), 1e-30)
        d = np.abs(want.astype(np.float64) - got)[sel]
        frac_bad = float((d > 2e-6 * scale).mean())
        assert frac_bad <= 1e-3, f"{k} under {perm} exchange: {frac_bad:.2%} of the compared cells differ by more than rounding (max {d.max():.3e}, scale {scale:.3e})"


# ---- CNN --------------------------------------------------------------------------------------------
def test_cnn_vs_reference_golden(dev, golden):
    """MultiScaleNet / FluidNet.forward vs torch-2.10-CPU golden vectors: |d| <= 1e-5 * |ref|max, relative to the
    reference's own magnitude (fp32 convolutions with a different summation order)."""
    from fluidnet_cxx_amd import FluidNet
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    c = golden("cnn")
    mconf = dict(model="ScaleNet", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True,
                 normalizeInputChan="UDiv", normalizeInputThreshold=1e-5, is3D=False)
    net = FluidNet.from_weights(mconf, make_scalenet_weights(0), dev)
    out = net.multiScale(T(c["x"], dev))
    assert_close_rel(N(out), c["multiscale"], 1e-5, "MultiScaleNet")
    p, U = net(T(c["fluidnet_in"], dev))
    assert_close_rel(N(p), c["fluidnet_p"], 1e-5, "FluidNet p"); assert_close_rel(N(U), c["fluidnet_U"], 1e-5, "FluidNet U")


@pytest.mark.parametrize("shape", [(1, 1, 36, 52), (2, 1, 64, 128), (1, 8, 12, 16), (1, 1, 44, 200), (1, 6, 20, 72)])
def test_cnn_vs_oracle(dev, oracle, shape):
    from fluidnet_cxx_amd import FluidNet
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    B, D, H, W = shape
    is3d = D > 1
    w = make_scalenet_weights(0, ndim=3 if is3d else 2)
    mconf = dict(model="ScaleNet", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True,
                 normalizeInputChan="UDiv", normalizeInputThreshold=1e-5, is3D=is3d)
    net = FluidNet.from_weights(mconf, w, dev)
    s = random_state(B, D, H, W, 0.5, seed=11)
    inp = np.concatenate([np.zeros_like(s["p"]), s["U"], s["flags"], s["rho"]], 1)
    p, U = net(T(inp, dev))
    blob = oracle.pack_weights(w, 3 if is3d else 2)
    po, Uo = oracle.fluidnet_forward(blob, inp)
    assert_close_rel(N(p), po, 1e-5, "FluidNet p"); assert_close_rel(N(U), Uo, 1e-5, "FluidNet U")


@pytest.mark.parametrize("shape", [(1, 1, 515, 509), (2, 1, 384, 352), (1, 16, 126, 130)])
def test_cnn_winograd_layers_vs_oracle(dev, oracle, shape):
    """Grids large enough for the full-resolution 3x3 layers to take the Winograd kernels (>= 1024 tiles; both the
    64-channel-group and the 32-channel instantiation), with partial tiles, an odd width and an odd height."""
    from fluidnet_cxx_amd import FluidNet
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    B, D, H, W = shape
    is3d = D > 1
    nd = 3 if is3d else 2
    w = make_scalenet_weights(0, ndim=nd)
    mconf = dict(model="ScaleNet", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True,
                 normalizeInputChan="UDiv", normalizeInputThreshold=1e-5, is3D=is3d)
    net = FluidNet.from_weights(mconf, w, dev)
    s = random_state(B, D, H, W, 0.5, seed=12)
    inp = np.concatenate([np.zeros_like(s["p"]), s["U"], s["flags"], s["rho"]], 1)
    p, U = net(T(inp, dev))
    po, Uo = oracle.fluidnet_forward(oracle.pack_weights(w, nd), inp)
    assert_close_rel(N(p), po, 1e-5, "FluidNet p"); assert_close_rel(N(U), Uo, 1e-5, "FluidNet U")
    if not is3d:
        # the MultiScaleNet alone, on inputs of O(1) magnitude
        x = np.random.default_rng(3).standard_normal((B, 2, 1, H, W)).astype(np.float32)
        assert_close_rel(N(net.multiScale(T(x, dev))), oracle.multiscale_forward(oracle.pack_weights(w, 2), x), 1e-5, "MultiScaleNet")


@pytest.mark.parametrize("shape", [(1, 1, 515, 509), (2, 1, 384, 352), (1, 1, 1024, 1024), (3, 1, 130, 700), (1, 16, 126, 130), (2, 5, 200, 96),
                                   (1, 4, 64, 512)])
def test_cnn_f4_vs_oracle(dev, oracle, shape):
    """FNX_PRECISION_FP32_F4: the 64- / 128-output-channel 3x3 layers of a 2D net in the Winograd F(4x4,3x3) domain (conv3_wino4_kernel,
    v_mfma_f32_16x16x4_f32; every other layer as in 'fp32') against the oracle at the modes' common tolerance 1e-5 |ref|max: partial
    tiles in x and y, odd sizes, batch, the benchmark size, and 3D nets (F(4x4) in (y, x), the three z taps as stages; boundary planes skip a tap).
    Since round 6 this is what the default mode 'fp32' runs; 'fp32_f2' keeps F(2x2) everywhere."""
    from fluidnet_cxx_amd import FluidNet
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    B, D, H, W = shape
    is3d = D > 1
    nd = 3 if is3d else 2
    w = make_scalenet_weights(0, ndim=nd)
    mconf = dict(model="ScaleNet", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True,
                 normalizeInputChan="UDiv", normalizeInputThreshold=1e-5, is3D=is3d)
    net = FluidNet.from_weights(dict(mconf, precisionMode="fp32_f4"), w, dev)
    x = np.random.default_rng(5).standard_normal((B, 2, D, H, W)).astype(np.float32)
    got = N(net.multiScale(T(x, dev) if is3d else T(x[:, :, 0], dev))).reshape(B, 1, D, H, W)
    if is3d:
        # 3D: F(4x4) in (y, x), the z taps as stages (launches that fill the chip; the coarser scales stay on the F(2x2) / direct kernels)
        want = oracle.multiscale_forward(oracle.pack_weights(w, 3), x)
        assert_close_rel(got, want, 1e-5, "3D MultiScaleNet, F(4x4) layers")
        assert_bitexact(got, N(FluidNet.from_weights(mconf, w, dev).multiScale(T(x, dev))).reshape(B, 1, D, H, W), "3D: the default mode IS fp32_f4")
        ref32 = FluidNet.from_weights(dict(mconf, precisionMode="fp32_f2"), w, dev)
        assert not np.array_equal(got, N(ref32.multiScale(T(x, dev))).reshape(B, 1, D, H, W)), "3D: the F(4x4) kernel did not run"
        return
    if H * W <= 600 * 600:
        want = oracle.multiscale_forward(oracle.pack_weights(w, 2), x)
        assert_close_rel(got, want, 1e-5, "MultiScaleNet, F(4x4) layers")
        assert_bitexact(got, N(FluidNet.from_weights(mconf, w, dev).multiScale(T(x[:, :, 0], dev))).reshape(B, 1, D, H, W), "the default mode IS fp32_f4")
        ref32 = FluidNet.from_weights(dict(mconf, precisionMode="fp32_f2"), w, dev)
        assert not np.array_equal(got, N(ref32.multiScale(T(x[:, :, 0], dev))).reshape(B, 1, D, H, W)), "2D: the F(4x4) kernel did not run"
    else:
        # benchmark size: against the F(2x2) mode, both within 1e-5 of the oracle (test_cnn_benchmark_size pins the default at this size)
        ref32 = FluidNet.from_weights(dict(mconf, precisionMode="fp32_f2"), w, dev)
        want = N(ref32.multiScale(T(x[:, :, 0], dev))).reshape(B, 1, D, H, W)
        assert_close_rel(got, want, 2e-5, "MultiScaleNet at 1024^2: F(4x4) against F(2x2)")
    if shape == (1, 1, 515, 509):
        s = random_state(B, D, H, W, 0.5, seed=12)
        inp = np.concatenate([np.zeros_like(s["p"]), s["U"], s["flags"], s["rho"]], 1)
        p, U = net(T(inp, dev))
        po, Uo = oracle.fluidnet_forward(oracle.pack_weights(w, nd), inp)
        assert_close_rel(N(p), po, 1e-5, "FluidNet p"); assert_close_rel(N(U), Uo, 1e-5, "FluidNet U")


def test_cnn_rejects_a_grid_the_net_cannot_take(dev):
    """A 3D grid with fewer than 4 planes has no quarter-resolution scale: the entry point refuses it with ITS OWN message (round 6: a
    failed launch used to surface whatever text the thread's last error had left -- a jacobi_pass message from an earlier test)."""
    from fluidnet_cxx_amd import FluidNet
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    mconf = dict(model="ScaleNet", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True,
                 normalizeInputChan="UDiv", normalizeInputThreshold=1e-5, is3D=True)
    net = FluidNet.from_weights(mconf, make_scalenet_weights(0, ndim=3), dev)
    with pytest.raises(RuntimeError, match="at least 4 cells per axis"):
        net.multiScale(torch.zeros(1, 2, 3, 64, 64, device=dev))


@pytest.mark.parametrize("shape", [(1, 1, 515, 509), (2, 1, 384, 352), (1, 16, 126, 130), (1, 6, 72, 300)])
def test_cnn_bf16x3_vs_oracle(dev, oracle, shape):
    """precisionMode 'bf16x3' (FNX_PRECISION_BF16X3: the same layers with the three bf16 products that involve no low piece, ah*bh +
    ah*bm + am*bh): an "accurate bf16" mode under its OWN label and tolerance -- 1e-4 of |ref|max against the oracle (the exact modes
    and bf16x6: 1e-5) -- on the shapes of the bf16x6 test; another kernel instantiation than bf16x6's (different bits), and its error
    stays well inside its tolerance (it measures 1.6e-5 .. 3e-5 of |ref|max: 16 significand bits per product, random signs)."""
    from fluidnet_cxx_amd import FluidNet
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    B, D, H, W = shape
    is3d = D > 1
    nd = 3 if is3d else 2
    w = make_scalenet_weights(0, ndim=nd)
    s = random_state(B, D, H, W, 0.5, seed=12)
    inp = np.concatenate([np.zeros_like(s["p"]), s["U"], s["flags"], s["rho"]], 1)
    po, Uo = oracle.fluidnet_forward(oracle.pack_weights(w, nd), inp)
    outs = {}
    for mode in ("bf16x3", "bf16x6"):
        mconf = dict(model="ScaleNet", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True,
                     normalizeInputChan="UDiv", normalizeInputThreshold=1e-5, is3D=is3d, precisionMode=mode)
        net = FluidNet.from_weights(mconf, w, dev)
        p, U = net(T(inp, dev))
        outs[mode] = N(p)
        tol = 1e-4 if mode == "bf16x3" else 1e-5
        assert_close_rel(N(p), po, tol, f"FluidNet p ({mode})"); assert_close_rel(N(U), Uo, tol, f"FluidNet U ({mode})")
    assert not np.array_equal(outs["bf16x3"], outs["bf16x6"]), "precisionMode='bf16x3' did not select another kernel"
    e3 = np.abs(outs["bf16x3"].astype(np.float64) - po).max()
    assert e3 <= 5e-5 * np.abs(po).max(), f"bf16x3 error {e3:.3e} = {e3 / np.abs(po).max():.2e} of |ref|max: more than the mode should cost"
    with pytest.raises(RuntimeError, match="precision_mode"):
        FluidNet.from_weights(dict(mconf, precisionMode="bf16x2"), w, dev)(T(inp, dev))


@pytest.mark.parametrize("shape", [(1, 1, 515, 509), (2, 1, 384, 352), (1, 16, 126, 130), (1, 6, 72, 300)])
def test_cnn_bf16x6_vs_oracle(dev, oracle, shape):
    """precisionMode 'bf16x6' (FNX_PRECISION_BF16X6: the 64/128-output-channel Winograd layers as six bf16 MFMA products per fp32
    product, conv3_wbf_kernel) at the SAME tolerance as the exact-fp32 modes -- 1e-5 of |ref|max against the oracle -- on grids
    with partial tiles, odd sizes, batch 2, 3D (z borders: two- and three-plane stage lists); and it is another kernel than the
    default's (different bits), no further from the oracle than a few times the default is."""
    from fluidnet_cxx_amd import FluidNet
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    B, D, H, W = shape
    is3d = D > 1
    nd = 3 if is3d else 2
    w = make_scalenet_weights(0, ndim=nd)
    s = random_state(B, D, H, W, 0.5, seed=12)
    inp = np.concatenate([np.zeros_like(s["p"]), s["U"], s["flags"], s["rho"]], 1)
    po, Uo = oracle.fluidnet_forward(oracle.pack_weights(w, nd), inp)
    outs = {}
    for mode in ("bf16x6", "fp32"):
        mconf = dict(model="ScaleNet", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True,
                     normalizeInputChan="UDiv", normalizeInputThreshold=1e-5, is3D=is3d, precisionMode=mode)
        net = FluidNet.from_weights(mconf, w, dev)
        p, U = net(T(inp, dev))
        outs[mode] = N(p)
        assert_close_rel(N(p), po, 1e-5, f"FluidNet p ({mode})"); assert_close_rel(N(U), Uo, 1e-5, f"FluidNet U ({mode})")
    assert not np.array_equal(outs["bf16x6"], outs["fp32"]), "precisionMode='bf16x6' did not select another kernel"
    e6 = np.abs(outs["bf16x6"].astype(np.float64) - po).max(); e32 = np.abs(outs["fp32"].astype(np.float64) - po).max()
    assert e6 <= 4.0 * e32 + 1e-7 * np.abs(po).max(), f"bf16x6 is {e6 / max(e32, 1e-300):.1f}x further from the oracle than fp32 ({e6:.3e} vs {e32:.3e})"
    # the MultiScaleNet alone, on inputs of O(1) magnitude
    x = np.random.default_rng(3).standard_normal((B, 2, D, H, W)).astype(np.float32)
    xt = T(x, dev) if is3d else T(x[:, :, 0], dev)
    want = oracle.multiscale_forward(oracle.pack_weights(w, nd), x)
    assert_close_rel(N(net.multiScale(xt)).reshape(want.shape), want, 1e-5, "MultiScaleNet")


@pytest.mark.parametrize("case", ["middle", "bottom", "top", "batch2_bf16x6"])
def test_multiscale_forward_nested_crops_vs_oracle(dev, oracle, ext, case):
    """fnx_multiscale_forward_crop (a z-slab rank's window: quarter-resolution tower on owned +- 48 planes, half- / full-resolution
    towers on owned +- 24 / 8) against the oracle's towers on the same nested windows -- every plane of the result, 1e-5 of
    |ref|max -- and, on the owned planes, against the UNTRIMMED pass over the whole domain (what the margins are for); a window
    that ends at a domain face is not trimmed there.  Refusals: trims that are not multiples of 4 or not nested."""
    from fluidnet_cxx_amd import FluidNet
    from fluidnet_cxx_amd.slab import SlabSimulator as S
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    G, MF, MH = S.NET_MARGIN, S.NET_MARGIN_FULL, S.NET_MARGIN_HALF
    B = 2 if case.startswith("batch2") else 1
    Dg, H, W, owned = 160, 16, 24, 16
    own = dict(middle=(72, 88), bottom=(0, 16), top=(144, 160), batch2_bf16x6=(72, 88))[case]
    e0, e1 = max(own[0] - G, 0), min(own[1] + G, Dg)
    cut_lo, cut_hi = own[0] - e0 == G, e1 - own[1] == G
    trim = [G - MF if cut_lo else 0, G - MF if cut_hi else 0, G - MH if cut_lo else 0, G - MH if cut_hi else 0]
    w = make_scalenet_weights(0, ndim=3)
    blob = oracle.pack_weights(w, 3)
    rng = np.random.default_rng(21)
    x = rng.standard_normal((B, 2, Dg, H, W)).astype(np.float32)
    x[:, 1] = rng.random((B, Dg, H, W)) < 0.1
    xw = np.ascontiguousarray(x[:, :, e0:e1])
    mconf = dict(model="ScaleNet", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True, normalizeInputChan="UDiv",
                 normalizeInputThreshold=1e-5, is3D=True, precisionMode="bf16x6" if case.endswith("bf16x6") else "fp32")
    net = FluidNet.from_weights(mconf, w, dev)
    got = N(net.multiScale(T(xw, dev), trim))
    want = oracle.multiscale_forward_crop(blob, xw, trim)
    assert got.shape == want.shape == (B, 1, e1 - e0 - trim[0] - trim[1], H, W)
    assert_close_rel(got, want, 1e-5, f"nested crops ({case}) vs the oracle's")
    full = oracle.multiscale_forward(blob, x, True)
    lo = e0 + trim[0]
    assert_close_rel(got[:, :, own[0] - lo:own[1] - lo], full[:, :, own[0]:own[1]], 1e-5, f"nested crops ({case}): owned planes vs the whole domain")
    if case == "middle":
        assert_bitexact(N(net.multiScale(T(xw, dev), [0, 0, 0, 0])), N(net.multiScale(T(xw, dev))), "no trim = the plain pass")
        for bad in ([40, 40, 22, 24], [40, 40, 44, 24], [-4, 40, 0, 24], [56, 56, 24, 24]):
            with pytest.raises(RuntimeError):
                net.multiScale(T(xw, dev), bad)


def test_fluidnet_built_like_the_reference_driver(dev, golden):
    """plume.py:119-123 verbatim: FluidNet(mconf, dropout=False) -> .cuda() -> .load_state_dict(state['state_dict']) ->
    forward; and a net moved / reloaded after its first forward repacks its weights."""
    from fluidnet_cxx_amd import FluidNet
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    c = golden("cnn")
    mconf = dict(model="ScaleNet", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True,
                 normalizeInputChan="UDiv", normalizeInputThreshold=1e-5, is3D=False, inputDim=2)
    state = {"state_dict": {k: torch.from_numpy(v) for k, v in make_scalenet_weights(0).items()}}
    net = FluidNet(mconf, dropout=False)
    if torch.cuda.is_available():
        net = net.cuda()
    net.load_state_dict(state["state_dict"])
    net.eval()
    p, U = net(T(c["fluidnet_in"], dev))
    assert_close_rel(N(p), c["fluidnet_p"], 1e-5, "FluidNet p"); assert_close_rel(N(U), c["fluidnet_U"], 1e-5, "FluidNet U")
    assert all(v.is_cuda for v in net.state_dict().values())
    other = {k: torch.from_numpy(v) for k, v in make_scalenet_weights(1).items()}
    net.load_state_dict(other)
    p2, _ = net(T(c["fluidnet_in"], dev))
    assert not torch.equal(p, p2), "load_state_dict after a forward did not repack the weights"
    net.load_state_dict(state["state_dict"])
    p3, _ = net(T(c["fluidnet_in"], dev))
    assert torch.equal(p, p3)


def test_raw_c_abi_jacobi_through_ctypes(dev, oracle):
    """The drop-in boundary without the torch shim: fnx_workspace_bytes + fnx_jacobi called through ctypes on raw device
    pointers (tensor.data_ptr()) and the null stream, compared with the oracle bit for bit; plus the error convention
    (status code + fnx_last_error)."""
    import ctypes
    from fluidnet_cxx_amd import build

    class FnxGrid(ctypes.Structure):
        _fields_ = [(n, ctypes.c_int) for n in ("B", "D", "H", "W", "is3D", "ref_quirks", "z_offset", "D_global", "k_begin", "k_end")]

    lib = ctypes.CDLL(build.LIB)
    lib.fnx_workspace_bytes.restype = ctypes.c_size_t
    lib.fnx_workspace_bytes.argtypes = [ctypes.POINTER(FnxGrid), ctypes.c_int]
    lib.fnx_last_error.restype = ctypes.c_char_p
    lib.fnx_jacobi.restype = ctypes.c_int
    lib.fnx_jacobi.argtypes = [ctypes.POINTER(FnxGrid)] + [ctypes.c_void_p] * 4 + [ctypes.c_float, ctypes.c_int,
                               ctypes.POINTER(ctypes.c_int), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    for (B, D, H, W) in ((2, 1, 50, 77), (1, 9, 20, 66)):
        is3d = D > 1
        s = random_state(B, D, H, W, 2.0, seed=21)
        div = oracle.velocity_divergence(s["U"], s["flags"])
        g = FnxGrid(B, D, H, W, int(is3d), 0, 0, 0, 0, 0)
        nbytes = lib.fnx_workspace_bytes(ctypes.byref(g), 2)         # FNX_OP_JACOBI
        assert nbytes > 0
        tf, td = T(s["flags"], dev), T(div, dev)
        p = torch.empty_like(tf); res = torch.zeros(1, device=dev); ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        iters = ctypes.c_int(0)
        torch.cuda.synchronize()
        rc = lib.fnx_jacobi(ctypes.byref(g), tf.data_ptr(), td.data_ptr(), p.data_ptr(), res.data_ptr(), 0.0, 13,
                            ctypes.byref(iters), ws.data_ptr(), nbytes, None)
        assert rc == 0, lib.fnx_last_error()
        torch.cuda.synchronize()
        po, ro, _ = oracle.jacobi(s["flags"], div, is3d, 0.0, 13)
        assert iters.value == 13
        assert_bitexact(N(p), po, f"raw C-ABI fnx_jacobi {(B, D, H, W)}")
        assert abs(float(res) - ro) <= 1e-5 * max(1.0, ro)
        rc = lib.fnx_jacobi(ctypes.byref(g), tf.data_ptr(), td.data_ptr(), p.data_ptr(), None, 0.0, 0, None, ws.data_ptr(), nbytes, None)
        assert rc == 1 and b"At least 1 iteration" in lib.fnx_last_error()          # FNX_EINVAL
        rc = lib.fnx_jacobi(ctypes.byref(g), tf.data_ptr(), td.data_ptr(), p.data_ptr(), None, 0.0, 3, None, ws.data_ptr(), 16, None)
        assert rc == 3 and b"workspace too small" in lib.fnx_last_error()           # FNX_EWORKSPACE


@pytest.mark.parametrize("shape", [(1, 1024, 1024), (256, 256, 256)])
def test_cnn_benchmark_size(dev, oracle, tmp_path, shape):
    """The CNN at the sizes bench.py times (configs[1] 1024^2, configs[3] 256^3): the launch geometries there (tile
    counts, 8-wave Winograd workgroups, multi-GiB ping-pong buffers) are otherwise only timed.
      (1) the whole field of the Winograd path against the direct implicit-GEMM MFMA kernels (precision_mode "fp32_direct")
          -- two independent kernel families, 1e-5 of |ref|max;
      (2) the oracle on crops: MultiScaleNet is local (receptive field < 48 cells at full resolution) and its resampling
          grids align for offsets that are multiples of 4, so the oracle on a crop must agree with the full-field result
          away from the crop's artificial edges -- domain corners / edges (true zero padding) and the interior."""
    from cnn_forward_helper import forward, make_input
    D, H, W = shape
    is3d = D > 1
    x = make_input(D, H, W, seed=5)
    got = forward(x)
    assert np.isfinite(got).all()
    direct = forward(x, precision_mode="fp32_direct")
    torch.cuda.empty_cache()
    assert not np.array_equal(got, direct), "precision_mode='fp32_direct' did not select another kernel"
    assert_close_rel(got, direct, 1e-5, f"Winograd vs direct MFMA conv at {shape}")
    # (3) the opt-in bf16x6 mode (six bf16 MFMA products per fp32 product) over the whole field, same tolerance
    b6 = forward(x, precision_mode="bf16x6")
    torch.cuda.empty_cache()
    assert not np.array_equal(got, b6), "precision_mode='bf16x6' did not select another kernel"
    assert_close_rel(b6, direct, 1e-5, f"bf16x6 Winograd vs direct MFMA conv at {shape}")
    # (4) the opt-in bf16x3 mode (the three products without a low piece): its own, looser tolerance
    b3 = forward(x, precision_mode="bf16x3")
    torch.cuda.empty_cache()
    assert not np.array_equal(b3, b6), "precision_mode='bf16x3' did not select another kernel"
    assert_close_rel(b3, direct, 1e-4, f"bf16x3 Winograd vs direct MFMA conv at {shape}")
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    blob = oracle.pack_weights(make_scalenet_weights(0, ndim=3 if is3d else 2), 3 if is3d else 2)
    M = 48                                                           # margin kept from a crop's artificial edges
    if is3d:
        crops = [((0, 64), (0, 72), (0, 80)), ((D - 64, D), (H - 72, H), (W - 80, W))]
    else:
        crops = [((0, 1), (0, 256), (0, 256)), ((0, 1), (H - 256, H), (W - 256, W)), ((0, 1), (384, 640), (512, 768)),
                 ((0, 1), (0, 192), (400, 720))]
    scale = float(np.abs(got).max())
    for (z0, z1), (y0, y1), (x0, x1) in crops:
        xc = np.ascontiguousarray(x[:, :, z0:z1, y0:y1, x0:x1])
        po = oracle.multiscale_forward(blob, xc)

        def valid(a0, a1, n):                                        # the part of [a0, a1) whose receptive field lies in the crop
            lo = a0 if a0 == 0 else a0 + M
            hi = a1 if a1 == n else a1 - M
            return lo, hi
        (vz0, vz1), (vy0, vy1), (vx0, vx1) = (valid(z0, z1, D) if is3d else (0, 1)), valid(y0, y1, H), valid(x0, x1, W)
        b = po[:, :, vz0 - z0:vz1 - z0, vy0 - y0:vy1 - y0, vx0 - x0:vx1 - x0]
        # every precision mode DIRECTLY against the oracle (not through another HIP kernel): fp32 and bf16x6 at 1e-5, bf16x3 at 1e-4
        for what, field, tol in (("fp32", got, 1e-5), ("bf16x6", b6, 1e-5), ("bf16x3", b3, 1e-4)):
            a = field[:, :, vz0:vz1, vy0:vy1, vx0:vx1]
            assert a.size > 0
            d = float(np.abs(a.astype(np.float64) - b).max())
            assert d <= tol * scale, f"{what}, crop z{z0}:{z1} y{y0}:{y1} x{x0}:{x1}: max |d| = {d:.3e} > {tol:.0e} * {scale:.3e}"


def test_sim64_convnet_vs_reference(dev, golden):
    from fluidnet_cxx_amd import FluidNet, simulate
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    s = golden("sim64")
    mconf = dict(PLUME_CFG, model="ScaleNet", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True,
                 normalizeInputChan="UDiv", is3D=False)
    net = FluidNet.from_weights(mconf, make_scalenet_weights(0), dev)
    for fused in (True, False):
        bd = to_dev(plume_state(64), dev)
        for it in range(1, 11):
            simulate(mconf, bd, net, "convnet", fused=fused)
            if it in (1, 3, 10):
                for k in ("U", "density", "p"):
                    assert_close_rel(N(bd[k]), s[f"convnet_{k}_{it}"], 1e-5, f"convnet {k} after {it} (fused={fused})")


def test_static_flags_reuses_mask_3d(dev, oracle, ext):
    """3D fused step with a caller-owned workspace: static_flags=True (mask kept from the previous step) gives the
    same bits as rebuilding it, and both match the oracle."""
    from fluidnet_cxx_amd import simulate
    cfg = dict(PLUME_CFG, jacobiIter=7)
    runs = []
    for static in (False, True, "bcs"):
        bd = to_dev(plume_state(24, D=12), dev)
        ws = torch.empty(ext.step_workspace_bytes(1, 12, 24, 24, True), dtype=torch.uint8, device=dev)
        for it in range(4):
            # "bcs": also the BC arrays are promised static -> class map built at step 2 (3), reused afterwards (7)
            sf = (0, 3, 7, 7)[it] if static == "bcs" else (static and it > 0)
            simulate(cfg, bd, None, "jacobi", workspace=ws, static_flags=sf)
        runs.append({k: N(bd[k]) for k in ("U", "density", "p")})
    st = plume_state(24, D=12)
    for it in range(4):
        st = oracle.simulate_step(st, cfg, "jacobi")
    for k in ("U", "density", "p"):
        assert_bitexact(runs[0][k], st[k], f"{k} (mask rebuilt)")
        assert_bitexact(runs[1][k], st[k], f"{k} (mask reused)")
        assert_bitexact(runs[2][k], st[k], f"{k} (mask and BC class map reused)")


@pytest.mark.parametrize("D", [14, 1])
def test_four_argument_simulate_detects_static_inputs(dev, oracle, ext, fl, monkeypatch, D):
    """The reference's own call -- simulate(mconf, batch_dict, net, method), four arguments (plume.py:237): the layer keeps the step
    workspace and derives FnxStepParams.static_flags from (data_ptr, _version) of flags and the BC arrays.  The bits climb 0 -> 3 -> 7
    on untouched inputs and fall back whenever one is written in place: an obstacle inserted between steps 5 and 6 (torch indexing),
    the inlet velocity changed between steps 7 and 8, flags reset by this package's own in-place generator (emptyDomain) between
    steps 9 and 10, and a NEW flags tensor with the old one's contents at step 11.  Every step bit-identical to the oracle, which
    gets the same edits."""
    from fluidnet_cxx_amd import _simulate, simulate
    _simulate.release_workspaces()
    res = 26
    cfg = dict(PLUME_CFG, jacobiIter=9)
    st = plume_state(res, D=D)
    bd = to_dev(st, dev)
    seen = []
    real = ext.simulate_step_

    def spy(*a, **k):
        seen.append(a[20])                                   # the static_flags argument
        return real(*a, **k)
    monkeypatch.setattr(_simulate.ext, "simulate_step_", spy)
    zs = slice(5, 9) if D > 1 else slice(None)
    for step in range(1, 13):
        if step == 6:                                        # an obstacle, in place
            bd["flags"][:, :, zs, 12:16, 9:14] = 2.0
            st["flags"] = st["flags"].copy(); st["flags"][:, :, zs, 12:16, 9:14] = 2.0
        if step == 8:                                        # a faster inlet, in place
            bd["UBC"].mul_(1.5)
            st["UBC"] = st["UBC"] * np.float32(1.5)
        if step == 10:                                       # the native in-place generator: the obstacle is gone again
            fl.emptyDomain(bd["flags"])
            st["flags"] = make_flags(1, D, res, res, boxes=False)
        if step == 11:                                       # a new tensor, same contents
            bd["flags"] = bd["flags"].clone()
        simulate(cfg, bd, None, "jacobi")
        st = oracle.simulate_step(st, cfg, "jacobi")
        for k in ("U", "density", "p"):
            assert_bitexact(N(bd[k]), st[k], f"{k} after step {step} (D={D})")
    #        step:  1  2  3  4  5 | 6 obstacle: the BC map stays | 8 inlet: the mask stays, map rebuilt at 9 | 10 flags | 11 new tensor
    assert seen == [0, 3, 7, 7, 7, 6, 7, 1, 3, 6, 6, 7], seen
    # an explicit static_flags / workspace still wins, and geom switches the automatic mode off
    seen.clear()
    simulate(cfg, bd, None, "jacobi", static_flags=0)
    ws = torch.empty(ext.step_workspace_bytes(1, D, res, res, D > 1), dtype=torch.uint8, device=dev)
    simulate(cfg, bd, None, "jacobi", workspace=ws)
    simulate(cfg, bd, None, "jacobi", workspace=ws, static_flags=True)
    if D > 1:
        simulate(cfg, bd, None, "jacobi", geom=ext.Geom())
    assert seen == [0, 0, 1] + ([0] if D > 1 else []), seen
    # forget_static_inputs(): after a write torch's counter cannot see (here through .data) the caller says so
    simulate(cfg, bd, None, "jacobi"); simulate(cfg, bd, None, "jacobi"); simulate(cfg, bd, None, "jacobi")
    seen.clear()
    bd["flags"].data[:, :, zs, 6:9, 6:9] = 2.0              # (.data: no version bump)
    _simulate.forget_static_inputs()
    simulate(cfg, bd, None, "jacobi")
    assert seen == [0], seen
    _simulate.release_workspaces()


@pytest.mark.parametrize("shape", [(2, 1, 40, 70), (1, 10, 20, 66)])
@pytest.mark.parametrize("method", ["jacobi", "convnet"])
def test_bc_class_map_same_bits(dev, ext, shape, method):
    """The BC stages with the class map of static BC arrays (identity cells skip their 8 BC loads) give the same bits as
    without, on random BC arrays: masks in {0, 1, 0.5}, values in {+0, -0, random} (a -0 value is NOT the identity:
    x + -0 keeps a -0 that x + 0 turns into +0), through the fused step of both methods and the two stage entry points."""
    from fluidnet_cxx_amd import FluidNet, simulate
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    B, D, H, W = shape
    is3d = D > 1
    rng = np.random.default_rng(8)
    s = random_state(B, D, H, W, 1.0, seed=31)
    nc = 3 if is3d else 2

    def bc(shape_):
        m = rng.choice(np.array([0.0, 1.0, 1.0, 1.0, 0.5], np.float32), size=shape_)
        v = rng.choice(np.array([0.0, 0.0, 0.0, -0.0, 1.0], np.float32), size=shape_) * rng.standard_normal(shape_).astype(np.float32)
        v[rng.random(shape_) < 0.5] = 0.0
        v[rng.random(shape_) < 0.05] = -0.0
        return m.astype(np.float32), v.astype(np.float32)
    UM, UV = bc((B, nc, D, H, W)); RM, RV = bc((B, 1, D, H, W))
    st0 = dict(p=np.zeros((B, 1, D, H, W), np.float32), U=s["U"] * 0.2, flags=s["flags"], density=s["rho"], UBC=UV, UBCInvMask=UM,
               densityBC=RV, densityBCInvMask=RM)
    cfg = dict(PLUME_CFG, jacobiIter=5, model="ScaleNet", inputChannels=dict(div=True, pDiv=False, UDiv=False),
               normalizeInput=True, normalizeInputChan="UDiv", is3D=is3d)
    net = FluidNet.from_weights(cfg, make_scalenet_weights(0, ndim=3 if is3d else 2), dev) if method == "convnet" else None
    runs = []
    for static in (False, True):
        bd = to_dev(st0, dev)
        ws = torch.empty(ext.step_workspace_bytes(B, D, H, W, is3d), dtype=torch.uint8, device=dev)
        for it in range(3):
            simulate(cfg, bd, net, method, workspace=ws, static_flags=(0, 3, 7)[it] if static else 0)
        runs.append({k: bd[k].clone() for k in ("U", "density", "p")})
    for k in ("U", "density", "p"):
        assert torch.equal(runs[0][k].view(torch.int32), runs[1][k].view(torch.int32)), f"{method} {k}: bits differ with the class map"
    # the stage entry points with an explicit class map
    bd = to_dev(st0, dev)
    cls = ext.bc_classify(bd["flags"], is3d, bd["UBC"], bd["UBCInvMask"], bd["densityBC"], bd["densityBCInvMask"])
    assert 0.02 < float((cls & 1).float().mean()) < 0.9 and 0.1 < float(((cls >> 1) & 1).float().mean()) < 0.9   # both classes occur
    Uadv, radv = T(s["U"] * 0.3, dev), T(s["rho"] * 0.7, dev)
    outs = []
    for c in (None, cls):
        b2 = {k: v.clone() for k, v in bd.items()}
        div = ext.pre_projection_(Uadv, radv, b2["p"], b2["U"], b2["flags"], b2["density"], b2["UBC"], b2["UBCInvMask"],
                                  b2["densityBC"], b2["densityBCInvMask"], 0.1, 0.25, [0.0, -1.0, 0.2], 0.0, True, c)
        b2["p"].copy_(torch.randn_like(b2["p"]).mul_(0).add_(div))       # any pressure field: use div itself
        ext.post_projection_(b2["p"], b2["U"], b2["flags"], b2["density"], b2["UBC"], b2["UBCInvMask"], b2["densityBC"],
                             b2["densityBCInvMask"], c)
        outs.append((div, b2["U"], b2["density"]))
    for a, b_ in zip(*outs):
        assert torch.equal(a.view(torch.int32), b_.view(torch.int32))


@pytest.mark.parametrize("shape", [(2, 1, 40, 70, 3.0), (1, 9, 20, 66, 2.0), (2, 12, 21, 130, 0.8), (1, 16, 33, 70, 6.0),
                                   (1, 7, 9, 11, 1.5), (1, 20, 64, 200, 0.3), (1, 10, 30, 63, 0.0)])
def test_advect_step_equals_the_two_advections(fl, ext, dev, shape):
    """fnx_advect_step (the step's fused advection; in 3D the z-marching stencil kernels with their in-register fast path
    and per-cell fallback lanes) == advectScalar + advectVelocity (the per-cell kernels, themselves pinned to the goldens
    and the oracle), bit for bit: CFL from 0 (sigma 0: every trace stays) over the all-fast-path range to mostly-fallback
    (sigma 6), obstacles and Empty cells, several x tiles, odd sizes, batch 2, and a compute window."""
    B, D, H, W, sigma = shape
    s = random_state(B, D, H, W, sigma, seed=21, empties=True)
    tf, tU, trho = T(s["flags"], dev), T(s["U"], dev), T(s["rho"], dev)
    for so in (False, True):
        r, u = ext.advect_step(0.13, trho, tU, tf, so, 0.7)
        want_r = N(fl.advectScalar(0.13, trho, tU, tf, "maccormackFluidNet", 1, so, 0.7, plan="cells"))
        want_u = N(fl.advectVelocity(0.13, tU, tU, tf, "maccormackFluidNet", 1, 0.7, plan="cells"))
        assert_bitexact(N(r), want_r, f"density so={so}")
        assert_bitexact(N(u), want_u, f"U so={so}")
        if D >= 9 and sigma * 0.13 * 5 < 1.0:
            # compute window (valid for CFL < 1: the forward pass covers the window widened by 2 planes): planes [3, D-3) only,
            # the rest of the output untouched
            ro, uo = torch.full_like(trho, 9.0), torch.full_like(tU, 9.0)
            ext.advect_step(0.13, trho, tU, tf, so, 0.7, ro, uo, ext.Geom(k_begin=3, k_end=D - 3))
            assert_bitexact(N(ro)[:, :, 3:D - 3], want_r[:, :, 3:D - 3], "window density")
            assert_bitexact(N(uo)[:, :, 3:D - 3], want_u[:, :, 3:D - 3], "window U")
            assert (N(ro)[:, :, :3] == 9.0).all() and (N(ro)[:, :, D - 3:] == 9.0).all() and (N(uo)[:, :, :3] == 9.0).all()
    if D > 1:
        # every trace towards +x,+y,+z (and then towards -x,-y,-z): the last (first) interior cell samples the far (near)
        # corner cell of the arrays, where the tile loader's 16-byte chunks hang over the end (start) of the tensors
        for sign in (-1.0, 1.0):
            tUn = (tU.abs() * sign).contiguous()
            r, u = ext.advect_step(0.13, trho, tUn, tf, False, 0.7)
            assert_bitexact(N(r), N(fl.advectScalar(0.13, trho, tUn, tf, "maccormackFluidNet", 1, False, 0.7, plan="cells")), f"density, U sign {sign}")
            assert_bitexact(N(u), N(fl.advectVelocity(0.13, tUn, tUn, tf, "maccormackFluidNet", 1, 0.7, plan="cells")), f"U, U sign {sign}")


@pytest.mark.parametrize("shape", [(2, 40, 70, 3.0), (1, 96, 200, 0.4), (1, 33, 130, 0.8), (1, 17, 64, 0.0), (2, 64, 129, 6.0), (1, 150, 67, 1.5),
                                   (1, 16, 192, 0.6), (3, 35, 258, 1.0), (1, 1101, 1500, 0.9)])
def test_advect2d_tile_kernels_equal_the_cell_kernels(fl, ext, dev, oracle, shape):
    """The 2D LDS tile kernels (fnx_advect_step's plan on grids of >= 1.5 M cells, here forced: plan='tiles') == one thread
    per cell (plan='cells') == advectScalar + advectVelocity == the oracle, bit for bit: CFL from 0 over the all-fast-path
    range to mostly-fallback lanes, obstacles and Empty cells, one to five x tiles, partial tiles in x and y, batch 1-3, both
    sample_outside_fluid settings, and every trace towards one corner (the chunks that hang over the tensors' ends)."""
    B, H, W, sigma = shape
    s = random_state(B, 1, H, W, sigma, seed=23, empties=True)
    tf, tU, trho = T(s["flags"], dev), T(s["U"], dev), T(s["rho"], dev)
    for so in (False, True):
        rt, ut = ext.advect_step(0.13, trho, tU, tf, so, 0.7, plan="tiles")
        rc, uc = ext.advect_step(0.13, trho, tU, tf, so, 0.7, plan="cells")
        ra, ua = ext.advect_step(0.13, trho, tU, tf, so, 0.7)                  # the plan fnx_advect_step picks by grid size
        assert_bitexact(N(ra), N(rc), f"density so={so}: auto vs cells"); assert_bitexact(N(ua), N(uc), f"U so={so}: auto vs cells")
        assert_bitexact(N(rt), N(rc), f"density so={so}: tiles vs cells")
        assert_bitexact(N(ut), N(uc), f"U so={so}: tiles vs cells")
        assert_bitexact(N(rt), N(fl.advectScalar(0.13, trho, tU, tf, "maccormackFluidNet", 1, so, 0.7)), f"density so={so}")
        assert_bitexact(N(ut), N(fl.advectVelocity(0.13, tU, tU, tf, "maccormackFluidNet", 1, 0.7)), f"U so={so}")
        if sigma > 0:        # (sigma 0 is a field of +0 / -0: the clamp's min / max of equal zeros of either sign is the C library's choice on the CPU)
            assert_bitexact(N(rt), oracle.advect_scalar(0.13, s["rho"], s["U"], s["flags"], "maccormackFluidNet", 1, so, 0.7), f"density so={so} vs oracle")
    if sigma > 0:
        assert_bitexact(N(ut), oracle.advect_vel(0.13, s["U"], s["U"], s["flags"], "maccormackFluidNet", 1, 0.7), "U vs oracle")
    for sign in (-1.0, 1.0):
        tUn = (tU.abs() * sign).contiguous()
        rt, ut = ext.advect_step(0.13, trho, tUn, tf, False, 0.7, plan="tiles")
        rc, uc = ext.advect_step(0.13, trho, tUn, tf, False, 0.7, plan="cells")
        assert_bitexact(N(rt), N(rc), f"density, U sign {sign}")
        assert_bitexact(N(ut), N(uc), f"U, U sign {sign}")


@pytest.mark.parametrize("shape", [(2, 1, 40, 70, 3.0), (1, 1, 96, 200, 0.4), (3, 1, 35, 258, 1.0), (1, 1, 150, 67, 0.0), (1, 9, 20, 66, 2.0),
                                   (2, 12, 21, 130, 0.8), (1, 16, 33, 70, 6.0), (1, 7, 9, 11, 1.5), (1, 20, 64, 200, 0.3)])
def test_standalone_advection_tile_plan(fl, ext, dev, oracle, shape):
    """The reference's own call pattern -- advect_scalar and advect_vel one at a time (cpp/advection.py:64,115) -- on the LDS tile
    kernels (the density-only / velocity-only instantiations: 3D default semantics by 'auto', 2D forced with plan='tiles') ==
    one thread per cell (plan='cells') == the oracle, bit for bit: CFL 0 to mostly-fallback, obstacles and Empty cells, batch 1-3,
    both sample_outside_fluid settings, compute windows, traces towards the tensors' corners, and orig != U (cells, whatever the plan)."""
    B, D, H, W, sigma = shape
    s = random_state(B, D, H, W, sigma, seed=29, empties=True)
    tf, tU, trho = T(s["flags"], dev), T(s["U"], dev), T(s["rho"], dev)
    M = "maccormackFluidNet"
    plans = ("tiles", "auto") if D > 1 else ("tiles",)
    uc = fl.advectVelocity(0.13, tU, tU, tf, M, 1, 0.7, plan="cells")
    for so in (False, True):
        rc = fl.advectScalar(0.13, trho, tU, tf, M, 1, so, 0.7, plan="cells")
        for plan in plans:
            assert_bitexact(N(fl.advectScalar(0.13, trho, tU, tf, M, 1, so, 0.7, plan=plan)), N(rc), f"density so={so}: {plan} vs cells")
        if sigma > 0:   # (sigma 0 is a field of +0 / -0: the sign of the clamp's min / max of equal zeros is the C library's choice on the CPU)
            assert_bitexact(N(rc), oracle.advect_scalar(0.13, s["rho"], s["U"], s["flags"], M, 1, so, 0.7), f"density so={so} vs oracle")
    for plan in plans:
        assert_bitexact(N(fl.advectVelocity(0.13, tU, tU, tf, M, 1, 0.7, plan=plan)), N(uc), f"U: {plan} vs cells")
    if sigma > 0:
        assert_bitexact(N(uc), oracle.advect_vel(0.13, s["U"], s["U"], s["flags"], M, 1, 0.7), "U vs oracle")
    # orig != U (the viscous velocity of simulate.py:66-69): no tiles for it -- 'tiles' must give the cell kernels' bits
    orig = (tU * 0.9 + 0.01).contiguous()
    assert_bitexact(N(fl.advectVelocity(0.13, orig, tU, tf, M, 1, 0.7, plan="tiles")), N(fl.advectVelocity(0.13, orig, tU, tf, M, 1, 0.7, plan="cells")), "orig != U")
    if sigma > 0:
        assert_bitexact(N(fl.advectVelocity(0.13, orig, tU, tf, M, 1, 0.7)), oracle.advect_vel(0.13, N(orig), s["U"], s["flags"], M, 1, 0.7), "orig != U vs oracle")
    # Euler and quirks mode keep their kernels under any plan
    assert_bitexact(N(fl.advectScalar(0.13, trho, tU, tf, "eulerFluidNet", 1, False, 0.7, plan="tiles")), N(fl.advectScalar(0.13, trho, tU, tf, "eulerFluidNet", 1, False, 0.7, plan="cells")), "euler")
    if D > 1:
        q = ext.Geom(ref_quirks=True)
        assert_bitexact(N(fl.advectScalar(0.13, trho, tU, tf, M, 1, False, 0.7, geom=q, plan="tiles")), N(fl.advectScalar(0.13, trho, tU, tf, M, 1, False, 0.7, geom=q, plan="cells")), "quirks")
    if D >= 9 and sigma * 0.13 * 5 < 1.0:
        # compute window: planes [3, D-3) only, the rest of `out` untouched
        ro, uo = torch.full_like(trho, 9.0), torch.full_like(tU, 9.0)
        gw = ext.Geom(k_begin=3, k_end=D - 3)
        ext.advect_scalar(0.13, trho, tU, tf, M, 1, False, 0.7, ro, gw, "tiles")
        ext.advect_vel(0.13, tU, tU, tf, M, 1, 0.7, uo, gw, "tiles")
        rc = fl.advectScalar(0.13, trho, tU, tf, M, 1, False, 0.7, plan="cells")
        assert_bitexact(N(ro)[:, :, 3:D - 3], N(rc)[:, :, 3:D - 3], "window density")
        assert_bitexact(N(uo)[:, :, 3:D - 3], N(uc)[:, :, 3:D - 3], "window U")
        assert (N(ro)[:, :, :3] == 9.0).all() and (N(ro)[:, :, D - 3:] == 9.0).all() and (N(uo)[:, :, :3] == 9.0).all() and (N(uo)[:, :, D - 3:] == 9.0).all()
    for sign in (-1.0, 1.0):
        # every trace towards one corner: the tile loader's 16-byte chunks hang over the end (start) of the tensors there
        tUn = (tU.abs() * sign).contiguous()
        assert_bitexact(N(fl.advectScalar(0.13, trho, tUn, tf, M, 1, False, 0.7, plan="tiles")), N(fl.advectScalar(0.13, trho, tUn, tf, M, 1, False, 0.7, plan="cells")), f"density, U sign {sign}")
        assert_bitexact(N(fl.advectVelocity(0.13, tUn, tUn, tf, M, 1, 0.7, plan="tiles")), N(fl.advectVelocity(0.13, tUn, tUn, tf, M, 1, 0.7, plan="cells")), f"U, U sign {sign}")


def test_cells_window_clamp_bounds_second_chunk(fl, ext, dev):
    """The compute window of the block above on the per-cell kernels, deep enough for two z chunks of their clamp-bounds reduction:
    planes [3, 23) of 26 widen to [1, 25), 24 planes, so the reduction's second 16-plane chunk starts at plane 17 from K0 = 1.  With
    sigma 1.0 and dt 0.13, |U dt| <= 1 (5 sigma), what the widening by two planes covers."""
    B, D, H, W, sigma = 1, 26, 12, 70, 1.0
    s = random_state(B, D, H, W, sigma, seed=29, empties=True)
    tf, tU, trho = T(s["flags"], dev), T(s["U"], dev), T(s["rho"], dev)
    M = "maccormackFluidNet"
    ro = torch.full_like(trho, 9.0)
    ext.advect_scalar(0.13, trho, tU, tf, M, 1, False, 0.7, ro, ext.Geom(k_begin=3, k_end=23), "cells")
    for plan in ("cells", "auto"):
        whole = fl.advectScalar(0.13, trho, tU, tf, M, 1, False, 0.7, plan=plan)
        assert_bitexact(N(ro)[:, :, 3:23], N(whole)[:, :, 3:23], f"window [3, 23) on cells vs the whole domain on {plan}")
    assert (N(ro)[:, :, :3] == 9.0).all() and (N(ro)[:, :, 23:] == 9.0).all(), "planes outside the window are untouched"


@pytest.mark.parametrize("D", [1, 10])
def test_tile_trace_division_extremes(fl, ext, dev, oracle, D):
    """The tile kernels take the three quotients d_i / length of a line trace from ONE refined reciprocal (fnx_advect_march.h: adiv3);
    the per-cell kernels and the oracle divide.  Velocity fields whose components mix magnitudes -- O(1), 1e-3, 1e-20, 1e-36,
    denormals, +0 / -0, 1e25 (a wave holding such a length takes the plain divisions), inf -- must give the same bits either way."""
    B, H, W = 2, 40, 130
    rng = np.random.default_rng(41)
    s = random_state(B, D, H, W, 1.0, seed=41, empties=True)
    scales = np.array([1.0, 1e-3, 1e-20, 1e-36, 1e-40, 0.0, -0.0, 3.0, 1e25], np.float32)
    pick = rng.integers(0, len(scales) - 1, size=s["U"].shape)          # per component and cell (1e25 only in a patch below)
    U = (s["U"] * scales[pick]).astype(np.float32)
    U[:, :, :, 5:8, 70:100] *= np.float32(1e25)                          # huge lengths: the waves there divide
    U[0, 0, :, 30, 20] = np.inf
    tf, tU, trho = T(s["flags"], dev), T(U, dev), T(s["rho"], dev)
    M = "maccormackFluidNet"
    for dt in (0.13, 1.0):
        for so in (False, True):
            a = fl.advectScalar(dt, trho, tU, tf, M, 1, so, 0.7, plan="tiles")
            b = fl.advectScalar(dt, trho, tU, tf, M, 1, so, 0.7, plan="cells")
            assert_bitexact(N(a), N(b), f"density, dt {dt}, so {so}: tiles vs cells")
        rt, ut = ext.advect_step(dt, trho, tU, tf, False, 0.7, plan="tiles")
        rc, uc = ext.advect_step(dt, trho, tU, tf, False, 0.7, plan="cells")
        assert_bitexact(N(rt), N(rc), f"fused density, dt {dt}"); assert_bitexact(N(ut), N(uc), f"fused U, dt {dt}")
        rs, us = ext.advect_step(dt, trho, tU, tf, False, 0.7, plan="tiles_split")     # (3D: the backward pass as two marches)
        assert_bitexact(N(rs), N(rc), f"split-backward density, dt {dt}"); assert_bitexact(N(us), N(uc), f"split-backward U, dt {dt}")
    Uf = np.where(np.isfinite(U), U, np.float32(0)).astype(np.float32)   # the oracle on the finite part of the field
    tUf = T(Uf, dev)
    assert_bitexact(N(fl.advectScalar(0.13, trho, tUf, tf, M, 1, False, 0.7, plan="tiles")), oracle.advect_scalar(0.13, s["rho"], Uf, s["flags"], M, 1, False, 0.7), "vs oracle")


def test_rollout_batch_of_two(dev, oracle):
    """Long-term loop with batch > 1 (fluid_net_train.py:349-373): every sample evolves exactly as it does alone."""
    from fluidnet_cxx_amd import rollout
    sts = [plume_state(48), plume_state(48)]
    sts[1]["U"] = sts[1]["U"] + np.float32(0.3)
    sts[1]["density"] = sts[1]["density"] + np.float32(0.05)
    bd = to_dev({k: np.concatenate([sts[0][k], sts[1][k]], 0) for k in sts[0]}, dev)
    rollout(PLUME_CFG, bd, None, "jacobi", 4)
    for b in range(2):
        st = sts[b]
        for _ in range(4):
            st = oracle.simulate_step(st, PLUME_CFG, "jacobi")
        for k in ("U", "density", "p"):
            assert_bitexact(N(bd[k])[b:b + 1], st[k], f"sample {b}: {k}")


@pytest.mark.parametrize("fused", [True, False])
def test_sim64_optional_stages_vs_reference(dev, golden, fused):
    """viscosity + correctScalar + gravity + periodic patches through simulate(): bit-exact against the reference, as
    branches of the native step (fused, the default) and operator by operator."""
    from fluidnet_cxx_amd import simulate
    from util import F2_CFG
    s = golden("sim64")
    mconf = dict(PLUME_CFG, **F2_CFG)
    bd = to_dev(plume_state(64), dev)
    for it in range(1, 7):
        simulate(mconf, bd, None, "jacobi", fused=fused)
        if it in (1, 3, 6):
            for k in ("U", "density", "p"):
                assert_bitexact(N(bd[k]), s[f"f2_{k}_{it}"], f"{k} after {it} steps")


def test_correct_scalar_strided_and_broadcast_inputs(dev, fl):
    """correctScalar (cpp/advection.py:9-12) on what the reference's plain tensor statement accepts and the native operator does not take
    as such: a strided view of a larger tensor as `src` (written in place, the rest of the parent untouched) and broadcast `div` / `flags`
    (one sample's fields for a batch) -- the native operator's bits, no torch arithmetic."""
    rng = np.random.default_rng(3)
    B, D, H, W = 2, 1, 20, 30
    big = T(rng.random((B, 3, D, H, W)).astype(np.float32), dev)
    div = T(rng.standard_normal((1, 1, D, H, W)).astype(np.float32), dev)
    flags = T(make_flags(1, D, H, W, boxes=True), dev)
    src_view = big[:, 1:2]                                             # non-contiguous for B > 1
    assert not src_view.is_contiguous()
    want = src_view.contiguous()
    fl.correctScalar(0.2, want, div.expand(B, 1, D, H, W).contiguous(), flags.expand(B, 1, D, H, W).contiguous())     # the native form
    keep0, keep2 = big[:, 0].clone(), big[:, 2].clone()
    fl.correctScalar(0.2, src_view, div, flags)
    assert torch.equal(big[:, 1:2], want)
    assert torch.equal(big[:, 0], keep0) and torch.equal(big[:, 2], keep2)
    with pytest.raises(AssertionError):
        fl.correctScalar(0.2, want, div.double(), flags)
    with pytest.raises(AssertionError):
        fl.correctScalar(0.2, want[:1], div.expand(B, 1, D, H, W), flags)


OPTIONAL_STAGES = [("viscosity", dict(viscosity=0.02)), ("gravity", dict(gravityScale=0.5)), ("correct", dict(correctScalar=True)),
                   ("periodic_y", {"periodic-x": False, "periodic-y": True}),          # rayleighTaylor.py:158-159
                   ("periodic_x", {"periodic-x": True, "periodic-y": False}),
                   ("periodic_keys_false", {"periodic-x": False, "periodic-y": False}),
                   ("all", dict(viscosity=0.02, gravityScale=0.5, correctScalar=True, **{"periodic-x": True, "periodic-y": True}))]


@pytest.mark.parametrize("name,extra", OPTIONAL_STAGES, ids=[c[0] for c in OPTIONAL_STAGES])
@pytest.mark.parametrize("D", [1, 12])
def test_fused_optional_stages_vs_oracle(dev, oracle, name, extra, D):
    """Every optional stage of lib/simulate.py as a branch of fnx_simulate_step (FnxStepParams.viscosity / gravity_scale /
    correct_scalar / periodic), alone and together, in 2D and 3D, with obstacles, an inflow BC and a developed flow: bit for
    bit the oracle's step and the operator-by-operator path's."""
    from fluidnet_cxx_amd import simulate
    extra = dict(extra)
    if D > 1:
        extra.pop("viscosity", None)                        # 2D only in the reference (viscosity.py:5)
        if not extra:
            pytest.skip("viscosity is 2D only")
    H, W = (40, 72) if D > 1 else (72, 136)
    st = plume_state(W, D)
    st = {k: np.ascontiguousarray(v[:, :, :, :H]) for k, v in st.items()}
    st["flags"] = make_flags(1, D, H, W, boxes=True)
    rng = np.random.default_rng(3)
    st["U"] = (st["U"] + rng.standard_normal(st["U"].shape).astype(np.float32) * np.float32(1.5)).astype(np.float32)
    st["density"] = rng.random(st["density"].shape).astype(np.float32)
    mconf = dict(PLUME_CFG, jacobiIter=9, **extra)
    bd_f, bd_u = to_dev(st, dev), to_dev(st, dev)
    ws = torch.empty(ext_step_bytes(bd_f), dtype=torch.uint8, device=dev)
    for it in range(3):
        simulate(mconf, bd_f, None, "jacobi", workspace=ws, static_flags=(0 if it == 0 else (3 if it == 1 else 7)))
        simulate(mconf, bd_u, None, "jacobi", fused=False)
        st = oracle.simulate_step(st, mconf, "jacobi")
        for k in ("U", "density", "p"):
            assert_bitexact(N(bd_f[k]), st[k], f"{name} D={D}: fused {k} after step {it + 1} vs oracle")
            assert_bitexact(N(bd_u[k]), st[k], f"{name} D={D}: operator path {k} after step {it + 1} vs oracle")


@pytest.mark.parametrize("D", [1, 10])
def test_fused_optional_stages_batch_of_two(dev, oracle, D):
    """All optional stages at once with a batch of two different samples: every sample evolves exactly as it does alone
    (the periodic patch kernels, the correction and the viscous velocity index the batch like the stages do)."""
    from fluidnet_cxx_amd import simulate
    extra = dict(gravityScale=0.5, correctScalar=True, **{"periodic-x": True, "periodic-y": True})
    if D == 1:
        extra["viscosity"] = 0.02
    H, W = (36, 70) if D > 1 else (60, 132)
    rng = np.random.default_rng(13)
    sts = []
    for b in range(2):
        st = plume_state(W, D)
        st = {k: np.ascontiguousarray(v[:, :, :, :H]) for k, v in st.items()}
        st["flags"] = make_flags(1, D, H, W, boxes=True, seed=b)
        st["U"] = (st["U"] + rng.standard_normal(st["U"].shape).astype(np.float32) * np.float32(1.0 + b)).astype(np.float32)
        st["density"] = rng.random(st["density"].shape).astype(np.float32)
        sts.append(st)
    mconf = dict(PLUME_CFG, jacobiIter=7, **extra)
    bd = to_dev({k: np.concatenate([sts[0][k], sts[1][k]], 0) for k in sts[0]}, dev)
    for _ in range(2):
        simulate(mconf, bd, None, "jacobi")
    for b in range(2):
        st = sts[b]
        for _ in range(2):
            st = oracle.simulate_step(st, mconf, "jacobi")
        for k in ("U", "density", "p"):
            assert_bitexact(N(bd[k])[b:b + 1], st[k], f"D={D} sample {b}: {k}")


def ext_step_bytes(bd):
    from fluidnet_cxx_amd._ext import ext
    f = bd["flags"]
    return ext.step_workspace_bytes(f.size(0), f.size(2), f.size(3), f.size(4), bd["U"].size(1) == 3)


def test_fused_optional_stages_refusals(dev):
    from fluidnet_cxx_amd import simulate
    bd = to_dev(plume_state(24, 8), dev)
    with pytest.raises((RuntimeError, AssertionError), match="2D|2d"):
        simulate(dict(PLUME_CFG, viscosity=0.1), bd, None, "jacobi")
    with pytest.raises(AssertionError, match="Viscosity must be positive"):
        simulate(dict(PLUME_CFG, viscosity=-0.1), to_dev(plume_state(24), dev), None, "jacobi")


def test_set_wall_bcs_stick_vs_reference(dev, fl, ext, golden, oracle):
    """setWallBcsStick: HIP == reference golden == oracle, bit for bit; also on a larger random case against the oracle."""
    z = golden("stick")
    for n in "ab":
        U = torch.from_numpy(z[f"{n}_U"]).to(dev)
        r = fl.setWallBcsStick(U, torch.from_numpy(z[f"{n}_flags"]).to(dev), torch.from_numpy(z[f"{n}_flags_stick"]).to(dev))
        assert r is None
        assert_bitexact(N(U), z[f"{n}_out"], f"setWallBcsStick {n}")
    rng = np.random.default_rng(5)
    flags = make_flags(2, 1, 96, 130, boxes=True)
    fs = flags.copy()
    sel = (flags == 2) & (rng.random(flags.shape) < 0.6)
    fs[sel] = 128
    fs[0, 0, 0, 40:44, 50:60] = 128                       # a few stick cells that are NOT obstacles
    U = rng.standard_normal((2, 2, 1, 96, 130)).astype(np.float32)
    tU = torch.from_numpy(U).to(dev)
    fl.setWallBcsStick(tU, torch.from_numpy(flags).to(dev), torch.from_numpy(fs).to(dev))
    assert_bitexact(N(tU), oracle.set_wall_bcs_stick(U, flags, fs), "setWallBcsStick random")
    with pytest.raises(RuntimeError, match="2D only"):
        f3 = torch.ones(1, 1, 4, 8, 8, device=dev)
        ext.set_wall_bcs_stick_(torch.zeros(1, 3, 4, 8, 8, device=dev), f3, f3.clone())


@pytest.mark.parametrize("fused", [True, False])
def test_sim64_stick_convnet_vs_reference(dev, golden, fused):
    """'flags_stick' in the batch (convnet method): setWallBcsStick before the second setConstVals and after the net, as a
    branch of the native step (FnxState.flags_stick) and operator by operator, against the reference."""
    from fluidnet_cxx_amd import FluidNet, simulate
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    z = golden("stick")
    mconf = dict(PLUME_CFG, model="ScaleNet", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True,
                 normalizeInputChan="UDiv", is3D=False)
    net = FluidNet.from_weights(mconf, make_scalenet_weights(0), dev)
    st = plume_state(64)
    st["flags"] = z["sim_flags"]; st["flags_stick"] = z["sim_flags_stick"]
    bd = to_dev(st, dev)
    for it in range(1, 4):
        simulate(mconf, bd, net, "convnet", fused=fused)
        for k in ("U", "density", "p"):
            assert_close_rel(N(bd[k]), z[f"sim_{k}_{it}"], 1e-5, f"stick convnet {k} after {it}")


# ---- properties at benchmark sizes ----------------------------------------------------------------------
@pytest.mark.parametrize("size", [(1, 1024, 1024), (1, 2048, 2048), (64, 128, 128), (256, 256, 256), (64, 512, 512)])
def test_properties_full_size(fl, ext, dev, size):
    D, H, W = size
    is3d = D > 1
    nc = 3 if is3d else 2
    flags = torch.zeros(1, 1, D, H, W, device=dev); fl.emptyDomain(flags)
    g = torch.Generator(device="cpu").manual_seed(1)
    rho = torch.rand(1, 1, D, H, W, generator=g).to(dev)
    U0 = torch.zeros(1, nc, D, H, W, device=dev)
    # zero velocity: advection is the identity on the interior, border -> 0 (measured on the reference)
    out = fl.advectScalar(0.1, rho, U0, flags)
    inner = (slice(None), slice(None), slice(1, -1) if is3d else slice(None), slice(1, -1), slice(1, -1))
    assert torch.equal(out[inner], rho[inner])
    assert float(out[..., 0, :].abs().max()) == 0 and float(out[..., :, 0].abs().max()) == 0
    assert float(fl.advectVelocity(0.1, U0, U0, flags).abs().max()) == 0
    # zero rhs -> zero pressure, zero residual
    p, res = fl.solveLinearSystemJacobi(flags, torch.zeros_like(rho), is3d, 0.0, 28)
    assert float(p.abs().max()) == 0 and float(res) == 0
    # Jacobi is linear in its rhs: J(2*d) == 2*J(d) exactly (power-of-two scaling is exact in fp32)
    div = (torch.rand(1, 1, D, H, W, generator=g) - 0.5).to(dev)
    p1, _ = fl.solveLinearSystemJacobi(flags, div, is3d, 0.0, 16)
    p2, _ = fl.solveLinearSystemJacobi(flags, 2 * div, is3d, 0.0, 16)
    assert torch.equal(2 * p1, p2)
    # launch plans agree: 16 sweeps from zero == 6 sweeps from zero continued by 10 more (pairs, a first pass that
    # knows p = 0, plane chunking: all different between the two routes)
    p6, _ = fl.solveLinearSystemJacobi(flags, div, is3d, 0.0, 6)
    ext.jacobi_sweeps_(flags, div, p6, is3d, 10)
    assert torch.equal(p6, p1)
    # setWallBcs is idempotent; divergence of a projected field shrinks
    U = (torch.randn(1, nc, D, H, W, generator=g)).to(dev)
    Ua = fl.setWallBcs(U.clone(), flags); Ub = fl.setWallBcs(Ua.clone(), flags)
    assert torch.equal(Ua, Ub)
    d0 = fl.velocityDivergence(Ua, flags)
    p, _ = fl.solveLinearSystemJacobi(flags, d0, is3d, 0.0, 200 if not is3d else 60)
    fl.velocityUpdate(p, Ua, flags); fl.setWallBcs(Ua, flags)
    d1 = fl.velocityDivergence(Ua, flags)
    assert float(d1.norm()) < 0.7 * float(d0.norm())
    # unit shift (euler, sample outside): exact one-cell shift away from the walls
    U1 = torch.zeros_like(U0); U1[:, 0] = 1.0
    sh = fl.advectScalar(1.0, rho, U1, flags, "eulerFluidNet", 1, True)
    assert torch.equal(sh[..., 2:-2, 3:-2], rho[..., 2:-2, 2:-3]) if not is3d else torch.equal(sh[:, :, 2:-2, 2:-2, 3:-2], rho[:, :, 2:-2, 2:-2, 2:-3])


# ---- driver-facing entry points ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 70, 130), (1, 10, 24, 66)])
def test_jacobi_sweeps_continue(fl, ext, dev, oracle, shape):
    """k more sweeps on an existing field == the same total number of sweeps from zero (every launch plan)."""
    B, D, H, W = shape
    is3d = D > 1
    s = random_state(B, D, H, W, 2.0, seed=5)
    tf = T(s["flags"], dev)
    div = fl.velocityDivergence(T(s["U"], dev), tf)
    for first, more in ((1, 1), (3, 2), (4, 5), (7, 9)):
        p, _ = fl.solveLinearSystemJacobi(tf, div, is3d, 0.0, first)
        ext.jacobi_sweeps_(tf, div, p, is3d, more)
        ref, _ = fl.solveLinearSystemJacobi(tf, div, is3d, 0.0, first + more)
        assert_bitexact(N(p), N(ref), f"{first}+{more} sweeps")
        po, _, _ = oracle.jacobi(s["flags"], N(div), is3d, 0.0, first + more)
        assert_bitexact(N(p), po, f"{first}+{more} sweeps vs oracle")


@pytest.mark.parametrize("shape,quirks", [((2, 1, 33, 70), False), ((1, 9, 14, 66), False), ((2, 7, 13, 67), True)],
                         ids=["2d", "3d", "3d-quirks"])
def test_fused_stages_equal_operator_sequence(fl, ext, dev, shape, quirks):
    """pre_projection_ / post_projection_ == setConstVals, addBuoyancy, setWallBcs, setConstVals, velocityDivergence /
    velocityUpdate, setWallBcs, setConstVals applied one by one (simulate.py:96-168), bit for bit -- in 3D the staging pass
    writes the divergence too (stage3d_kernel<.,.,DIV>: the staged components of the +1 neighbours re-derived per cell), with
    random BC masks (no identity-BC shortcut) and, third case, in the reference's 3D quirks mode."""
    B, D, H, W = shape
    is3d = D > 1
    geom = ext.Geom(ref_quirks=True) if quirks else None
    kw = dict(geom=geom) if quirks else {}
    s = random_state(B, D, H, W, 2.0, seed=9)
    rng = np.random.default_rng(1)
    nc = 3 if is3d else 2
    UBC = rng.standard_normal((B, nc, D, H, W)).astype(np.float32)
    Um = (rng.random((B, nc, D, H, W)) > 0.2).astype(np.float32)
    rBC = rng.random((B, 1, D, H, W)).astype(np.float32) * 0.3
    rm = (rng.random((B, 1, D, H, W)) > 0.2).astype(np.float32)
    tf = T(s["flags"], dev)
    bd = dict(UBC=T(UBC, dev), UBCInvMask=T(Um, dev), densityBC=T(rBC, dev), densityBCInvMask=T(rm, dev))
    # operator sequence
    U, rho, p = T(s["U"], dev), T(s["rho"], dev), T(s["p"], dev)
    fl.setConstVals(dict(bd), p, U, tf, rho)
    fl.addBuoyancy(U, tf, rho, [0.1, -0.25, 0.05], 0.02, 0.1, **kw)
    fl.setWallBcs(U, tf, **kw)
    fl.setConstVals(dict(bd), p, U, tf, rho)
    div_ref = fl.velocityDivergence(U, tf, **kw)
    # fused
    U2, rho2 = torch.empty_like(U), torch.empty_like(rho)
    div = ext.pre_projection_(T(s["U"], dev), T(s["rho"], dev), p, U2, tf, rho2, bd["UBC"], bd["UBCInvMask"], bd["densityBC"],
                              bd["densityBCInvMask"], 0.1, 1.0, [-0.1, 0.25, -0.05], 0.02, True, **kw)
    assert_bitexact(N(U2), N(U), "pre_projection U"); assert_bitexact(N(rho2), N(rho), "pre_projection rho")
    assert_bitexact(N(div), N(div_ref), "pre_projection div")
    fl.velocityUpdate(p, U, tf, **kw); fl.setWallBcs(U, tf, **kw); fl.setConstVals(dict(bd), p, U, tf, rho)
    ext.post_projection_(p, U2, tf, rho2, bd["UBC"], bd["UBCInvMask"], bd["densityBC"], bd["densityBCInvMask"], **kw)
    assert_bitexact(N(U2), N(U), "post_projection U"); assert_bitexact(N(rho2), N(rho), "post_projection rho")


def test_profile_hooks(fl, ext, dev):
    flags = torch.zeros(1, 1, 1, 256, 256, device=dev); fl.emptyDomain(flags)
    div = torch.randn(1, 1, 1, 256, 256, device=dev)
    ext.profile_enable(True)
    fl.solveLinearSystemJacobi(flags, div, False, 0.0, 12)
    torch.cuda.synchronize()
    ms, n = ext.profile_read(0)
    ext.profile_enable(False)
    # 12 sweeps with the residual wanted = ONE deep launch of 11 sweeps on a small grid (49 workgroup tiles, each on its own
    # CU) + the last sweep on its own
    assert n == 2 and 0 < ms < 50, (ms, n)


def test_standalone_cpp_host_on_the_c_abi(dev):
    """examples/cabi_plume.cpp: a C++ program with nothing but the HIP runtime and include/fluidnet_hip.h (no torch in its
    process) runs 20 steps of the 128^2 plume through fnx_simulate_step; its field hashes equal the Python path's."""
    import os
    import subprocess
    from fluidnet_cxx_amd import fluid, simulate
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(repo, "examples", "cabi_plume.bin")
    if not os.path.isfile(exe):                     # normally built by __graft_entry__.build(); hipcc is on the GPU box too
        from fluidnet_cxx_amd import build
        build.build_examples()
    assert os.path.isfile(exe), "examples/cabi_plume.bin missing and could not be built"
    out = subprocess.run([exe, "20", "128"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = dict(l.split() for l in out.stdout.splitlines()[:3])

    def fnv1a(a):
        h = 1469598103934665603
        for byte in a.tobytes():
            h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        return f"{h:016x}"

    res = 128
    bd = dict(p=torch.zeros(1, 1, 1, res, res, device=dev), U=torch.zeros(1, 2, 1, res, res, device=dev),
              flags=torch.zeros(1, 1, 1, res, res, device=dev), density=torch.zeros(1, 1, 1, res, res, device=dev))
    fluid.emptyDomain(bd["flags"]); fluid.createPlumeBCs(bd, 0.1, 2, 0.145)
    for _ in range(20):
        simulate(PLUME_CFG, bd, None, "jacobi")
    for k in ("U", "density", "p"):
        assert got[k] == fnv1a(N(bd[k])), k


def test_roctx_ranges_do_not_change_results(dev, ext, oracle):
    """fnx_roctx_enable: ranges around the kernel classes (for rocprofv3 --marker-trace); a step with them on is the same step."""
    from fluidnet_cxx_amd import simulate
    st = plume_state(48)
    bd = to_dev(st, dev)
    ext.roctx_enable(True)
    try:
        simulate(PLUME_CFG, bd, None, "jacobi")
    finally:
        ext.roctx_enable(False)
    st = oracle.simulate_step(st, PLUME_CFG, "jacobi")
    for k in ("U", "density", "p"):
        assert_bitexact(N(bd[k]), st[k], k)
