"""addViscosity and setWallBcsStick in 3D on the GPU (fnx_viscous.hip) against the numpy model whose axis is a loop variable
(viscous_model_nd.py), and the 3D viscous step of simulate().  The native step has no 3D viscous stage (fnx_simulate_step refuses
it, tests/test_step_host.py holds it to that), so the step runs on the operator path, and what it is compared with is the same
operators composed by hand in the order of the reference's simulate.py.

Both operators are selects, negations, adds, multiplies and one IEEE division in a fixed order, so the model's float32 run is the
expected BITS: no tolerance anywhere in this file.  Shapes: (B, D, H, W) = (2, 5, 9, 13) and (1, 10, 11, 67), those of
semantics3d_cases.OWN -- W = 67 crosses the marching kernel's x tile at 64, H = 9 and 11 its 8 rows, D = 10 its z chunk of 8, and
(2, 5, 9, 13) is smaller than a tile in every direction.  The states (viscous_cases.state3d): a plate one plane thick, a bar along z,
single obstacle cells, Empty cells, Stick on whole blocks with their edges and corners, on a random part of the rest and on two fluid
cells, and a Stick cell with three fluid transverse neighbours (the division by 3)."""
import numpy as np
import pytest
import torch

import semantics3d_cases as C
import viscous_cases as VC
from util import assert_bitexact

pytestmark = pytest.mark.gpu

SHAPES = list(VC.SHAPES_3D)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def T(x, dev):
    return torch.from_numpy(np.array(x, order="C", copy=True)).to(dev)      # the cases' arrays are read-only


def N(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("name", SHAPES)
def test_operators_equal_the_model(dev, name):
    """fluid.addViscosity and fluid.setWallBcsStick (in place), and the out-of-place forms, on every cell"""
    from fluidnet_cxx_amd import fluid
    from fluidnet_cxx_amd._ext import ext
    s, want = VC.state3d(name), VC.model3d(name)
    n = np.stack(VC.contributions(s["flags"], s["flags_stick"], 3))
    assert (n == 3).any() and (n == 4).any(), "the state must reach the divisions by 3 and by 4"
    flags, stick = T(s["flags"], dev), T(s["flags_stick"], dev)
    U = T(s["U"], dev)
    assert fluid.addViscosity(VC.DT, U, flags, VC.NU) is None
    assert_bitexact(N(U), want["add_viscosity"], f"addViscosity {name}")
    U = T(s["U"], dev)
    assert fluid.setWallBcsStick(U, flags, stick) is None
    assert_bitexact(N(U), want["set_wall_bcs_stick"], f"setWallBcsStick {name}")
    U, out = T(s["U"], dev), torch.full(s["U"].shape, float("nan"), device=dev)
    assert ext.add_viscosity_out(VC.DT, U, flags, VC.NU, out) is out
    assert_bitexact(N(out), want["add_viscosity"], f"add_viscosity_out {name}")
    assert_bitexact(N(U), s["U"], "add_viscosity_out must not write U")
    out = torch.full(s["U"].shape, float("nan"), device=dev)
    assert ext.set_wall_bcs_stick_out(U, flags, stick, out) is out
    assert_bitexact(N(out), want["set_wall_bcs_stick"], f"set_wall_bcs_stick_out {name}")


def _batch(name, dev, stick=False):
    s = VC.state3d(name)
    rng = np.random.default_rng(5)
    rho = rng.random(s["flags"].shape).astype(np.float32)
    bd = dict(p=torch.zeros(s["flags"].shape, device=dev), U=T(s["U"] * np.float32(0.5), dev), flags=T(s["flags"], dev), density=T(rho, dev))
    if stick:
        bd["flags_stick"] = T(s["flags_stick"], dev)
    return bd


M = "maccormackFluidNet"


def _step_by_hand(cfg, bd, net, method):
    """one step of simulate.py:28-171 for a state with a density and no BC arrays, operator by operator: the viscous velocity is what
    is advected (:66-69, :85-93), buoyancy, then Jacobi between two setWallBcs, or the net between two setWallBcsStick (:129-130, :165-166)"""
    from fluidnet_cxx_amd import fluid
    dt, flags = cfg["dt"], bd["flags"]
    orig = bd["U"].clone()
    fluid.addViscosity(dt, orig, flags, cfg["viscosity"])
    rho = fluid.advectScalar(dt, bd["density"], bd["U"], flags, M, 1, cfg["sampleOutsideFluid"], cfg["maccormackStrength"])
    U = fluid.advectVelocity(dt, orig, bd["U"], flags, M, 1, cfg["maccormackStrength"])
    gv = cfg["gravityVec"]
    gravity = (torch.tensor([gv["x"], gv["y"], gv["z"]], dtype=torch.float32) * (-cfg["buoyancyScale"])).tolist()
    U = fluid.addBuoyancy(U, flags, rho, gravity, cfg["operatingDensity"], dt)
    if method == "jacobi":
        U = fluid.setWallBcs(U, flags)
        div = fluid.velocityDivergence(U, flags)
        p, _ = fluid.solveLinearSystemJacobi(flags=flags, div=div, is_3d=True, p_tol=0.0, max_iter=cfg["jacobiIter"])
        fluid.velocityUpdate(pressure=p, U=U, flags=flags)
        U = fluid.setWallBcs(U, flags)
    else:
        fluid.setWallBcsStick(U, flags, bd["flags_stick"])
        p, U = net(torch.cat((bd["p"], U, flags, rho), 1))
        fluid.setWallBcsStick(U, flags, bd["flags_stick"])
    bd.update(p=p, U=U, density=rho)


@pytest.mark.parametrize("name", SHAPES)
def test_viscous_step_equals_operators_by_hand(dev, name):
    """simulate(..., fused=False) in 3D with viscosity > 0, Jacobi-7: the bits of the operators composed by hand after one step and
    after three; the viscosity does act (the inviscid native step differs), and the native step is refused as before"""
    from fluidnet_cxx_amd import simulate
    cfg = dict(C.STEP_CFG, dt=0.1, viscosity=VC.NU)
    sim, hand, inviscid = _batch(name, dev), _batch(name, dev), _batch(name, dev)
    simulate(dict(cfg, viscosity=0), inviscid, None, "jacobi")
    for step in (1, 2, 3):
        simulate(cfg, sim, None, "jacobi", fused=False)
        _step_by_hand(cfg, hand, None, "jacobi")
        if step in (1, 3):
            for k in ("p", "U", "density"):
                assert_bitexact(N(sim[k]), N(hand[k]), f"{name}: {k} after step {step}, simulate(fused=False) vs the operators by hand")
        if step == 1:
            assert not torch.equal(sim["U"], inviscid["U"])
    assert torch.isfinite(sim["U"]).all()
    before = N(sim["U"])
    with pytest.raises(RuntimeError, match="2D only in the native step"):
        simulate(cfg, sim, None, "jacobi")
    assert_bitexact(N(sim["U"]), before, "a refused step wrote U")


def test_stick_convnet_step_equals_operators_by_hand(dev):
    """flags_stick with 'convnet' on seeded weights (the 3D net needs 4 planes: the (2, 5, 9, 13) state), with viscosity as well: such
    a state takes the operator path whatever `fused` says; one step and three against the operators by hand"""
    from fluidnet_cxx_amd import FluidNet, simulate
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    cfg = dict(C.STEP_CFG, dt=0.1, viscosity=VC.NU, model="ScaleNet", inputChannels=dict(div=True, pDiv=False, UDiv=False),
               normalizeInput=True, normalizeInputChan="UDiv", normalizeInputThreshold=1e-5, is3D=True)
    net = FluidNet.from_weights(cfg, make_scalenet_weights(0, ndim=3), dev)
    sim, hand, slip, default = _batch("small", dev, True), _batch("small", dev, True), _batch("small", dev), _batch("small", dev, True)
    simulate(cfg, slip, net, "convnet", fused=False)
    for step in (1, 2, 3):
        simulate(cfg, sim, net, "convnet", fused=False)
        _step_by_hand(cfg, hand, net, "convnet")
        if step in (1, 3):
            for k in ("p", "U", "density"):
                assert_bitexact(N(sim[k]), N(hand[k]), f"{k} after step {step}, simulate(fused=False) vs the operators by hand")
        if step == 1:
            assert not torch.equal(sim["U"], slip["U"])
    # without viscosity the reference's four-argument call runs such a state too
    nv = dict(cfg, viscosity=0)
    simulate(nv, default, net, "convnet")
    again = _batch("small", dev, True)
    simulate(nv, again, net, "convnet", fused=False)
    for k in ("p", "U", "density"):
        assert_bitexact(N(default[k]), N(again[k]), f"{k}: the default call vs fused=False")


def test_2d_operators_unchanged(dev, oracle):
    """the 2D calls still run the 2D kernels: the reference's bits (its (i-1, j-1) neighbour, its corner sums) on one 33 x 20 state"""
    from fluidnet_cxx_amd import fluid
    s = VC.state2d(20, 33, 1)
    flags = T(s["flags"], dev)
    U = T(s["U"], dev)
    fluid.addViscosity(VC.DT, U, flags, VC.NU)
    assert_bitexact(N(U), oracle.add_viscosity(VC.DT, s["U"], s["flags"], VC.NU), "2D addViscosity")
    U = T(s["U"], dev)
    fluid.setWallBcsStick(U, flags, T(s["flags_stick"], dev))
    assert_bitexact(N(U), oracle.set_wall_bcs_stick(s["U"], s["flags"], s["flags_stick"]), "2D setWallBcsStick")


def test_refusals(dev):
    from fluidnet_cxx_amd import simulate
    from fluidnet_cxx_amd._ext import ext
    from fluidnet_cxx_amd.slab import NativeSlabSimulator, SlabLayout
    cfg = dict(C.STEP_CFG, dt=0.1, viscosity=VC.NU)
    # an aliased output
    s = VC.state3d("small")
    U, flags, stick = T(s["U"], dev), T(s["flags"], dev), T(s["flags_stick"], dev)
    with pytest.raises(RuntimeError, match="add_viscosity: U_out must not alias U_in"):
        ext.add_viscosity_out(VC.DT, U, flags, VC.NU, U)
    with pytest.raises(RuntimeError, match="set_wall_bcs_stick: U_out must not alias U_in"):
        ext.set_wall_bcs_stick_out(U, flags, stick, U)
    assert_bitexact(N(U), s["U"], "a refused call wrote U")
    # ref_quirks has nothing to reproduce in 3D: simulate() says so on both paths, for the viscosity and for flags_stick
    quirks = ext.Geom(ref_quirks=True)
    for fused in (True, False):
        bd = _batch("small", dev, True)
        with pytest.raises(RuntimeError, match="no 3D form with ref_quirks"):
            simulate(cfg, bd, None, "jacobi", geom=quirks, fused=fused)
        with pytest.raises(RuntimeError, match="no 3D form with ref_quirks"):
            simulate(dict(cfg, viscosity=0), bd, None, "convnet", geom=quirks, fused=fused)
        assert_bitexact(N(bd["U"]), s["U"] * np.float32(0.5), "a refused step wrote U")
    # the z-slab driver keeps refusing the viscosity
    bd = _batch("tile", dev)
    sim = NativeSlabSimulator(SlabLayout(bd["flags"].size(2), 1, 0, 5), cfg)
    with pytest.raises(RuntimeError, match="slab_step: the optional stages \\(viscosity"):
        sim.step(bd)
