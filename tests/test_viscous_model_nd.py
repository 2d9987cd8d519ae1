"""The numpy model of addViscosity and setWallBcsStick (viscous_model_nd.py) -- CPU part.

1. With nd = 2 and ref_quirks the float32 model IS the reference: oracle.add_viscosity and oracle.set_wall_bcs_stick bit for bit, on
   random states with boxes, a protrusion, a wall one cell thick, Empty cells, Stick obstacle cells and Stick fluid cells.  This ties
   the rules the model states with the axis as a loop variable to the reference, as the 2D goldens do for fluid_model_nd.py.
2. The 3D model in float32 and float64 differs by rounding only (no decision of either operator depends on arithmetic).
3. Properties of the default semantics that can be checked by hand: a flat no-slip floor mirrors a uniform tangential flow, the
   viscous step then lowers the first fluid layer by exactly 2 coef u, and no normal component survives on a fluid/obstacle face."""
import numpy as np
import pytest

import viscous_cases as VC
import viscous_model_nd as V
from util import assert_bitexact


@pytest.mark.parametrize("H,W,seed", [(20, 33, 1), (16, 16, 2)])
@pytest.mark.parametrize("open_border", [False, True])
def test_quirks_model_is_the_oracle(oracle, H, W, seed, open_border):
    s = VC.state2d(H, W, seed, open_border=open_border)
    got = V.add_viscosity(VC.DT, s["U"], s["flags"], VC.NU, 2, ref_quirks=True)
    assert got.dtype == np.float32
    assert_bitexact(got, oracle.add_viscosity(VC.DT, s["U"], s["flags"], VC.NU), f"add_viscosity {H}x{W}")
    got = V.set_wall_bcs_stick(s["U"], s["flags"], s["flags_stick"], 2, ref_quirks=True)
    assert got.dtype == np.float32
    assert_bitexact(got, oracle.set_wall_bcs_stick(s["U"], s["flags"], s["flags_stick"]), f"set_wall_bcs_stick {H}x{W}")


def test_quirks_are_visible():
    """the two modes differ on these states (a model whose switch did nothing would pass the test above in either mode)"""
    s = VC.state2d(20, 33, 1)
    assert not np.array_equal(V.add_viscosity(VC.DT, s["U"], s["flags"], VC.NU, 2, ref_quirks=True),
                              V.add_viscosity(VC.DT, s["U"], s["flags"], VC.NU, 2))
    assert not np.array_equal(V.set_wall_bcs_stick(s["U"], s["flags"], s["flags_stick"], 2, ref_quirks=True),
                              V.set_wall_bcs_stick(s["U"], s["flags"], s["flags_stick"], 2))
    with pytest.raises(AssertionError, match="nothing to reproduce"):
        V.add_viscosity(VC.DT, np.zeros((1, 3, 3, 3, 3), np.float32), np.ones((1, 1, 3, 3, 3), np.float32), VC.NU, 3, ref_quirks=True)


@pytest.mark.parametrize("name", list(VC.SHAPES_3D))
def test_float32_against_float64(name):
    """Rounding only.  addViscosity: a chain of at most 10 roundings (6 adds, 6u, the subtraction, coef * s, the last add) of values
    bounded by 12 max|U| (the sum of six neighbours and 6u), so |d| <= 10 * 2^-24 * 12 max|U|.  setWallBcsStick: at most 3 subtractions
    and a division of values bounded by 4 max|U|: |d| <= 4 * 2^-24 * 4 max|U|."""
    s = VC.state3d(name)
    umax = float(np.abs(s["U"]).max())
    for op, bound in (("add_viscosity", 10 * 12), ("set_wall_bcs_stick", 4 * 4)):
        a, b = VC.model3d(name, np.float32)[op], VC.model3d(name, np.float64)[op]
        assert a.dtype == np.float32 and b.dtype == np.float64
        d = float(np.abs(a.astype(np.float64) - b).max())
        print(f"{name} {op}: float32 against float64 {d:.3e}, bound {bound * 2.0 ** -24 * umax:.3e}")
        assert d <= bound * 2.0 ** -24 * umax
        assert d > 0 or op == "set_wall_bcs_stick"
    n = VC.contributions(s["flags"], s["flags_stick"], 3)
    assert {1, 2, 3, 4} <= set(np.unique(np.stack(n)).tolist()), "the states must reach every divisor, n = 3 among them"


def _floor_state():
    """a floor two cells thick (j = 0, 1) under a uniform flow (u, 0, w) that fills every cell, the walls included: free slip"""
    D, H, W = 9, 8, 9
    f = np.full((1, 1, D, H, W), V.FLUID, np.float32)
    f[:, :, :, 0] = f[:, :, :, -1] = f[..., 0] = f[..., -1] = f[:, :, 0] = f[:, :, -1] = V.OBST
    f[:, :, :, 1] = V.OBST
    fs = f.copy()
    fs[:, :, :, 0:2] = V.STICK
    U = np.zeros((1, 3, D, H, W), np.float32)
    U[:, 0], U[:, 2] = 0.5, 0.25
    return f, fs, U


def test_flat_stick_floor_mirrors_the_flow():
    f, fs, U = _floor_state()
    out = V.set_wall_bcs_stick(U, f, fs, 3)
    # the top layer of the floor, away from the side walls: one fluid transverse neighbour (above), so the ghost value is -u
    inner = (slice(None), slice(2, 7), 1, slice(2, 7))
    assert (out[:, 0][inner] == -0.5).all() and (out[:, 2][inner] == -0.25).all()
    assert (out[:, 1][:, :, 0:3] == 0).all()                               # the normal component in and on the floor
    assert (out[:, :, :, 0] == 0).all()                                    # the lower layer has no fluid neighbour: its slip value, 0
    # dt * viscosity = 1/8: every sum below is exact in float32
    coef = 0.125
    stick = V.add_viscosity(0.25, out, f, 0.5, 3)
    slip = V.add_viscosity(0.25, U, f, 0.5, 3)
    first = (slice(None), slice(3, 6), 2, slice(3, 6))                      # first fluid layer, two cells away from the side walls
    for c, u in ((0, 0.5), (2, 0.25)):
        assert (slip[:, c][first] == u).all()
        assert (stick[:, c][first] == u - 2 * coef * u).all()
    assert stick.dtype == np.float32


@pytest.mark.parametrize("nd,seed", [(2, 3), (2, 4), (3, 5), (3, 6), (3, 7)])
def test_no_normal_velocity_through_a_wall_face(nd, seed):
    """for every flag field, protrusions and single cells included: after the operator the component on a face between a fluid cell
    and an obstacle cell is 0 (what the wall-face rule of the default semantics is for; the reference's corner sums let a one-cell
    protrusion keep one)"""
    s = VC.state2d(14, 17, seed, B=1, fluid_stick=False) if nd == 2 else VC.random3d(7, 8, 9, seed)
    out = V.set_wall_bcs_stick(s["U"], s["flags"], s["flags_stick"], nd)
    f = s["flags"][:, 0]
    faces = 0
    for c in range(nd):
        lo = V._sh(f, c, -1, 0.0)
        wall = ((f == V.FLUID) & (lo == V.OBST)) | ((f == V.OBST) & (lo == V.FLUID))
        faces += int(wall.sum())
        assert (out[:, c][wall] == 0).all(), (nd, seed, c)
    assert faces > 50
    if nd == 2:                                                              # the reference's rule does let one through on these states
        ref = V.set_wall_bcs_stick(s["U"], s["flags"], s["flags_stick"], 2, ref_quirks=True)
        print("reference rule: non-zero normal components on wall faces:",
              sum(int((ref[:, c][((f == V.FLUID) & (V._sh(f, c, -1, 0.0) == V.OBST)) | ((f == V.OBST) & (V._sh(f, c, -1, 0.0) == V.FLUID))] != 0).sum())
                  for c in range(2)))
