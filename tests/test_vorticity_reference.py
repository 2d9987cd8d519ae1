"""The numpy model of vorticity confinement (tests/vorticity_reference.py): its float32 evaluation against its float64 one, and the
properties the operator's statement implies.  The GPU kernels are held to the float32 model bit for bit (test_vorticity_gpu.py)."""
import numpy as np
import pytest

import vorticity_reference as VR
from util import assert_bitexact

SHAPES = [(2, 2, 1, 40, 48), (2, 3, 20, 24, 28)]


def _case(shape, seed=3):
    B, nc, D, H, W = shape
    return VR.sine_field(shape, seed), VR.case_flags(B, D, H, W)


@pytest.mark.parametrize("shape", SHAPES)
def test_float32_model_against_float64(shape):
    """the stated order in float32 is within 1e-5 of max |dU| of its float64 evaluation, no cell left out"""
    U, f = _case(shape)
    o32 = VR.confine(U, f, 0.5, np.float32)
    o64 = VR.confine(U, f, 0.5, np.float64)
    assert o32.dtype == np.float32 and o64.dtype == np.float64
    dU = np.abs(o64 - U).max()
    err = np.abs(o32 - o64).max()
    # how close any cell comes to either threshold (|w|^2, |grad n|^2 against 1e-6): a cell on the other side of one in float32
    # would be an O(1) difference, not a rounding one
    _, w, n, _ = VR.fields(U, 0.5, np.float64)
    I = VR.interior((shape[0],) + shape[2:])
    s = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    print(f"\n{shape}: max|dU| = {dU:.3e}, |f32 - f64| = {err:.3e} = {err / dU:.2e} of it; min |w|^2 over the interior = {s[I].min():.3e}")
    assert dU > 0.05
    assert err <= 1e-5 * dU


@pytest.mark.parametrize("shape", SHAPES)
def test_amplitude_zero_returns_the_input_bits(shape):
    U, f = _case(shape)
    U[0, 0, 0, 5, 5] = -0.0
    assert_bitexact(VR.confine(U, f, 0.0), U, "amp 0")


@pytest.mark.parametrize("shape", [(1, 2, 1, 30, 34), (1, 3, 18, 20, 22)])
def test_constant_curl_is_left_alone_away_from_the_border(shape):
    """a velocity linear in the coordinates has a constant curl: |w| has no gradient, so no force -- four or more cells from the
    border (nearer to it the zero fields outside the interior make a gradient)"""
    B, nc, D, H, W = shape
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    U = np.zeros(shape, np.float32)
    U[0, 0] = 0.25 * y - 0.125 * z + 1.0
    U[0, 1] = -0.5 * x + 0.25 * z
    if nc == 3:
        U[0, 2] = 0.125 * x + 0.375 * y
    f = np.ones((B, 1, D, H, W), np.float32)
    out = VR.confine(U, f, 0.5)
    inner = (slice(None), slice(None), slice(4, D - 4) if D > 1 else slice(None), slice(4, H - 4), slice(4, W - 4))
    assert_bitexact(out[inner], U[inner], "constant curl")
    assert np.abs(out - U).max() > 0           # (the border region does feel a force: the test is not vacuous)


@pytest.mark.parametrize("shape", SHAPES)
def test_components_at_and_inside_obstacles_do_not_change(shape):
    U, f = _case(shape)
    out = VR.confine(U, f, 0.5)
    fc = f[:, 0]
    for a in range(shape[1]):
        fm = np.roll(fc, 1, (3, 2, 1)[a])
        still = (fc == VR.OBST) | (fm == VR.OBST)
        assert still[VR.interior((shape[0],) + shape[2:])].any()
        assert_bitexact(out[:, a][still], U[:, a][still], f"component {a} at an obstacle")
        # an empty cell under an empty neighbour does not change either (addGravity's condition)
        ee = (fc == VR.EMPTY) & (fm == VR.EMPTY)
        assert ee.any()
        assert_bitexact(out[:, a][ee], U[:, a][ee], f"component {a} between empty cells")
    I = VR.interior((shape[0],) + shape[2:])
    assert_bitexact(out[:, 0][~I], U[:, 0][~I], "border cells")
    assert (out != U).mean() > 0.5


@pytest.mark.parametrize("shape", SHAPES)
def test_samples_of_a_batch_are_independent(shape):
    U, f = _case(shape)
    out = VR.confine(U, f, 0.5)
    for b in range(shape[0]):
        assert_bitexact(VR.confine(U[b:b + 1], f[b:b + 1], 0.5), out[b:b + 1], f"sample {b}")
    U2 = U.copy(); U2[1] = 0
    assert_bitexact(VR.confine(U2, f, 0.5)[0], out[0], "sample 0 beside another sample 1")


def test_2d_never_touches_a_third_component():
    shape = SHAPES[0]
    U, f = _case(shape)
    out = VR.confine(U, f, 0.5)
    assert out.shape == U.shape and out.shape[1] == 2
    c, w, n, F = VR.fields(U, 0.5)
    for z in (c[2], w[0], w[1], F[2]):
        assert not z.any()
    assert np.array_equal(n, np.where(w[2] * w[2] > np.float32(1e-6), np.abs(w[2]), 0).astype(np.float32))
    # the same field as the middle planes of a 3D one that does not vary in z (and has no z velocity) gets the same x, y forces
    D = 9
    U3 = np.zeros((shape[0], 3, D) + shape[3:], np.float32)
    U3[:, :2] = U[:, :, 0][:, :, None]
    F3 = VR.fields(U3, 0.5)[3]
    for a in range(2):
        assert_bitexact(F3[a][:, 4], F[a][:, 0], f"F_{'xy'[a]} of the z-invariant 3D field")
    assert not F3[2][:, 4].any()
