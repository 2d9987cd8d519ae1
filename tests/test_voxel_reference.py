"""The numpy model of the mesh voxeliser (tests/voxel_reference.py) against what it claims to compute: exact ray casts along all three
axes, createBox3D's half-open box, the analytic ball and box, and the closure of its rows.  No GPU."""
import numpy as np
import pytest

import voxel_reference as VR

FIXTURES = VR.fixtures()


@pytest.fixture(scope="module")
def model():
    return {name: VR.voxelize_model(VR.GRID, v, f) for name, (v, f) in FIXTURES.items()}


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_model_is_the_exact_ray_cast(model, name):
    """every cell, along x, y and z.  A cell point that lies exactly on the snapped surface has no side: such cells are counted exactly
    and left out, and the fixtures in general position have none.  The integer box has them by construction (its low faces); there the
    tie convention -- a crossing at the point counts as before it -- must give the half-open box along every axis."""
    v, f = FIXTURES[name]
    inside, open_rows, bad = model[name]
    assert bad == 0
    for axis in range(3):
        cast, surface = VR.exact_cast(VR.GRID, v, f, axis)
        print(f"{name} axis {axis}: {int(inside.sum())} cells inside, {int(surface.sum())} on the surface, "
              f"{int(((cast != inside) & ~surface).sum())} differ")
        assert (surface.sum() == 0) == (name != "integer_box")
        assert np.array_equal(cast[~surface], inside[~surface]), f"{name}, axis {axis}: {int(((cast != inside) & ~surface).sum())} cells differ"
        if name == "integer_box":
            assert np.array_equal(cast, inside), f"tie convention along axis {axis}"


def test_integer_box_is_the_half_open_box(model):
    inside, open_rows, bad = model["integer_box"]
    (x0, y0, z0), (x1, y1, z1) = VR.BOX_LO, VR.BOX_HI
    assert np.array_equal(inside, VR.box_model(VR.GRID, x0, x1, y0, y1, z0, z1))
    assert inside.sum() == (x1 - x0) * (y1 - y0) * (z1 - z0) and (open_rows, bad) == (0, 0)


def _points():
    D, H, W = VR.GRID
    k, j, i = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    return np.stack([i, j, k], axis=-1).astype(np.float64)


def test_icosphere_against_the_analytic_ball():
    """an inscribed mesh: its faces sag below the sphere by at most r - sqrt(r^2 - e^2 / 3) (the circumradius of a face is at most
    e / sqrt(3), e its longest edge), the snap moves a vertex by at most sqrt(3) / 128 < 1 / 64"""
    v, f = VR.placed(VR.icosphere(3), VR.BALL_R, VR.BALL_C)
    inside, open_rows, bad = VR.voxelize_model(VR.GRID, v, f)
    assert (open_rows, bad) == (0, 0)
    tri = v.astype(np.float64)[f]
    e = max(np.linalg.norm(tri[:, n] - tri[:, (n + 1) % 3], axis=1).max() for n in range(3))
    r = VR.BALL_R
    sag = r - np.sqrt(r * r - e * e / 3.0)
    d = np.linalg.norm(_points() - np.asarray(VR.BALL_C), axis=-1)
    ball = d <= r
    band = (d > r - (sag + 2.0 / 64)) & (d <= r + 1.0 / 64)
    print(f"longest edge {e:.4f}, sag {sag:.4f}: {int(ball.sum())} cells in the ball, {int(band.sum())} in the band, "
          f"{int(((inside != ball) & ~band).sum())} differ outside it")
    assert not ((inside != ball) & ~band).any()
    assert band.sum() <= 0.05 * ball.sum()


def test_rotated_box_against_its_signed_distance(model):
    inside, open_rows, bad = model["rotated_box"]
    R = VR.rotation(VR.ROT_SEED)
    local = (_points() - np.asarray(VR.ROT_C)) @ R              # R^T (p - c), row-wise
    q = np.abs(local) - np.asarray(VR.ROT_HALF)
    sd = np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(axis=-1), 0.0)
    band = np.abs(sd) <= 0.02
    print(f"rotated box: {int((sd < 0).sum())} cells inside, {int(band.sum())} in the band, {int(((inside != (sd < 0)) & ~band).sum())} differ outside it")
    assert not ((inside != (sd < 0)) & ~band).any()
    assert (open_rows, bad) == (0, 0)


def test_rows_close(model):
    for name, (inside, open_rows, bad) in model.items():
        assert open_rows == 0 and bad == 0, name
    v, f = VR.placed(VR.torus(6.0, 2.5), 1.0, (17.4, 9.7, 5.8), VR.rotation(7))
    assert VR.voxelize_model(VR.GRID, v, f)[1:] == (0, 0)
    for name in ("integer_box", "icosphere"):
        v, f = FIXTURES[name]
        assert VR.voxelize_model(VR.GRID, v, f[1:])[1] > 0, f"{name} without a face must have open rows"


def test_bad_faces_are_skipped_and_counted():
    v, f = FIXTURES["icosphere"]
    want = VR.voxelize_model(VR.GRID, v, f[3:])
    f2 = f.copy()
    f2[0, 1] = len(v)
    f2[1, 0] = -1
    v2 = np.concatenate([v, [[np.nan, 1, 1], [1, np.inf, 1], [1, 1, 3e4]]]).astype(np.float32)
    f2[2] = (len(v), 0, 1)
    extra = np.array([[len(v) + 1, 0, 1], [len(v) + 2, 0, 1]], dtype=np.int32)
    inside, open_rows, bad = VR.voxelize_model(VR.GRID, v2, np.concatenate([f2, extra]))
    assert bad == 5 and open_rows == want[1] and np.array_equal(inside, want[0])


def test_primitive_models():
    shape = (9, 11, 13)
    s = VR.sphere_model(shape, 6.0, 5.0, 4.0, 3.3)
    assert np.array_equal(s[4], VR.cylinder_model(shape, 6.0, 5.0, 3.3)[4])
    assert s[4, 5, 6] and not s[0, 0, 0] and s.sum() == sum(
        (i - 6) ** 2 + (j - 5) ** 2 + (k - 4) ** 2 <= 3.3 ** 2 for k in range(9) for j in range(11) for i in range(13))
    b = VR.box_model(shape, 2, 5.5, 1, 3, 0, 2)
    assert b.sum() == 4 * 2 * 2 and b[0, 1, 2] and b[1, 2, 5] and not b[2, 1, 2] and not b[0, 3, 2]
