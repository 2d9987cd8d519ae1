"""Properties of the numpy model of the 3D scene generator (tests/scene_reference.py) itself, on the CPU: the GPU
kernels are pinned to this model bit for bit (tests/test_scenes3d_gpu.py), so what holds here holds for them."""
import numpy as np

import scene_reference as S3

SEED = 20263
D, H, W = GRID = 20, 24, 28
DEFAULTS, STREAMS = S3.DEFAULTS[3], S3.STREAMS[3]


def test_the_model_is_deterministic_and_slot_independent():
    ids = [41, 5, 90000]
    a = S3.turbulence(SEED, ids, GRID, **DEFAULTS)
    b = S3.turbulence(SEED, ids, GRID, **DEFAULTS)
    fa, fb = S3.obstacles(SEED, ids, GRID, **DEFAULTS), S3.obstacles(SEED, ids, GRID, **DEFAULTS)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(fa, fb)
    one = S3.turbulence(SEED, [5], GRID, **DEFAULTS)
    assert np.array_equal(one[0][0], a[0][1]) and np.array_equal(one[1][0], a[1][1])
    assert np.array_equal(S3.obstacles(SEED, [5], GRID, **DEFAULTS)[0], fa[1])
    other = S3.turbulence(SEED + 1, [5], GRID, **DEFAULTS)
    assert not np.array_equal(other[0], one[0])
    assert S3.turbulence(SEED, [5], GRID, with_density=False, **DEFAULTS)[1] is None


def test_default_primitives_stay_clear_of_the_border_shell():
    """centre offsets within 0.3 m and sizes up to 0.12 m (m = min(D, H, W)) reach 0.42 m from the grid centre (m - 1) / 2; the shell's
    inner face lies at (m - 1) / 2 - 1 along the shortest axis, so from m = 20 on nothing touches the shell"""
    seen = 0
    for scene in range(200):
        for box, cx, cy, cz, a2, b2, c2 in S3.primitives(SEED, scene, GRID, **DEFAULTS):
            ext = np.sqrt(np.float64(max(a2, b2, c2) if box else a2))
            for c, n in ((cx, W), (cy, H), (cz, D)):
                assert c - ext > 1.0 and c + ext < n - 2.0, (scene, c, ext, n)
            seen += 1
    assert seen > 200
    fl = S3.obstacles(SEED, list(range(8)), GRID, **DEFAULTS)
    assert set(np.unique(fl)) == {1.0, 2.0}
    shell = np.ones((D, H, W), bool)
    shell[1:-1, 1:-1, 1:-1] = False
    assert np.all(fl[:, 0][:, shell] == 2.0) and np.all(fl[:, 0, 1, 1:-1, 1:-1] == 1.0) and (fl == 1.0).mean() > 0.5


def test_the_curl_is_divergence_free_up_to_its_roundings():
    """A velocity component is fl(fl(a' - a) - fl(b' - b)) of four potential values.  With u = 2^-24 and M the largest potential
    difference, each inner subtraction errs by at most u M and the outer one by at most u |U| <= 2 u M (1 + u): a component is the exact
    combination of its four potential values + e, |e| <= 4 u M (the second-order term is swallowed by the margin of the first-order
    ones, which cannot all be attained).  The MAC divergence of a cell adds six components whose exact parts cancel term by term, and
    the model's divergence is taken in float64 of the float32 values (no further rounding): |div| <= 6 * 4 u M = 24 * 2^-24 M."""
    ids = [7, 1000003]
    for name, prm in (("defaults", DEFAULTS), ("rough", dict(DEFAULTS, octaves=5, wavelength=16.0, amplitude=50.0))):
        U, _ = S3.turbulence(SEED, ids, GRID, **prm)
        div = np.abs(S3.interior_divergence(U)).reshape(len(ids), -1).max(axis=1)
        for b, scene in enumerate(ids):
            M = S3.max_potential_difference(SEED, scene, GRID, **prm)
            print(f"SCENE3D_DIV {name} scene {scene}: max|div| {div[b]:.3e}  bound 24 * 2^-24 * {M:.4f} = {24 * 2.0 ** -24 * M:.3e}  "
                  f"max|U| {np.abs(U[b]).max():.4f}")
            assert div[b] <= 24 * 2.0 ** -24 * M
        assert np.abs(U).max() > 0.1


def test_density_is_in_range_and_not_constant():
    _, rho = S3.turbulence(SEED, [3, 4], GRID, **DEFAULTS)
    assert rho.min() >= 0.0 and rho.max() <= 1.0 and rho.std() > 0.05


def test_the_lattice_address_is_injective_at_the_ends_of_the_range():
    """the points a grid of MAX_AXIS cells per axis can reach (0 .. MAX_AXIS + 1 per axis), every stream base and octave: no two
    (stream word, counter) pairs coincide, and none lands on a stream another user of the hash owns"""
    ends = [0, 1, 2, 255, 256, 257, 65535 // 2, S3.MAX_AXIS - 1, S3.MAX_AXIS, S3.MAX_AXIS + 1]
    rng = np.random.default_rng(0)
    pts = [(x, y, z) for x in ends for y in ends for z in ends] + [tuple(int(v) for v in rng.integers(0, S3.MAX_AXIS + 2, 3)) for _ in range(2000)]
    seen = {}
    for s0 in (*STREAMS["PSI"].values(), STREAMS["RHO"]):
        for o in (0, S3.MAX_OCTAVES - 1):
            for p in set(pts):
                stream, ctr = S3.lattice_address(s0, o, *p)
                assert 0 <= stream < 2 ** 32 and 0 <= ctr < 2 ** 32
                assert (stream & 0xff) not in {0, 64, 65, STREAMS["OBST"]} | set(range(16, 24)) | set(range(32, 40))
                assert seen.setdefault((stream, ctr), (s0, o, p)) == (s0, o, p)
    bases = [STREAMS["OBST"], *STREAMS["PSI"].values(), STREAMS["RHO"]]
    ranges = [set([bases[0]])] + [set(range(b, b + S3.MAX_OCTAVES)) for b in bases[1:]]
    assert sum(len(r) for r in ranges) == len(set().union(*ranges))
