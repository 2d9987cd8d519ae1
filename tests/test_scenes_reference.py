"""The numpy model of the scene generator (tests/scene_reference.py) on its own: what a scene is, before any kernel is compared with it."""
import numpy as np

import scene_reference as SR

SEED = 20240


def _scene(ids, H=64, W=64, seed=SEED, **over):
    prm = dict(SR.DEFAULTS[2], **over)
    flags = SR.obstacles(seed, ids, (H, W), **prm)
    U, rho = SR.turbulence(seed, ids, (H, W), **prm)
    return flags, U, rho


def test_the_hash_is_a_function_of_its_four_arguments():
    assert int(SR.hash32(1, 2, 3, 4)) == int(SR.hash32(1, 2, 3, 4))
    seen = {int(SR.hash32(*a)) for a in [(1, 2, 3, 4), (2, 2, 3, 4), (1, 3, 3, 4), (1, 2, 4, 4), (1, 2, 3, 5)]}
    assert len(seen) == 5
    # the mixing function, written out once more on Python integers
    x = (1 + 0x9e3779b9) & 0xffffffff
    for v in (None, 2, 3, 4):
        if v is not None:
            x ^= v
        x ^= x >> 16; x = (x * 0x7feb352d) & 0xffffffff; x ^= x >> 15; x = (x * 0x846ca68b) & 0xffffffff; x ^= x >> 16
    assert int(SR.hash32(1, 2, 3, 4)) == x
    u = SR.uniform(SR.scene_key(7, 8, 9), np.arange(4096))
    assert u.dtype == np.float32 and u.min() >= 0 and u.max() < 1 and 0.45 < u.mean() < 0.55


def test_the_host_hash_of_the_package_is_the_same_function():
    import importlib.util
    import os
    # fluidnet_cxx_amd/training.py imports the extension; its hash is plain Python, so take the three functions from the source text
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fluidnet_cxx_amd", "training.py")).read()
    start, end = src.index("def _mix32"), src.index("def host_normal")
    ns = {}
    exec(src[start:end], ns)
    for a in [(1, 2, 3, 4), (0, 0, 0, 0), (0xffffffff, 77, 64, 0xffff0000), (SEED, 5, 65, 31)]:
        assert ns["host_hash"](*a) == int(SR.hash32(*a)), a
        assert ns["host_uniform"](*a) == float(SR.uniform(SR.scene_key(*a[:3]), a[3])), a


def test_same_seed_and_scene_same_arrays_distinct_scenes_distinct_arrays():
    a, b = _scene([3, 11, 4]), _scene([3, 11, 4])
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    # a scene's arrays do not depend on its slot or on the batch around it
    c = _scene([11])
    for x, y in zip(a, c):
        assert np.array_equal(x[1], y[0])
    ids = list(range(0, 24, 3))
    flags, U, rho = _scene(ids)
    for i in range(len(ids)):
        for j in range(i + 1, len(ids)):
            assert not np.array_equal(U[i], U[j]) and not np.array_equal(rho[i], rho[j]), (i, j)
    withprims = [i for i, s in enumerate(ids) if SR.primitives(SEED, s, (64, 64), **SR.DEFAULTS[2])]
    assert len(withprims) >= 4
    assert len({flags[i].tobytes() for i in withprims}) == len(withprims)
    other = _scene([3, 11, 4], seed=SEED + 1)
    assert not np.array_equal(other[1], a[1])


def test_flags_hold_fluid_and_obstacle_inside_an_intact_ring():
    for H, W in ((64, 64), (37, 53), (128, 96)):
        flags = SR.obstacles(SEED, range(16), (H, W), **SR.DEFAULTS[2])
        assert flags.dtype == np.float32 and set(np.unique(flags)) <= {1.0, 2.0}
        f = flags[:, 0, 0]
        assert (f[:, 0, :] == 2).all() and (f[:, -1, :] == 2).all() and (f[:, :, 0] == 2).all() and (f[:, :, -1] == 2).all()


def test_fluid_fraction_stays_inside_its_bounds():
    """SR.DEFAULTS[2] at 64 x 64: at most four primitives, each inside a box of half extent 0.12 * 64 = 7.68 cells, which covers at most
    15 x 15 = 225 cell centres, so at least 62 * 62 - 4 * 225 = 2944 of the 4096 cells stay fluid (0.718); a scene without primitives
    has the 62 * 62 interior cells (0.9385) and nothing has more.  Over 64 scene ids the count of primitives is uniform on 0 .. 4, so
    the mean lies strictly below the upper bound: at most 0.93 would need fewer than ~40 covered cells per scene on average, while one
    smallest primitive alone (half extent 0.03 * 64 = 1.92: a disc of 9 cells or more) comes with four in five scenes -- asserted
    loosely as mean <= 0.93."""
    flags = SR.obstacles(SEED, range(64), (64, 64), **SR.DEFAULTS[2])
    frac = (flags[:, 0, 0] == 1.0).mean(axis=(1, 2))
    print("fluid fraction over 64 scenes: min %.4f mean %.4f max %.4f" % (frac.min(), frac.mean(), frac.max()))
    assert frac.min() >= 2944 / 4096 and frac.max() <= 3844 / 4096
    assert frac.mean() <= 0.93


def test_turbulence_is_divergence_free_up_to_rounding():
    """interior divergence before any BC: four rounded differences (each within 2^-24 |U|) and, evaluated in float32, three additions"""
    for H, W in ((64, 64), (37, 53)):
        _, U, _ = _scene([0, 5, 9, 1000003], H, W)
        bound = 8 * 2.0 ** -24 * float(np.abs(U).max())
        d64 = SR.interior_divergence(U)
        u = U
        d32 = ((u[:, 0, 0, 1:-1, 2:] - u[:, 0, 0, 1:-1, 1:-1]) + u[:, 1, 0, 2:, 1:-1]) - u[:, 1, 0, 1:-1, 1:-1]
        print("max |div| float64 %.3e float32 %.3e bound %.3e max|U| %.3f" % (np.abs(d64).max(), np.abs(d32).max(), bound, np.abs(U).max()))
        assert np.abs(d64).max() <= bound and np.abs(d32).max() <= bound
        assert np.abs(U).max() > 0.05          # a field, not zeros


def test_density_lies_in_the_unit_interval():
    _, _, rho = _scene(range(8))
    assert rho.dtype == np.float32 and rho.min() >= 0.0 and rho.max() <= 1.0
    assert (rho == 0).any() and (rho > 0.2).any()
    assert SR.turbulence(SEED, [1], (16, 16), with_density=False, **SR.DEFAULTS[2])[1] is None
