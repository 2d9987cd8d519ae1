"""A numpy model of the training scene generator in 2D and 3D (include/fluidnet_hip.h: fnx_scene_obstacles, fnx_scene_turbulence and their
3d entry points), written from the header's statement.  Integer operations on uint32 (wrapping), float32 add / subtract / multiply /
compare and int <-> float conversion only, each expression in the stated order (numpy neither contracts a*b+c nor reorders): the kernels
are bit-identical to this model, the rule tests/vorticity_reference.py sets for the confinement.

A grid is (H, W) or (D, H, W); its fields are (B, C, 1, H, W) resp. (B, C, D, H, W).  Cell (i, j[, k]) = (x, y[, z]) = array axes
(W, H[, D]): axis a of the grid is the a-th array axis from the right.  Every rule is stated once over the axes of the grid; what differs
by dimension is in STREAMS, DEFAULTS and _curl, the way fluidnet_cxx_amd/csrc/fnx_scenes.hip keeps it in Streams<IS3D> and one
`if constexpr`.  The sampler draws its per-call choices from the same hash on Python integers (fluidnet_cxx_amd/training.py: host_hash);
tests/test_scenes_reference.py pins the two together.
"""
import functools
import operator

import numpy as np

FLUID, OBST = np.float32(1.0), np.float32(2.0)
MAX_PRIMITIVES, MAX_OCTAVES = 16, 8
MAX_AXIS = 32768                        # the largest D, H or W the 3D entry points accept
COUNT_CTR = 0xffff0000
F = np.float32

# Stream bases (the low byte of the stream word) by dimension.  OBST: the obstacle primitives, primitive t drawing at the counters
# PRIM_STRIDE * t + d -- d = 0 disc / box, with NA axes d = 1 .. NA the centre's offsets along x, y[, z] and NA + 1 .. 2 NA the radius
# resp. the half extents.  PSI: {axis of the potential's component: base}, octave o at base + o -- 2D has the one stream function (the z
# component), 3D a vector potential.  RHO: the density, octave o at base + o.
STREAMS = {2: dict(OBST=0, PRIM_STRIDE=8, PSI={2: 16}, RHO=32),
           3: dict(OBST=80, PRIM_STRIDE=16, PSI={0: 96, 1: 112, 2: 128}, RHO=144)}

# the parameter sets the samplers use (fluidnet_cxx_amd.training: SCENE_DEFAULTS, SCENE3D_DEFAULTS) -- repeated here so that the model
# stands alone
DEFAULTS = {2: dict(n_min=0, n_max=4, centre_min=-0.3, centre_max=0.3, size_min=0.03, size_max=0.12, octaves=4, wavelength=32.0,
                    amplitude=8.0, density_scale=1.0),
            3: dict(n_min=0, n_max=4, centre_min=-0.3, centre_max=0.3, size_min=0.03, size_max=0.12, octaves=3, wavelength=16.0,
                    amplitude=4.0, density_scale=1.0)}


def mix32(x):
    x = np.asarray(x, np.uint64) & 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def scene_key(seed, scene, stream):
    return mix32(mix32(mix32((int(seed) + 0x9e3779b9) & 0xffffffff) ^ (int(scene) & 0xffffffff)) ^ int(stream))


def hash32(seed, scene, stream, counter):
    return mix32(scene_key(seed, scene, stream) ^ (np.asarray(counter, np.uint64) & 0xffffffff))


def uniform(key, counter):
    """(hash >> 8) * 2^-24 as float32, elementwise over `counter`"""
    h = mix32(np.asarray(key, np.uint64) ^ (np.asarray(counter, np.uint64) & 0xffffffff))
    return (h >> 8).astype(np.float32) * F(2.0 ** -24)


def lattice_address(stream0, octave, lx, ly, lz=0):
    """(stream word, counter) of the lattice value at the integer point (lx, ly[, lz]): the plane goes into the stream word above its low
    byte (2D has the one plane 0), x and y into the counter with 16 bits each"""
    return (int(lz) << 8) | (int(stream0) + int(octave)), ly * 65536 + lx


def _field(grid):
    """the (D, H, W) of a field on `grid`"""
    return (1,) * (3 - len(grid)) + tuple(grid)


def _along(a, na, v):
    """the 1-D array v laid along axis a of an na-axis grid, to broadcast against the grid's arrays"""
    return v.reshape([-1 if ax == na - 1 - a else 1 for ax in range(na)])


def primitives(seed, scene, grid, n_min, n_max, centre_min, centre_max, size_min, size_max, **_):
    """[(is_box, cx, cy[, cz], a^2, b^2[, c^2])] of one scene, float32"""
    na, S = len(grid), STREAMS[len(grid)]
    key = scene_key(seed, scene, S["OBST"])
    n = n_min + int(F(uniform(key, COUNT_CTR)) * F(n_max - n_min + 1))
    n = min(n, n_max)
    m = F(min(grid))
    cmin, cmax, smin, smax = F(centre_min), F(centre_max), F(size_min), F(size_max)
    out = []
    for t in range(n):
        c = S["PRIM_STRIDE"] * t
        box = int(mix32(key ^ np.uint64(c)) >> 31)
        ctr, r2 = [], []
        for a in range(na):
            off = cmin + F(uniform(key, c + 1 + a)) * (cmax - cmin)
            ctr.append(F(F(0.5) * F(grid[na - 1 - a] - 1) + off * m))
        for a in range(na):
            r = (smin + F(uniform(key, c + 1 + na + a)) * (smax - smin)) * m
            r2.append(F(r * r))
        out.append((box, *ctr, *r2))
    return out


def obstacles(seed, scene_ids, grid, **prm):
    """flags (B,1,D,H,W) float32: a border one cell wide united with the scene's discs / balls and boxes"""
    na = len(grid)
    flags = np.empty((len(scene_ids), 1) + _field(grid), np.float32)
    coord = [_along(a, na, np.arange(grid[na - 1 - a], dtype=np.float32)) for a in range(na)]
    for b, scene in enumerate(scene_ids):
        obst = np.zeros(grid, bool)
        for ax in range(na):
            np.moveaxis(obst, ax, 0)[[0, -1]] = True
        for box, *q in primitives(seed, scene, grid, **prm):
            d2 = [(coord[a] - q[a]) * (coord[a] - q[a]) for a in range(na)]
            if box:
                obst |= functools.reduce(operator.and_, [d2[a] <= q[na + a] for a in range(na)])
            else:
                obst |= functools.reduce(operator.add, d2) <= q[na]                # (dx2 + dy2) + dz2
        flags[b, 0] = np.where(obst, OBST, FLUID).reshape(_field(grid))
    return flags


def _smooth(t):
    return (t * t) * (F(3.0) - F(2.0) * t)


def fractal_noise(seed, scene, stream0, octaves, f0, *point):
    """sum_o 2^-o noise_o at the integer points (i, j[, k]) (int arrays that broadcast to one shape), float32; the lattice values around
    a point are blended along x, then y, then -- between the two planes whose index sits in the stream word -- z"""
    shape = np.broadcast(*point).shape
    point = [np.broadcast_to(a, shape) for a in point]
    acc = np.zeros(shape, np.float32)
    gain, f = F(1.0), F(f0)
    for o in range(octaves):
        x = [a.astype(np.float32) * f for a in point]
        l = [v.astype(np.int64) for v in x]
        s = [_smooth(v - q.astype(np.float32)) for v, q in zip(x, l)]

        def plane(az):
            """the blend along x and y in the lattice plane(s) az"""
            key = np.empty(shape, np.uint64)
            for q in np.unique(az):
                key[az == q] = scene_key(seed, scene, lattice_address(stream0, o, 0, 0, q)[0])

            def lat(ax, ay):
                return F(2.0) * uniform(key, lattice_address(stream0, o, ax, ay)[1]) - F(1.0)
            v00, v10, v01, v11 = lat(l[0], l[1]), lat(l[0] + 1, l[1]), lat(l[0], l[1] + 1), lat(l[0] + 1, l[1] + 1)
            a = v00 + s[0] * (v10 - v00)
            c = v01 + s[0] * (v11 - v01)
            return a + s[1] * (c - a)
        if len(point) == 2:
            val = plane(np.zeros(shape, np.int64))
        else:
            lo, hi = plane(l[2]), plane(l[2] + 1)
            val = lo + s[2] * (hi - lo)
        acc = acc + gain * val
        gain, f = gain * F(0.5), f * F(2.0)
    return acc


def _points(n):
    """the integer points 0 .. n[ax] - 1 per array axis as (i, j[, k]): x first"""
    return np.meshgrid(*[np.arange(v) for v in n], indexing="ij")[::-1]


def potential(seed, scene, grid, octaves, wavelength, amplitude, **_):
    """{axis a: psi_a}, each float32 on the grid's nodes (n + 1 per axis): psi_a at the integer point (i, j[, k]) = array index [[k, ]j, i]"""
    f0 = F(1.0) / F(wavelength)
    nodes = _points([n + 1 for n in grid])
    return {a: F(amplitude) * fractal_noise(seed, scene, s0, octaves, f0, *nodes) for a, s0 in STREAMS[len(grid)]["PSI"].items()}


def _curl(psi, grid):
    """The discrete curl of the potential on the cell edges -> [U_x, U_y[, U_z]] on the cells.  Two formulas, as in the kernel: a stream
    function's curl and a three-component potential's are not copies of each other."""
    c = tuple(slice(0, n) for n in grid)
    up = lambda a: tuple(slice(1, n + 1) if ax == len(grid) - 1 - a else slice(0, n) for ax, n in enumerate(grid))    # + e_a
    if len(grid) == 2:
        p = psi[2]
        return [p[up(1)] - p[c], F(0.0) - (p[up(0)] - p[c])]
    px, py, pz = psi[0], psi[1], psi[2]
    return [(pz[up(1)] - pz[c]) - (py[up(2)] - py[c]), (px[up(2)] - px[c]) - (pz[up(0)] - pz[c]), (py[up(0)] - py[c]) - (px[up(1)] - px[c])]


def turbulence(seed, scene_ids, grid, octaves, wavelength, amplitude, density_scale, with_density=True, **_):
    """(U (B,NA,D,H,W), density (B,1,D,H,W) or None), float32"""
    B, na, field = len(scene_ids), len(grid), _field(grid)
    U = np.empty((B, na) + field, np.float32)
    rho = np.empty((B, 1) + field, np.float32) if with_density else None
    f0 = F(1.0) / F(wavelength)
    for b, scene in enumerate(scene_ids):
        for a, u in enumerate(_curl(potential(seed, scene, grid, octaves, wavelength, amplitude), grid)):
            U[b, a] = u.reshape(field)
        if with_density:
            r = F(density_scale) * fractal_noise(seed, scene, STREAMS[na]["RHO"], octaves, f0, *_points(grid))
            rho[b, 0] = np.where(r < 0, F(0.0), np.where(r > 1, F(1.0), r)).reshape(field)
    return U, rho


def max_potential_difference(seed, scene, grid, **prm):
    """the largest |psi_a(point + e_b) - psi_a(point)| over the components and the axes b != a the curl differences (float64 of the
    float32 values)"""
    na = len(grid)
    return max(float(np.abs(np.diff(p.astype(np.float64), axis=na - 1 - b)).max())
               for a, p in potential(seed, scene, grid, **prm).items() for b in range(na) if b != a)


def _interior(na, up=None):
    """the index of one component (B, D, H, W) at the interior cells of a grid of na axes, or at their + e_up neighbours"""
    return (slice(None),) + tuple(0 if a >= na else slice(2, None) if a == up else slice(1, -1) for a in (2, 1, 0))


def interior_divergence(U):
    """the discrete divergence of the MAC field on the interior cells, float64 of the float32 values, summed in the order x, y[, z]"""
    u = U.astype(np.float64)
    na = U.shape[1]
    return functools.reduce(operator.add, [u[:, a][_interior(na, a)] - u[:, a][_interior(na)] for a in range(na)])
