"""A numpy model of the 3D training scene generator (include/fluidnet_hip.h: fnx_scene_obstacles3d, fnx_scene_turbulence3d), written
from the header's statement, under the rule of tests/scene_reference.py: integer operations on uint32 (wrapping), float32 add /
subtract / multiply / compare and int <-> float conversion only, each expression in the stated order.  The kernels are bit-identical
to this model.  The hash is that of the 2D model (scene_reference.mix32, scene_key, uniform).

Cell (i, j, k) = (x, y, z) = array axes (W, H, D) of a (B, C, D, H, W) field.
"""
import numpy as np

import scene_reference as SR
from scene_reference import F, FLUID, MAX_OCTAVES, MAX_PRIMITIVES, OBST, mix32, scene_key, uniform      # noqa: F401

STREAM_OBST3, STREAM_PSIX, STREAM_PSIY, STREAM_PSIZ, STREAM_RHO3, COUNT_CTR = 80, 96, 112, 128, 144, 0xffff0000
MAX_AXIS = 32768                        # the largest D, H or W the entry points accept

# the parameter set the sampler uses (fluidnet_cxx_amd.training3d.SCENE3D_DEFAULTS) -- repeated here so that the model stands alone
DEFAULTS = dict(n_min=0, n_max=4, centre_min=-0.3, centre_max=0.3, size_min=0.03, size_max=0.12, octaves=3, wavelength=16.0,
                amplitude=4.0, density_scale=1.0)


def lattice_address(stream0, octave, lx, ly, lz):
    """(stream word, counter) of the lattice value at the integer point (lx, ly, lz): the plane goes into the stream word above its low
    byte, x and y into the counter with 16 bits each"""
    return (int(lz) << 8) | (int(stream0) + int(octave)), int(ly) * 65536 + int(lx)


def primitives(seed, scene, D, H, W, n_min, n_max, centre_min, centre_max, size_min, size_max, **_):
    """[(is_box, cx, cy, cz, a^2, b^2, c^2)] of one scene, float32.  Primitive t draws at the counters 16 t + d: d = 0 ball / box,
    1..3 the centre's offsets along x, y, z, 4..6 the radius resp. the half extents along x, y, z."""
    key = scene_key(seed, scene, STREAM_OBST3)
    n = n_min + int(F(uniform(key, COUNT_CTR)) * F(n_max - n_min + 1))
    n = min(n, n_max)
    m = F(min(D, H, W))
    cmin, cmax, smin, smax = F(centre_min), F(centre_max), F(size_min), F(size_max)
    out = []
    for t in range(n):
        c = 16 * t
        box = int(mix32(key ^ np.uint64(c)) >> 31)
        ox = cmin + F(uniform(key, c + 1)) * (cmax - cmin)
        oy = cmin + F(uniform(key, c + 2)) * (cmax - cmin)
        oz = cmin + F(uniform(key, c + 3)) * (cmax - cmin)
        cx = F(0.5) * F(W - 1) + ox * m
        cy = F(0.5) * F(H - 1) + oy * m
        cz = F(0.5) * F(D - 1) + oz * m
        ra = (smin + F(uniform(key, c + 4)) * (smax - smin)) * m
        rb = (smin + F(uniform(key, c + 5)) * (smax - smin)) * m
        rc = (smin + F(uniform(key, c + 6)) * (smax - smin)) * m
        out.append((box, F(cx), F(cy), F(cz), F(ra * ra), F(rb * rb), F(rc * rc)))
    return out


def obstacles(seed, scene_ids, D, H, W, **prm):
    """flags (B,1,D,H,W) float32: a border shell one cell wide united with the scene's balls and boxes"""
    flags = np.empty((len(scene_ids), 1, D, H, W), np.float32)
    x = np.arange(W, dtype=np.float32)[None, None, :]
    y = np.arange(H, dtype=np.float32)[None, :, None]
    z = np.arange(D, dtype=np.float32)[:, None, None]
    for b, scene in enumerate(scene_ids):
        obst = np.zeros((D, H, W), bool)
        obst[0] = obst[-1] = True
        obst[:, 0] = obst[:, -1] = True
        obst[:, :, 0] = obst[:, :, -1] = True
        for box, cx, cy, cz, a2, b2, c2 in primitives(seed, scene, D, H, W, **prm):
            dx, dy, dz = x - cx, y - cy, z - cz
            dx2, dy2, dz2 = dx * dx, dy * dy, dz * dz
            obst |= ((dx2 <= a2) & (dy2 <= b2) & (dz2 <= c2)) if box else ((dx2 + dy2) + dz2 <= a2)
        flags[b, 0] = np.where(obst, OBST, FLUID)
    return flags


def _smooth(t):
    return (t * t) * (F(3.0) - F(2.0) * t)


def fractal_noise(seed, scene, stream0, octaves, f0, i, j, k):
    """sum_o 2^-o noise_o at the integer points (i, j, k) (int arrays that broadcast to one shape), float32; the eight lattice values
    around a point are blended along x, then y, then z"""
    shape = np.broadcast(i, j, k).shape
    i, j, k = (np.broadcast_to(a, shape) for a in (i, j, k))
    acc = np.zeros(shape, np.float32)
    gain, f = F(1.0), F(f0)
    for o in range(octaves):
        x, y, z = i.astype(np.float32) * f, j.astype(np.float32) * f, k.astype(np.float32) * f
        lx, ly, lz = x.astype(np.int64), y.astype(np.int64), z.astype(np.int64)
        sx, sy, sz = _smooth(x - lx.astype(np.float32)), _smooth(y - ly.astype(np.float32)), _smooth(z - lz.astype(np.float32))
        planes = np.unique(np.concatenate([lz.ravel(), lz.ravel() + 1]))
        keys = {int(q): scene_key(seed, scene, lattice_address(stream0, o, 0, 0, q)[0]) for q in planes}

        def plane(az):
            key = np.empty(shape, np.uint64)
            for q in np.unique(az):
                key[az == q] = keys[int(q)]

            def lat(ax, ay):
                return F(2.0) * uniform(key, ay * 65536 + ax) - F(1.0)
            v00, v10, v01, v11 = lat(lx, ly), lat(lx + 1, ly), lat(lx, ly + 1), lat(lx + 1, ly + 1)
            a = v00 + sx * (v10 - v00)
            c = v01 + sx * (v11 - v01)
            return a + sy * (c - a)
        lo, hi = plane(lz), plane(lz + 1)
        acc = acc + gain * (lo + sz * (hi - lo))
        gain, f = gain * F(0.5), f * F(2.0)
    return acc


def potential(seed, scene, D, H, W, octaves, wavelength, amplitude, **_):
    """(psi_x, psi_y, psi_z), each (D+1, H+1, W+1) float32: psi_a at the integer point (i, j, k) = array index [k, j, i]"""
    f0 = F(1.0) / F(wavelength)
    k, j, i = np.meshgrid(np.arange(D + 1), np.arange(H + 1), np.arange(W + 1), indexing="ij")
    return tuple(F(amplitude) * fractal_noise(seed, scene, s0, octaves, f0, i, j, k) for s0 in (STREAM_PSIX, STREAM_PSIY, STREAM_PSIZ))


def turbulence(seed, scene_ids, D, H, W, octaves, wavelength, amplitude, density_scale, with_density=True, **_):
    """(U (B,3,D,H,W), density (B,1,D,H,W) or None), float32: the discrete curl of the potential on the cell edges"""
    B = len(scene_ids)
    U = np.empty((B, 3, D, H, W), np.float32)
    rho = np.empty((B, 1, D, H, W), np.float32) if with_density else None
    f0 = F(1.0) / F(wavelength)
    c = (slice(0, D), slice(0, H), slice(0, W))
    pk, pj, pi = (slice(1, D + 1), c[1], c[2]), (c[0], slice(1, H + 1), c[2]), (c[0], c[1], slice(1, W + 1))
    for b, scene in enumerate(scene_ids):
        px, py, pz = potential(seed, scene, D, H, W, octaves, wavelength, amplitude)
        U[b, 0] = (pz[pj] - pz[c]) - (py[pk] - py[c])
        U[b, 1] = (px[pk] - px[c]) - (pz[pi] - pz[c])
        U[b, 2] = (py[pi] - py[c]) - (px[pj] - px[c])
        if with_density:
            k, j, i = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
            r = F(density_scale) * fractal_noise(seed, scene, STREAM_RHO3, octaves, f0, i, j, k)
            rho[b, 0] = np.where(r < 0, F(0.0), np.where(r > 1, F(1.0), r))
    return U, rho


def max_potential_difference(seed, scene, D, H, W, **prm):
    """the largest |psi_a(point + e_b) - psi_a(point)| over the components and the axes the curl differences (float64 of the float32 values)"""
    px, py, pz = (p.astype(np.float64) for p in potential(seed, scene, D, H, W, **prm))
    d = lambda p, ax: float(np.abs(np.diff(p, axis=ax)).max())           # array axes (k, j, i) = (0, 1, 2)
    return max(d(px, 1), d(px, 0), d(py, 2), d(py, 0), d(pz, 2), d(pz, 1))


def interior_divergence(U):
    """the discrete divergence of the MAC field on the interior cells, float64 of the float32 values"""
    u = U.astype(np.float64)
    m = (slice(None), slice(1, -1), slice(1, -1), slice(1, -1))
    return ((u[:, 0, 1:-1, 1:-1, 2:] - u[:, 0][m]) + (u[:, 1, 1:-1, 2:, 1:-1] - u[:, 1][m])) + (u[:, 2, 2:, 1:-1, 1:-1] - u[:, 2][m])
