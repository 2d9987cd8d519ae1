"""A numpy model of the training scene generator (include/fluidnet_hip.h: fnx_scene_obstacles, fnx_scene_turbulence), written from
the header's statement.  Integer operations on uint32 (wrapping), float32 add / subtract / multiply / compare and int <-> float
conversion only, each expression in the stated order (numpy neither contracts a*b+c nor reorders): the kernels are bit-identical to
this model, the rule tests/vorticity_reference.py sets for the confinement.

Cell (i, j) = (x, y) = array axes (W, H) of a (B, C, 1, H, W) field.  The sampler draws its per-call choices from the same hash on
Python integers (fluidnet_cxx_amd/training.py: host_hash); tests/test_scenes_reference.py pins the two together.
"""
import numpy as np

FLUID, OBST = np.float32(1.0), np.float32(2.0)
MAX_PRIMITIVES, MAX_OCTAVES = 16, 8
STREAM_OBST, STREAM_PSI, STREAM_RHO, COUNT_CTR = 0, 16, 32, 0xffff0000
F = np.float32
_U = np.uint32

# the parameter set the sampler uses (fluidnet_cxx_amd.training.SCENE_DEFAULTS) -- repeated here so that the model stands alone
DEFAULTS = dict(n_min=0, n_max=4, centre_min=-0.3, centre_max=0.3, size_min=0.03, size_max=0.12, octaves=4, wavelength=32.0,
                amplitude=8.0, density_scale=1.0)


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


def primitives(seed, scene, H, W, n_min, n_max, centre_min, centre_max, size_min, size_max, **_):
    """[(is_box, cx, cy, a^2, b^2)] of one scene, float32"""
    key = scene_key(seed, scene, STREAM_OBST)
    n = n_min + int(F(uniform(key, COUNT_CTR)) * F(n_max - n_min + 1))
    n = min(n, n_max)
    m = F(min(H, W))
    cmin, cmax, smin, smax = F(centre_min), F(centre_max), F(size_min), F(size_max)
    out = []
    for t in range(n):
        c = 8 * t
        box = int(mix32(key ^ np.uint64(c)) >> 31)
        ox = cmin + F(uniform(key, c + 1)) * (cmax - cmin)
        oy = cmin + F(uniform(key, c + 2)) * (cmax - cmin)
        cx = F(0.5) * F(W - 1) + ox * m
        cy = F(0.5) * F(H - 1) + oy * m
        ra = (smin + F(uniform(key, c + 3)) * (smax - smin)) * m
        rb = (smin + F(uniform(key, c + 4)) * (smax - smin)) * m
        out.append((box, F(cx), F(cy), F(ra * ra), F(rb * rb)))
    return out


def obstacles(seed, scene_ids, H, W, **prm):
    """flags (B,1,1,H,W) float32"""
    flags = np.empty((len(scene_ids), 1, 1, H, W), np.float32)
    x = np.arange(W, dtype=np.float32)[None, :]
    y = np.arange(H, dtype=np.float32)[:, None]
    for b, scene in enumerate(scene_ids):
        obst = np.zeros((H, W), bool)
        obst[0, :] = obst[-1, :] = True
        obst[:, 0] = obst[:, -1] = True
        for box, cx, cy, a2, b2 in primitives(seed, scene, H, W, **prm):
            dx, dy = x - cx, y - cy
            dx2, dy2 = dx * dx, dy * dy
            obst |= ((dx2 <= a2) & (dy2 <= b2)) if box else (dx2 + dy2 <= a2)
        flags[b, 0, 0] = np.where(obst, OBST, FLUID)
    return flags


def _smooth(t):
    return (t * t) * (F(3.0) - F(2.0) * t)


def fractal_noise(seed, scene, stream0, octaves, f0, i, j):
    """sum_o 2^-o noise_o at the integer points (i, j) (int arrays of one shape), float32"""
    acc = np.zeros(np.broadcast(i, j).shape, np.float32)
    gain, f = F(1.0), F(f0)
    for o in range(octaves):
        key = scene_key(seed, scene, stream0 + o)
        x, y = i.astype(np.float32) * f, j.astype(np.float32) * f
        lx, ly = x.astype(np.int64), y.astype(np.int64)
        sx, sy = _smooth(x - lx.astype(np.float32)), _smooth(y - ly.astype(np.float32))

        def lat(ax, ay):
            return F(2.0) * uniform(key, ay * 65536 + ax) - F(1.0)
        v00, v10, v01, v11 = lat(lx, ly), lat(lx + 1, ly), lat(lx, ly + 1), lat(lx + 1, ly + 1)
        a = v00 + sx * (v10 - v00)
        c = v01 + sx * (v11 - v01)
        acc = acc + gain * (a + sy * (c - a))
        gain, f = gain * F(0.5), f * F(2.0)
    return acc


def turbulence(seed, scene_ids, H, W, octaves, wavelength, amplitude, density_scale, with_density=True, **_):
    """(U (B,2,1,H,W), density (B,1,1,H,W) or None), float32"""
    B = len(scene_ids)
    U = np.empty((B, 2, 1, H, W), np.float32)
    rho = np.empty((B, 1, 1, H, W), np.float32) if with_density else None
    f0 = F(1.0) / F(wavelength)
    amp = F(amplitude)
    jn, in_ = np.meshgrid(np.arange(H + 1), np.arange(W + 1), indexing="ij")
    for b, scene in enumerate(scene_ids):
        psi = amp * fractal_noise(seed, scene, STREAM_PSI, octaves, f0, in_, jn)           # (H+1, W+1) nodes
        U[b, 0, 0] = psi[1:, :W] - psi[:H, :W]
        U[b, 1, 0] = F(0.0) - (psi[:H, 1:] - psi[:H, :W])
        if with_density:
            r = F(density_scale) * fractal_noise(seed, scene, STREAM_RHO, octaves, f0, in_[:H, :W], jn[:H, :W])
            rho[b, 0, 0] = np.where(r < 0, F(0.0), np.where(r > 1, F(1.0), r))
    return U, rho


def interior_divergence(U):
    """the discrete divergence of the MAC field on the interior cells, float64 of the float32 values"""
    u = U.astype(np.float64)
    return (u[:, 0, 0, 1:-1, 2:] - u[:, 0, 0, 1:-1, 1:-1]) + (u[:, 1, 0, 2:, 1:-1] - u[:, 1, 0, 1:-1, 1:-1])
