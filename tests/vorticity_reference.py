"""A numpy model of vorticity confinement (include/fluidnet_hip.h: fnx_add_vorticity_confinement), written from the operator's
statement, with the arithmetic's dtype as a parameter: float32 evaluates every step in the stated order (numpy neither contracts
a*b+c nor reorders, and its float32 sqrt and division are correctly rounded), float64 is the yardstick of that order's error.

Cell (i, j, k) = (x, y, z) = array axes (W, H, D) of a (B, C, D, H, W) field.  Interior: 1 <= i <= W-2, 1 <= j <= H-2 and, in 3D,
1 <= k <= D-2; in 2D (D = 1, two components) every plane counts.  Every intermediate field is 0 outside the interior.
"""
import numpy as np

FLUID, OBST, EMPTY = 1.0, 2.0, 4.0
_AXIS = (3, 2, 1)            # x, y, z as axes of (B, D, H, W)


def _at(f, a, d):
    """f(cell + d e_a) (wraps round at the array's edge: only ever read from interior cells, whose neighbours exist)"""
    return np.roll(f, -d, _AXIS[a])


def interior(shape):
    B, D, H, W = shape
    m = np.zeros((B, D, H, W), bool)
    if D == 1:
        m[:, :, 1:H - 1, 1:W - 1] = True
    else:
        m[:, 1:D - 1, 1:H - 1, 1:W - 1] = True
    return m


def _norm(v, T):
    s = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
    return np.where(s > T(1e-6), np.sqrt(s), T(0))


def fields(U, amp, dtype=np.float32):
    """(c, w, n, F) of the operator, each a list of three (B, D, H, W) arrays (n a single one)"""
    T = np.dtype(dtype).type
    B, nc, D, H, W = U.shape
    is3d = nc == 3
    assert is3d or D == 1
    u = [U[:, a].astype(T) for a in range(nc)]
    I = interior((B, D, H, W))
    half, zero = T(0.5), np.zeros((B, D, H, W), T)
    keep = lambda f: np.where(I, f, T(0))
    # 1. centred velocity
    c = [keep(half * (u[a] + _at(u[a], a, 1))) for a in range(nc)] + ([] if is3d else [zero])
    d = lambda f, a: _at(f, a, 1) - _at(f, a, -1)
    # 2. curl and its norm
    w = [keep(half * (d(c[2], 1) - d(c[1], 2))) if is3d else zero,
         keep(half * (d(c[0], 2) - d(c[2], 0))) if is3d else zero,
         keep(half * (d(c[1], 0) - d(c[0], 1)))]
    n = keep(_norm(w, T))
    # 3. force
    g = [half * d(n, 0), half * d(n, 1), half * d(n, 2) if is3d else zero]
    m = _norm(g, T)
    ok = m > T(1e-6)
    with np.errstate(divide="ignore", invalid="ignore"):
        gh = [np.where(ok, ga / m, T(0)) for ga in g]
    a_ = T(amp)
    F = [keep((gh[1] * w[2] - gh[2] * w[1]) * a_), keep((gh[2] * w[0] - gh[0] * w[2]) * a_), keep((gh[0] * w[1] - gh[1] * w[0]) * a_)]
    return c, w, n, F


def confine(U, flags, amp, dtype=np.float32):
    """U + the confinement force, (B, 2|3, D, H, W) of `dtype`; flags (B, 1, D, H, W)"""
    T = np.dtype(dtype).type
    B, nc, D, H, W = U.shape
    _, _, _, F = fields(U, amp, dtype)
    I = interior((B, D, H, W))
    fc = flags[:, 0]
    out = U.astype(T).copy()
    for a in range(nc):
        fm = _at(fc, a, -1)
        cond = I & ((fc == FLUID) | (fc == EMPTY)) & ((fm == FLUID) | ((fm == EMPTY) & (fc == FLUID)))
        out[:, a] = np.where(cond, out[:, a] + T(0.5) * (_at(F[a], a, -1) + F[a]), out[:, a])
    return out


def sine_field(shape, seed, modes=6, noise=0.05):
    """(B, nc, D, H, W) float32: `modes` random sine modes per component plus white noise of `noise` times their amplitude"""
    B, nc, D, H, W = shape
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    U = np.zeros(shape, np.float64)
    for b in range(B):
        for a in range(nc):
            for _ in range(modes):
                k = rng.integers(1, 5, 3) * 2 * np.pi / np.array([max(D, 2), H, W])
                ph = rng.uniform(0, 2 * np.pi, 3)
                U[b, a] += rng.uniform(0.3, 1.0) * np.sin(k[0] * z + ph[0]) * np.sin(k[1] * y + ph[1]) * np.sin(k[2] * x + ph[2])
    U += noise * rng.standard_normal(shape)
    return U.astype(np.float32)


def case_flags(B, D, H, W):
    """obstacle borders, an obstacle box and a patch of empty cells (the box and the patch where the grid has room for them)"""
    f = np.full((B, 1, D, H, W), FLUID, np.float32)
    f[:, :, :, 0, :] = OBST; f[:, :, :, -1, :] = OBST; f[:, :, :, :, 0] = OBST; f[:, :, :, :, -1] = OBST
    if D > 1:
        f[:, :, 0] = OBST; f[:, :, -1] = OBST
    zs = slice(None) if D < 6 else slice(D // 3, D // 3 + 3)
    if H >= 12 and W >= 12:
        f[:, :, zs, H // 3:H // 3 + 4, W // 4:W // 4 + 5] = OBST
        ze = slice(None) if D < 6 else slice(D // 2, D // 2 + 2)
        f[:, :, ze, 2 * H // 3:2 * H // 3 + 3, W // 2:W // 2 + 4] = EMPTY
    return f
