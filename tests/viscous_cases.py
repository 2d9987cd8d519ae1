"""States shared by test_viscous_model_nd.py (CPU) and test_viscous3d_gpu.py (GPU): random 2D states for the quirks model against the
oracle, and the 3D states of semantics3d_cases.OWN with a stick field.  Every array is built once per process and never modified."""
import functools

import numpy as np

import semantics3d_cases as C
import viscous_model_nd as V

DT, NU = 0.1, 0.7            # coef = 0.07: inside the stable range of both dimensions, and no power of two


def _freeze(s):
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


def _stick_subset(rng, flags, share):
    fs = flags.copy()
    fs[(flags == V.OBST) & (rng.random(flags.shape) < share)] = V.STICK
    return fs


@functools.lru_cache(maxsize=None)
def state2d(H, W, seed, B=2, fluid_stick=True, open_border=False):
    """border wall, random obstacle boxes, a one-cell protrusion on the first box, a wall one cell thick, a few Empty cells; a random
    subset of the obstacle cells (the border's included) is Stick, and with fluid_stick so are two fluid cells (the reference tests the
    stick field alone, so a Stick cell need not be an obstacle).  open_border: one fluid Stick cell on each of the faces i = 0 and
    j = H - 1, where the reference reads its own flag through the clamped neighbour index."""
    rng = np.random.default_rng(seed)
    f = np.full((B, 1, 1, H, W), V.FLUID, np.float32)
    f[:, :, :, 0] = f[:, :, :, -1] = f[..., 0] = f[..., -1] = V.OBST
    for b in range(B):
        for n in range(3):
            h, w = rng.integers(1, 4, 2)
            j, i = rng.integers(2, H - 2 - h), rng.integers(2, W - 2 - w)
            f[b, 0, 0, j:j + h, i:i + w] = V.OBST
            if n == 0:
                f[b, 0, 0, j - 1, i] = V.OBST                      # a one-cell protrusion
        j = int(rng.integers(3, H - 3))
        f[b, 0, 0, j, 2:W // 2] = V.OBST                           # a wall one cell thick
        for _ in range(3):
            f[b, 0, 0, rng.integers(1, H - 1), rng.integers(1, W - 1)] = V.EMPTY
    if open_border:
        f[:, 0, 0, 5, 0] = f[:, 0, 0, H - 1, 7] = V.FLUID
    fs = _stick_subset(rng, f, 0.6)
    if open_border:
        fs[:, 0, 0, 5, 0] = fs[:, 0, 0, H - 1, 7] = V.STICK
    if fluid_stick:
        for b in range(B):
            jj, ii = np.nonzero(f[b, 0, 0] == V.FLUID)
            for q in rng.choice(len(jj), 2, replace=False):
                fs[b, 0, 0, jj[q], ii[q]] = V.STICK
    U = rng.standard_normal((B, 2, 1, H, W)).astype(np.float32)
    return _freeze(dict(flags=f, flags_stick=fs, U=U))


def random3d(D, H, W, seed, B=1):
    """a random 3D flag field with boxes, single cells (protrusions among them) and Empty cells; Stick is a subset of the obstacles"""
    rng = np.random.default_rng(seed)
    f = np.full((B, 1, D, H, W), V.FLUID, np.float32)
    f[:, :, :, 0] = f[:, :, :, -1] = f[..., 0] = f[..., -1] = f[:, :, 0] = f[:, :, -1] = V.OBST
    for b in range(B):
        for _ in range(4):
            d, h, w = rng.integers(1, 4, 3)
            k, j, i = rng.integers(1, D - d), rng.integers(1, H - h), rng.integers(1, W - w)
            f[b, 0, k:k + d, j:j + h, i:i + w] = V.OBST
        for _ in range(6):
            f[b, 0, rng.integers(1, D - 1), rng.integers(1, H - 1), rng.integers(1, W - 1)] = V.OBST
        for _ in range(3):
            f[b, 0, rng.integers(1, D - 1), rng.integers(1, H - 1), rng.integers(1, W - 1)] = V.EMPTY
    U = rng.standard_normal((B, 3, D, H, W)).astype(np.float32)
    return _freeze(dict(flags=f, flags_stick=_stick_subset(rng, f, 0.7), U=U))


SHAPES_3D = {"small": (2, 5, 9, 13), "tile": (1, 10, 11, 67)}     # the shapes of semantics3d_cases.OWN


@functools.lru_cache(maxsize=None)
def state3d(name):
    """the obstacles of semantics3d_cases (a plate one plane thick, a bar along z, single cells, Empty cells) plus one obstacle cell
    beside a single one, which gives that one three fluid transverse neighbours; Stick: the whole plate or bar with its edges and
    corners, the single cells, a random 60 % of the rest (the domain walls included) and two fluid cells"""
    B, D, H, W = SHAPES_3D[name]
    rng = np.random.default_rng(71 + D)
    f = C._own_flags(B, D, H, W)
    if name == "tile":
        f[:, :, 3, 4, 11] = V.OBST                                 # beside the single cell (3, 4, 10)
        whole = [(slice(5, 6), slice(2, 7), slice(20, 40)), (slice(3, 4), slice(4, 5), slice(10, 12)), (slice(7, 8), slice(2, 3), slice(50, 51))]
    else:
        f[:, :, 2, 4, 7] = V.OBST                                  # beside the single cell (2, 4, 6)
        whole = [(slice(1, 4), slice(6, 7), slice(9, 10)), (slice(2, 3), slice(4, 5), slice(6, 8))]
    fs = _stick_subset(rng, f, 0.6)
    for k, j, i in whole:
        fs[:, :, k, j, i] = np.where(f[:, :, k, j, i] == V.OBST, V.STICK, fs[:, :, k, j, i])
    for b in range(B):
        kk, jj, ii = np.nonzero(f[b, 0] == V.FLUID)
        for q in rng.choice(len(kk), 2, replace=False):
            fs[b, 0, kk[q], jj[q], ii[q]] = V.STICK
    U = rng.standard_normal((B, 3, D, H, W)).astype(np.float32)
    return _freeze(dict(flags=f, flags_stick=fs, U=U))


def contributions(flags, flags_stick, nd):
    """per component c, the number n of fluid transverse neighbours of every Stick cell (0 elsewhere): what the ghost value divides by"""
    f = np.asarray(flags)[:, 0]
    S = np.asarray(flags_stick)[:, 0] == V.STICK
    fluid = f == V.FLUID
    out = []
    for c in range(nd):
        n = np.zeros(f.shape, int)
        for a in range(nd):
            if a != c:
                n += V._sh(fluid, a, -1, False).astype(int) + V._sh(fluid, a, 1, False)
        out.append(np.where(S, n, 0))
    return out


@functools.lru_cache(maxsize=None)
def model3d(name, dtype=np.float32):
    """both operators of the 3D model on state3d(name): the float32 run is the expected bits"""
    s = state3d(name)
    o = dict(add_viscosity=V.add_viscosity(DT, s["U"], s["flags"], NU, 3, dtype=dtype),
             set_wall_bcs_stick=V.set_wall_bcs_stick(s["U"], s["flags"], s["flags_stick"], 3, dtype=dtype))
    return _freeze(o)
