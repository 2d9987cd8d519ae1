"""The numpy model of the 3D obstacle generators (fluid.createSphere, fluid.createBox3D, fluid.voxelizeMesh), the exact
ray cast the model is held to, and the mesh builders of the tests.

Cell (i, j, k) sits at the point (x, y, z) = (i, j, k).  Arrays are (D, H, W) = (z, y, x).

The voxeliser's rule, as the model states it (every row of the grid against every face, no bounding boxes):
  snap      q = rint(float64(v) * 64) as int64; a face is bad -- skipped and counted -- if an index is outside [0, V), a coordinate is
            NaN or Inf, or |q| > 2^20
  cover     with p = (64 j, 64 k), face (a, b, c) covers the row (j, k) iff an odd number of its three edges, projected to (y, z), are
            crossed; edge (a, b) is crossed iff (a.z > p.z) != (b.z > p.z) and, the ends ordered so that a.z < b.z,
            (b.y - a.y) (p.z - a.z) - (p.y - a.y) (b.z - a.z) > 0, in int64
  position  n = (b - a) x (c - a) in int64; in float64, in this order: num = n.y (p.y - a.y) + n.z (p.z - a.z), x = a.x - num / n.x,
            i0 = clamp(ceil(x * (1 / 64)), 0, W); the crossing toggles every cell i >= i0 of the row (i0 == W toggles no cell but counts
            for the row's parity)
  fill      a cell is inside iff the number of toggles at or before it is odd; a row whose parity at index W is odd is open
"""
from fractions import Fraction

import numpy as np

SNAP = 64
QMAX = 1 << 20
OBSTACLE, FLUID, EMPTY = 2.0, 1.0, 4.0


# ---- primitives ---------------------------------------------------------------------------------------------------------------------
def _index_grids(shape):
    D, H, W = shape
    k, j, i = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    return i.astype(np.float32), j.astype(np.float32), k.astype(np.float32)


def sphere_model(shape, cx, cy, cz, radius):
    """dx*dx + dy*dy + dz*dz <= r*r in float32, summed in that order (r*r squared in double, then rounded)"""
    x, y, z = _index_grids(shape)
    dx, dy, dz = x - np.float32(cx), y - np.float32(cy), z - np.float32(cz)
    return (dx * dx + dy * dy) + dz * dz <= np.float32(float(radius) * float(radius))


def cylinder_model(shape, cx, cy, radius):
    x, y, _ = _index_grids(shape)
    dx, dy = x - np.float32(cx), y - np.float32(cy)
    return dx * dx + dy * dy <= np.float32(float(radius) * float(radius))


def box_model(shape, x0, x1, y0, y1, z0, z1):
    x, y, z = _index_grids(shape)
    f = np.float32
    return (x >= f(x0)) & (x < f(x1)) & (y >= f(y0)) & (y < f(y1)) & (z >= f(z0)) & (z < f(z1))


# ---- the voxeliser ------------------------------------------------------------------------------------------------------------------
def snap_faces(vertices, faces):
    """-> (tri int64 (F', 3 vertices, 3 xyz) of the good faces, number of bad faces)"""
    vertices = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    V = len(vertices)
    scaled = vertices.astype(np.float64) * SNAP
    with np.errstate(invalid="ignore"):
        vert_ok = (np.isfinite(scaled) & (np.abs(scaled) <= QMAX + 1)).all(axis=1)       # (before any conversion to an integer)
    q = np.zeros((V, 3), dtype=np.int64)
    q[vert_ok] = np.rint(scaled[vert_ok]).astype(np.int64)
    vert_ok &= (np.abs(q) <= QMAX).all(axis=1)
    in_range = ((faces >= 0) & (faces < V)).all(axis=1)
    good = in_range.copy()
    good[in_range] = vert_ok[faces[in_range]].all(axis=1)
    return q[faces[good]], int((~good).sum())


def _crossed(ay, az, by, bz, py, pz):
    """the edge rule, elementwise on int64 arrays"""
    straddle = (az > pz) != (bz > pz)
    swap = az > bz
    lo_y, lo_z = np.where(swap, by, ay), np.where(swap, bz, az)
    hi_y, hi_z = np.where(swap, ay, by), np.where(swap, az, bz)
    s = (hi_y - lo_y) * (pz - lo_z) - (py - lo_y) * (hi_z - lo_z)
    return straddle & (s > 0)


def voxelize_model(shape, vertices, faces):
    """-> (inside bool (D, H, W), open rows, bad faces)"""
    D, H, W = shape
    tri, bad = snap_faces(vertices, faces)
    toggles = np.zeros((D, H, W + 1), dtype=np.int64)
    if len(tri):
        a, b, c = (tri[:, n, :, None] for n in range(3))               # (F, 3, 1)
        kk, jj = np.meshgrid(np.arange(D), np.arange(H), indexing="ij")
        kk, jj = kk.reshape(1, -1), jj.reshape(1, -1)                   # (1, rows)
        py, pz = jj.astype(np.int64) * SNAP, kk.astype(np.int64) * SNAP
        cover = (_crossed(a[:, 1], a[:, 2], b[:, 1], b[:, 2], py, pz) ^ _crossed(b[:, 1], b[:, 2], c[:, 1], c[:, 2], py, pz) ^
                 _crossed(c[:, 1], c[:, 2], a[:, 1], a[:, 2], py, pz))  # (F, rows)
        u, v = b - a, c - a
        nx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
        ny = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
        nz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
        fi, ri = np.nonzero(cover)
        assert (nx[fi, 0] != 0).all(), "an edge-on face covers nothing"
        f64 = np.float64
        num = ny[fi, 0].astype(f64) * (py[0, ri] - a[fi, 1, 0]).astype(f64) + nz[fi, 0].astype(f64) * (pz[0, ri] - a[fi, 2, 0]).astype(f64)
        x = a[fi, 0, 0].astype(f64) - num / nx[fi, 0].astype(f64)
        i0 = np.clip(np.ceil(x * (1.0 / SNAP)), 0, W).astype(np.int64)
        np.add.at(toggles, (kk[0, ri], jj[0, ri], i0), 1)
    parity = np.cumsum(toggles, axis=2) & 1
    return parity[:, :, :W].astype(bool), int(parity[:, :, W].sum()), bad


def apply_model(flags, inside, sample=None):
    """what a generator does to flags (B, 1, D, H, W): obstacle where inside, every other cell untouched"""
    out = flags.copy()
    for b in (range(flags.shape[0]) if sample is None else [sample]):
        out[b, 0][inside] = OBSTACLE
    return out


# ---- the exact ray cast -------------------------------------------------------------------------------------------------------------
def exact_cast(shape, vertices, faces, axis):
    """Even-odd ray cast of the SNAPPED mesh along `axis` (0 x, 1 y, 2 z) in exact arithmetic: integer cover tests of the lines, the
    crossing positions as fractions.  A cell is inside iff an odd number of crossings lie at or before its point -- for a point off
    the surface that is the ray cast; a point ON the surface (a crossing itself) falls on the side the half-open convention gives it.
    -> (inside bool (D, H, W), on_surface bool (D, H, W))."""
    D, H, W = shape
    tri, _ = snap_faces(vertices, faces)
    n_of = {0: W, 1: H, 2: D}
    ua, va = [(1, 2), (2, 0), (0, 1)][axis]                 # the two axes of the projection
    inside = np.zeros((D, H, W), dtype=bool)
    surface = np.zeros((D, H, W), dtype=bool)
    lines = [(p, q) for q in range(n_of[va]) for p in range(n_of[ua])]
    pu = np.array([p for p, _ in lines], dtype=np.int64).reshape(1, -1) * SNAP
    pv = np.array([q for _, q in lines], dtype=np.int64).reshape(1, -1) * SNAP
    a, b, c = (tri[:, n, :, None] for n in range(3))
    cover = (_crossed(a[:, ua], a[:, va], b[:, ua], b[:, va], pu, pv) ^ _crossed(b[:, ua], b[:, va], c[:, ua], c[:, va], pu, pv) ^
             _crossed(c[:, ua], c[:, va], a[:, ua], a[:, va], pu, pv))
    crossings = {}
    for f, l in zip(*np.nonzero(cover)):
        A, B, C = (tuple(int(t) for t in tri[f, n]) for n in range(3))
        U, V = [B[n] - A[n] for n in range(3)], [C[n] - A[n] for n in range(3)]
        n = [U[1] * V[2] - U[2] * V[1], U[2] * V[0] - U[0] * V[2], U[0] * V[1] - U[1] * V[0]]
        assert n[axis] != 0
        num = n[ua] * (int(pu[0, l]) - A[ua]) + n[va] * (int(pv[0, l]) - A[va])
        crossings.setdefault(int(l), []).append(Fraction(A[axis]) - Fraction(num, n[axis]))
    for l, ts in crossings.items():
        for m in range(n_of[axis]):
            pos = [0, 0, 0]
            pos[axis], pos[ua], pos[va] = m, lines[l][0], lines[l][1]
            t = m * SNAP
            inside[pos[2], pos[1], pos[0]] = sum(1 for s in ts if s <= t) & 1
            surface[pos[2], pos[1], pos[0]] = any(s == t for s in ts)
    return inside, surface


# ---- meshes -------------------------------------------------------------------------------------------------------------------------
def icosphere(n):
    """the unit icosahedron subdivided n times onto the unit sphere: 20 * 4^n faces.  -> (vertices float64 (V, 3), faces int32 (F, 3))"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], dtype=np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                  [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], dtype=np.int64)
    for _ in range(n):
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        key = e.min(axis=1) * len(v) + e.max(axis=1)
        uniq, inv = np.unique(key, return_inverse=True)
        mid = v[uniq // len(v)] + v[uniq % len(v)]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        ab, bc, ca = (len(v) + inv.reshape(3, -1))
        A, B, C = f[:, 0], f[:, 1], f[:, 2]
        f = np.concatenate([np.stack([A, ab, ca], 1), np.stack([B, bc, ab], 1), np.stack([C, ca, bc], 1), np.stack([ab, bc, ca], 1)])
        v = np.concatenate([v, mid])
    return v, f.astype(np.int32)


def box_mesh(lo, hi):
    """the 12 triangles of the axis-aligned box lo..hi"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    v = np.array([[(lo, hi)[(n >> d) & 1][d] for d in range(3)] for n in range(8)], dtype=np.float64)     # bit d of n: the high side of axis d
    f = np.array([[0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3],      # x = lo, x = hi
                  [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6],      # y = lo, y = hi
                  [0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5]], dtype=np.int32)
    return v, f


def torus(R, r, nu=24, nv=12):
    """a torus about the z axis: centre-line radius R, tube radius r, nu x nv quads as 2 nu nv triangles"""
    u, w = np.meshgrid(np.arange(nu) * (2 * np.pi / nu), np.arange(nv) * (2 * np.pi / nv), indexing="ij")
    v = np.stack([(R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)], axis=-1).reshape(-1, 3)
    iu, iw = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    p00, p10 = iu * nv + iw, ((iu + 1) % nu) * nv + iw
    p01, p11 = iu * nv + (iw + 1) % nv, ((iu + 1) % nu) * nv + (iw + 1) % nv
    f = np.concatenate([np.stack([p00, p10, p11], -1).reshape(-1, 3), np.stack([p00, p11, p01], -1).reshape(-1, 3)])
    return v, f.astype(np.int32)


def rotation(seed):
    """a seeded random rotation matrix"""
    q, r = np.linalg.qr(np.random.RandomState(seed).randn(3, 3))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def placed(mesh, scale=1.0, offset=(0.0, 0.0, 0.0), rot=None):
    """(vertices, faces) scaled (a number or one per axis), rotated and moved; vertices as the float32 the voxeliser takes"""
    v, f = mesh
    v = v * np.asarray(scale, dtype=np.float64)
    if rot is not None:
        v = v @ rot.T
    return (v + np.asarray(offset, dtype=np.float64)).astype(np.float32), f


# ---- the fixtures of tests/test_voxel_reference.py and tests/test_voxelize_gpu.py ------------------------------------------------------
GRID = (12, 20, 36)                                          # (D, H, W)
BOX_LO, BOX_HI = (2, 3, 1), (7, 8, 6)
BALL_R, BALL_C = 5.2, (17.3, 9.6, 5.9)
ROT_HALF, ROT_C, ROT_SEED = (6.1, 3.3, 2.2), (17.2, 9.9, 6.1), 36


def fixtures():
    """name -> (vertices float32, faces int32): the four closed fixtures on GRID"""
    return {
        "integer_box": placed(box_mesh(BOX_LO, BOX_HI)),
        "icosphere": placed(icosphere(2), BALL_R, BALL_C),
        "icosphere_clipped": placed(icosphere(2), BALL_R, (1.2, 9.6, 10.4)),
        "rotated_box": placed(box_mesh([-h for h in ROT_HALF], ROT_HALF), 1.0, ROT_C, rotation(ROT_SEED)),
    }
