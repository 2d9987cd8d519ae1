"""Dimension-generic numpy model of the fluid operators (TEST INFRASTRUCTURE): advectScalar, advectVelocity, addBuoyancy,
addGravity, setWallBcs, plus velocityDivergence / velocityUpdate and the chain of one Jacobi time step.

Written from the rules of SURVEY.md sections A / B and the operator semantics of include/fluidnet_hip.h -- not from
oracle/fluid_oracle.c.  Every rule is stated once for "an axis a"; the functions loop over `axes = (x, y)` (velocity with
two channels) or `(x, y, z)` (three channels) and no rule is written for z on its own.  The 2D rules are pinned bit-for-bit
to the reference (tests/golden/ops_2d_*), so a model that reproduces those goldens with the axis as a loop variable states
what "z is treated as x and y are" means in 3D default mode (ref_quirks = 0).  Quirks mode (Q10-Q15) and z-slab views are
not modelled.

Arrays are (B, C, D, H, W), x fastest; axis a lives in array dimension 4 - a and in velocity channel a.  `dtype` selects the
arithmetic (np.float64: the model proper; np.float32: the same expressions in the kernels' precision, which is what the
tolerances of the tests are measured from).  Cells are vectorised; the line trace is a loop over unit steps with the set
of rays still travelling.

WHERE THE REFERENCE IS ANISOTROPIC BY CONSTRUCTION -- the only places below that name an axis.  A difference between this
model and the kernels / the oracle that is not on this list is a finding.
 1. NEST: interpolation reduces the corner pairs along y first, then x, then z, and the fluid-aware variant falls back
    corner by corner in that order (reference grid.cpp:118-269, with Q15 repaired: the g/h corners read the flag at x0+1).
    Rounding-level for plain interpolation, value-level beside non-fluid corners for the fluid-aware one.
 2. The ray/box test picks the exit plane by "first axis wins" on ties, axes in the order x, y, z
    (calc_line_trace.cpp:73-149); np.argmax over an axis-ordered array is that rule.
 3. SHUFFLE: on an interior non-fluid cell advectVel's semi-Lagrange pass writes (src_y, 0, src_z) (Q1,
    fluids_init.cpp:413-416): channel x receives y's value, channel y is zeroed, channel z is kept.
 4. WALLBC_SKIP_AT_0: setWallBcs at index 0 of an axis: for x and y the lower neighbour clamps to the cell itself, for z the
    rule is skipped on the plane k = 0 (set_wall_bcs.py:54-84).
 5. The border test has no z term in 2D (fluids_init.cpp:313-320), and a 2D position has z = 0.5 with zero displacement:
    both follow from looping over the axes present.
 6. MacCormackCorrectMAC skips the correction when the cell below along the component's axis is not fluid, tested only
    when the index along that axis is > 0 (fluids_init.cpp:473-496): always true on the interior cells the operator
    writes, so no axis is named for it.
 7. velocityUpdate: the 2D reference also updates fluid/empty faces (velocity_update.py:47-149); the 3D rule is the
    fluid-fluid term alone (solver_cpp/src/projection/update_vel.cpp:58-117).  EMPTY_FACE_TERMS names the dimension.
 8. Summation orders that name an axis only through the loop order x, y, z: divergence ((ux - ux+) + uy) - uy+, then
    + (uz - uz+) (velocity_divergence.py:61-65); the 2-norm of the displacement.  Rounding-level.
"""
import numpy as np

FLUID, OBST, EMPTY = 1.0, 2.0, 4.0
HIT_MARGIN = 1e-5           # calc_line_trace.cpp:7
EPSILON = 1e-12             # calc_line_trace.cpp:8

NEST = (1, 0, 2)            # exception 1: reduction order of the interpolation
SHUFFLE = {0: 1, 1: None, 2: 2}   # exception 3: channel -> source channel on interior non-fluid cells (None: zero)
WALLBC_SKIP_AT_0 = (2,)     # exception 4: axes whose setWallBcs rule is skipped at index 0 (the others clamp to the cell)
EMPTY_FACE_TERMS = (2,)     # exception 7: numbers of axes for which velocityUpdate has the fluid/empty face terms


class _Grid:
    """index bookkeeping of one (B, *, D, H, W) problem with `nd` axes"""

    def __init__(self, flags, nd, dtype):
        B, _, D, H, W = flags.shape
        assert nd in (2, 3) and (nd == 3 or D == 1)
        self.B, self.nd, self.dtype = B, nd, dtype
        self.shape = (B, 1, D, H, W)
        self.n = (W, H, D)[:nd]
        self.stride = (1, W, H * W)[:nd]
        self.cells = D * H * W
        self.N = B * self.cells
        g = np.arange(self.N)
        self.base = (g // self.cells) * self.cells
        r = g - self.base
        self.idx = [(r // self.stride[a]) % self.n[a] for a in range(nd)]
        f = np.asarray(flags).reshape(-1)
        self.fluid, self.obst, self.empty = f == FLUID, f == OBST, f == EMPTY
        self.border = np.zeros(self.N, bool)
        for a in range(nd):
            self.border |= (self.idx[a] < 1) | (self.idx[a] > self.n[a] - 2)
        self.inner = ~self.border
        self.size = np.array(self.n, dtype).reshape(nd, 1)

    def chans(self, U):
        U = np.asarray(U)
        assert U.shape[1] == self.nd and U.shape[0] == self.B
        return [U[:, c].reshape(-1).astype(self.dtype) for c in range(self.nd)]

    def scalar(self, s):
        return np.asarray(s).reshape(-1).astype(self.dtype)

    def out(self, chans):
        sh = (self.B,) + self.shape[2:]
        return np.stack([c.reshape(sh) for c in chans], 1)

    def cell(self, base, q):
        g = base.copy()
        for a in range(self.nd):
            g += q[a] * self.stride[a]
        return g


# ---- MAC sampling -------------------------------------------------------------------------
def _centred(G, U, cells):
    """velocity at the cell centre: the mean of the two faces along every axis"""
    return [G.dtype(0.5) * (U[a][cells] + U[a][cells + G.stride[a]]) for a in range(G.nd)]


def _at_face(G, U, cells, c):
    """velocity at the lower face along axis c: component c itself, every other component a the mean of its four faces around
    that point, summed in the order (cell, cell - e_c, cell + e_a, cell + e_a - e_c)"""
    v = []
    for a in range(G.nd):
        if a == c:
            v.append(U[a][cells])
        else:
            ec, ea = G.stride[c], G.stride[a]
            v.append(G.dtype(0.25) * (((U[a][cells] + U[a][cells - ec]) + U[a][cells + ea]) + U[a][cells + ea - ec]))
    return v


# ---- interpolation ------------------------------------------------------------------------
def _interp(G, field, base, pos, fluid=None):
    """multilinear sample of the flat scalar `field` at `pos` (nd, N).  Weights come from the unclamped integer part of
    pos - 0.5, the corner index is clamped to [0, n - 2] afterwards, then every weight is clamped to [0, 1].  With `fluid`
    (flat mask) the pairs reduce fluid-aware: neither corner fluid -> (0, not fluid); one -> its value; both -> the
    weighted mean; a sample that ends not fluid is taken again plainly."""
    one = G.dtype(1)
    q0, w = [], []
    for a in range(G.nd):
        p = pos[a] - G.dtype(0.5)
        q = np.trunc(p)
        hi = p - q
        lo = one - hi
        q0.append(np.clip(q.astype(np.int64), 0, G.n[a] - 2))
        w.append((np.clip(lo, 0, 1), np.clip(hi, 0, 1)))
    corners = {}
    for code in range(1 << G.nd):
        off = tuple((code >> a) & 1 for a in range(G.nd))
        g = G.cell(base, [q0[a] + off[a] for a in range(G.nd)])
        corners[off] = (field[g], None if fluid is None else fluid[g])

    def reduce(aware):
        cur = {k: (v, f if aware else None) for k, (v, f) in corners.items()}
        for a in [a for a in NEST if a < G.nd]:
            nxt = {}
            for k, (lo, flo) in cur.items():
                if k[a] != 0:
                    continue
                hi, fhi = cur[k[:a] + (1,) + k[a + 1:]]
                mean = lo * w[a][0] + hi * w[a][1]
                if aware:
                    val = np.where(flo & fhi, mean, np.where(flo, lo, np.where(fhi, hi, G.dtype(0))))
                    nxt[k[:a] + (None,) + k[a + 1:]] = (val, flo | fhi)
                else:
                    nxt[k[:a] + (None,) + k[a + 1:]] = (mean, None)
            cur = nxt
        (res,) = cur.values()
        return res

    plain, _ = reduce(False)
    if fluid is None:
        return plain
    val, ok = reduce(True)
    return np.where(ok, val, plain)


# ---- line trace ---------------------------------------------------------------------------
def _outside(G, P):
    return ((P <= 0) | (P >= G.size)).any(0)


def _blocked(G, base, P):
    """P is inside the domain and its cell is not fluid"""
    out = _outside(G, P)
    q = [np.clip(np.trunc(P[a]).astype(np.int64), 0, G.n[a] - 1) for a in range(G.nd)]
    return ~out & ~G.fluid[G.cell(base, q)]


def _ray_box(G, origin, dirn, ctr):
    """Graphics-Gems ray/box hit (SURVEY A.3 case 2; the origin-inside-the-box behaviour is Q7): (hit, point)"""
    m, d = G.dtype(HIT_MARGIN), G.dtype
    lo, hi = (ctr - d(0.5)) - m, (ctr + d(0.5)) + m
    left, right = origin < lo, origin > hi
    mid = ~left & ~right
    cand = np.where(left, lo, np.where(right, hi, d(0)))
    inside = mid.all(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(~inside & ~mid & (dirn != 0), (cand - origin) / dirn,
                     np.where((~inside & mid) | (dirn == 0), d(-1), d(0)))
    which = np.argmax(t, 0)                                   # exception 2: the first axis wins a tie
    cols = np.arange(t.shape[1])
    fin = t[which, cols]
    hit = ~((fin < 0) & ~inside)
    coord = origin + fin * dirn
    coord[which, cols] = cand[which, cols]
    other = np.arange(G.nd)[:, None] != which[None, :]
    hit &= ~(other & ((coord < lo - d(1e-6)) | (coord > hi + d(1e-6)))).any(0)
    return hit, coord


TRACE_STATS = {"border": 0, "blocked": 0}    # rays that took case 1 / case 2 since the caller last zeroed it (coverage of the states)


def _trace(G, base, pos, delta):
    """end point of the ray pos -> pos + delta that stops in front of the domain border and of non-fluid cells"""
    d = G.dtype
    m, eps = d(HIT_MARGIN), d(EPSILON)
    res = pos.copy()
    length = np.sqrt((delta * delta).sum(0))
    go = ~_outside(G, pos) & ~_blocked(G, base, pos) & (length > eps)
    live = np.nonzero(go)[0]
    p0, new, L, bs = pos[:, live], pos[:, live].copy(), length[live], base[live]
    dirn = delta[:, live] / L
    cur = np.zeros(live.size, d)
    for _ in range(sum(G.n) + 8):
        keep = cur < L - m
        res[:, live[~keep]] = new[:, ~keep]
        live, p0, new, L, bs, dirn, cur = live[keep], p0[:, keep], new[:, keep], L[keep], bs[keep], dirn[:, keep], cur[keep]
        if live.size == 0:
            break
        step = np.minimum(L - cur, d(1))
        nxt = new + dirn * step
        done = np.zeros(live.size, bool)
        out = _outside(G, nxt)
        TRACE_STATS["border"] += int(out.sum())
        if out.any():
            # case 1: intersect the line pos -> nxt (from the ORIGINAL pos, Q9) with the border faces it crosses
            dl = nxt - p0
            ok = np.abs(dl) >= eps
            with np.errstate(divide="ignore", invalid="ignore"):
                g_lo = np.where((nxt <= m) & ok, (m - p0) / dl, np.inf)
                g_hi = np.where((nxt >= G.size - m) & ok, ((G.size - m) - p0) / dl, np.inf)
            gam = np.minimum(g_lo, g_hi).min(0)
            valid = (gam >= 0) & (gam < np.inf)
            with np.errstate(invalid="ignore"):
                ip = np.where(valid, gam * dl + p0, np.clip(nxt, m, G.size - m)).astype(d)
            free = out & ~_blocked(G, bs, ip)
            new[:, free] = ip[:, free]
            done |= free
            stuck = out & ~free
            nxt[:, stuck] = ip[:, stuck]
        blk = _blocked(G, bs, nxt) & ~done
        TRACE_STATS["blocked"] += int(blk.sum())
        if blk.any():
            # case 2: back off to the blocker's box, up to four times
            failed = np.zeros(live.size, bool)
            for _ in range(4):
                todo = blk & ~failed & _blocked(G, bs, nxt)
                if not todo.any():
                    break
                hit, coord = _ray_box(G, new[:, todo], dirn[:, todo], np.trunc(nxt[:, todo]) + d(0.5))
                t = np.nonzero(todo)[0]
                failed[t[~hit]] = True
                nxt[:, t[hit]] = coord[:, hit]
            ok = blk & ~failed & ~_blocked(G, bs, nxt)
            new[:, ok] = nxt[:, ok]
            done |= blk
        adv = ~done
        new[:, adv] = nxt[:, adv]
        cur = cur + np.where(adv, step, d(0))
        res[:, live[done]] = new[:, done]
        live, p0, new, L, bs, dirn, cur = live[adv], p0[:, adv], new[:, adv], L[adv], bs[adv], dirn[:, adv], cur[adv]
    res[:, live] = new
    return res


# ---- advectScalar -------------------------------------------------------------------------
def _centres(G, cells):
    return np.stack([G.idx[a][cells].astype(G.dtype) + G.dtype(0.5) for a in range(G.nd)])


def _sl_scalar(G, dt, src, U, outside):
    """one semi-Lagrange pass: 0 on the border, src on interior non-fluid cells, the sample at the traced point on fluid cells;
    also the traced point (the cell centre where nothing is traced)"""
    dst = np.where(G.inner, src, G.dtype(0))
    pos = _centres(G, np.arange(G.N))
    cells = np.nonzero(G.inner & G.fluid)[0]
    disp = np.stack([(-dt) * c for c in _centred(G, U, cells)])
    back = _trace(G, G.base[cells], pos[:, cells], disp)
    dst[cells] = _interp(G, src, G.base[cells], back, None if outside else G.fluid)
    pos[:, cells] = back
    return dst, pos


def advect_scalar(dt, src, U, flags, method="maccormackFluidNet", sample_outside_fluid=False, strength=0.75,
                  dtype=np.float64):
    nd = np.asarray(U).shape[1]
    G = _Grid(flags, nd, dtype)
    dt, s, u = dtype(dt), G.scalar(src), G.chans(U)
    fwd, fpos = _sl_scalar(G, dt, s, u, sample_outside_fluid)
    if method == "eulerFluidNet":
        return fwd.reshape(G.shape)
    assert method == "maccormackFluidNet"
    bwd, _ = _sl_scalar(G, -dt, fwd, u, sample_outside_fluid)
    dst = np.where(G.fluid, fwd + (dtype(strength) * dtype(0.5)) * (s - bwd), fwd)      # every cell, border included (Q3)
    # clamp to the source values of the 3^nd cells around the traced point that are fluid (or any, sampling outside)
    cells = np.nonzero(G.inner)[0]
    q0 = [np.clip(np.trunc(fpos[a, cells]).astype(np.int64), 0, G.n[a] - 1) for a in range(nd)]
    mn = np.full(cells.size, np.inf, dtype); mx = -mn
    for code in range(3 ** nd):
        off = [(code // 3 ** a) % 3 - 1 for a in range(nd)]
        q = [q0[a] + off[a] for a in range(nd)]
        ok = np.ones(cells.size, bool)
        for a in range(nd):
            ok &= (q[a] >= 0) & (q[a] < G.n[a])
        g = G.cell(G.base[cells], [np.clip(q[a], 0, G.n[a] - 1) for a in range(nd)])
        if not sample_outside_fluid:
            ok &= G.fluid[g]
        mn = np.where(ok, np.minimum(mn, s[g]), mn)
        mx = np.where(ok, np.maximum(mx, s[g]), mx)
    dst[cells] = np.where(mn <= mx, np.maximum(mn, np.minimum(mx, dst[cells])), fwd[cells])
    return dst.reshape(G.shape)


# ---- advectVelocity -----------------------------------------------------------------------
def _sl_mac(G, dt, src, U):
    dst = [np.zeros(G.N, G.dtype) for _ in range(G.nd)]
    solid = np.nonzero(G.inner & ~G.fluid)[0]
    cells = np.nonzero(G.inner & G.fluid)[0]
    ctr = _centres(G, cells)
    for c in range(G.nd):
        if SHUFFLE[c] is not None:                             # exception 3
            dst[c][solid] = src[SHUFFLE[c]][solid]
        v = _at_face(G, U, cells, c)
        pos = np.stack([ctr[a] + v[a] * (-dt) for a in range(G.nd)])
        dst[c][cells] = _interp(G, src[c], G.base[cells], pos)
    return dst


def advect_velocity(dt, orig, U, flags, method="maccormackFluidNet", strength=0.75, dtype=np.float64):
    nd = np.asarray(U).shape[1]
    G = _Grid(flags, nd, dtype)
    dt, o, u = dtype(dt), G.chans(orig), G.chans(U)
    fwd = _sl_mac(G, dt, o, u)
    if method == "eulerFluidNet":
        return G.out(fwd)
    assert method == "maccormackFluidNet"
    bwd = _sl_mac(G, -dt, fwd, u)
    cells = np.nonzero(G.inner)[0]
    out = [np.zeros(G.N, dtype) for _ in range(nd)]
    for c in range(nd):
        skip = ~G.fluid[cells] | ~G.fluid[cells - G.stride[c]]                       # (exception 6)
        corr = fwd[c][cells] + (dtype(strength) * dtype(0.5)) * (o[c][cells] - bwd[c][cells])
        val = np.where(skip, fwd[c][cells], corr)
        # clamp to orig_c on the 2^nd corners around the integer parts of (index -+ dt * face velocity)
        v = [x * dt for x in _at_face(G, u, cells, c)]
        mn = np.full(cells.size, np.inf, dtype); mx = -mn
        for sign in (-1, 1):
            q0 = [np.clip(np.trunc(G.idx[a][cells].astype(dtype) + dtype(sign) * v[a]).astype(np.int64), 0, G.n[a] - 2)
                  for a in range(nd)]
            for code in range(1 << nd):
                g = G.cell(G.base[cells], [q0[a] + ((code >> a) & 1) for a in range(nd)])
                mn = np.minimum(mn, o[c][g]); mx = np.maximum(mx, o[c][g])
        out[c][cells] = np.maximum(np.minimum(val, mx), mn)
    return G.out(out)


# ---- source terms and boundary conditions ---------------------------------------
def add_buoyancy(U, flags, rho, gravity, rho_star, dt, dtype=np.float64):
    """U_a += (g_a dt) (0.5 (rho + rho[-e_a]) - rho*) on interior fluid cells whose lower neighbour along a is fluid"""
    nd = np.asarray(U).shape[1]
    G = _Grid(flags, nd, dtype)
    u, r = G.chans(U), G.scalar(rho)
    cells = np.nonzero(G.inner & G.fluid)[0]
    for a in range(nd):
        t = cells[G.fluid[cells - G.stride[a]]]
        u[a][t] = u[a][t] + (dtype(gravity[a]) * dtype(dt)) * ((dtype(0.5) * (r[t] + r[t - G.stride[a]])) - dtype(rho_star))
    return G.out(u)


def add_gravity(U, flags, gravity, dt, dtype=np.float64):
    """U_a += g_a dt on interior fluid / empty cells whose lower neighbour along a is fluid, or empty beside a fluid cell"""
    nd = np.asarray(U).shape[1]
    G = _Grid(flags, nd, dtype)
    u = G.chans(U)
    cells = np.nonzero(G.inner & (G.fluid | G.empty))[0]
    for a in range(nd):
        lo = cells - G.stride[a]
        t = cells[G.fluid[lo] | (G.empty[lo] & G.fluid[cells])]
        u[a][t] = u[a][t] + dtype(gravity[a]) * dtype(dt)
    return G.out(u)


def set_wall_bcs(U, flags, dtype=np.float64):
    """on every fluid / obstacle cell (border included): U_a = 0 if the lower neighbour along a is an obstacle, or the cell is
    an obstacle and that neighbour is fluid"""
    nd = np.asarray(U).shape[1]
    G = _Grid(flags, nd, dtype)
    u = G.chans(U)
    cells = np.nonzero(G.fluid | G.obst)[0]
    for a in range(nd):
        c = cells[G.idx[a][cells] > 0] if a in WALLBC_SKIP_AT_0 else cells               # exception 4
        lo = c - np.where(G.idx[a][c] > 0, G.stride[a], 0)
        z = c[G.obst[lo] | (G.obst[c] & G.fluid[lo])]
        u[a][z] = 0
    return G.out(u)


def velocity_divergence(U, flags, dtype=np.float64):
    """-div u on interior cells, 0 on the border and in obstacles"""
    nd = np.asarray(U).shape[1]
    G = _Grid(flags, nd, dtype)
    u = G.chans(U)
    cells = np.nonzero(G.inner & ~G.obst)[0]
    d = np.zeros(G.N, dtype)
    acc = (u[0][cells] - u[0][cells + G.stride[0]]) + u[1][cells]
    acc = acc - u[1][cells + G.stride[1]]
    for a in range(2, nd):
        acc = acc + (u[a][cells] - u[a][cells + G.stride[a]])
    d[cells] = acc
    return d.reshape(G.shape)


def velocity_update(p, U, flags, dtype=np.float64):
    """interior faces: U_a -= p - p[-e_a] between two fluid cells, 0 on every other face (2D: plus the fluid/empty terms)"""
    nd = np.asarray(U).shape[1]
    G = _Grid(flags, nd, dtype)
    u, P = G.chans(U), G.scalar(p)
    cells = np.nonzero(G.inner)[0]
    for a in range(nd):
        lo = cells - G.stride[a]
        fc, fl, ec, el = G.fluid[cells], G.fluid[lo], G.empty[cells], G.empty[lo]
        val = np.where(fc & fl, u[a][cells] - (P[cells] - P[lo]), dtype(0))
        if nd in EMPTY_FACE_TERMS:                                                         # exception 7
            val = np.where(fc & el, u[a][cells] - P[cells], np.where(ec & fl, u[a][cells] + P[lo], val))
        u[a][cells] = val
    return G.out(u)


def jacobi_sweeps(flags, div, nsweeps, dtype=np.float64):
    """`nsweeps` Jacobi sweeps from p = 0 written as p <- p + (div - A p) / denom on the active cells, A the pressure matrix of
    tests/poisson_reference.py (no solver model of its own)"""
    import poisson_reference as PR
    is3d = np.asarray(flags).shape[2] > 1
    p = np.zeros(np.asarray(div).shape, dtype)
    for b in range(p.shape[0]):
        A, act = PR.matrix(np.asarray(flags)[b, 0], is3d)
        A = A.astype(dtype)
        rhs = np.asarray(div)[b, 0].reshape(-1).astype(dtype)
        x = np.zeros(rhs.size, dtype)
        for _ in range(nsweeps):
            x = np.where(act, x + (rhs - A @ x) / dtype(6 if is3d else 4), dtype(0)).astype(dtype)
        p[b, 0] = x.reshape(p.shape[2:])
    return p


def jacobi_step(U, flags, rho, dt, strength, sample_outside_fluid, buoyancy_scale, gravity_vec, rho_star, nsweeps,
                dtype=np.float64):
    """one simulate(..., 'jacobi') step without boundary-condition arrays: advect, buoyancy, setWallBcs, divergence,
    `nsweeps` Jacobi sweeps, velocity update, setWallBcs.  Returns (p, U, density)."""
    rho1 = advect_scalar(dt, rho, U, flags, "maccormackFluidNet", sample_outside_fluid, strength, dtype)
    U1 = advect_velocity(dt, U, U, flags, "maccormackFluidNet", strength, dtype)
    g = [dtype(x) * dtype(-buoyancy_scale) for x in gravity_vec]
    U1 = add_buoyancy(U1, flags, rho1, g, rho_star, dt, dtype)
    U1 = set_wall_bcs(U1, flags, dtype)
    div = velocity_divergence(U1, flags, dtype)
    p = jacobi_sweeps(flags, div, nsweeps, dtype)
    U1 = velocity_update(p, U1, flags, dtype)
    return p, set_wall_bcs(U1, flags, dtype), rho1
