"""Dimension-generic numpy model of the two viscous-flow operators (TEST INFRASTRUCTURE): addViscosity and setWallBcsStick over
`nd` axes, in the style of fluid_model_nd.py.  The axis is a loop variable; component c lives on the low face of axis c (array
dimension 4 - c of a (B, C, D, H, W) field, x fastest); flags are compared as floats; `dtype` selects the arithmetic.

Both operators are selects, negations, adds, multiplies and one divide in a fixed order, every one of them a single rounding and none
contracted into an FMA.  So the float32 run of this model is not an approximation of what the kernels compute: it is the expected
bits (as with vorticity_reference.py and render_reference.py).

`ref_quirks` exists for nd = 2 only and turns the model into the reference's 2D operators (oracle.add_viscosity,
oracle.set_wall_bcs_stick) bit for bit; it names every place where the reference is not the rule stated for "an axis".  In 3D the
reference cannot run (viscosity.py never defines mask_fluid_k; set_wall_bcs_stick.py:85-87 has misspelt names), so there is nothing to
reproduce and the default semantics are the only ones.
"""
import numpy as np

FLUID, OBST, EMPTY, STICK = 1.0, 2.0, 4.0, 128.0


def _sh(A, a, d, fill=0):
    """out[x] = A[x + d e_a] where that cell is inside the domain, `fill` elsewhere (A: (B, D, H, W), axis a in dimension 3 - a)"""
    out = np.full_like(A, fill)
    ax = A.ndim - 1 - a
    src, dst = [slice(None)] * A.ndim, [slice(None)] * A.ndim
    if d > 0:
        dst[ax], src[ax] = slice(0, -d), slice(d, None)
    else:
        dst[ax], src[ax] = slice(-d, None), slice(0, d)
    out[tuple(dst)] = A[tuple(src)]
    return out


def _shc(A, a, d):
    """out[x] = A[clamp(x + d e_a)]: the reference's i_l = max(i - 1, 0), i_r = min(i + 1, n - 1)"""
    ax = A.ndim - 1 - a
    n = A.shape[ax]
    return np.take(A, np.clip(np.arange(n) + d, 0, n - 1), axis=ax)


def _setup(U, flags, nd, dtype):
    U, flags = np.asarray(U), np.asarray(flags)
    assert nd in (2, 3) and U.shape[1] == nd and (nd == 3 or U.shape[2] == 1) and flags.shape[1] == 1
    f = flags[:, 0].astype(np.float32)
    idx = np.indices(f.shape)[::-1][:nd]                       # idx[a]: the index along axis a (x, y, z)
    return [U[:, c].astype(dtype) for c in range(nd)], f, idx


def add_viscosity(dt, U, flags, viscosity, nd, ref_quirks=False, dtype=np.float32):
    """One explicit Euler step of the viscous term on the MAC faces: for an interior cell x and component c
        m   = 1 if flags(x) == Fluid and flags(x - e_c) == Fluid else 0
        s   = u(x+e_0) + u(x+e_1) [+ u(x+e_2)]; s = s + u(x-e_0); s = s + u(x-e_1) [; s = s + u(x-e_2)]; s = s - (2 nd) u(x)
        out = m (u(x) + coef s),   coef = float32(double(dt) * double(viscosity))
    and the cells of the one-cell border keep their value.  The update is stable for coef <= 1 / (2 nd) (1/4 in 2D, 1/6 in 3D); nothing
    checks that, because the reference checks nothing.
    ref_quirks (nd = 2): the second low neighbour is the reference's (i-1, j-1) instead of (i, j-1) (viscosity.py:57-70)."""
    assert not ref_quirks or nd == 2, "ref_quirks has nothing to reproduce in 3D"
    u, f, idx = _setup(U, flags, nd, dtype)
    coef = dtype(np.float32(float(dt) * float(viscosity)))
    inner = np.ones(f.shape, bool)
    for a in range(nd):
        inner &= (idx[a] >= 1) & (idx[a] <= f.shape[f.ndim - 1 - a] - 2)
    fluid = f == FLUID
    out = []
    with np.errstate(all="ignore"):
        for c in range(nd):
            q = u[c]
            m = (fluid & _sh(fluid, c, -1, False)).astype(dtype)
            s = _sh(q, 0, 1) + _sh(q, 1, 1)
            if nd == 3:
                s = s + _sh(q, 2, 1)
            for a in range(nd):
                lo = _sh(q, a, -1)
                if ref_quirks and a == 1:
                    lo = _sh(_sh(q, 0, -1), 1, -1)
                s = s + lo
            s = s - dtype(2 * nd) * q
            out.append(np.where(inner, m * (q + coef * s), q))
    return np.stack(out, 1)


def _slip(u, f, S, idx, nd, dtype):
    """the slip value s_c(x): 0 on an obstacle cell; else 0 where the cell is Fluid or Stick, x_c > 0 and its low neighbour along c is
    an obstacle; else the input"""
    obst, fluid = f == OBST, f == FLUID
    zero = dtype(0)
    return [np.where(obst, zero, np.where((fluid | S) & (idx[c] > 0) & (_sh(f, c, -1) == OBST), zero, u[c])) for c in range(nd)]


def set_wall_bcs_stick(U, flags, flags_stick, nd, ref_quirks=False, dtype=np.float32):
    """No-slip walls.  Three phases, all reading the INPUT field:
    slip value s_c(x) (see _slip): what setWallBcs would leave on the faces of an obstacle;
    ghost value, at cells with flags_stick(x) == Stick, for every component c: walk the transverse axes a != c in ascending order,
        low neighbour before high neighbour; every neighbour y inside the domain with flags(y) == Fluid contributes s_c(y).  With
        n >= 1 contributions t = -s_c(y_1), t = t - s_c(y_k) for the rest, and the value is t / float(n) (one IEEE division; exact for
        n = 1, 2, 4).  With n = 0 the slip value stays.
        Default semantics: the ghost value is written only where the face of c is not a fluid/obstacle wall face, i.e. not when
        x_c > 0 and flags(x - e_c) == Fluid: there the slip value stays, which is 0 on an obstacle cell.
    other cells keep their slip value.
    ref_quirks (nd = 2), set_wall_bcs_stick.py:57-157 as the 2D kernel has it: the neighbour's flag is read at the clamped index while
    a neighbour outside contributes 0; the "both" test of the x component reads the lower neighbour twice (:131), so its mean is taken
    whenever the lower neighbour is fluid, with whatever the upper one's slip value is; 0.5 * replaces / 2; the corner sums of
    :138-156 zero a component; there is no wall-face rule."""
    assert not ref_quirks or nd == 2, "ref_quirks has nothing to reproduce in 3D"
    u, f, idx = _setup(U, flags, nd, dtype)
    S = np.asarray(flags_stick)[:, 0].astype(np.float32) == STICK
    fluid, obst = f == FLUID, f == OBST
    slip = _slip(u, f, S, idx, nd, dtype)
    if ref_quirks:
        half, zero = dtype(0.5), dtype(0)
        uu, vv = slip
        f_l, f_r = _shc(fluid, 0, -1), _shc(fluid, 0, 1)
        v_l, v_r = _sh(slip[1], 0, -1), _sh(slip[1], 0, 1)
        vv = np.where(S & f_l, -v_l, vv)
        vv = np.where(S & f_r, -v_r, vv)
        vv = np.where(S & f_l & f_r, half * ((-v_l) - v_r), vv)
        f_d, f_u = _shc(fluid, 1, -1), _shc(fluid, 1, 1)
        u_d, u_u = _sh(slip[0], 1, -1), _sh(slip[0], 1, 1)
        uu = np.where(S & f_d, -u_d, uu)
        uu = np.where(S & f_u, -u_u, uu)
        uu = np.where(S & f_d, half * ((-u_d) - u_u), uu)
        cont = fluid | obst | S
        ls, rs = (cont & _shc(S, 0, -1)).astype(int), (cont & _shc(S, 0, 1)).astype(int)
        bs, us = (cont & _shc(S, 1, -1)).astype(int), (cont & _shc(S, 1, 1)).astype(int)
        s2 = 2 * S.astype(int)
        uu = np.where(s2 + 2 * ls + bs + us == 3, zero, uu)
        vv = np.where(s2 + ls + 2 * bs + rs == 3, zero, vv)
        return np.stack([uu, vv], 1)
    out = []
    for c in range(nd):
        t = np.zeros(f.shape, dtype)
        n = np.zeros(f.shape, np.int32)
        for a in range(nd):
            if a == c:
                continue
            for d in (-1, 1):
                there = _sh(fluid, a, d, False)
                v = _sh(slip[c], a, d)
                t = np.where(there, np.where(n == 0, -v, t - v), t)
                n = n + there
        with np.errstate(all="ignore"):
            ghost = t / np.maximum(n, 1).astype(dtype)
        wall_face = (idx[c] > 0) & _sh(fluid, c, -1, False)
        out.append(np.where(S & (n >= 1) & ~wall_face, ghost, slip[c]))
    return np.stack(out, 1)
