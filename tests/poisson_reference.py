"""Float64 model of the pressure system the Jacobi solve converges to -- the operator of fnx_pcg / fnx_poisson_apply
(include/fluidnet_hip.h).  On an active cell (neither border nor obstacle):
    (denom - n_obs) p_i - sum_{active nbr j} p_j = div_i
denom 4 (2D) / 6 (3D); obstacle neighbours are Neumann (the Jacobi substitutes p_i), except the z ones in 3D quirks mode
(they contribute 0); a non-obstacle border neighbour contributes 0 (Dirichlet).  Other cells: p = 0."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

OBST = 2.0


def _border(shape, is3d):
    D, H, W = shape
    k, j, i = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    b = (i == 0) | (i == W - 1) | (j == 0) | (j == H - 1)
    if is3d:
        b |= (k == 0) | (k == D - 1)
    return b


def matrix(flags, is3d, quirks=False):
    """A of one sample (flags (D,H,W)) over all D*H*W cells as scipy CSR (float64), and the flat mask of active cells.  Rows
    and columns of inactive cells are zero."""
    f = np.asarray(flags)
    D, H, W = f.shape
    obst = f == OBST
    act = ~obst & ~_border(f.shape, is3d)
    idx = np.arange(D * H * W).reshape(D, H, W)
    diag = np.where(act, 6.0 if is3d else 4.0, 0.0)
    ks, js, is_ = np.nonzero(act)
    rows, cols, vals = [], [], []
    offs = [(0, 0, -1, False), (0, 0, 1, False), (0, -1, 0, False), (0, 1, 0, False)]
    if is3d:
        offs += [(-1, 0, 0, True), (1, 0, 0, True)]
    for dk, dj, di, zdir in offs:
        nk, nj, ni = ks + dk, js + dj, is_ + di
        sub = obst[nk, nj, ni] & (not (zdir and quirks))
        diag[ks[sub], js[sub], is_[sub]] -= 1.0
        c = act[nk, nj, ni]
        rows.append(idx[ks[c], js[c], is_[c]]); cols.append(idx[nk[c], nj[c], ni[c]]); vals.append(-np.ones(int(c.sum())))
    rows.append(idx.ravel()); cols.append(idx.ravel()); vals.append(diag.ravel())
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(D * H * W,) * 2)
    return A, act.ravel()


def is_singular(A, act):
    """no active row has a positive row sum (no Dirichlet contact): constants on the active cells are null vectors"""
    rs = np.asarray(A.sum(axis=1)).ravel()
    return bool(act.any()) and not bool((rs[act] > 0.5).any())


def apply(flags, p, is3d, quirks=False):
    """A p for (B,1,D,H,W) arrays, float64"""
    out = np.zeros(p.shape, np.float64)
    for b in range(p.shape[0]):
        A, _ = matrix(flags[b, 0], is3d, quirks)
        out[b, 0] = (A @ np.asarray(p[b, 0], np.float64).ravel()).reshape(p.shape[2:])
    return out


def project(flags, div, is3d, quirks=False):
    """the right-hand side the solve works with: div on the active cells, minus its active mean on singular samples"""
    out = np.zeros(div.shape, np.float64)
    for b in range(div.shape[0]):
        A, act = matrix(flags[b, 0], is3d, quirks)
        r = np.where(act, np.asarray(div[b, 0], np.float64).ravel(), 0.0)
        if is_singular(A, act):
            r[act] -= r[act].mean()
        out[b, 0] = r.reshape(div.shape[2:])
    return out


def solve(flags, div, is3d, quirks=False):
    """p* per sample (float64): the exact solution on one connected fluid region; singular samples with the projected div and
    active-cell mean zero (spsolve with one pinned cell, then the mean shifted away)"""
    out = np.zeros(div.shape, np.float64)
    rhs_all = project(flags, div, is3d, quirks)
    for b in range(div.shape[0]):
        A, act = matrix(flags[b, 0], is3d, quirks)
        ia = np.nonzero(act)[0]
        Aa = A[ia][:, ia].tocsc()
        rhs = rhs_all[b, 0].ravel()[ia]
        x = np.zeros(ia.size)
        if is_singular(A, act):
            x[1:] = spla.spsolve(Aa[1:, 1:], rhs[1:])
            x -= x.mean()
        else:
            x = spla.spsolve(Aa, rhs)
        o = np.zeros(A.shape[0])
        o[ia] = x
        out[b, 0] = o.reshape(div.shape[2:])
    return out


def vcycle(flags, r, is3d, quirks=False, omega=2.0 / 3.0, corr=1.8, coarsest_sweeps=16):
    """z = M^-1 r of one sample (flags, r: (D,H,W)), float64: the preconditioner fnx_pcg_precondition applies -- 2:1 aggregation in
    every axis (one-cell remainders) down to every axis <= 4, Galerkin P^T A P, damped Jacobi 2 + 2 on the degrees of freedom with a
    positive diagonal, coarse correction x corr, the coarsest level by `coarsest_sweeps` sweeps from zero"""
    A, dof = matrix(flags, is3d, quirks)
    shape = np.asarray(flags).shape
    levels = [(A.tocsr(), dof)]
    Ps = []
    while shape[2] > 4 or shape[1] > 4 or (is3d and shape[0] > 4):
        D, H, W = shape
        cs = ((D + 1) // 2 if is3d else D, (H + 1) // 2, (W + 1) // 2)
        k, j, i = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
        parent = (((k // 2 if is3d else k) * cs[1] + j // 2) * cs[2] + i // 2).ravel()
        f = np.nonzero(levels[-1][1])[0]
        P = sp.csr_matrix((np.ones(f.size), (f, parent[f])), shape=(D * H * W, cs[0] * cs[1] * cs[2]))
        Ac = (P.T @ levels[-1][0] @ P).tocsr()
        levels.append((Ac, np.asarray(P.sum(axis=0)).ravel() > 0))
        Ps.append(P)
        shape = cs

    def smooth(A, dof, b, x):
        d = A.diagonal()
        up = dof & (d > 0)
        y = np.where(dof, x, 0.0)
        y[up] = y[up] + omega * (b - A @ x)[up] / d[up]
        return y

    def cycle(l, b):
        A, dof = levels[l]
        x = np.zeros(A.shape[0])
        if l == len(levels) - 1:
            for _ in range(coarsest_sweeps):
                x = smooth(A, dof, b, x)
            return x
        x = smooth(A, dof, b, smooth(A, dof, b, x))
        xc = cycle(l + 1, Ps[l].T @ np.where(dof, b - A @ x, 0.0))
        x = x + corr * (Ps[l] @ xc)
        return smooth(A, dof, b, smooth(A, dof, b, x))

    return cycle(0, np.where(dof, np.asarray(r, np.float64).ravel(), 0.0)).reshape(np.asarray(flags).shape)
