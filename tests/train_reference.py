"""The float64 yardstick of the training loss and of a training run, in 2D and 3D: torch statements of the operators around the net --
divergence and its adjoint, velocity update, wall BCs -- for grids whose cells are fluid or obstacle (what the scene generator makes), the
four terms of the training loss (fluid_net_train.py:276-285, fnx_train_loss / fnx_train_loss3d) with their gradients, and torch's autograd
and torch.optim.Adam on the CPU over the model of FluidNet.forward that tests/cnn_grad_reference.py builds from these operators and the
float64 net.  dtype is a parameter: float64 is the yardstick, float32 measures what float32 arithmetic costs on the same inputs.
tests/test_train_reference.py (2D) and tests/test_train_reference_3d.py pin the operators to the oracle's and to tests/fluid_model_nd.py.

Fields are (B,C,D,H,W) torch tensors with D = 1 in 2D; cell (i, j[, k]) = axes (W, H[, D]).  Every operator is stated once for "an axis"
and loops over the axes the field has; the one rule that names an axis is WALLBC_SKIP_AT_0."""
import numpy as np
import torch

import cnn_grad_reference as G

FLUID, OBST = 1.0, 2.0
_AXES = ((0, 4), (1, 3), (2, 2))                  # (velocity channel, tensor axis) of x, y, z
WALLBC_SKIP_AT_0 = (2,)     # setWallBcs at index 0 of an axis: for x and y the -1 neighbour clamps to the cell itself, for z the rule is
#                             skipped on plane 0 (set_wall_bcs.py:54-84; exception 4 of tests/fluid_model_nd.py)


def axes(f):
    """the (velocity channel, tensor axis) pairs of the grid a field lives on: a 2D field has depth 1 and no z"""
    return _AXES[:2 if f.shape[2] == 1 else 3]


def _shift(f, ax):
    """f(cell - e) along tensor axis `ax` with zeros (False) shifted in"""
    out = torch.zeros_like(f)
    n = f.shape[ax]
    out.narrow(ax, 1, n - 1).copy_(f.narrow(ax, 0, n - 1))
    return out


def _cells(f, up=None):
    """the index of the interior cells of f's grid, or of their +1 neighbours along tensor axis `up`"""
    return (Ellipsis,) + tuple(slice(2, None) if ax == up else slice(1, -1) for _, ax in reversed(axes(f)))


def interior(flags):
    a = torch.zeros_like(flags, dtype=torch.bool)
    a[_cells(flags)] = True
    return a


def active(flags):
    """interior and not an obstacle: where velocityDivergence is evaluated"""
    return interior(flags) & (flags != OBST)


def divergence(U, flags):
    """velocity_divergence.py:46-74, divergence_kernel: ((u(c) - u(c + ex)) + v(c)) - v(c + ey), then + (w(c) - w(c + ez)), on the active
    cells, 0 elsewhere"""
    (u, x), (v, y), *rest = [(U[:, a:a + 1], ax) for a, ax in axes(U)]
    c = _cells(U)
    acc = ((u[c] - u[_cells(U, x)]) + v[c]) - v[_cells(U, y)]
    for w, z in rest:
        acc = acc + (w[c] - w[_cells(U, z)])
    d = torch.zeros_like(u)
    d[c] = acc
    return d * active(flags).to(U.dtype)


def divergence_adjoint(g, flags):
    """J^T g of the map above: dL/du_a(q) = A(q) g(q) - A(q - e_a) g(q - e_a)"""
    ag = g * active(flags).to(g.dtype)
    return torch.cat([ag - _shift(ag, ax) for _, ax in axes(g)], 1)


def velocity_update(p, U, flags):
    """velocity_update.py:47-149 without empty cells (in 3D: update_vel.cpp:58-117): on interior cells u_a <- m_ff (u_a - (p - p(c - e_a)))
    with m_ff = the cell and its -e_a neighbour are both fluid, border cells untouched"""
    f = flags == FLUID
    faces = torch.cat([f & _shift(f, ax) for _, ax in axes(U)], 1)
    grad = torch.cat([p - _shift(p, ax) for _, ax in axes(U)], 1)
    return torch.where(interior(flags), faces.to(U.dtype) * (U - grad), U)


def wall_mask(flags):
    """setWallBcs (set_wall_bcs.py:4-86) as a bool mask on U: in fluid and obstacle cells, border included, component a is zeroed where
    the -e_a neighbour is an obstacle, or the cell is an obstacle and that neighbour fluid -- between fluid and obstacle cells a face keeps
    its velocity only between two fluid cells.  The neighbour of a cell at index 0 is the cell itself, but for WALLBC_SKIP_AT_0."""
    cell = (flags == FLUID) | (flags == OBST)
    keep = []
    for a, ax in axes(flags):
        low = flags.narrow(ax, 0, 1)
        fm = torch.cat((low, flags.narrow(ax, 0, flags.shape[ax] - 1)), ax)
        zero = cell & ((fm == OBST) | ((flags == OBST) & (fm == FLUID)))
        if a in WALLBC_SKIP_AT_0:
            zero.narrow(ax, 0, 1).fill_(False)
        keep.append(~zero)
    return torch.cat(keep, 1)


def set_wall_bcs(U, flags):
    return U * wall_mask(flags).to(U.dtype)


fluidnet_forward = G.fluidnet_forward          # the chain around the net is stated once, from the operators above


def div_l2(U, flags):
    return (divergence(U, flags) ** 2).mean()


def loss_terms(out_p, out_U, flags, target_p, lam):
    """fluid_net_train.py:276-285 -> (total, [pL2, divL2, pL1, divL1]) in the tensors' dtype"""
    d = divergence(out_U, flags)
    e = out_p - target_p if target_p is not None else torch.zeros_like(out_p)
    terms = [(e ** 2).mean(), (d ** 2).mean(), e.abs().mean(), d.abs().mean()]
    return sum(l * t for l, t in zip(lam, terms)), terms


def loss_and_gradients(p, U, flags, t, lam, dtype):
    """the loss and its gradients in torch on the CPU in `dtype`: value (5 numbers: the four terms and the total), grad_p, grad_U.  The
    gradient with respect to U is the adjoint of the divergence (pinned to the oracle's by tests/test_train_reference.py and
    tests/test_train_reference_3d.py) applied to dL/d div, as the kernel forms it."""
    cast = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    p, U, flags, t = cast(p), cast(U), cast(flags), cast(t)
    N = p.numel()
    d = divergence(U, flags)
    e = p - t
    total, terms = loss_terms(p, U, flags, t, lam)
    g_div = (2.0 * lam[1] * d + lam[3] * torch.sign(d)) / N
    gU = divergence_adjoint(g_div, flags)
    gp = (2.0 * lam[0] * e + lam[2] * torch.sign(e)) / N
    vals = np.array([float(v) for v in terms] + [float(total)], np.float64)
    return vals, gp.double().numpy(), gU.double().numpy()


def _flags_of(data, dtype):
    return torch.from_numpy(np.ascontiguousarray(G.split_input(data)[1])).to(dtype)


def held_out_loss(params, batches, thr=1e-5):
    """mean divL2 of the net's U over `batches` (arrays (B,5,1,H,W) or (B,6,D,H,W))"""
    dtype = next(iter(params.values())).dtype
    with torch.no_grad():
        v = [float(div_l2(fluidnet_forward(params, d, thr)[1], _flags_of(d, dtype))) for d in batches]
    return sum(v) / len(v)


def adam_run(weights, batches, held_out, lr, dtype):
    """K = len(batches) Adam iterations on divL2 (the reference's lambdas) from `weights`, in `dtype` on the CPU.
    Returns (held-out divL2 before, after, the training losses)."""
    params = G.as_params(weights, dtype)
    opt = torch.optim.Adam(list(params.values()), lr=lr)
    first = held_out_loss(params, held_out)
    losses = []
    for data in batches:
        opt.zero_grad()
        _, U = fluidnet_forward(params, data)
        loss = div_l2(U, _flags_of(data, dtype))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return first, held_out_loss(params, held_out), losses


def kaiming_weights(seed, ndim):
    """the trainer's initial weights (fluidnet_cxx_amd.training.kaiming_init) as name -> float32 array, built without the extension"""
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    w = make_scalenet_weights(0, ndim=ndim)
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    for k in G.PARAM_NAMES:
        if k.endswith(".weight"):
            t = torch.empty(w[k].shape, dtype=torch.float32)
            torch.nn.init.kaiming_uniform_(t, generator=gen)
            w[k] = t.numpy()
    return w


def cpu_batches(oracle, seed, n, B, grid, scene=None, dt=0.1, first_id=0):
    """n data batches (B,5,1,H,W) or (B,6,D,H,W) float32 made on the CPU alone: scenes of the numpy model (tests/scene_reference.py) on
    `grid` = (H, W) or (D, H, W) with the parameters `scene` (the dimension's defaults if None), the oracle's setWallBcs, a converged
    projection (tests/poisson_reference.py: solve), then one advection of the velocity by itself and setWallBcs -- a divergent field in
    the scene's geometry, the kind of input the sampler hands out."""
    import poisson_reference as PR
    import scene_reference as SR
    scene = SR.DEFAULTS[len(grid)] if scene is None else scene
    out = []
    for q in range(n):
        ids = list(range(first_id + q * B, first_id + (q + 1) * B))
        flags = SR.obstacles(seed, ids, grid, **scene)
        U, rho = SR.turbulence(seed, ids, grid, **scene)
        U = oracle.set_wall_bcs(U, flags)
        p = PR.solve(flags, oracle.velocity_divergence(U, flags), len(grid) == 3).astype(np.float32)
        U = oracle.set_wall_bcs(oracle.velocity_update(p, U, flags), flags)
        U = oracle.set_wall_bcs(oracle.advect_vel(dt, U, U, flags, strength=0.6), flags)
        out.append(np.concatenate([p, U, flags, rho], 1).astype(np.float32))
    return out
