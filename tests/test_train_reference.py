"""tests/train_reference.py (the float64 yardstick of a training run) pinned to the oracle's operators: its torch statements of the
divergence and its adjoint, the velocity update, the wall BCs and FluidNet.forward around a given net are the oracle's, in float32 bit
for bit where the arithmetic is one rounding per element and within rounding where it is not."""
import numpy as np
import torch

import cnn_grad_reference as G
import scene_reference as SR
import train_reference as TR
from cnn_reference import propagating_weights
from util import assert_bitexact, assert_close_rel

B, H, W = 3, 37, 53


def _case():
    flags = SR.obstacles(5, [2, 9, 31], (H, W), **dict(SR.DEFAULTS[2], n_min=2, n_max=4))
    rng = np.random.default_rng(3)
    U = rng.standard_normal((B, 2, 1, H, W)).astype(np.float32)
    p = rng.standard_normal((B, 1, 1, H, W)).astype(np.float32)
    return flags, U, p


def T(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def test_operators_are_the_oracles(oracle):
    flags, U, p = _case()
    assert (flags == 2).sum() > B * (2 * H + 2 * W - 4)                 # obstacles inside the ring
    # (+ 0: a masked product leaves -0 where the oracle writes +0)
    assert_bitexact(TR.divergence(T(U), T(flags)).numpy() + np.float32(0), oracle.velocity_divergence(U, flags) + np.float32(0), "divergence")
    assert_bitexact(TR.divergence_adjoint(T(p), T(flags)).numpy() + np.float32(0), oracle.velocity_divergence_backward(p, flags) + np.float32(0), "adjoint")
    assert_bitexact(TR.velocity_update(T(p), T(U), T(flags)).numpy() + np.float32(0), oracle.velocity_update(p, U, flags) + np.float32(0),
                    "velocity update")
    assert_bitexact(TR.set_wall_bcs(T(U), T(flags)).numpy() + np.float32(0), oracle.set_wall_bcs(U, flags) + np.float32(0), "wall BCs")
    # the adjoint is the transpose: <J u, g> = <u, J^T g> in float64
    u64, g64, f64 = T(U, torch.float64), T(p, torch.float64), T(flags, torch.float64)
    lhs = float((TR.divergence(u64, f64) * g64).sum())
    rhs = float((u64 * TR.divergence_adjoint(g64, f64)).sum())
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
    # and what autograd makes of the forward statement
    u = u64.clone().requires_grad_(True)
    (TR.divergence(u, f64) * g64).sum().backward()
    assert torch.equal(u.grad, TR.divergence_adjoint(g64, f64))


def test_fluidnet_forward_is_the_oracles_around_the_same_net(oracle):
    flags, U, p = _case()
    rho = np.zeros_like(p)
    inp = np.concatenate([p, U, flags, rho], 1)
    w = propagating_weights(2)
    params = G.as_params(w, requires_grad=False)

    def net(x):                                                        # x (B,2,1,H,W) float32 -> p (B,1,1,H,W)
        with torch.no_grad():
            return G.forward(params, T(x[:, :, 0], torch.float64)).numpy()[:, :, None]
    want_p, want_U = oracle.fluidnet_forward(None, inp, 1e-5, net=net)
    with torch.no_grad():
        got_p, got_U = TR.fluidnet_forward(params, T(inp, torch.float64))
    assert_close_rel(got_p.numpy(), want_p, 2e-6, "p")
    assert_close_rel(got_U.numpy(), want_U, 2e-6, "U")
    assert float(np.abs(want_U).max()) > 0.1


def test_loss_terms_are_the_means_of_the_reference():
    flags, U, p = _case()
    t = np.random.default_rng(4).standard_normal(p.shape).astype(np.float32)
    lam = (1.0, 1.0, 0.5, 0.5)
    total, terms = TR.loss_terms(T(p, torch.float64), T(U, torch.float64), T(flags, torch.float64), T(t, torch.float64), lam)
    d = TR.divergence(T(U, torch.float64), T(flags, torch.float64))
    mse, l1 = torch.nn.MSELoss(), torch.nn.L1Loss()
    want = [mse(T(p, torch.float64), T(t, torch.float64)), mse(d, torch.zeros_like(d)), l1(T(p, torch.float64), T(t, torch.float64)),
            l1(d, torch.zeros_like(d))]
    for a, b in zip(terms, want):
        assert abs(float(a) - float(b)) <= 1e-14 * abs(float(b))
    assert abs(float(total) - sum(l * float(b) for l, b in zip(lam, want))) <= 1e-13 * float(total)
