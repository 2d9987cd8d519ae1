"""tests/train_reference_3d.py (the float64 yardstick of the 3D training loss) pinned to the oracle's operators on a 3D state with
obstacle boxes: its torch statements of the divergence and its adjoint are the oracle's, in float32 bit for bit."""
import numpy as np
import torch

import train_reference_3d as T3
from util import assert_bitexact, random_state

B, D, H, W = 2, 6, 12, 13


def T(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def test_divergence_and_adjoint_are_the_oracles(oracle):
    s = random_state(B, D, H, W, 0.5, seed=21, boxes=True)
    flags, U, g = s["flags"], s["U"], s["p"]
    shell = 2 * (D * H + D * (W - 2) + (H - 2) * (W - 2))
    assert (flags == 2).sum() > B * shell                              # obstacles inside the shell
    # (+ 0: a masked product leaves -0 where the oracle writes +0)
    assert_bitexact(T3.divergence(T(U), T(flags)).numpy() + np.float32(0), oracle.velocity_divergence(U, flags) + np.float32(0), "divergence")
    assert_bitexact(T3.divergence_adjoint(T(g), T(flags)).numpy() + np.float32(0),
                    oracle.velocity_divergence_backward(g, flags) + np.float32(0), "adjoint")
    # the adjoint is the transpose: <J u, g> = <u, J^T g> in float64, and what autograd makes of the forward statement
    u64, g64, f64 = T(U, torch.float64), T(g, torch.float64), T(flags, torch.float64)
    lhs = float((T3.divergence(u64, f64) * g64).sum())
    rhs = float((u64 * T3.divergence_adjoint(g64, f64)).sum())
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
    u = u64.clone().requires_grad_(True)
    (T3.divergence(u, f64) * g64).sum().backward()
    assert torch.equal(u.grad, T3.divergence_adjoint(g64, f64))


def test_loss_terms_are_the_four_means():
    s = random_state(B, D, H, W, 0.5, seed=22, boxes=True)
    p, U, f = T(s["p"], torch.float64), T(s["U"], torch.float64), T(s["flags"], torch.float64)
    t = torch.zeros_like(p)
    total, terms = T3.loss_terms(p, U, f, t, (1.0, 2.0, 3.0, 4.0))
    d = T3.divergence(U, f)
    want = [float((p * p).sum()) / p.numel(), float((d * d).sum()) / p.numel(), float(p.abs().sum()) / p.numel(), float(d.abs().sum()) / p.numel()]
    assert np.allclose([float(v) for v in terms], want, rtol=1e-13)
    assert abs(float(total) - sum(l * w for l, w in zip((1.0, 2.0, 3.0, 4.0), want))) <= 1e-12 * float(total)
    assert float(T3.loss_terms(p, U, f, None, (1.0, 1.0, 1.0, 1.0))[1][0]) == 0.0
