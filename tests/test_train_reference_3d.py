"""tests/train_reference.py (the float64 yardstick of the training loss and of the chain around the net) on 3D fields.  On a state with
obstacle boxes its torch statements of the divergence and its adjoint are the oracle's, in float32 bit for bit; on a small grid with
every kind of face its velocity update and wall BCs are those of tests/fluid_model_nd.py, the float64 model of the 3D default semantics."""
import numpy as np
import torch

import fluid_model_nd as M
import train_reference as T3
from util import assert_bitexact, random_state

B, D, H, W = 2, 6, 12, 13


def T(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _transpose_and_autograd(U, g, flags):
    """the adjoint is the transpose: <J u, g> = <u, J^T g> in float64, and what autograd makes of the forward statement"""
    u64, g64, f64 = T(U, torch.float64), T(g, torch.float64), T(flags, torch.float64)
    lhs = float((T3.divergence(u64, f64) * g64).sum())
    rhs = float((u64 * T3.divergence_adjoint(g64, f64)).sum())
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
    u = u64.clone().requires_grad_(True)
    (T3.divergence(u, f64) * g64).sum().backward()
    assert torch.equal(u.grad, T3.divergence_adjoint(g64, f64))


def test_divergence_and_adjoint_are_the_oracles(oracle):
    s = random_state(B, D, H, W, 0.5, seed=21, boxes=True)
    flags, U, g = s["flags"], s["U"], s["p"]
    shell = 2 * (D * H + D * (W - 2) + (H - 2) * (W - 2))
    assert (flags == 2).sum() > B * shell                              # obstacles inside the shell
    # (+ 0: a masked product leaves -0 where the oracle writes +0)
    assert_bitexact(T3.divergence(T(U), T(flags)).numpy() + np.float32(0), oracle.velocity_divergence(U, flags) + np.float32(0), "divergence")
    assert_bitexact(T3.divergence_adjoint(T(g), T(flags)).numpy() + np.float32(0),
                    oracle.velocity_divergence_backward(g, flags) + np.float32(0), "adjoint")
    _transpose_and_autograd(U, g, flags)


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


# ---- the chain's other two operators on a grid with every kind of face -----------------------------------------------------------------
SMALL = (2, 5, 6, 7)                                                   # (B, D, H, W)
BOX = (slice(2, 3), slice(2, 4), slice(2, 5))                          # 1 x 2 x 3 obstacle cells inside the shell


def _small_case():
    """the border shell and one interior box: obstacle-fluid faces along every axis (the box's sides), obstacle-obstacle faces (inside the
    box and the shell) and plane 0; float64 values, so that each model rounds an element once"""
    b, d, h, w = SMALL
    flags = np.full((b, 1, d, h, w), M.FLUID)
    flags[:, :, [0, -1]] = flags[:, :, :, [0, -1]] = flags[:, :, :, :, [0, -1]] = M.OBST
    flags[(slice(None), slice(None)) + BOX] = M.OBST
    rng = np.random.default_rng(31)
    return flags, rng.standard_normal((b, 3, d, h, w)), rng.standard_normal((b, 1, d, h, w))


def test_the_small_grid_has_every_kind_of_face():
    flags = _small_case()[0]
    obst = flags[0, 0] == M.OBST
    inner = np.zeros_like(obst)
    inner[1:-1, 1:-1, 1:-1] = True
    for ax in range(3):
        lo = np.roll(obst, 1, axis=ax)                                  # the -1 neighbour (interior cells only: no wrap)
        assert (inner & obst & ~lo).any() and (inner & ~obst & lo & np.roll(inner, 1, axis=ax)).any(), ax      # fluid | obstacle, both ways
        assert (inner & obst & lo & np.roll(inner, 1, axis=ax)).any() == (BOX[ax].stop - BOX[ax].start > 1), ax    # obstacle | obstacle inside
    assert obst[0].all() and (inner & ~obst).sum() == 3 * 4 * 5 - 6


def test_velocity_update_and_wall_bcs_are_the_float64_model_of_the_3d_semantics():
    """Both sides take the same float64 operands in the same order -- u - (p - p(c - e)), resp. u kept or zeroed -- so every element is
    the same one or two roundings and the comparison is exact (==: a masked product leaves -0 where the model writes +0)."""
    flags, U, p = _small_case()
    f, u, pt = T(flags, torch.float64), T(U, torch.float64), T(p, torch.float64)
    got = T3.velocity_update(pt, u, f).numpy()
    assert np.array_equal(got, M.velocity_update(p, U, flags))
    assert not np.array_equal(got, U) and np.array_equal(got[:, :, 0], U[:, :, 0])           # the interior moves, the border stays
    got = T3.set_wall_bcs(u, f).numpy()
    assert np.array_equal(got, M.set_wall_bcs(U, flags))
    assert np.array_equal(got, U * T3.wall_mask(f).numpy())
    # the exception the model carries: z has no rule on plane 0, where x and y clamp the neighbour to the cell itself (an obstacle there)
    assert np.array_equal(got[:, 2, 0], U[:, 2, 0]) and np.all(U[:, 2, 0] != 0)
    assert not got[:, 0, :, :, 0].any() and not got[:, 1, :, 0, :].any()
    assert not got[:, 2, 1:][:, flags[0, 0, 1:] == M.OBST].any()                              # every other obstacle cell loses its w
    # a composition as the chain applies it
    assert np.array_equal(T3.set_wall_bcs(T3.velocity_update(pt, u, f), f).numpy(), M.set_wall_bcs(M.velocity_update(p, U, flags), flags))


def test_adjoint_is_the_transpose_on_the_small_grid():
    flags, U, g = _small_case()
    _transpose_and_autograd(U, g, flags)
