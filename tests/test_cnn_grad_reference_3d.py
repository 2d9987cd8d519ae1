"""The 3D gradient yardstick (tests/cnn_grad_reference.py) against what it must agree with, on the CPU: its forward is
multiscale_fp64(ndim=3), its FluidNet-level chain is the oracle's operators around that net, its gradients are the central differences of
its own forward, and the test inputs leave no parameter gradient empty (a kernel that wrote zeros there would otherwise pass)."""
import numpy as np
import pytest
import torch

import cnn_grad_reference as G
from cnn_reference import multiscale_fp64, net_input, propagating_weights

SMALL = (2, 5, 8, 13)          # towers (1, 2, 3) and (2, 4, 6): the finite-difference checks need no more than every index path once


@pytest.fixture(scope="module")
def weights():
    return propagating_weights(3)


def _directions(weights, n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        d = {k: rng.standard_normal(weights[k].shape) for k in G.PARAM_NAMES}
        norm = np.sqrt(sum(float((v ** 2).sum()) for v in d.values()))
        out.append({k: v / norm for k, v in d.items()})
    return out


def _fd_agreement(loss_of, grads, weights, h=1e-4):
    """max over three random unit directions of |<g, d> - (L(w + h d) - L(w - h d)) / 2h| / |<g, d>|"""
    worst = 0.0
    for d in _directions(weights, 3, seed=5):
        plus = {k: np.asarray(weights[k], np.float64) + h * d[k] for k in G.PARAM_NAMES}
        minus = {k: np.asarray(weights[k], np.float64) - h * d[k] for k in G.PARAM_NAMES}
        fd = (loss_of(plus) - loss_of(minus)) / (2 * h)
        an = sum(float((grads[k] * d[k]).sum()) for k in G.PARAM_NAMES)
        worst = max(worst, abs(an - fd) / abs(an))
    return worst


def test_forward_is_the_float64_model(weights):
    for shape in (SMALL, G.S1):
        x = G.case_inputs(shape)[0]
        keep = {}
        with torch.no_grad():
            p = G.forward(G.as_params(weights, requires_grad=False), torch.from_numpy(x.astype(np.float64)), keep=keep).numpy()
        want, (c4, c2, c1) = multiscale_fp64(weights, x, 3, towers=True)
        assert np.array_equal(p, want), shape
        assert np.array_equal(keep[3].numpy(), c4) and np.array_equal(keep[9].numpy(), c2) and np.array_equal(keep[15].numpy(), c1)
        q, h = G.tower_sizes(shape[1:])
        assert list(keep["xq"].shape[2:]) == q and list(keep["in2"].shape[2:]) == h and keep["in2"].shape[1] == 3
    assert G.tower_sizes(G.S1[1:]) == ([1, 2, 9], [3, 5, 18]) and G.tower_sizes(G.S2[1:]) == ([2, 3, 17], [4, 7, 35])


def test_gradients_agree_with_central_differences(weights):
    """Under imposed masks (the base point's own decisions) the loss is a polynomial in the parameters, so central differences at
    h = 1e-4 along a unit direction are exact up to the h^2 term.  Measured agreement: 2.1e-10 (net), 1.3e-9 (FluidNet-level chain, which
    also agrees to 1.4e-7 with the chain rule over the oracle's float32 adjoints); bound 1e-6."""
    x, wp = G.case_inputs(SMALL)
    g, _, masks = G.gradients(weights, x, wp)

    def loss_of(w):
        with torch.no_grad():
            p = G.forward(G.as_params(w, requires_grad=False), torch.from_numpy(x.astype(np.float64)), masks)
        return float((p * torch.from_numpy(wp.astype(np.float64))).sum())
    worst = _fd_agreement(loss_of, g, weights)
    print(f"\nCNN3D_FD net {worst:.3e}")
    assert worst <= 1e-6


def test_fluidnet_chain_agrees_with_central_differences_and_the_oracle(oracle, weights):
    inp, w_p, w_U = G.fluidnet_case(SMALL)
    g, (p, U), masks = G.fluidnet_gradients(weights, inp, w_p, w_U)

    def loss_of(w):
        with torch.no_grad():
            pp, UU = G.fluidnet_forward(G.as_params(w, requires_grad=False), inp, masks=masks)
        return float((pp * torch.from_numpy(w_p.astype(np.float64))).sum() + (UU * torch.from_numpy(w_U.astype(np.float64))).sum())
    worst = _fd_agreement(loss_of, g, weights)
    print(f"\nCNN3D_FD fluidnet {worst:.3e}")
    assert worst <= 1e-6
    # the same chain from the oracle's float32 operators around the float64 net: float32 rounding of the stages apart, the same (p, U)
    po, Uo = oracle.fluidnet_forward(None, inp, 1e-5, net=lambda x: multiscale_fp64(weights, x, 3))
    assert np.abs(p - po).max() <= 1e-5 * np.abs(po).max() and np.abs(U - Uo).max() <= 1e-5 * np.abs(Uo).max()
    assert np.abs(Uo).max() > 0 and np.array_equal(U == 0, Uo == 0)
    # and the chain rule the native backward applies: g_net = s g_p + velocity_update_backward_p(s setWallBcs(g_U))
    B = inp.shape[0]
    s = oracle.scale_std(inp[:, 1:4], 1e-5).reshape(B, 1, 1, 1, 1)
    _, gp_u = oracle.velocity_update_backward(s * oracle.set_wall_bcs(w_U, inp[:, 4:5]), inp[:, 4:5])
    keep = {}
    with torch.no_grad():
        G.fluidnet_forward(G.as_params(weights, requires_grad=False), inp, masks=masks, keep=keep)
    g2, _, _ = G.gradients(weights, keep["in1"][:, 0:2].numpy(), s * w_p + gp_u, masks=masks)
    worst2, _ = G.worst_rel(g2, g)
    print(f"CNN3D_CHAIN autograd chain against the oracle's adjoints {worst2:.3e}")
    assert worst2 <= 1e-5


@pytest.mark.parametrize("shape", G.GPU_SHAPES[3], ids=lambda s: "x".join(map(str, s)))
def test_case_inputs_reach_every_parameter(weights, shape):
    """no parameter tensor's gradient is all zero and no (co, ci) slice of a weight gradient is, but for the taps that only see padding"""
    x, wp = G.case_inputs(shape)
    g, _, _ = G.gradients(weights, x, wp)
    dead = G.structural_zero_taps(shape)
    if shape == G.S1:
        assert sorted(dead) == sorted(L["name"] + ".weight" for L in G.LAYERS[:4])
        for m in dead.values():
            assert m[0].all() and m[2].all() and not m[1].any()
    else:
        assert not dead
    for k in G.PARAM_NAMES:
        assert np.abs(g[k]).max() > 0, k
        if k.endswith(".weight"):
            live = np.abs(g[k]).reshape(g[k].shape[0], g[k].shape[1], -1)
            if k in dead:
                assert np.all(g[k][:, :, dead[k]] == 0), k
                live = live[:, :, ~dead[k].ravel()]
            assert (live.max(axis=2) > 0).all(), f"{k}: a (co, ci) slice of the float64 gradient is all zero"
