"""The CPU oracle's MultiScale net (oracle/cnn_oracle.c) against an independent float64 model of the reference net
(tests/cnn_reference.py), on the benchmark's weights and on weights under which every layer shows in the output; and a guard that
those weights keep doing so.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cnn_reference import multiscale_fp64, net_input, propagating_weights, resample
from util import assert_close_rel

# the GPU suite's tolerance for the exact-fp32 modes (tests/test_parity_gpu.py, tests/test_cnn_fp64_gpu.py)
GPU_RTOL = 1e-5
# the oracle (double accumulation, float32 activations) measures 0.5 .. 1e-7 of |ref|max against the float64 model
ORACLE_RTOL = 1e-6


def _weights(kind, ndim):
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    return make_scalenet_weights(0, ndim=ndim) if kind == "seed0" else propagating_weights(ndim)


@pytest.mark.parametrize("size", [(13, 26), (64, 32), (9, 13), (18, 26), (5, 7), (37, 53), (1, 3)])
def test_resample_is_torch_interpolate(size):
    """resample is F.interpolate(bilinear / trilinear, align_corners=False): the same values where the size ratio makes the
    sample positions exact in float32, and within the float32 rounding of the positions elsewhere."""
    t = torch.from_numpy(np.random.default_rng(1).standard_normal((2, 3, 18, 26)))
    exact = all(np.log2(n_in / n).is_integer() for n_in, n in zip(t.shape[2:], size))
    want = F.interpolate(t, size=list(size), mode="bilinear", align_corners=False)
    d = (resample(t, size) - want).abs().max().item()
    assert d <= (1e-14 if exact else 2e-5), (size, d)
    t3 = torch.from_numpy(np.random.default_rng(2).standard_normal((1, 2, 9, 14, 22)))
    size3 = (4, 7, 11) if exact else (2, 3, 5)
    want3 = F.interpolate(t3, size=list(size3), mode="trilinear", align_corners=False)
    d3 = (resample(t3, size3) - want3).abs().max().item()
    assert d3 <= (1e-14 if exact else 2e-5), (size3, d3)


# (B, D, H, W, ramp): D == 1 is the 2D net.  Sizes that are not multiples of 4 in every axis; the minimum of 4 planes and the
# 5..7 planes whose quarter-resolution tower has a single plane; an input whose amplitude grows 10^4-fold across x.
SHAPES = [(1, 1, 37, 53, None), (2, 1, 30, 41, None), (1, 1, 37, 53, 1e4), (1, 1, 4, 6, None),
          (1, 9, 14, 22, None), (2, 4, 13, 18, None), (1, 7, 13, 18, None), (1, 9, 14, 22, 1e4)]


@pytest.mark.parametrize("weights", ["seed0", "propagating"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s[:4]) + ("_ramp" if s[4] else ""))
def test_oracle_multiscale_vs_fp64(oracle, shape, weights):
    B, D, H, W, ramp = shape
    nd = 3 if D > 1 else 2
    w = _weights(weights, nd)
    x = net_input(B, D, H, W, seed=7, ramp=ramp)
    want = multiscale_fp64(w, x, nd)
    got = oracle.multiscale_forward(oracle.pack_weights(w, nd), x, nd == 3)
    assert_close_rel(got, want, ORACLE_RTOL, f"oracle MultiScaleNet {shape} ({weights} weights)")


@pytest.fixture(scope="module")
def slab_case():
    """A 104-plane 3D domain, its float64 forward on the propagating weights, and the windows of z-slab ranks that own 8 planes."""
    w = propagating_weights(3)
    x = net_input(1, 104, 13, 18, seed=21)
    return w, x, multiscale_fp64(w, x, 3)


@pytest.mark.parametrize("case", ["bottom", "middle", "top"])
def test_oracle_crop_vs_fp64(oracle, slab_case, case):
    """ora_multiscale_forward_crop on a z-slab rank's nested windows (quarter-resolution tower on owned +- NET_MARGIN planes,
    half- / full-resolution towers on owned +- NET_MARGIN_HALF / _FULL; a window that ends at a domain face is not trimmed
    there), against the float64 forward over the whole domain on the owned planes."""
    from fluidnet_cxx_amd.slab import SlabSimulator as S
    G, MF, MH = S.NET_MARGIN, S.NET_MARGIN_FULL, S.NET_MARGIN_HALF
    w, x, full = slab_case
    Dg = x.shape[2]
    own = dict(bottom=(0, 8), middle=(48, 56), top=(96, 104))[case]
    e0, e1 = max(own[0] - G, 0), min(own[1] + G, Dg)
    cut_lo, cut_hi = own[0] - e0 == G, e1 - own[1] == G
    trim = [G - MF if cut_lo else 0, G - MF if cut_hi else 0, G - MH if cut_lo else 0, G - MH if cut_hi else 0]
    got = oracle.multiscale_forward_crop(oracle.pack_weights(w, 3), np.ascontiguousarray(x[:, :, e0:e1]), trim)
    lo = e0 + trim[0]
    assert_close_rel(got[:, :, own[0] - lo:own[1] - lo], full[:, :, own[0]:own[1]], ORACLE_RTOL,
                     f"oracle nested crops ({case}): owned planes vs the float64 whole domain")


@pytest.mark.parametrize("ndim,shape", [(2, (1, 1, 64, 96)), (3, (1, 12, 20, 24))])
def test_propagating_weights_expose_every_tower(ndim, shape):
    """In the float64 model: zeroing ONE tap of the first layer of any tower (a tap of output channel 0 / input channel 0, the
    corner or the centre, whichever matters more) moves the output by at least 100x the GPU tolerance.  The first layer's
    signal passes through every later layer of its tower, so this fails if the test weights let any tower fade out again --
    as make_scalenet_weights(0) does (the quarter-resolution tower: ~1e-7 of |ref|max)."""
    from fluidnet_cxx_amd.weights import scalenet_layers
    w = propagating_weights(ndim)
    x = net_input(*shape, seed=3)
    ref = multiscale_fp64(w, x, ndim)
    scale = np.abs(ref).max()
    for tower in ("convN_4", "convN_2", "convN_1"):
        L = next(L for L in scalenet_layers(2, ndim) if L["tower"] == tower)
        moved = []
        for tap in (0, L["k"] // 2):
            w2 = dict(w)
            a = w2[L["name"] + ".weight"].copy()
            a[(0, 0) + (tap,) * ndim] = 0.0
            w2[L["name"] + ".weight"] = a
            moved.append(np.abs(multiscale_fp64(w2, x, ndim) - ref).max() / scale)
        assert max(moved) >= 100 * GPU_RTOL, f"{ndim}D {tower}: one dropped tap moves the output by {max(moved):.2e} of |ref|max"
