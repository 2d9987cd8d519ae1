"""An independent float64 model of the MultiScale pressure net, and test weights under which every layer shows in the output.

multiscale_fp64 is MultiScaleNet.forward (reference pytorch/lib/multi_scale_net.py:118-127) in float64 on the CPU: torch's
own F.conv2d / F.conv3d (the 3D net is the Conv3d / trilinear analogue that SURVEY.md 8c defines) and F.interpolate's
bilinear / trilinear resampling (align_corners=False).  The resampling is written out per axis (resample) so that it can take
its sample positions in float32, as torch does for the float32 net: at a size ratio that is not a power of two (37 -> 18)
F.interpolate in float64 samples up to ~1e-6 cells elsewhere, which moves the net's output by ~1.5e-6 of |ref|max -- more than
the rounding of a float32 forward.  It shares no code with the CPU oracle (oracle/cnn_oracle.c) or the HIP kernels, so either
can be checked against it.

make_scalenet_weights(0) (what the benchmark and the goldens use) follows torch's default init, under which activations shrink
at every layer: about 85 % of |out| is the biases' constant, and a defect in the quarter-resolution tower moves the output by
1e-7..1e-6 of |ref|max, inside every CNN tolerance.  propagating_weights scales the same hashed values so that activations stay
O(1) through all 17 layers (tests/test_cnn_reference.py::test_propagating_weights_expose_every_tower guards that)."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from fluidnet_cxx_amd.weights import make_scalenet_weights, scalenet_layers  # noqa: E402

TOWERS = ("convN_4", "convN_2", "convN_1")


def propagating_weights(ndim=2, seed=0):
    """make_scalenet_weights(seed, ndim=ndim) scaled to He-uniform: weights x sqrt(6) for a layer followed by ReLU, x sqrt(3)
    otherwise (variance 2 / fan_in and 1 / fan_in), biases x 0.1.  float32, the same names and shapes."""
    w = make_scalenet_weights(seed, ndim=ndim)
    for L in scalenet_layers(2, ndim):
        g = np.sqrt(6.0) if L["relu"] else np.sqrt(3.0)
        w[L["name"] + ".weight"] = (w[L["name"] + ".weight"].astype(np.float64) * g).astype(np.float32)
        w[L["name"] + ".bias"] = (w[L["name"] + ".bias"].astype(np.float64) * 0.1).astype(np.float32)
    return w


def _axis_weights(n_in, n_out):
    """(n_out, n_in) float64 matrix of linear interpolation along one axis, align_corners=False, with the sample positions
    computed in float32 as torch computes them for a float32 tensor (and as the kernels and the oracle do):
    src = (n_in / n_out) * (dst + 0.5) - 0.5, clamped at 0; the right neighbour clamped at n_in - 1."""
    f = np.float32
    scale = f(n_in) / f(n_out)
    src = np.maximum(scale * (np.arange(n_out, dtype=f) + f(0.5)) - f(0.5), f(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = (src - i0.astype(f)).astype(np.float64)
    m = np.zeros((n_out, n_in))
    np.add.at(m, (np.arange(n_out), i0), 1.0 - l1)
    np.add.at(m, (np.arange(n_out), i1), l1)
    return m


def resample(t, size):
    """Linear (bilinear / trilinear) resampling of a float64 (B,C,...) tensor to `size`, align_corners=False: the
    interpolation of F.interpolate, one axis after the other, at torch's float32 sample positions (see _axis_weights)."""
    import torch
    for ax, n in enumerate(size):
        n_in = t.shape[2 + ax]
        if n_in == n:
            continue
        m = torch.from_numpy(_axis_weights(n_in, n))
        t = torch.movedim(torch.tensordot(t, m, dims=([2 + ax], [1])), -1, 2 + ax)
    return t.contiguous()


def _tower(t, layers, params, conv):
    import torch.nn.functional as F
    for L in layers:
        t = conv(t, params[L["name"] + ".weight"], params[L["name"] + ".bias"], padding=L["k"] // 2)
        if L["relu"]:
            t = F.relu(t)
    return t


def multiscale_fp64(weights, x, ndim, towers=False):
    """MultiScaleNet.forward in float64 on the CPU.  x: (B,2,H,W) or (B,2,1,H,W) for ndim 2, (B,2,D,H,W) for ndim 3 (any
    float array; taken as float64).  Returns p shaped like x with one channel; towers=True also returns the three tower outputs
    (quarter, half, full resolution; the full one before the final 1x1) as float64 arrays in the net's own rank."""
    import torch
    import torch.nn.functional as F
    x = np.asarray(x)
    squeeze = ndim == 2 and x.ndim == 5
    if squeeze:
        assert x.shape[2] == 1, x.shape
        x = x[:, :, 0]
    assert x.ndim == ndim + 2 and x.shape[1] == 2, (ndim, x.shape)
    conv = F.conv2d if ndim == 2 else F.conv3d
    params = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in weights.items()}
    layers = scalenet_layers(2, ndim)
    by_tower = {t: [L for L in layers if L["tower"] == t] for t in TOWERS}
    final = [L for L in layers if L["tower"] == "final"]

    with torch.no_grad():
        xt = torch.from_numpy(np.ascontiguousarray(x, np.float64))
        size = list(xt.shape[2:])
        quarter = [int(i * 0.25) for i in size]                        # the reference's size rule (multi_scale_net.py:119-120)
        half = [int(i * 0.5) for i in size]
        c4 = _tower(resample(xt, quarter), by_tower["convN_4"], params, conv)
        c2 = _tower(torch.cat((resample(xt, half), resample(c4, half)), 1), by_tower["convN_2"], params, conv)
        c1 = _tower(torch.cat((resample(xt, size), resample(c2, size)), 1), by_tower["convN_1"], params, conv)
        p = _tower(c1, final, params, conv).numpy()
    if squeeze:
        p = p[:, :, None]
    if towers:
        return p, (c4.numpy(), c2.numpy(), c1.numpy())
    return p


def net_input(B, D, H, W, seed, ramp=None):
    """x (B,2,D,H,W) float32: channel 0 ~ N(0,1) (the scaled divergence), channel 1 a 20 % random occupancy;
    ramp=A multiplies channel 0 by a linear ramp across x from 1 to A."""
    rng = np.random.default_rng(seed)
    x = np.empty((B, 2, D, H, W), np.float32)
    x[:, 0] = rng.standard_normal((B, D, H, W), dtype=np.float32)
    x[:, 1] = rng.random((B, D, H, W)) < 0.2
    if ramp is not None:
        x[:, 0] *= np.linspace(1.0, ramp, W, dtype=np.float32)
    return x
