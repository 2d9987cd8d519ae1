"""The float64 model of the MultiScale pressure net (tests/cnn_reference.py) made differentiable: torch's autograd over the same
construction (resample at float32 sample positions, F.conv2d, ReLU), 2D, as the yardstick of the native backward pass.

ReLU masks.  A float32 implementation and the float64 model disagree on the sign of a handful of pre-activations that lie within
rounding of zero, and every such flip moves a weight gradient by one pixel's term (2e-3 of a tensor's max, measured) -- far more
than the rounding of everything else (1e-6).  So the model can take its ReLU decisions from outside: masks[l] (bool, the shape of
layer l's output) replaces relu(z) by z * mask, i.e. the model differentiates the piecewise-linear branch the implementation under
test took.  masks_from_tape reads them off the native tape (saved output > 0, torch's rule).

Layers are numbered as in scalenet_layers(): 0..3 quarter resolution, 4..9 half, 10..15 full, 16 the final 1x1."""
import numpy as np

from cnn_reference import TOWERS, resample
from fluidnet_cxx_amd.weights import scalenet_layers

LAYERS = scalenet_layers(2, 2)
PARAM_NAMES = [L["name"] + sfx for L in LAYERS for sfx in (".weight", ".bias")]
RELU_LAYERS = [l for l, L in enumerate(LAYERS) if L["relu"]]


def _resample(t, size):
    r = resample(t.double(), size)                     # the interpolation matrices are float64; a float32 model rounds the result
    return r.to(t.dtype)


def forward(params, xt, masks=None, keep=None):
    """params: name -> torch tensor (float64, or float32 for the float32 model); xt (B,2,H,W) of the same dtype.  Returns p (B,1,H,W).
    masks: {layer index: bool array} imposed instead of the ReLU decisions (every ReLU layer or none).
    keep: a dict that receives {layer index: output after ReLU} and {"xq" / "in2" / "in1": tower input}."""
    import torch
    import torch.nn.functional as F
    size = list(xt.shape[2:])
    quarter = [int(i * 0.25) for i in size]                # the reference's size rule (multi_scale_net.py:119-120)
    half = [int(i * 0.5) for i in size]
    index = {L["name"]: l for l, L in enumerate(LAYERS)}

    def tower(t, name):
        for L in LAYERS:
            if L["tower"] != name:
                continue
            l = index[L["name"]]
            t = F.conv2d(t, params[L["name"] + ".weight"], params[L["name"] + ".bias"], padding=L["k"] // 2)
            if L["relu"]:
                t = F.relu(t) if masks is None else t * torch.as_tensor(masks[l]).to(t.dtype)
            if keep is not None:
                keep[l] = t
        return t

    def first(name, t):
        if keep is not None:
            keep[name] = t
        return t

    c4 = tower(first("xq", _resample(xt, quarter)), TOWERS[0])
    c2 = tower(first("in2", torch.cat((_resample(xt, half), _resample(c4, half)), 1)), TOWERS[1])
    c1 = tower(first("in1", torch.cat((_resample(xt, size), _resample(c2, size)), 1)), TOWERS[2])
    return tower(c1, "final")


def as_params(weights, dtype=None, requires_grad=True):
    import torch
    dtype = dtype or torch.float64
    return {k: torch.from_numpy(np.asarray(weights[k], np.float64)).to(dtype).requires_grad_(requires_grad) for k in PARAM_NAMES}


def gradients(weights, x, grad_p, masks=None, dtype=None):
    """Gradient of sum(grad_p * p) with respect to the 34 parameter tensors.  x (B,2,H,W), grad_p (B,1,H,W): arrays.
    Returns (grads: name -> float64 array, p: float64 array, own: {l: bool array}, the ReLU decisions this run took -- the imposed
    ones if masks were given)."""
    import torch
    dtype = dtype or torch.float64
    params = as_params(weights, dtype)
    keep = {}
    xt = torch.from_numpy(np.ascontiguousarray(x, np.float64)).to(dtype)
    p = forward(params, xt, masks, keep)
    loss = (p * torch.from_numpy(np.ascontiguousarray(grad_p, np.float64)).to(dtype)).sum()
    loss.backward()
    grads = {k: params[k].grad.detach().double().numpy() for k in PARAM_NAMES}
    own = {l: (keep[l].detach() > 0).numpy() for l in RELU_LAYERS} if masks is None else dict(masks)
    return grads, p.detach().double().numpy(), own


GPU_SHAPES = [(2, 255, 508), (3, 199, 215), (2, 37, 53)]          # (B, H, W) of tests/test_cnn_train_gpu.py (from test_cnn_fp64_gpu.py)


def case_inputs(shape):
    """The inputs of the gradient tests at `shape`: x (B,2,H,W) float32 and the fixed random w_p (B,1,H,W) of the loss sum(w_p p)"""
    from cnn_reference import net_input
    B, H, W = shape
    x = net_input(B, 1, H, W, seed=B + 1 + H + W)[:, :, 0].copy()
    wp = np.random.default_rng(7).standard_normal((B, 1, H, W)).astype(np.float32)
    return x, wp


def tape_views(tape, layout, B):
    """tape: flat float32 array; layout: ext.multiscale_tape_layout(B, H, W) -> {name: (B,C,H,W) view}"""
    return {name: tape[off:off + B * C * H * W].reshape(B, C, H, W) for name, off, C, H, W in layout}


def masks_from_tape(tape, layout, B):
    v = tape_views(tape, layout, B)
    return {l: v[f"y{l}"] > 0 for l in RELU_LAYERS}


def worst_rel(got, want, skip=()):
    """max over the parameter tensors (but `skip`) of max|got - want| / max|want|, and the per-tensor figures"""
    per = {k: float(np.abs(np.asarray(got[k], np.float64) - want[k]).max() / np.abs(want[k]).max()) for k in PARAM_NAMES if k not in skip}
    return max(per.values()), per


def e32(weights, x, grad_p, skip=()):
    """The rounding a float32 backward pass has on these inputs: torch float32 on the CPU against the float64 model that takes the
    float32 run's own ReLU decisions; worst parameter tensor (but `skip`), max|g32 - g64| / max|g64|."""
    import torch
    g32, _, m32 = gradients(weights, x, grad_p, dtype=torch.float32)
    g64, _, _ = gradients(weights, x, grad_p, masks=m32)
    return worst_rel(g32, g64, skip)[0]


def e32_per_tensor(weights, x, grad_p, skip=()):
    """e32 and the same figure for every parameter tensor on its own: (worst, {name: max|g32 - g64| / max|g64|})"""
    import torch
    g32, _, m32 = gradients(weights, x, grad_p, dtype=torch.float32)
    g64, _, _ = gradients(weights, x, grad_p, masks=m32)
    return worst_rel(g32, g64, skip)


def split_blob(blob):
    """The gradient blob (the layout of blob_from_state_dict) -> name -> array of the parameter's shape"""
    out, off = {}, 0
    for L in LAYERS:
        shp = (L["cout"], L["cin"], L["k"], L["k"])
        n = int(np.prod(shp))
        out[L["name"] + ".weight"] = blob[off:off + n].reshape(shp); off += n
        out[L["name"] + ".bias"] = blob[off:off + L["cout"]]; off += L["cout"]
    assert off == blob.size, (off, blob.size)
    return out
