"""The float64 model of the 16-channel bank net and of its Conv3d counterpart (tests/banknet_reference.py: banknet_forward64) made
differentiable: torch's autograd over the same statement of the net, on four or five dimensions, as the yardstick of the native backward
pass (fnx_banknet_train.hip, fnx_banknet3d_train.hip), and the FluidNet-level chain around it through cnn_grad_reference's operators.
The dimension is read off the input: x (B,2,H,W) or (B,2,D,H,W), inp with 5 or 6 channels.

ReLU masks, by the reasoning of cnn_grad_reference.py: a float32 implementation and the float64 model disagree on the sign of
pre-activations within rounding of zero, and each flip moves a weight gradient by a cell's whole term.  So the model can take its ReLU
decisions from outside: masks[name] (bool, the shape of that ReLU's output) replaces relu(z) by z * mask.  masks_from_tape reads them
off the native tape (saved output > 0, torch's rule).  The ReLU outputs carry the tape's names: a; h1, b1 / h2, b2 / h4, b4 (block.0 and
block.2 at full, half and quarter resolution); c2a, c2b (the two applications of conv2); c3.  The tape also holds a2, a4 (the
average-pooled a), t (the sum of the three levels) and x.
"""
import numpy as np

import cnn_grad_reference as G
from fluidnet_cxx_amd.weights import banknet_layers

LAYERS = banknet_layers()
PARAM_NAMES = [L["name"] + sfx for L in LAYERS for sfx in (".weight", ".bias")]
RELU_NAMES = ["a", "h1", "b1", "h2", "b2", "h4", "b4", "c2a", "c2b", "c3"]
TAPE_NAMES = ["a", "h1", "b1", "a2", "h2", "b2", "a4", "h4", "b4", "t", "c2a", "c2b", "c3", "x"]
BANK_TENSORS = [n for n in PARAM_NAMES if n.startswith("convBank.")]
FACTOR, OWN_FLOOR = 8.0, 6e-7        # _check_grads's constants of tests/test_cnn_train_gpu.py


def forward(params, xt, masks=None, keep=None, drop_level=None, drop_conv2=None):
    """params: name -> torch tensor; xt (B,2,H,W) or (B,2,D,H,W) of the same dtype -> p (B,1,...).
    masks: {name: bool array} imposed instead of the ReLU decisions (every ReLU or none).
    keep: a dict that receives every tape entry but x ({name: tensor}).
    drop_level (0: full, 1: half, 2: quarter) / drop_conv2 (0, 1): detach that level's bank / that application of conv2 from the
    parameters' graph -- what the CPU checks use to show how much of a shared tensor's gradient each use carries."""
    import torch
    import torch.nn.functional as F
    convnd, pool = (F.conv2d, F.avg_pool2d) if xt.dim() == 4 else (F.conv3d, F.avg_pool3d)

    def relu(z, name):
        t = F.relu(z) if masks is None else z * torch.as_tensor(masks[name]).to(z.dtype)
        if keep is not None:
            keep[name] = t
        return t

    def conv(t, name, pad, detach=False):
        w, b = params[name + ".weight"], params[name + ".bias"]
        return convnd(t, w.detach() if detach else w, b.detach() if detach else b, padding=pad)

    def bank(t, tag, detach):
        return relu(conv(relu(conv(t, "convBank.block.0", 1, detach), "h" + tag), "convBank.block.2", 1, detach), "b" + tag)

    def up(t, r):                           # nearest, over the trailing axes
        for axis in range(2, t.dim()):
            t = t.repeat_interleave(r, axis)
        return t

    a = relu(conv(xt, "conv1", 1), "a")
    a2, a4 = pool(a, 2), pool(a, 4)
    t = (bank(a, "1", drop_level == 0) + up(bank(a2, "2", drop_level == 1), 2)) + up(bank(a4, "4", drop_level == 2), 4)
    if keep is not None:
        keep.update(a2=a2, a4=a4, t=t)
    t = relu(conv(t, "conv2", 0, drop_conv2 == 0), "c2a")
    t = relu(conv(t, "conv2", 0, drop_conv2 == 1), "c2b")
    t = relu(conv(t, "conv3", 0), "c3")
    return conv(t, "convOut", 0)


def as_params(weights, dtype=None, requires_grad=True):
    import torch
    dtype = dtype or torch.float64
    return {k: torch.from_numpy(np.asarray(weights[k], np.float64)).to(dtype).requires_grad_(requires_grad) for k in PARAM_NAMES}


def _finish(params, keep, masks, loss):
    loss.backward()
    grads = {k: params[k].grad.detach().double().numpy() for k in PARAM_NAMES}
    own = {n: (keep[n].detach() > 0).numpy() for n in RELU_NAMES} if masks is None else dict(masks)
    return grads, own


def gradients(weights, x, grad_p, masks=None, dtype=None, keep=None, **drop):
    """Gradient of sum(grad_p * p) with respect to the twelve parameter tensors -> (grads: name -> float64 array, p float64 array, the
    ReLU decisions this run took -- the imposed ones if masks were given).  keep: receives every tape entry but x."""
    import torch
    dtype = dtype or torch.float64
    params, keep = as_params(weights, dtype), ({} if keep is None else keep)
    p = forward(params, G._to(x, dtype), masks, keep, **drop)
    grads, own = _finish(params, keep, masks, (p * G._to(grad_p, dtype)).sum())
    return grads, p.detach().double().numpy(), own


def tape_views(tape, layout, B):
    """tape: flat float32 array; layout: ext.banknet_tape_layout(B, H, W) or ext.banknet3d_tape_layout(B, D, H, W)
    -> {name: (B,C,h,w) or (B,C,d,h,w) view}"""
    return {name: tape[off:off + B * C * int(np.prod(sizes))].reshape(B, C, *sizes) for name, off, C, *sizes in layout}


def masks_from_tape(tape, layout, B):
    v = tape_views(tape, layout, B)
    return {n: v[n] > 0 for n in RELU_NAMES}


def worst_rel(got, want, skip=()):
    per = {k: float(np.abs(np.asarray(got[k], np.float64) - want[k]).max() / np.abs(want[k]).max()) for k in PARAM_NAMES if k not in skip}
    return max(per.values()), per


def e32_per_tensor(weights, x, grad_p):
    """The rounding a float32 backward pass has on these inputs: torch float32 on the CPU against the float64 model under the float32
    run's own ReLU decisions.  (worst tensor, {name: max|g32 - g64| / max|g64|})"""
    import torch
    g32, _, m32 = gradients(weights, x, grad_p, dtype=torch.float32)
    g64, _, _ = gradients(weights, x, grad_p, masks=m32)
    return worst_rel(g32, g64)


def e32(weights, x, grad_p):
    return e32_per_tensor(weights, x, grad_p)[0]


def split_blob(blob):
    """the gradient blob (the layout of the weights blob, of either dimension) -> name -> array of the parameter's shape"""
    ndim = 2 if blob.size == sum(L["cout"] * (L["cin"] * L["k"] ** 2 + 1) for L in LAYERS) else 3
    out, off = {}, 0
    for L in LAYERS:
        shp = (L["cout"], L["cin"]) + (L["k"],) * ndim
        n = int(np.prod(shp))
        out[L["name"] + ".weight"] = blob[off:off + n].reshape(shp); off += n
        out[L["name"] + ".bias"] = blob[off:off + L["cout"]]; off += L["cout"]
    assert off == blob.size, (off, blob.size)
    return out


def check_grads(got, g64, e32_shape, own, label, skip=()):
    """_check_grads's rule of tests/test_cnn_train_gpu.py: every tensor within FACTOR x the shape's e32, every weight tensor within
    FACTOR x max(its own float32 error, OWN_FLOOR).  Prints the ratios, then asserts."""
    worst, per = worst_rel(got, g64, skip)
    e32_shape = max(v for k, v in own.items() if k not in skip) if skip else e32_shape
    k = max(per, key=per.get)
    print(f"\nBANK_GRAD_ERR {label} {k} {worst:.3e} e32 {e32_shape:.3e} ratio {worst / e32_shape:.2f} median {np.median(list(per.values())):.3e}")
    r = {t: per[t] / max(own[t], OWN_FLOOR) for t in per if t.endswith(".weight")}
    t = max(r, key=r.get)
    print(f"BANK_GRAD_OWN {label} worst weight tensor {t} {per[t]:.3e} / max(own {own[t]:.3e}, {OWN_FLOOR:g}) = {r[t]:.2f}")
    sharp = {t: v for t, v in r.items() if not v <= FACTOR}
    assert not sharp, f"{label}: weight tensors beyond {FACTOR:g} x their own float32 error: {sharp}"
    bad = {k: v for k, v in per.items() if not v <= FACTOR * e32_shape}
    assert not bad, f"{label}: beyond {FACTOR:g} x e32 = {FACTOR * e32_shape:.3e}: {bad}"


# ---- the FluidNet-level chain: cnn_grad_reference's operators with the bank net in the middle -------------------------------------
def fluidnet_forward(params, inp, thr=1e-5, masks=None, keep=None, x_net=None, scale=None):
    """inp (B,5,1,H,W) or (B,6,D,H,W) array [p, U, flags, density] -> (p, U) torch tensors (B,.,D,H,W); x_net / scale as in
    cnn_grad_reference.  The net sees the 2D state without its depth axis."""
    import torch
    import train_reference as TR
    dtype = next(iter(params.values())).dtype
    U0, flags = G.split_input(np.asarray(inp, np.float64))
    B, ndim = U0.shape[:2]
    U, ft = G._to(U0, dtype), G._to(flags, dtype)
    s = torch.clamp(U.reshape(B, -1).std(dim=1, unbiased=True), min=thr) if scale is None else G._to(scale, dtype)
    s = s.reshape(B, 1, 1, 1, 1)
    if x_net is None:
        xt = torch.cat((TR.divergence(U, ft) / s, G._to(G.occupancy(flags, ndim), dtype)), 1)
        xt = xt[:, :, 0] if ndim == 2 else xt
    else:
        xt = G._to(x_net, dtype)
    p = forward(params, xt, masks, keep)
    p = p[:, :, None] if ndim == 2 else p
    U = TR.velocity_update(p, U / s, ft)
    return p * s, TR.set_wall_bcs(U * s, ft)


def fluidnet_gradients(weights, inp, w_p, w_U, thr=1e-5, masks=None, dtype=None, x_net=None, scale=None):
    """Gradient of sum(w_p p) + sum(w_U U) (either weight may be None) over fluidnet_forward -> (grads, (p, U) float64 arrays, masks)"""
    import torch
    dtype = dtype or torch.float64
    params, keep = as_params(weights, dtype), {}
    p, U = fluidnet_forward(params, inp, thr, masks, keep, x_net, scale)
    loss = 0.0
    if w_p is not None:
        loss = loss + (p * G._to(w_p, dtype)).sum()
    if w_U is not None:
        loss = loss + (U * G._to(w_U, dtype)).sum()
    grads, own = _finish(params, keep, masks, loss)
    return grads, (p.detach().double().numpy(), U.detach().double().numpy()), own


def fluidnet_e32(weights, inp, w_p, w_U, thr=1e-5, x_net=None, scale=None):
    import torch
    g32, _, m32 = fluidnet_gradients(weights, inp, w_p, w_U, thr, dtype=torch.float32, x_net=x_net, scale=scale)
    g64, _, _ = fluidnet_gradients(weights, inp, w_p, w_U, thr, masks=m32, x_net=x_net, scale=scale)
    return worst_rel(g32, g64)
