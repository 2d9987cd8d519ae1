"""The float64 model of the Conv3d bank net (tests/banknet3d_reference.py) made differentiable: torch's autograd over the statement of the
net on five dimensions, as the yardstick of the native backward pass (fnx_banknet3d_train.hip), and the FluidNet-level chain around it
through cnn_grad_reference's operators.  What is free of the dimension comes from tests/banknet_grad_reference.py: the parameter and tape
names, as_params, the ReLU-mask rule (see there), worst_rel, check_grads and its constants.

The tape's names are the 2D ones: a; h1, b1 / h2, b2 / h4, b4 (block.0 and block.2 at full, half and quarter resolution); a2, a4 the
average-pooled a; t the sum of the three levels; c2a, c2b (the two applications of conv2); c3.
"""
import numpy as np

import cnn_grad_reference as G
from banknet_grad_reference import (BANK_TENSORS, FACTOR, LAYERS, OWN_FLOOR, PARAM_NAMES, RELU_NAMES, TAPE_NAMES, _finish, as_params,
                                    check_grads, worst_rel)

__all__ = ["BANK_TENSORS", "FACTOR", "LAYERS", "OWN_FLOOR", "PARAM_NAMES", "RELU_NAMES", "TAPE_NAMES", "as_params", "check_grads", "worst_rel"]


def _up(t, r):
    return t.repeat_interleave(r, 2).repeat_interleave(r, 3).repeat_interleave(r, 4)


def forward(params, xt, masks=None, keep=None, drop_level=None, drop_conv2=None):
    """params: name -> torch tensor (5-D weights); xt (B,2,D,H,W) of the same dtype -> p (B,1,D,H,W).
    masks, keep, drop_level (0: full, 1: half, 2: quarter), drop_conv2 (0, 1): as in banknet_grad_reference.forward."""
    import torch
    import torch.nn.functional as F

    def relu(z, name):
        t = F.relu(z) if masks is None else z * torch.as_tensor(masks[name]).to(z.dtype)
        if keep is not None:
            keep[name] = t
        return t

    def conv(t, name, pad, detach=False):
        w, b = params[name + ".weight"], params[name + ".bias"]
        return F.conv3d(t, w.detach() if detach else w, b.detach() if detach else b, padding=pad)

    def bank(t, tag, detach):
        return relu(conv(relu(conv(t, "convBank.block.0", 1, detach), "h" + tag), "convBank.block.2", 1, detach), "b" + tag)

    a = relu(conv(xt, "conv1", 1), "a")
    a2, a4 = F.avg_pool3d(a, 2), F.avg_pool3d(a, 4)
    t = (bank(a, "1", drop_level == 0) + _up(bank(a2, "2", drop_level == 1), 2)) + _up(bank(a4, "4", drop_level == 2), 4)
    if keep is not None:
        keep.update(a2=a2, a4=a4, t=t)
    t = relu(conv(t, "conv2", 0, drop_conv2 == 0), "c2a")
    t = relu(conv(t, "conv2", 0, drop_conv2 == 1), "c2b")
    t = relu(conv(t, "conv3", 0), "c3")
    return conv(t, "convOut", 0)


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
    """tape: flat float32 array; layout: ext.banknet3d_tape_layout(B, D, H, W) -> {name: (B,C,d,h,w) view}"""
    return {name: tape[off:off + B * C * d * h * w].reshape(B, C, d, h, w) for name, off, C, d, h, w in layout}


def masks_from_tape(tape, layout, B):
    v = tape_views(tape, layout, B)
    return {n: v[n] > 0 for n in RELU_NAMES}


def e32_per_tensor(weights, x, grad_p):
    """The rounding a float32 backward pass has on these inputs: torch float32 on the CPU against the float64 model under the float32
    run's own ReLU decisions.  (worst tensor, {name: max|g32 - g64| / max|g64|})"""
    import torch
    g32, _, m32 = gradients(weights, x, grad_p, dtype=torch.float32)
    g64, _, _ = gradients(weights, x, grad_p, masks=m32)
    return worst_rel(g32, g64)


def split_blob(blob):
    """the gradient blob (the layout of the weights blob) -> name -> array of the parameter's 5-D shape"""
    out, off = {}, 0
    for L in LAYERS:
        shp = (L["cout"], L["cin"], L["k"], L["k"], L["k"])
        n = int(np.prod(shp))
        out[L["name"] + ".weight"] = blob[off:off + n].reshape(shp); off += n
        out[L["name"] + ".bias"] = blob[off:off + L["cout"]]; off += L["cout"]
    assert off == blob.size, (off, blob.size)
    return out


# ---- the FluidNet-level chain: cnn_grad_reference's operators with the Conv3d bank net in the middle ---------------------------------
def fluidnet_forward(params, inp, thr=1e-5, masks=None, keep=None, x_net=None, scale=None):
    """inp (B,6,D,H,W) array [p, U, flags, density] -> (p, U) torch tensors; x_net / scale as in cnn_grad_reference"""
    import torch
    import train_reference as TR
    dtype = next(iter(params.values())).dtype
    U0, flags = G.split_input(np.asarray(inp, np.float64))
    B = U0.shape[0]
    assert U0.shape[1] == 3
    U, ft = G._to(U0, dtype), G._to(flags, dtype)
    s = torch.clamp(U.reshape(B, -1).std(dim=1, unbiased=True), min=thr) if scale is None else G._to(scale, dtype)
    s = s.reshape(B, 1, 1, 1, 1)
    if x_net is None:
        xt = torch.cat((TR.divergence(U, ft) / s, G._to(G.occupancy(flags, 3), dtype)), 1)
    else:
        xt = G._to(x_net, dtype)
    p = forward(params, xt, masks, keep)
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
