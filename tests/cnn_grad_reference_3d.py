"""The float64 model of the 3D MultiScale pressure net made differentiable: torch's autograd over resample (float32 sample positions,
tests/cnn_reference.py) + F.conv3d + ReLU, as the yardstick of the native 3D backward pass -- the scheme of tests/cnn_grad_reference.py
for (B,C,D,H,W) tensors, and a float64 statement of the FluidNet-level chain around the net (fluidnet_forward).

ReLU masks.  As in 2D: a float32 implementation and the float64 model disagree on the sign of a handful of pre-activations within
rounding of zero, and each flip moves a weight gradient by one voxel's term.  masks[l] (bool, the shape of layer l's output) replaces
relu(z) by z * mask, i.e. the model differentiates the piecewise-linear branch the implementation under test took; masks_from_tape reads
them off the native tape (saved output > 0, torch's rule).

Layers are numbered as in scalenet_layers(): 0..3 quarter resolution, 4..9 half, 10..15 full, 16 the final 1x1x1."""
import numpy as np

from cnn_reference import TOWERS, resample
from fluidnet_cxx_amd.weights import scalenet_layers

LAYERS = scalenet_layers(2, 3)
PARAM_NAMES = [L["name"] + sfx for L in LAYERS for sfx in (".weight", ".bias")]
RELU_LAYERS = [l for l, L in enumerate(LAYERS) if L["relu"]]

# (B, D, H, W) of tests/test_cnn_train3d_gpu.py.  S1: towers (1, 2, 9) and (3, 5, 18) -- B > 1, a quarter-resolution depth of 1, H not a
# multiple of the 4-row tile, two x tiles (the second with 5 columns), upsampling ratios that are not 2.  S2: towers (2, 3, 17) and
# (4, 7, 35) -- odd D, three x tiles (the last with 6 columns), a partial row tile.
S1 = (2, 6, 10, 37)
S2 = (1, 9, 14, 70)
GPU_SHAPES = [S1, S2]


def tower_sizes(size):
    """the reference's size rule (multi_scale_net.py:119-120) per axis"""
    return [int(i * 0.25) for i in size], [int(i * 0.5) for i in size]


def _resample(t, size):
    r = resample(t.double(), size)                     # the interpolation matrices are float64; a float32 model rounds the result
    return r.to(t.dtype)


def forward(params, xt, masks=None, keep=None):
    """params: name -> torch tensor (float64, or float32 for the float32 model); xt (B,2,D,H,W) of the same dtype.  Returns p (B,1,D,H,W).
    masks: {layer index: bool array} imposed instead of the ReLU decisions (every ReLU layer or none).
    keep: a dict that receives {layer index: output after ReLU} and {"xq" / "in2" / "in1": tower input}."""
    import torch
    import torch.nn.functional as F
    size = list(xt.shape[2:])
    quarter, half = tower_sizes(size)
    index = {L["name"]: l for l, L in enumerate(LAYERS)}

    def tower(t, name):
        for L in LAYERS:
            if L["tower"] != name:
                continue
            l = index[L["name"]]
            t = F.conv3d(t, params[L["name"] + ".weight"], params[L["name"] + ".bias"], padding=L["k"] // 2)
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


def _to(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dtype)


def gradients(weights, x, grad_p, masks=None, dtype=None):
    """Gradient of sum(grad_p * p) with respect to the 34 parameter tensors.  x (B,2,D,H,W), grad_p (B,1,D,H,W): arrays.
    Returns (grads: name -> float64 array, p: float64 array, own: {l: bool array}, the ReLU decisions this run took -- the imposed
    ones if masks were given)."""
    import torch
    dtype = dtype or torch.float64
    params = as_params(weights, dtype)
    keep = {}
    p = forward(params, _to(x, dtype), masks, keep)
    (p * _to(grad_p, dtype)).sum().backward()
    grads = {k: params[k].grad.detach().double().numpy() for k in PARAM_NAMES}
    own = {l: (keep[l].detach() > 0).numpy() for l in RELU_LAYERS} if masks is None else dict(masks)
    return grads, p.detach().double().numpy(), own


def case_inputs(shape):
    """The inputs of the gradient tests at `shape`: x (B,2,D,H,W) float32 and the fixed random w_p (B,1,D,H,W) of the loss sum(w_p p)"""
    from cnn_reference import net_input
    B, D, H, W = shape
    x = net_input(B, D, H, W, seed=B + 1 + D + H + W)
    wp = np.random.default_rng(7).standard_normal((B, 1, D, H, W)).astype(np.float32)
    return x, wp


def tape_views(tape, layout, B):
    """tape: flat float32 array; layout: ext.multiscale3d_tape_layout(B, D, H, W) -> {name: (B,C,D,H,W) view}"""
    return {name: tape[off:off + B * C * D * H * W].reshape(B, C, D, H, W) for name, off, C, D, H, W in layout}


def masks_from_tape(tape, layout, B):
    v = tape_views(tape, layout, B)
    return {l: v[f"y{l}"] > 0 for l in RELU_LAYERS}


def worst_rel(got, want, skip=()):
    """max over the parameter tensors (but `skip`) of max|got - want| / max|want|, and the per-tensor figures"""
    per = {k: float(np.abs(np.asarray(got[k], np.float64) - want[k]).max() / np.abs(want[k]).max()) for k in PARAM_NAMES if k not in skip}
    return max(per.values()), per


def e32_per_tensor(weights, x, grad_p, skip=()):
    """The rounding a float32 backward pass has on these inputs: torch float32 on the CPU against the float64 model that takes the
    float32 run's own ReLU decisions.  (worst parameter tensor (but `skip`), {name: max|g32 - g64| / max|g64|})"""
    import torch
    g32, _, m32 = gradients(weights, x, grad_p, dtype=torch.float32)
    g64, _, _ = gradients(weights, x, grad_p, masks=m32)
    return worst_rel(g32, g64, skip)


def split_blob(blob):
    """The gradient blob (the layout of blob_from_state_dict(ndim=3)) -> name -> array of the parameter's shape"""
    out, off = {}, 0
    for L in LAYERS:
        shp = (L["cout"], L["cin"], L["k"], L["k"], L["k"])
        n = int(np.prod(shp))
        out[L["name"] + ".weight"] = blob[off:off + n].reshape(shp); off += n
        out[L["name"] + ".bias"] = blob[off:off + L["cout"]]; off += L["cout"]
    assert off == blob.size, (off, blob.size)
    return out


def structural_zero_taps(shape):
    """{weight name: bool (k,k,k) array} of the taps that only ever see padding at `shape`, so that their gradient is exactly 0: tap dz
    of a layer on a tower of depth Dt reads plane z + dz - k // 2 for z in [0, Dt), all outside [0, Dt) when |dz - k // 2| >= Dt (and the
    same per axis).  At S1 the quarter tower has depth 1: every dz != 1 tap of its four layers."""
    quarter, half = tower_sizes(shape[1:])
    dims = {TOWERS[0]: quarter, TOWERS[1]: half, TOWERS[2]: list(shape[1:]), "final": list(shape[1:])}
    out = {}
    for L in LAYERS:
        k = L["k"]
        dead = np.zeros((k, k, k), bool)
        for ax, n in enumerate(dims[L["tower"]]):
            off = np.abs(np.arange(k) - k // 2) >= n
            dead |= off.reshape([-1 if a == ax else 1 for a in range(3)])
        if dead.any():
            out[L["name"] + ".weight"] = dead
    return out


# ---------------------------------------------------------------------------------------------------
# The FluidNet-level chain in float64 (model.py:76-227 on a 3D grid, default 3D semantics): div = velocityDivergence(UDiv, flags),
# s = clamp(unbiased std of UDiv per sample, thr), x = [div / s, occupancy], p = net(x), velocityUpdate(p, UDiv / s), p s, U s, setWallBcs.
# Written with torch operators over whole arrays, independent of the oracle's per-cell loops and of the kernels.
# ---------------------------------------------------------------------------------------------------
FLUID, OBST = 1.0, 2.0


def _interior(shape):
    m = np.zeros(shape, bool)
    m[..., 1:-1, 1:-1, 1:-1] = True
    return m


def fluidnet_forward(params, inp, thr=1e-5, masks=None, keep=None, x_net=None, scale=None):
    """inp (B,6,D,H,W) array [p, Ux, Uy, Uz, flags, density] -> (p, U) torch tensors of params' dtype.
    x_net / scale: the net's input and the per-sample scale taken from outside (the implementation under test) instead of this model's
    own -- neither depends on the parameters."""
    import torch
    dtype = next(iter(params.values())).dtype
    inp = np.asarray(inp, np.float64)
    U0, flags = inp[:, 1:4], inp[:, 4:5]
    B = inp.shape[0]
    inner = _interior(flags.shape)
    Ut = _to(U0, dtype)
    if scale is None:
        s = torch.clamp(Ut.reshape(B, -1).std(dim=1, unbiased=True), min=thr)
    else:
        s = _to(scale, dtype)
    s = s.reshape(B, 1, 1, 1, 1)
    if x_net is None:
        # velocity_divergence.py:46-74: 0 on the border and in obstacle cells
        nxt = lambda a, ax: torch.roll(Ut[:, a:a + 1], -1, dims=ax)
        div = (Ut[:, 0:1] - nxt(0, 4)) + (Ut[:, 1:2] - nxt(1, 3)) + (Ut[:, 2:3] - nxt(2, 2))
        div = div * _to(inner & (flags != OBST), dtype)
        occ = np.where(flags == FLUID, 0.0, np.where(flags == OBST, 1.0, flags))
        xt = torch.cat((div / s, _to(occ, dtype)), 1)
    else:
        xt = _to(x_net, dtype)
    p = forward(params, xt, masks, keep)
    # velocity_update.py (3D intent): on interior cells U_a = [fluid and the -1 neighbour along a fluid] (U_a - (p - p_minus)); the border keeps U
    Us = Ut / s
    comps = []
    for a, ax in ((0, 4), (1, 3), (2, 2)):
        fm = np.roll(flags, 1, axis=ax)
        ff = _to((flags == FLUID) & (fm == FLUID), dtype)
        upd = ff * (Us[:, a:a + 1] - (p - torch.roll(p, 1, dims=ax)))
        it = _to(inner, dtype)
        comps.append(it * upd + (1 - it) * Us[:, a:a + 1])
    U = torch.cat(comps, 1) * s
    p = p * s
    return p, U * _to(wall_mask(flags), dtype)


def wall_mask(flags):
    """setWallBcs (set_wall_bcs.py:45-84) as a 0/1 mask on U (B,3,D,H,W): in fluid and obstacle cells component a is zeroed where the -1
    neighbour along a is an obstacle, or the cell is an obstacle and that neighbour fluid (the neighbour index clamps at the low face in
    x and y; z has no rule on plane 0)."""
    flags = np.asarray(flags)
    B, _, D, H, W = flags.shape
    keep = np.ones((B, 3, D, H, W))
    cell = (flags == FLUID) | (flags == OBST)
    for a, ax in ((0, 4), (1, 3), (2, 2)):
        fm = np.roll(flags, 1, axis=ax)
        lo = [slice(None)] * 5
        lo[ax] = slice(0, 1)
        fm[tuple(lo)] = flags[tuple(lo)]                    # clamped neighbour: the cell itself
        zero = cell & ((fm == OBST) | ((flags == OBST) & (fm == FLUID)))
        if a == 2:
            zero[:, :, 0] = False
        keep[:, a:a + 1][zero] = 0.0
    return keep


def fluidnet_gradients(weights, inp, w_p, w_U, thr=1e-5, masks=None, dtype=None, x_net=None, scale=None):
    """Gradient of sum(w_p p) + sum(w_U U) over fluidnet_forward with respect to the 34 parameter tensors.
    Returns (grads, (p, U) float64 arrays, own masks)."""
    import torch
    dtype = dtype or torch.float64
    params = as_params(weights, dtype)
    keep = {}
    p, U = fluidnet_forward(params, inp, thr, masks, keep, x_net, scale)
    ((p * _to(w_p, dtype)).sum() + (U * _to(w_U, dtype)).sum()).backward()
    grads = {k: params[k].grad.detach().double().numpy() for k in PARAM_NAMES}
    own = {l: (keep[l].detach() > 0).numpy() for l in RELU_LAYERS} if masks is None else dict(masks)
    return grads, (p.detach().double().numpy(), U.detach().double().numpy()), own


def fluidnet_e32(weights, inp, w_p, w_U, thr=1e-5, skip=(), x_net=None, scale=None):
    """e32_per_tensor for the FluidNet-level loss"""
    import torch
    g32, _, m32 = fluidnet_gradients(weights, inp, w_p, w_U, thr, dtype=torch.float32, x_net=x_net, scale=scale)
    g64, _, _ = fluidnet_gradients(weights, inp, w_p, w_U, thr, masks=m32, x_net=x_net, scale=scale)
    return worst_rel(g32, g64, skip)


def fluidnet_case(shape, seed=13):
    """inp (B,6,D,H,W) float32 with a closed domain and an interior obstacle box in the flags, and the loss weights w_p, w_U"""
    B, D, H, W = shape
    rng = np.random.default_rng(seed)
    flags = np.full((B, 1, D, H, W), FLUID, np.float32)
    flags[:, :, 0] = OBST; flags[:, :, -1] = OBST
    flags[:, :, :, 0] = OBST; flags[:, :, :, -1] = OBST
    flags[:, :, :, :, 0] = OBST; flags[:, :, :, :, -1] = OBST
    flags[:, :, D // 3:D // 3 + 2, H // 3:H // 3 + 3, W // 3:W // 3 + 5] = OBST
    inp = np.zeros((B, 6, D, H, W), np.float32)
    inp[:, 1:4] = rng.standard_normal((B, 3, D, H, W)).astype(np.float32) * 0.5
    inp[:, 4:5] = flags
    inp[:, 5] = rng.random((B, D, H, W)).astype(np.float32)
    w_p = rng.standard_normal((B, 1, D, H, W)).astype(np.float32)
    w_U = rng.standard_normal((B, 3, D, H, W)).astype(np.float32)
    return inp, w_p, w_U
