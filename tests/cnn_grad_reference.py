"""The float64 model of the MultiScale pressure net (tests/cnn_reference.py) made differentiable, in 2D and 3D: torch's autograd over the
same construction (resample at float32 sample positions, F.conv2d on (B,C,H,W) resp. F.conv3d on (B,C,D,H,W), ReLU), as the yardstick of
the native backward passes -- and a float64 statement of the FluidNet-level chain around the net (fluidnet_forward).  The dimension is
that of the tensors passed in; what differs by it is in CONV, GPU_SHAPES, INPUT_CHANNELS and occupancy.

ReLU masks.  A float32 implementation and the float64 model disagree on the sign of a handful of pre-activations that lie within
rounding of zero, and every such flip moves a weight gradient by one pixel's (voxel's) term (2e-3 of a tensor's max, measured in 2D) --
far more than the rounding of everything else (1e-6).  So the model can take its ReLU decisions from outside: masks[l] (bool, the shape
of layer l's output) replaces relu(z) by z * mask, i.e. the model differentiates the piecewise-linear branch the implementation under
test took.  masks_from_tape reads them off the native tape (saved output > 0, torch's rule).

Layers are numbered as in scalenet_layers(): 0..3 quarter resolution, 4..9 half, 10..15 full, 16 the final 1x1(x1)."""
import numpy as np

from cnn_reference import TOWERS, resample
from fluidnet_cxx_amd.weights import scalenet_layers

LAYERS = scalenet_layers(2, 2)                      # names, channels and k of a layer are those of both dimensions: a kernel is k^ndim
assert LAYERS == scalenet_layers(2, 3)
PARAM_NAMES = [L["name"] + sfx for L in LAYERS for sfx in (".weight", ".bias")]
RELU_LAYERS = [l for l, L in enumerate(LAYERS) if L["relu"]]
CONV = {2: "conv2d", 3: "conv3d"}                   # torch.nn.functional's name by the number of grid axes of the tensor

# The shapes of the GPU gradient tests.  2D: (B, H, W) of tests/test_cnn_train_gpu.py (from test_cnn_fp64_gpu.py).  3D: (B, D, H, W) of
# tests/test_cnn_train3d_gpu.py.  S1: towers (1, 2, 9) and (3, 5, 18) -- B > 1, a quarter-resolution depth of 1, H not a multiple of the
# 4-row tile, two x tiles (the second with 5 columns), upsampling ratios that are not 2.  S2: towers (2, 3, 17) and (4, 7, 35) -- odd D,
# three x tiles (the last with 6 columns), a partial row tile.
S1 = (2, 6, 10, 37)
S2 = (1, 9, 14, 70)
GPU_SHAPES = {2: [(2, 255, 508), (3, 199, 215), (2, 37, 53)], 3: [S1, S2]}


def tower_sizes(size):
    """the reference's size rule (multi_scale_net.py:119-120) per axis"""
    return [int(i * 0.25) for i in size], [int(i * 0.5) for i in size]


def _resample(t, size):
    r = resample(t.double(), size)                     # the interpolation matrices are float64; a float32 model rounds the result
    return r.to(t.dtype)


def forward(params, xt, masks=None, keep=None):
    """params: name -> torch tensor (float64, or float32 for the float32 model); xt (B,2,H,W) or (B,2,D,H,W) of the same dtype.  Returns
    p, one channel of xt's shape.
    masks: {layer index: bool array} imposed instead of the ReLU decisions (every ReLU layer or none).
    keep: a dict that receives {layer index: output after ReLU} and {"xq" / "in2" / "in1": tower input}."""
    import torch
    import torch.nn.functional as F
    size = list(xt.shape[2:])
    conv = getattr(F, CONV[len(size)])
    quarter, half = tower_sizes(size)
    index = {L["name"]: l for l, L in enumerate(LAYERS)}

    def tower(t, name):
        for L in LAYERS:
            if L["tower"] != name:
                continue
            l = index[L["name"]]
            t = conv(t, params[L["name"] + ".weight"], params[L["name"] + ".bias"], padding=L["k"] // 2)
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


def _backward(params, keep, masks, loss):
    """(grads: name -> float64 array, own: {l: bool array}, the ReLU decisions of the run that filled `keep` -- the imposed ones if masks
    were given) of the scalar `loss`"""
    loss.backward()
    grads = {k: params[k].grad.detach().double().numpy() for k in PARAM_NAMES}
    own = {l: (keep[l].detach() > 0).numpy() for l in RELU_LAYERS} if masks is None else dict(masks)
    return grads, own


def gradients(weights, x, grad_p, masks=None, dtype=None):
    """Gradient of sum(grad_p * p) with respect to the 34 parameter tensors.  x (B,2,[D,]H,W), grad_p (B,1,[D,]H,W): arrays.
    Returns (grads: name -> float64 array, p: float64 array, own: {l: bool array}, the ReLU decisions this run took -- the imposed
    ones if masks were given)."""
    import torch
    dtype = dtype or torch.float64
    params = as_params(weights, dtype)
    keep = {}
    p = forward(params, _to(x, dtype), masks, keep)
    grads, own = _backward(params, keep, masks, (p * _to(grad_p, dtype)).sum())
    return grads, p.detach().double().numpy(), own


def case_inputs(shape):
    """The inputs of the gradient tests at `shape` = (B, [D,] H, W): x (B,2,[D,]H,W) float32 and the fixed random w_p (B,1,[D,]H,W) of the
    loss sum(w_p p)"""
    from cnn_reference import net_input
    B, *grid = shape
    D, H, W = [1] * (3 - len(grid)) + grid
    x = net_input(B, D, H, W, seed=B + 1 + sum(grid)).reshape((B, 2, *grid))
    wp = np.random.default_rng(7).standard_normal((B, 1, *grid)).astype(np.float32)
    return x, wp


def tape_views(tape, layout, B):
    """tape: flat float32 array; layout: ext.multiscale_tape_layout(B, H, W) or ext.multiscale3d_tape_layout(B, D, H, W), entries
    (name, offset, C, [D,] H, W) -> {name: (B,C,[D,]H,W) view}"""
    return {name: tape[off:off + B * int(np.prod(dims))].reshape(B, *dims) for name, off, *dims in layout}


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


def e32(weights, x, grad_p, skip=()):
    """the worst tensor's figure of e32_per_tensor"""
    return e32_per_tensor(weights, x, grad_p, skip)[0]


def split_blob(blob, ndim):
    """The gradient blob (the layout of blob_from_state_dict(ndim=ndim)) -> name -> array of the parameter's shape"""
    out, off = {}, 0
    for L in LAYERS:
        shp = (L["cout"], L["cin"]) + (L["k"],) * ndim
        n = int(np.prod(shp))
        out[L["name"] + ".weight"] = blob[off:off + n].reshape(shp); off += n
        out[L["name"] + ".bias"] = blob[off:off + L["cout"]]; off += L["cout"]
    assert off == blob.size, (off, blob.size)
    return out


def structural_zero_taps(shape):
    """{weight name: bool (k,)*ndim array} of the taps that only ever see padding at `shape` = (B, [D,] H, W), so that their gradient is
    exactly 0: tap d of a layer on a tower of n cells along an axis reads cell q + d - k // 2 for q in [0, n), all outside [0, n) when
    |d - k // 2| >= n.  At S1 the quarter tower has depth 1: every dz != 1 tap of its four layers.  At the 2D test shapes: none."""
    grid = list(shape[1:])
    quarter, half = tower_sizes(grid)
    dims = {TOWERS[0]: quarter, TOWERS[1]: half, TOWERS[2]: grid, "final": grid}
    out = {}
    for L in LAYERS:
        k = L["k"]
        dead = np.zeros((k,) * len(grid), bool)
        for ax, n in enumerate(dims[L["tower"]]):
            off = np.abs(np.arange(k) - k // 2) >= n
            dead |= off.reshape([-1 if a == ax else 1 for a in range(len(grid))])
        if dead.any():
            out[L["name"] + ".weight"] = dead
    return out


# ---------------------------------------------------------------------------------------------------
# The FluidNet-level chain (model.py:76-227, lib/model.py:118-227; in 3D the default 3D semantics): div = velocityDivergence(UDiv, flags),
# s = clamp(unbiased std of UDiv per sample, thr), x = [div / s, occupancy], p = net(x), velocityUpdate(p, UDiv / s), p s, U s, setWallBcs.
# The operators are the torch statements of tests/train_reference.py over whole arrays, independent of the oracle's per-cell loops and of
# the kernels; fields are (B,C,D,H,W) with D = 1 in 2D, where the net itself takes (B,C,H,W).
# ---------------------------------------------------------------------------------------------------
FLUID, OBST = 1.0, 2.0
INPUT_CHANNELS = {5: 2, 6: 3}              # channels of the input [p, U, flags, density] -> ndim: U has one channel per axis


def split_input(inp):
    """(U, flags) of an input array (B,5,1,H,W) or (B,6,D,H,W)"""
    nd = INPUT_CHANNELS[inp.shape[1]]
    return inp[:, 1:1 + nd], inp[:, 1 + nd:2 + nd]


def occupancy(flags, ndim):
    """The net's second input channel.  The 2D model (lib/model.py) feeds the test flags == obstacle; the 3D one flagsToOccupancy's map of
    the flag values (fluid -> 0, obstacle -> 1, any other value itself).  On grids of fluid and obstacle cells the two agree."""
    if ndim == 2:
        return (flags == OBST).astype(np.float64)
    return np.where(flags == FLUID, 0.0, np.where(flags == OBST, 1.0, flags))


def fluidnet_forward(params, inp, thr=1e-5, masks=None, keep=None, x_net=None, scale=None):
    """inp (B,5,1,H,W) or (B,6,D,H,W) array [p, U, flags, density] -> (p, U) torch tensors of params' dtype, shaped like inp's fields.
    x_net / scale: the net's input and the per-sample scale taken from outside (the implementation under test) instead of this model's
    own -- neither depends on the parameters."""
    import torch
    import train_reference as TR
    dtype = next(iter(params.values())).dtype
    U0, flags = split_input(np.asarray(inp, np.float64))
    B, nd = U0.shape[:2]
    U, ft = _to(U0, dtype), _to(flags, dtype)
    if scale is None:
        s = torch.clamp(U.reshape(B, -1).std(dim=1, unbiased=True), min=thr)          # model.py:14-21: unbiased, clamp(thr, inf)
    else:
        s = _to(scale, dtype)
    s = s.reshape(B, 1, 1, 1, 1)
    if x_net is None:
        xt = torch.cat((TR.divergence(U, ft) / s, _to(occupancy(flags, nd), dtype)), 1)
        xt = xt[:, :, 0] if nd == 2 else xt
    else:
        xt = _to(x_net, dtype)
    p = forward(params, xt, masks, keep)
    p = p[:, :, None] if nd == 2 else p
    U = TR.velocity_update(p, U / s, ft)
    return p * s, TR.set_wall_bcs(U * s, ft)


def fluidnet_gradients(weights, inp, w_p, w_U, thr=1e-5, masks=None, dtype=None, x_net=None, scale=None):
    """Gradient of sum(w_p p) + sum(w_U U) over fluidnet_forward with respect to the 34 parameter tensors.
    Returns (grads, (p, U) float64 arrays, own masks)."""
    import torch
    dtype = dtype or torch.float64
    params = as_params(weights, dtype)
    keep = {}
    p, U = fluidnet_forward(params, inp, thr, masks, keep, x_net, scale)
    grads, own = _backward(params, keep, masks, (p * _to(w_p, dtype)).sum() + (U * _to(w_U, dtype)).sum())
    return grads, (p.detach().double().numpy(), U.detach().double().numpy()), own


def fluidnet_e32(weights, inp, w_p, w_U, thr=1e-5, skip=(), x_net=None, scale=None):
    """e32_per_tensor for the FluidNet-level loss"""
    import torch
    g32, _, m32 = fluidnet_gradients(weights, inp, w_p, w_U, thr, dtype=torch.float32, x_net=x_net, scale=scale)
    g64, _, _ = fluidnet_gradients(weights, inp, w_p, w_U, thr, masks=m32, x_net=x_net, scale=scale)
    return worst_rel(g32, g64, skip)


def fluidnet_case(shape, seed=13):
    """inp (B,5,1,H,W) or (B,6,D,H,W) float32 for `shape` = (B, [D,] H, W) with a closed domain and an interior obstacle box in the flags,
    and the loss weights w_p, w_U"""
    B, *grid = shape
    nd = len(grid)
    field = [1] * (3 - nd) + grid
    rng = np.random.default_rng(seed)
    flags = np.full((B, 1, *field), FLUID, np.float32)
    for ax in range(5 - nd, 5):
        np.moveaxis(flags, ax, 0)[[0, -1]] = OBST
    box = [slice(n // 3, n // 3 + e) for n, e in zip(grid, (2, 3, 5)[3 - nd:])]
    flags[(Ellipsis, *box)] = OBST
    inp = np.zeros((B, 3 + nd, *field), np.float32)
    inp[:, 1:1 + nd] = rng.standard_normal((B, nd, *field)).astype(np.float32) * 0.5
    inp[:, 1 + nd:2 + nd] = flags
    inp[:, 2 + nd] = rng.random((B, *field)).astype(np.float32)
    w_p = rng.standard_normal((B, 1, *field)).astype(np.float32)
    w_U = rng.standard_normal((B, nd, *field)).astype(np.float32)
    return inp, w_p, w_U
