"""Training of the Conv3d bank net on the GPU (fnx_banknet3d_train.hip): the tape forward against the inference forward and the float64
model, the native backward against the float64 model under the native ReLU decisions (tests/banknet3d_grad_reference.py) at
banknet3d_reference.SHAPES3D and at one shape whose launches have more items than workgroups, under weights with which every level and
both applications of conv2 carry a share of the gradient (tests/test_banknet3d_train_host.py shows that they do), the sums over the shared
weights, reproducibility, graph replay, the 3D ScaleNet's training calls around a bank training call, the FluidNet-level chain, the
autograd module and simulate() with the training net."""
import numpy as np
import pytest
import torch

import banknet3d_grad_reference as BG
import cnn_grad_reference as G
from banknet3d_reference import SHAPES3D, bank3d_input, propagating_bank3d_weights
from util import PLUME_CFG, assert_bitexact, assert_close_rel, plume_state

pytestmark = pytest.mark.gpu

MODES = ["fp32", "fp32_direct", "fp32_f4", "fp32_f2"]
MCONF = dict(PLUME_CFG, model="FluidNet3D", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True,
             normalizeInputChan="UDiv", inputDim=3, is3D=True)
# (2,32,64,64): the tail and conv1 have 4096 units of 64 cells on 512 workgroups, the full level's weight gradients 2 x 16 x 2 tiles x 8
# chunks = 512 items on 256 workgroups, so a workgroup accumulates over several items in every kind of launch with partial sums
MANY_ITEMS = (2, 32, 64, 64)
FLUID_SHAPES = [(2, 8, 12, 20), (1, 12, 20, 36)]
BATCH = (2, 8, 12, 20)


def _id(s):
    return "x".join(map(str, s))


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    from fluidnet_cxx_amd._ext import ext
    return ext


@pytest.fixture(scope="module")
def weights():
    return propagating_bank3d_weights(0)


@pytest.fixture(scope="module")
def images(dev, ext, weights):
    from fluidnet_cxx_amd.model import _bank_keys, blob_from_state_dict
    blob = torch.from_numpy(blob_from_state_dict(weights, keys=_bank_keys())).to(dev)
    return ext.banknet3d_pack(blob), ext.banknet3d_pack_t(blob)


@pytest.fixture(scope="module")
def case():
    """(x, w_p) per shape: x is bank3d_input, the loss is sum(w_p p) with default_rng(7) normals"""
    cache = {}

    def get(shape):
        if shape not in cache:
            cache[shape] = (bank3d_input(*shape), np.random.default_rng(7).standard_normal((shape[0], 1) + shape[1:]).astype(np.float32))
        return cache[shape]
    return get


@pytest.fixture(scope="module")
def native(dev, ext, images, case):
    """the native forward_train + backward per (shape, mode), run once"""
    cache = {}

    def get(shape, mode="fp32"):
        if (shape, mode) not in cache:
            x, wp = case(shape)
            xt, gp = T(x, dev), T(wp, dev)
            p, tape = ext.banknet3d_forward_train(images[0], xt, mode)
            blob = ext.banknet3d_backward(images[1], xt, gp, tape, mode)
            cache[(shape, mode)] = dict(xt=xt, gp=gp, p=p, tape=tape, tape_np=N(tape), blob=blob, layout=ext.banknet3d_tape_layout(*shape))
        return cache[(shape, mode)]
    return get


@pytest.fixture(scope="module")
def forward64(weights, case):
    """every tape entry of the float64 forward per shape, computed once"""
    cache = {}

    def get(shape):
        if shape not in cache:
            keep = {}
            with torch.no_grad():
                BG.forward(BG.as_params(weights, requires_grad=False), torch.from_numpy(case(shape)[0].astype(np.float64)), keep=keep)
            cache[shape] = {k: v.numpy() for k, v in keep.items()}
        return cache[shape]
    return get


@pytest.fixture(scope="module")
def yardstick(weights, case):
    """the shape's e32 and every tensor's own float32 error, computed once per shape"""
    cache = {}

    def get(shape):
        if shape not in cache:
            cache[shape] = BG.e32_per_tensor(weights, *case(shape))
        return cache[shape]
    return get


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES3D, ids=_id)
def test_training_forward(dev, weights, native, forward64, shape, mode):
    """p has the inference forward's bits; every tape entry but x is within the CNN tolerance of the float64 forward's tensor"""
    from fluidnet_cxx_amd import FluidNet
    n = native(shape, mode)
    inf = FluidNet.from_weights(dict(MCONF, precisionMode=mode), weights, dev)
    assert_bitexact(N(n["p"]), N(inf.bank(n["xt"])), f"training forward p {_id(shape)} {mode}")
    views = BG.tape_views(n["tape_np"], n["layout"], shape[0])
    assert list(views) == BG.TAPE_NAMES
    keep = forward64(shape)
    for name, got in views.items():
        if name == "x":                       # written by the FluidNet-level forward only
            continue
        want = keep[name]
        print(f"BANK3D_TAPE_ERR {_id(shape)} {mode} {name} {np.abs(got - want).max() / np.abs(want).max():.3e}")
        assert_close_rel(got, want, 1e-5, f"tape entry {name} {_id(shape)} {mode}")


@pytest.mark.parametrize("shape", SHAPES3D + [MANY_ITEMS], ids=_id)
def test_backward_vs_float64(weights, case, native, yardstick, shape):
    """the twelve gradients against the float64 model under the native ReLU decisions"""
    n = native(shape)
    x, wp = case(shape)
    g64, _, _ = BG.gradients(weights, x, wp, masks=BG.masks_from_tape(n["tape_np"], n["layout"], shape[0]))
    e32, own = yardstick(shape)
    BG.check_grads(BG.split_blob(N(n["blob"])), g64, e32, own, _id(shape))


@pytest.mark.parametrize("shape", [(2, 4, 36, 68), (1, 20, 12, 132)], ids=_id)
@pytest.mark.parametrize("scale", ["block", "full"])
def test_shared_weight_sums(dev, ext, images, weights, case, native, shape, scale):
    """with grad_p zeroed outside a 4 x 4 x 4 block (one quarter-level cell, eight half-level cells), and at full scale with another
    w_p, the gradients of the bank tensors and of conv2 are the model's sums over the three levels / the two applications"""
    n = native(shape)
    x, wp = case(shape)
    B, D, H, W = shape
    if scale == "block":
        m = np.zeros_like(wp)
        z0, y0, x0 = 4 * (D // 8), 4 * (H // 8), 4 * (W // 8)
        m[:, :, z0:z0 + 4, y0:y0 + 4, x0:x0 + 4] = 1
        wp = wp * m
    else:
        wp = np.random.default_rng(11).standard_normal(wp.shape).astype(np.float32)
    blob = ext.banknet3d_backward(images[1], n["xt"], T(wp, dev), n["tape"], "fp32")
    g64, _, _ = BG.gradients(weights, x, wp, masks=BG.masks_from_tape(n["tape_np"], n["layout"], B))
    e32, own = BG.e32_per_tensor(weights, x, wp)
    BG.check_grads(BG.split_blob(N(blob)), g64, e32, own, f"{_id(shape)} {scale}")


def test_two_calls_same_bits_and_inputs_untouched(dev, ext, images, case, native):
    shape = (1, 12, 20, 36)
    n = native(shape)
    x, wp = case(shape)
    again = ext.banknet3d_backward(images[1], n["xt"], n["gp"], n["tape"], "fp32")
    assert_bitexact(N(again), N(n["blob"]), "backward, second call")
    p2, tape2 = ext.banknet3d_forward_train(images[0], n["xt"], "fp32")
    assert_bitexact(N(p2), N(n["p"]), "forward_train p, second call")
    lay = {name: (off, C * d * h * w * shape[0]) for name, off, C, d, h, w in n["layout"]}
    for name, (off, cnt) in lay.items():
        if name != "x":
            assert_bitexact(N(tape2)[off:off + cnt], n["tape_np"][off:off + cnt], f"tape entry {name}, second call")
    assert_bitexact(N(n["xt"]), x, "x after the backward")
    assert_bitexact(N(n["gp"]), wp, "grad_p after the backward")
    assert_bitexact(N(n["tape"]), n["tape_np"], "tape after the backward")


def test_graph_replay(dev, ext, images, case, native):
    """forward_train + backward captured on one stream replay to the eager bits"""
    n = native(BATCH)
    xs, gs = n["xt"].clone(), n["gp"].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):                    # warm the allocator outside the capture
            p, tape = ext.banknet3d_forward_train(images[0], xs, "fp32")
            ext.banknet3d_backward(images[1], xs, gs, tape, "fp32")
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        p, tape = ext.banknet3d_forward_train(images[0], xs, "fp32")
        blob = ext.banknet3d_backward(images[1], xs, gs, tape, "fp32")
    blob.zero_()
    p.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert_bitexact(N(p), N(n["p"]), "graph replay p")
    assert_bitexact(N(blob), N(n["blob"]), "graph replay gradients")


def test_scalenet3d_training_is_undisturbed(dev, ext, images, case):
    """a 3D ScaleNet forward_train / backward has the same bits before and after a bank training call on the same stream"""
    from fluidnet_cxx_amd.model import blob_from_state_dict
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    sblob = torch.from_numpy(blob_from_state_dict(make_scalenet_weights(0, ndim=3), ndim=3)).to(dev)
    spk, spt = ext.scalenet_pack(sblob, True), ext.scalenet3d_pack_t(sblob)
    x, wp = case(BATCH)
    xt, gp = T(x, dev), T(wp, dev)

    def scalenet():
        p, tape = ext.multiscale3d_forward_train(spk, xt, "fp32")
        return N(p), N(ext.multiscale3d_backward(spt, gp, tape, "fp32"))
    before = scalenet()
    p, tape = ext.banknet3d_forward_train(images[0], xt, "fp32")
    ext.banknet3d_backward(images[1], xt, gp, tape, "fp32")
    after = scalenet()
    assert_bitexact(after[0], before[0], "3D ScaleNet training forward around a bank training call")
    assert_bitexact(after[1], before[1], "3D ScaleNet backward around a bank training call")


@pytest.fixture(scope="module")
def fluid_native(dev, ext, images):
    cache = {}

    def get(shape):
        if shape not in cache:
            inp, w_p, w_U = G.fluidnet_case(shape)
            it = T(inp, dev)
            p, U, tape, scale, flags = ext.fluidnet_bank3d_forward_train(images[0], it, 1e-5, "fp32")
            cache[shape] = dict(inp=inp, w_p=w_p, w_U=w_U, it=it, p=p, U=U, tape=tape, scale=scale, flags=flags,
                                layout=ext.banknet3d_tape_layout(*shape))
        return cache[shape]
    return get


@pytest.mark.parametrize("shape", FLUID_SHAPES, ids=_id)
@pytest.mark.parametrize("which", ["both", "p_only", "U_only"])
def test_fluidnet_level_gradients(dev, ext, images, weights, fluid_native, shape, which):
    """the FluidNet-level backward against the float64 chain, with x_net and the scale taken from the native run; (p, U) of the
    training forward are the inference forward's bits"""
    n = fluid_native(shape)
    B = shape[0]
    w_p = None if which == "U_only" else n["w_p"]
    w_U = None if which == "p_only" else n["w_U"]
    p_inf, U_inf = ext.fluidnet_bank3d_forward(images[0], n["it"], 1e-5, "fp32")
    assert_bitexact(N(n["p"]), N(p_inf), "training forward p")
    assert_bitexact(N(n["U"]), N(U_inf), "training forward U")
    gp = T(np.zeros_like(n["w_p"]) if w_p is None else w_p, dev)
    gU = T(np.zeros_like(n["w_U"]) if w_U is None else w_U, dev)
    blob = ext.fluidnet_bank3d_backward(images[1], n["flags"], n["scale"], gp, gU, n["tape"], "fp32")
    tape_np = N(n["tape"])
    x_net = BG.tape_views(tape_np, n["layout"], B)["x"].astype(np.float64)
    scale = N(n["scale"]).astype(np.float64)
    masks = BG.masks_from_tape(tape_np, n["layout"], B)
    g64, _, _ = BG.fluidnet_gradients(weights, n["inp"], w_p, w_U, masks=masks, x_net=x_net, scale=scale)
    e32, own = BG.fluidnet_e32(weights, n["inp"], w_p, w_U, x_net=x_net, scale=scale)
    # Without grad_p the gradient of convOut's bias is zero in exact arithmetic: a constant added to p leaves velocityUpdate's
    # differences, and so U, where they were.  What either implementation returns there is a residue of cancellation, no yardstick and
    # nothing to hold a relative bound against: it is held to the CNN tolerance 1e-5 of the gradient of convOut's weight instead.
    skip = ("convOut.bias",) if which == "U_only" else ()
    got = BG.split_blob(N(blob))
    BG.check_grads(got, g64, e32, own, f"fluidnet {_id(shape)} {which}", skip)
    for k in skip:
        assert np.abs(got[k]).max() <= 1e-5 * np.abs(g64["convOut.weight"]).max(), (k, got[k], np.abs(g64["convOut.weight"]).max())


def _train_net(dev, weights):
    from fluidnet_cxx_amd import FluidNetBankTrain3D
    net = FluidNetBankTrain3D(MCONF)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in weights.items()})
    return net.to(dev).train()


def test_autograd_fills_the_twelve_gradients(dev, ext, images, weights, fluid_native):
    """FluidNetBankTrain3D(...)(input_) + backward() gives every parameter the ABI call's bits; gp = None and gU = None each work"""
    shape = FLUID_SHAPES[0]
    n = fluid_native(shape)
    net = _train_net(dev, weights)
    names = [k for k, _ in net.named_parameters()]
    assert names == BG.PARAM_NAMES
    w_p, w_U = T(n["w_p"], dev), T(n["w_U"], dev)
    for which in ("both", "p_only", "U_only"):
        net.zero_grad()
        p, U = net(n["it"])
        assert_bitexact(N(p), N(n["p"]), "module forward p")
        loss = (p * w_p).sum() + (U * w_U).sum() if which == "both" else ((p * w_p).sum() if which == "p_only" else (U * w_U).sum())
        loss.backward()
        gp = w_p if which != "U_only" else torch.zeros_like(w_p)
        gU = w_U if which != "p_only" else torch.zeros_like(w_U)
        want = BG.split_blob(N(ext.fluidnet_bank3d_backward(images[1], n["flags"], n["scale"], gp, gU, n["tape"], "fp32")))
        for k, q in net.named_parameters():
            assert q.grad is not None, k
            assert_bitexact(N(q.grad), want[k], f"{which}: .grad of {k}")
    # the net alone
    x = T(bank3d_input(*BATCH), dev)
    net.zero_grad()
    net.bank(x).sum().backward()
    pq, tape = ext.banknet3d_forward_train(images[0], x, "fp32")
    want = BG.split_blob(N(ext.banknet3d_backward(images[1], x, torch.ones_like(pq), tape, "fp32")))
    for k, q in net.named_parameters():
        assert_bitexact(N(q.grad), want[k], f"net.bank: .grad of {k}")


def test_simulate_with_the_training_net(dev, weights):
    """simulate(..., net, 'convnet') under no_grad: the training net gives the bits of FluidNet holding the same weights (two steps of a
    12 x 24 x 24 plume)"""
    from fluidnet_cxx_amd import FluidNet, _simulate, simulate
    nets = [_train_net(dev, weights), FluidNet.from_weights(MCONF, weights, dev).eval()]
    out = []
    for net in nets:
        bd = {k: T(v, dev) for k, v in plume_state(24, D=12).items()}
        with torch.no_grad():
            for _ in range(2):
                simulate(MCONF, bd, net, "convnet")
        out.append({k: N(bd[k]) for k in ("U", "density", "p")})
    _simulate.release_workspaces()
    for k in out[0]:
        assert_bitexact(out[0][k], out[1][k], f"simulate with the training net: {k}")
