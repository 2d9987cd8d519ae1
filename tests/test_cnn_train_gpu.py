"""The native training path of the 2D pressure net against torch's float64 autograd over the float64 model of the net
(tests/cnn_grad_reference.py), on weights under which every layer shows in the output (propagating_weights).

The float64 model takes its ReLU decisions from the implementation under test (the tape's saved outputs > 0): free decisions differ
in a handful of pre-activations within rounding of zero, and each flip moves a weight gradient by 2e-3 of its max -- that would
hide real defects behind a loose bound.

Tolerance rule for gradients: per shape, e32 = the worst-tensor error of torch float32 on the CPU against the float64 model under
the float32 run's own masks; the native gradient of every parameter tensor must be within 8 e32 of the float64 one under the native
masks, as a fraction of the tensor's max (4x: the F(4x4) forward measures 2.5e-6 where torch float32 measures 6e-7; 2x: the
weight gradient's pixel sums run in another order than oneDNN's).  On top of that every weight tensor is held to 8 x its OWN float32
error (_check_grads; measured: at most 5.3 x, the F(4x4) mode at (3, 199, 215); 1.3 .. 3.9 x elsewhere).  Shapes: those of tests/test_cnn_fp64_gpu.py, so that the
input-gradient convolutions reach every branch of the forward's launchers."""
import numpy as np
import pytest
import torch

import cnn_grad_reference as G
from cnn_reference import net_input, propagating_weights
from util import assert_bitexact, assert_close_rel, random_state

pytestmark = pytest.mark.gpu

MODES = ["fp32", "fp32_f2", "fp32_direct"]
SHAPES = G.GPU_SHAPES[2]                                      # (B, H, W)
FACTOR = 8.0
OWN_FLOOR = 6e-7


def _id(s):
    return "x".join(str(v) for v in s)


def _mconf(mode, **kw):
    return dict(model="ScaleNet", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True,
                normalizeInputChan="UDiv", normalizeInputThreshold=1e-5, is3D=False, precisionMode=mode, **kw)


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
    return propagating_weights(2)


@pytest.fixture(scope="module")
def images(dev, ext, weights):
    from fluidnet_cxx_amd.model import blob_from_state_dict
    blob = torch.from_numpy(blob_from_state_dict(weights)).to(dev)
    return ext.scalenet_pack(blob, False), ext.scalenet_pack_t(blob)


@pytest.fixture(scope="module")
def case(weights):
    """shape -> (x (B,2,H,W), w_p (B,1,H,W), e32, {tensor: its own float32 error}): the inputs and the float32 yardstick, once per shape"""
    cache = {}

    def get(shape):
        if shape not in cache:
            x, wp = G.case_inputs(shape)
            cache[shape] = (x, wp) + G.e32_per_tensor(weights, x, wp)
        return cache[shape]
    return get


@pytest.fixture(scope="module")
def native(dev, ext, images, case):
    """(shape, mode) -> the native training forward and backward of the case, and the float64 gradient under the native masks"""
    cache = {}

    def get(shape, mode):
        if (shape, mode) not in cache:
            x, wp = case(shape)[:2]
            B, H, W = shape
            xt, gt = torch.from_numpy(x).to(dev), torch.from_numpy(wp).to(dev)
            p, tape = ext.multiscale_forward_train(images[0], xt, mode)
            grad = ext.multiscale_backward(images[1], gt, tape, mode)
            tape_np = tape.cpu().numpy()
            layout = ext.multiscale_tape_layout(B, H, W)
            g64, _, _ = G.gradients(propagating_weights(2), x, wp, masks=G.masks_from_tape(tape_np, layout, B))
            cache[(shape, mode)] = dict(xt=xt, gt=gt, p=p, tape=tape, tape_np=tape_np, layout=layout, grad=grad, g64=g64)
        return cache[(shape, mode)]
    return get


def _check_grads(got, g64, e32, label, skip=(), own=None):
    worst, per = G.worst_rel(got, g64, skip)
    k = max(per, key=per.get)
    print(f"\nCNN_GRAD_ERR {label} {k} {worst:.3e} e32 {e32:.3e} ratio {worst / e32:.2f} median {np.median(list(per.values())):.3e}")
    if own is not None:
        # The shape's e32 is set by its worst-conditioned tensor (a bias gradient whose terms cancel), which leaves the weight gradients --
        # what the MFMA kernel produces -- a bound many times their own rounding.  So every WEIGHT tensor is also held to 8 x its own
        # float32 error, floored at 6e-7 (torch float32's forward rounding on these weights, the figure the factor 8 was derived from) so
        # that one tensor on which the CPU's float32 sum happens to round well does not set the bar.  Bias tensors stay on the shape's
        # e32: their own float32 error is a residue of cancellation (6e-8 .. 3e-5 measured), not a yardstick.
        r = {t: per[t] / max(own[t], OWN_FLOOR) for t in per if t.endswith(".weight")}
        t = max(r, key=r.get)
        print(f"CNN_GRAD_OWN {label} worst weight tensor {t} {per[t]:.3e} / max(own {own[t]:.3e}, {OWN_FLOOR:g}) = {r[t]:.2f}")
        sharp = {t: v for t, v in r.items() if not v <= FACTOR}
        assert not sharp, f"{label}: weight tensors beyond {FACTOR:g} x their own float32 error: {sharp}"
    bad = {k: v for k, v in per.items() if not v <= FACTOR * e32}
    assert not bad, f"{label}: beyond {FACTOR:g} x e32 = {FACTOR * e32:.3e}: {bad}"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_training_forward(dev, ext, images, weights, case, native, shape, mode):
    """p has the inference forward's bits; every tape entry is within the forward tolerance of the float64 forward's tensor"""
    from fluidnet_cxx_amd import FluidNet
    n = native(shape, mode)
    inf = FluidNet.from_weights(_mconf(mode), weights, dev)
    assert_bitexact(n["p"].cpu().numpy(), inf.multiScale(n["xt"]).cpu().numpy(), f"training forward p {_id(shape)} {mode}")
    keep = {}
    with torch.no_grad():
        G.forward(G.as_params(weights, requires_grad=False), torch.from_numpy(case(shape)[0].astype(np.float64)), keep=keep)
    views = G.tape_views(n["tape_np"], n["layout"], shape[0])
    assert len(views) == 19
    worst = 0.0
    for name, got in views.items():
        want = keep[int(name[1:])] if name[0] == "y" else keep[name]
        want = want.numpy()
        worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    print(f"\nCNN_TAPE_ERR {_id(shape)} {mode} worst entry {worst:.3e}")
    for name, got in views.items():
        want = keep[int(name[1:])] if name[0] == "y" else keep[name]
        assert_close_rel(got, want.numpy(), 1e-5, f"tape entry {name} {_id(shape)} {mode}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_backward_vs_masked_fp64(case, native, shape, mode):
    n = native(shape, mode)
    _check_grads(G.split_blob(n["grad"].cpu().numpy(), 2), n["g64"], case(shape)[2], f"{_id(shape)} {mode}", own=case(shape)[3])


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_plain_weight_gradient_kernel_agrees(ext, images, case, native, shape):
    """multiscale_backward_plain: the thin layers' kernel for every layer -- the same bound, and an independent check of the MFMA kernel"""
    n = native(shape, "fp32")
    grad = ext.multiscale_backward_plain(images[1], n["gt"], n["tape"], "fp32")
    _check_grads(G.split_blob(grad.cpu().numpy(), 2), n["g64"], case(shape)[2], f"{_id(shape)} fp32 plain")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_backward_is_reproducible_and_leaves_its_inputs(ext, images, native, case, shape, mode):
    n = native(shape, mode)
    again = ext.multiscale_backward(images[1], n["gt"], n["tape"], mode)
    assert_bitexact(again.cpu().numpy(), n["grad"].cpu().numpy(), "second backward call")
    B = shape[0]
    entries = lambda t: G.tape_views(t, n["layout"], B).items()            # (the padding between entries is not part of the tape)
    for (name, a), (_, b) in zip(entries(n["tape"].cpu().numpy()), entries(n["tape_np"])):
        assert_bitexact(a, b, f"tape entry {name} after the backward")
    assert_bitexact(n["gt"].cpu().numpy(), case(shape)[1], "grad_p after the backward")
    assert_bitexact(n["xt"].cpu().numpy(), case(shape)[0], "x after the backward")
    p2, tape2 = ext.multiscale_forward_train(images[0], n["xt"], mode)
    for (name, a), (_, b) in zip(entries(tape2.cpu().numpy()), entries(n["tape_np"])):
        assert_bitexact(a, b, f"tape entry {name} of a second training forward")
    assert_bitexact(p2.cpu().numpy(), n["p"].cpu().numpy(), "p of a second training forward")


def _fluidnet_loss(fluid, p, U, flags, target_p, lam):
    """fluid_net_train.py:276-285: pL2 + divL2 + pL1 + divL1 with their lambdas (MSELoss / L1Loss, the divergence's target zero)"""
    div = fluid.velocityDivergence(U.contiguous(), flags)
    return (lam[0] * ((p - target_p) ** 2).mean() + lam[1] * (div ** 2).mean() +
            lam[2] * (p - target_p).abs().mean() + lam[3] * div.abs().mean())


# (pL2Lambda, divL2Lambda, pL1Lambda, divL1Lambda): the reference's trainConfig.yaml, and a set with every term switched on
LAMBDAS = {"reference": (0.0, 1.0, 0.0, 0.0), "all_terms": (1.0, 1.0, 0.5, 0.5)}


# Gradients that vanish identically: the bias of the final 1x1 and the bias of the 8-channel layer before it shift p by a constant.
# Where the loss has no term in p (the reference's lambdas) only the divergence of U sees p, through its differences, so these two
# gradients are sums that cancel exactly: g = sum(g_net) resp. w_final[c] sum(g_net), 1e-7 of their terms in float32 and float64
# alike, and max|g - g64| / max|g64| compares one rounding residue with another (measured: 2.3, with e32 = 6.1 from the same two
# tensors, which would admit any gradient for the other 32).  There they are left out of e32 and of the relative rule and bounded by
# the rounding of their own sum instead: |g - g64| <= 8 e32 max|w| sum|g_net|.
NULL_BIASES = ("multiScale.final.bias", "multiScale.convN_1.encode.10.bias")


@pytest.mark.parametrize("lam", list(LAMBDAS))
@pytest.mark.parametrize("mode", MODES)
def test_fluidnet_level_gradients(dev, ext, oracle, weights, mode, lam):
    from fluidnet_cxx_amd import FluidNetTrain, fluid
    B, H, W = 2, 64, 96
    s = random_state(B, 1, H, W, 0.5, seed=13, boxes=True)
    inp = torch.from_numpy(np.concatenate([np.zeros_like(s["p"]), s["U"], s["flags"], s["rho"]], 1)).to(dev)
    flags = inp[:, 3:4].contiguous()
    target_p = torch.from_numpy(np.random.default_rng(17).standard_normal((B, 1, 1, H, W)).astype(np.float32)).to(dev)
    net = FluidNetTrain(_mconf(mode))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    net.to(dev)
    p, U = net(inp)
    p.retain_grad(); U.retain_grad()
    _fluidnet_loss(fluid, p, U, flags, target_p, LAMBDAS[lam]).backward()
    # the same forward through the extension, for the tape and the scale (deterministic: the same bits)
    p2, U2, tape, scale, flags2 = ext.fluidnet_forward_train(net.packed, inp, 1e-5, mode)
    assert_bitexact(p2.cpu().numpy(), p.detach().cpu().numpy(), "p of the two forwards")
    assert_bitexact(U2.cpu().numpy(), U.detach().cpu().numpy(), "U of the two forwards")
    assert_bitexact(flags2.cpu().numpy(), s["flags"], "flags channel")
    # g_net from the oracle's adjoints (pinned to the reference's autograd by tests/test_grad.py)
    g_p, g_U, sc = p.grad.cpu().numpy(), U.grad.cpu().numpy(), scale.cpu().numpy().reshape(B, 1, 1, 1, 1)
    _, gp_u = oracle.velocity_update_backward(sc * oracle.set_wall_bcs(g_U, s["flags"]), s["flags"])
    g_net = (sc * g_p + gp_u)[:, :, 0]
    layout = ext.multiscale_tape_layout(B, H, W)
    tape_np = tape.cpu().numpy()
    x_net = G.tape_views(tape_np, layout, B)["in1"][:, 0:2].copy()      # resampling to the same size is the identity
    skip = NULL_BIASES if LAMBDAS[lam][0] == 0 and LAMBDAS[lam][2] == 0 else ()
    e32 = G.e32(weights, x_net, g_net, skip)
    g64, _, _ = G.gradients(weights, x_net, g_net, masks=G.masks_from_tape(tape_np, layout, B))
    got = {k: v.grad.cpu().numpy() for k, v in net.named_parameters()}
    _check_grads(got, g64, e32, f"fluidnet {_id((B, H, W))} {mode} {lam}", skip)
    terms = float(np.abs(g_net.astype(np.float64)).sum())
    for k in skip:
        wmax = 1.0 if k == "multiScale.final.bias" else float(np.abs(weights["multiScale.final.weight"]).max())
        d = float(np.abs(got[k] - g64[k]).max())
        print(f"CNN_GRAD_NULL {k} |g - g64| {d:.3e} max|g64| {np.abs(g64[k]).max():.3e} sum|terms| {wmax * terms:.3e}")
        assert d <= FACTOR * e32 * wmax * terms, k


def test_short_training_run(dev, ext, weights):
    """8 steps of plain SGD at rate 1e-4 on mean((p - t)^2), natively and with the float64 model (free ReLU: the loss is continuous
    across a flip).  On the CPU the float64 loss goes 2.105 -> 1.273, falling at every step, and torch float32 ends within 1e-7 of
    that fall.  Bound on the final loss: 2 mean|p - t| 1e-5 |p|max (float64 values of the last step) -- what the forward tolerance
    1e-5 |ref|max allows the loss to move if every pixel erred the same way."""
    from fluidnet_cxx_amd import FluidNet, FluidNetTrain, fluid
    x = net_input(4, 1, 64, 96, seed=3)[:, :, 0].copy()
    t = np.random.default_rng(9).standard_normal((4, 1, 64, 96))
    lr, steps = 1e-4, 8
    # float64
    params = G.as_params(weights)
    xt64, t64 = torch.from_numpy(x.astype(np.float64)), torch.from_numpy(t)
    ref = []
    for step in range(steps + 1):
        p64 = G.forward(params, xt64)
        loss = ((p64 - t64) ** 2).mean()
        ref.append(float(loss.detach()))
        if step == steps:
            break
        loss.backward()
        with torch.no_grad():
            for q in params.values():
                q -= lr * q.grad
                q.grad = None
    bound = 2.0 * float((p64 - t64).abs().mean()) * 1e-5 * float(p64.abs().max())
    # native
    net = FluidNetTrain(_mconf("fp32"))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    net.to(dev)
    opt = torch.optim.SGD(net.parameters(), lr=lr)
    xt, tt = torch.from_numpy(x).to(dev), torch.from_numpy(t.astype(np.float32)).to(dev)
    got = []
    for step in range(steps + 1):
        opt.zero_grad()
        p = net.multiScale(xt)
        loss = ((p.double() - tt.double()) ** 2).mean()
        got.append(float(loss.detach()))
        if step == steps:
            break
        loss.backward()
        opt.step()
    print(f"\nCNN_TRAIN_LOSS float64 {ref[0]:.6f} -> {ref[-1]:.6f}  native {got[0]:.6f} -> {got[-1]:.6f}  "
          f"|final difference| {abs(got[-1] - ref[-1]):.3e} bound {bound:.3e}")
    assert all(b < a for a, b in zip(ref, ref[1:])), ref
    assert all(b < a for a, b in zip(got, got[1:])), got
    assert abs(got[-1] - ref[-1]) <= bound
    # the trained weights in the inference class: the same forward bits
    with torch.no_grad():
        p_trained = net.multiScale(xt)
    inf = FluidNet(_mconf("fp32"), dropout=False)
    inf.load_state_dict(net.state_dict())
    inf.to(dev)
    assert_bitexact(inf.multiScale(xt).cpu().numpy(), p_trained.cpu().numpy(), "FluidNet with the trained state_dict")
    # one Adam step on the FluidNet-level loss: every parameter tensor changes, and so does the next forward
    s = random_state(2, 1, 64, 96, 0.5, seed=13, boxes=True)
    inp = torch.from_numpy(np.concatenate([np.zeros_like(s["p"]), s["U"], s["flags"], s["rho"]], 1)).to(dev)
    target_p = torch.zeros(2, 1, 1, 64, 96, device=dev)
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    with torch.no_grad():
        p0, U0 = net(inp)
    adam = torch.optim.Adam(net.parameters())
    adam.zero_grad()
    p, U = net(inp)
    assert_bitexact(p.detach().cpu().numpy(), p0.cpu().numpy(), "training and no_grad forward of FluidNetTrain")
    _fluidnet_loss(fluid, p, U, inp[:, 3:4].contiguous(), target_p, LAMBDAS["all_terms"]).backward()
    adam.step()
    for k, v in net.named_parameters():
        assert not torch.equal(v.detach(), before[k]), f"{k} did not change in the Adam step"
    with torch.no_grad():
        p1, U1 = net(inp)
    assert not torch.equal(p1, p0) and not torch.equal(U1, U0)


@pytest.mark.parametrize("fused", [True, False])
def test_simulate_under_no_grad_with_the_training_net(dev, weights, fused):
    """fluid_net_train.py:356-360: the long-term-divergence rollout runs lib.simulate under no_grad with the net that is being trained.
    Three convnet steps of the 64 x 64 plume with a FluidNetTrain in train() mode: the bits of the same steps through a FluidNet
    loaded from its state_dict (the fused step asks the net for packed_for(device); the operator path calls net(data))."""
    from fluidnet_cxx_amd import FluidNet, FluidNetTrain, simulate
    from util import PLUME_CFG, plume_state
    mconf = dict(PLUME_CFG, **_mconf("fp32"))
    net = FluidNetTrain(mconf)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    net.to(dev).train()
    inf = FluidNet(mconf, dropout=False)
    inf.load_state_dict(net.state_dict())
    inf.to(dev)
    a = {k: torch.from_numpy(v).to(dev) for k, v in plume_state(64).items()}
    b = {k: v.clone() for k, v in a.items()}
    for _ in range(3):
        with torch.no_grad():
            simulate(mconf, a, net, "convnet", fused=fused)
        simulate(mconf, b, inf, "convnet", fused=fused)
    assert net.training
    for k in ("p", "U", "density"):
        assert_bitexact(a[k].cpu().numpy(), b[k].cpu().numpy(), f"{k} after 3 convnet steps (fused={fused})")
    assert float(a["U"].abs().max()) > 0


def test_swapped_weight_images_are_refused(dev, ext, images):
    """packed and packed_t look alike and differ in size: a swapped pair is an error before anything is launched"""
    x = torch.zeros(1, 2, 16, 16, device=dev)
    with pytest.raises(RuntimeError, match="scalenet_pack"):
        ext.multiscale_forward_train(images[1], x, "fp32")
    _, tape = ext.multiscale_forward_train(images[0], x, "fp32")
    with pytest.raises(RuntimeError, match="scalenet_pack_t"):
        ext.multiscale_backward(images[0], torch.zeros(1, 1, 16, 16, device=dev), tape, "fp32")


def test_out_of_scope_cases_raise(dev, ext, images):
    from fluidnet_cxx_amd import FluidNetTrain
    x3 = torch.zeros(1, 2, 8, 16, 16, device=dev)
    with pytest.raises(RuntimeError, match="2D only"):
        ext.multiscale_forward_train(images[0], x3, "fp32")
    with pytest.raises(RuntimeError, match="2D only"):
        ext.fluidnet_forward_train(images[0], torch.zeros(1, 6, 8, 16, 16, device=dev), 1e-5, "fp32")
    x = torch.zeros(1, 2, 16, 16, device=dev)
    _, tape = ext.multiscale_forward_train(images[0], x, "fp32")
    for mode in ("bf16x6", "bf16x3"):
        with pytest.raises(RuntimeError, match="fp32 arithmetic only"):
            ext.multiscale_forward_train(images[0], x, mode)
        with pytest.raises(RuntimeError, match="fp32 arithmetic only"):
            ext.multiscale_backward(images[1], torch.zeros(1, 1, 16, 16, device=dev), tape, mode)
    net = FluidNetTrain(_mconf("fp32")).to(dev)
    inp = torch.zeros(1, 5, 1, 16, 16, device=dev, requires_grad=True)
    with pytest.raises(RuntimeError, match="requires_grad"):
        net(inp)
    with pytest.raises(RuntimeError, match="requires_grad"):
        net.multiScale(torch.zeros(1, 2, 16, 16, device=dev, requires_grad=True))
