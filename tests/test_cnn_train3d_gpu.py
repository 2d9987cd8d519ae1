"""The native training path of the 3D pressure net against torch's float64 autograd over the float64 model of the net
(tests/cnn_grad_reference.py), on weights under which every layer shows in the output (propagating_weights(3)).

As in 2D (tests/test_cnn_train_gpu.py) the float64 model takes its ReLU decisions from the implementation under test (the tape's saved
outputs > 0), and the tolerance rule is that test's, with its constants: per shape, e32 = the worst-tensor error of torch float32 on the
CPU against the float64 model under the float32 run's own masks; the native gradient of every parameter tensor must be within 8 e32 of
the float64 one under the native masks, as a fraction of the tensor's max, and every weight tensor within 8 x its OWN float32 error,
floored at 6e-7.  e32 is re-measured here by the same computation on the 3D shapes, so it already contains the longer sums of 27 and
125 taps.

Shapes (B, D, H, W): S1 = (2, 6, 10, 37) -- towers (1, 2, 9) and (3, 5, 18): B > 1, a quarter-resolution depth of 1 (every dz != 1 tap of
that tower only sees padding: its weight gradient is exactly 0), H not a multiple of the 4-row tile, two x tiles (the second with 5
columns), upsampling ratios that are not 2; S2 = (1, 9, 14, 70) -- towers (2, 3, 17) and (4, 7, 35): odd D, three x tiles (the last
with 6 columns), a partial row tile."""
import numpy as np
import pytest
import torch

import cnn_grad_reference as G
from cnn_reference import _axis_weights, net_input, propagating_weights
from util import assert_bitexact, assert_close_rel

pytestmark = pytest.mark.gpu

FACTOR = 8.0                                                  # tests/test_cnn_train_gpu.py: FACTOR, OWN_FLOOR
OWN_FLOOR = 6e-7
CASES = [(G.S1, "fp32"), (G.S1, "fp32_f2"), (G.S1, "fp32_direct"), (G.S2, "fp32")]


def _id(s):
    return "x".join(str(v) for v in s)


CASE_IDS = [f"{_id(s)}-{m}" for s, m in CASES]


def _mconf(mode, **kw):
    return dict(model="ScaleNet", inputChannels=dict(div=True, pDiv=False, UDiv=False), normalizeInput=True,
                normalizeInputChan="UDiv", normalizeInputThreshold=1e-5, is3D=True, inputDim=3, precisionMode=mode, **kw)


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
    return propagating_weights(3)


@pytest.fixture(scope="module")
def images(dev, ext, weights):
    from fluidnet_cxx_amd.model import blob_from_state_dict
    blob = torch.from_numpy(blob_from_state_dict(weights, 3)).to(dev)
    return ext.scalenet_pack(blob, True), ext.scalenet3d_pack_t(blob)


@pytest.fixture(scope="module")
def case(weights):
    """shape -> (x (B,2,D,H,W), w_p (B,1,D,H,W), e32, {tensor: its own float32 error}): the inputs and the float32 yardstick, once per shape"""
    cache = {}

    def get(shape):
        if shape not in cache:
            x, wp = G.case_inputs(shape)
            cache[shape] = (x, wp) + G.e32_per_tensor(weights, x, wp)
        return cache[shape]
    return get


@pytest.fixture(scope="module")
def native(dev, ext, images, case, weights):
    """(shape, mode) -> the native training forward and backward of the case, and the float64 gradient under the native masks"""
    cache = {}

    def get(shape, mode):
        if (shape, mode) not in cache:
            x, wp = case(shape)[:2]
            B, D, H, W = shape
            xt, gt = torch.from_numpy(x).to(dev), torch.from_numpy(wp).to(dev)
            p, tape = ext.multiscale3d_forward_train(images[0], xt, mode)
            grad = ext.multiscale3d_backward(images[1], gt, tape, mode)
            tape_np = tape.cpu().numpy()
            layout = ext.multiscale3d_tape_layout(B, D, H, W)
            g64, _, _ = G.gradients(weights, x, wp, masks=G.masks_from_tape(tape_np, layout, B))
            cache[(shape, mode)] = dict(xt=xt, gt=gt, p=p, tape=tape, tape_np=tape_np, layout=layout, grad=grad, g64=g64)
        return cache[(shape, mode)]
    return get


def _check_grads(got, g64, e32, label, skip=(), own=None):
    worst, per = G.worst_rel(got, g64, skip)
    k = max(per, key=per.get)
    print(f"\nCNN3D_GRAD_ERR {label} {k} {worst:.3e} e32 {e32:.3e} ratio {worst / e32:.2f} median {np.median(list(per.values())):.3e}")
    if own is not None:
        r = {t: per[t] / max(own[t], OWN_FLOOR) for t in per if t.endswith(".weight")}
        t = max(r, key=r.get)
        print(f"CNN3D_GRAD_OWN {label} worst weight tensor {t} {per[t]:.3e} / max(own {own[t]:.3e}, {OWN_FLOOR:g}) = {r[t]:.2f}")
        sharp = {t: v for t, v in r.items() if not v <= FACTOR}
        assert not sharp, f"{label}: weight tensors beyond {FACTOR:g} x their own float32 error: {sharp}"
    bad = {k: v for k, v in per.items() if not v <= FACTOR * e32}
    assert not bad, f"{label}: beyond {FACTOR:g} x e32 = {FACTOR * e32:.3e}: {bad}"


def _check_zero_taps(got, shape, label):
    dead = G.structural_zero_taps(shape)
    assert bool(dead) == (shape == G.S1)
    for k, m in dead.items():
        v = got[k][:, :, m]
        assert v.size and not v.any(), f"{label}: {k} has {int(np.count_nonzero(v))} non-zero gradients at taps that only see padding"


@pytest.mark.parametrize("shape,mode", CASES, ids=CASE_IDS)
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
    want = {name: (keep[int(name[1:])] if name[0] == "y" else keep[name]).numpy() for name in views}
    worst = max(float(np.abs(views[k] - want[k]).max() / np.abs(want[k]).max()) for k in views)
    print(f"\nCNN3D_TAPE_ERR {_id(shape)} {mode} worst entry {worst:.3e}")
    for name, got in views.items():
        assert_close_rel(got, want[name], 1e-5, f"tape entry {name} {_id(shape)} {mode}")


@pytest.mark.parametrize("shape,mode", CASES, ids=CASE_IDS)
def test_backward_vs_masked_fp64(case, native, shape, mode):
    n = native(shape, mode)
    got = G.split_blob(n["grad"].cpu().numpy(), 3)
    _check_zero_taps(got, shape, f"{_id(shape)} {mode}")
    _check_grads(got, n["g64"], case(shape)[2], f"{_id(shape)} {mode}", own=case(shape)[3])


@pytest.mark.parametrize("shape", G.GPU_SHAPES[3], ids=_id)
def test_plain_weight_gradient_kernel_agrees(ext, images, case, native, shape):
    """multiscale3d_backward_plain: the thin layers' kernel for every layer -- the same bound, and an independent check of the MFMA kernel"""
    n = native(shape, "fp32")
    got = G.split_blob(ext.multiscale3d_backward_plain(images[1], n["gt"], n["tape"], "fp32").cpu().numpy(), 3)
    _check_zero_taps(got, shape, f"{_id(shape)} fp32 plain")
    _check_grads(got, n["g64"], case(shape)[2], f"{_id(shape)} fp32 plain", own=case(shape)[3])


@pytest.mark.parametrize("shape,mode", CASES, ids=CASE_IDS)
def test_backward_is_reproducible_and_leaves_its_inputs(ext, images, native, case, shape, mode):
    n = native(shape, mode)
    again = ext.multiscale3d_backward(images[1], n["gt"], n["tape"], mode)
    assert_bitexact(again.cpu().numpy(), n["grad"].cpu().numpy(), "second backward call")
    B = shape[0]
    entries = lambda t: G.tape_views(t, n["layout"], B).items()            # (the padding between entries is not part of the tape)
    for (name, a), (_, b) in zip(entries(n["tape"].cpu().numpy()), entries(n["tape_np"])):
        assert_bitexact(a, b, f"tape entry {name} after the backward")
    assert_bitexact(n["gt"].cpu().numpy(), case(shape)[1], "grad_p after the backward")
    assert_bitexact(n["xt"].cpu().numpy(), case(shape)[0], "x after the backward")


# Past the Winograd kernels' fill thresholds.  At S1 and S2 every launch of the MFMA family is too small for them, so all modes run the
# implicit-GEMM kernel there; real training shapes run F(4x4) / F(2x2) for the input gradients.  At (2, 32, 64, 64) the full-resolution
# tower has 2 x 4 x 64 = 512 F(4x4) tiles per 64 output channels (threshold: one per CU) and 2 x 8 x 64 = 1024 F(2x2) tiles per 32 or
# 64 output channels (thresholds 1024 and 512), so `fp32` runs F(4x4) where Cout % 64 == 0 and F(2x2) elsewhere, and `fp32_f2` F(2x2).
BIG = (2, 32, 64, 64)


@pytest.fixture(scope="module")
def big(dev, ext, images):
    """one fp32_direct training forward at BIG and, on that one tape, the backward in each mode and with the plain weight gradient"""
    x, wp = G.case_inputs(BIG)
    xt, gt = torch.from_numpy(x).to(dev), torch.from_numpy(wp).to(dev)
    p, tape = ext.multiscale3d_forward_train(images[0], xt, "fp32_direct")
    grads = {m: G.split_blob(ext.multiscale3d_backward(images[1], gt, tape, m).cpu().numpy(), 3) for m in ("fp32_direct", "fp32", "fp32_f2")}
    grads["plain"] = G.split_blob(ext.multiscale3d_backward_plain(images[1], gt, tape, "fp32_direct").cpu().numpy(), 3)
    return dict(xt=xt, grads=grads)


@pytest.mark.parametrize("mode", ["fp32", "fp32_f2", "plain"])
def test_winograd_input_gradients_on_one_tape(case, big, mode):
    """The input-gradient convolutions through the forward's F(4x4) / F(2x2) launchers on packed3d_t (the Winograd images of the
    transposed, tap-flipped 3x3x3 weights), and the plain weight-gradient kernel, against the `fp32_direct` backward on the SAME tape
    and the same grad_p: the ReLU masks and every weight-gradient launch are then identical, and the modes differ in the arithmetic of
    the input-gradient convolutions alone (`plain`: of the weight gradients alone).

    Bound: 8 e32 per tensor, e32 the float32 yardstick of S2.  The float64 model of this shape would cost about a TFLOP on the CPU per
    run; e32 is the relative rounding of float32 sums whose terms have random signs (error and sum both grow with the square root of
    their length), so it does not grow with the grid, and S2 is the larger of the two shapes where it is measured (1.1e-5; S1 3.0e-6).
    The `fp32_direct` backward itself is held to the float64 model at S1 and S2, where it runs the same kernels as here.  A wrong
    offset or pack argument in the Winograd images gives errors of order 1, not 1e-5."""
    e32 = case(G.S2)[2]
    ref, got = big["grads"]["fp32_direct"], big["grads"][mode]
    worst, per = G.worst_rel(got, ref)
    k = max(per, key=per.get)
    print(f"\nCNN3D_WINO {_id(BIG)} {mode} against fp32_direct on one tape: worst {k} {worst:.3e} e32(S2) {e32:.3e} ratio {worst / e32:.2f}")
    bad = {k: v for k, v in per.items() if not v <= FACTOR * e32}
    assert not bad, f"{mode}: beyond {FACTOR:g} x e32 = {FACTOR * e32:.3e} of the fp32_direct backward: {bad}"
    # another path did run: the Winograd kernels (the fp64 plain sums) do not give the implicit GEMM's (the MFMA kernel's) bits
    assert any(not np.array_equal(got[k], ref[k]) for k in G.PARAM_NAMES), f"{mode} gave the fp32_direct backward's bits in every tensor"


def test_winograd_training_forward_has_the_inference_bits(dev, ext, images, weights, big):
    """the taped forward through the F(4x4) / F(2x2) launches at BIG: p is the inference forward's"""
    from fluidnet_cxx_amd import FluidNet
    for mode in ("fp32", "fp32_f2"):
        p, _ = ext.multiscale3d_forward_train(images[0], big["xt"], mode)
        inf = FluidNet.from_weights(_mconf(mode), weights, dev)
        assert_bitexact(p.cpu().numpy(), inf.multiScale(big["xt"]).cpu().numpy(), f"training forward p {_id(BIG)} {mode}")


def _joints(shape):
    q, h = G.tower_sizes(shape[1:])
    return [(q, h), (h, list(shape[1:]))]


@pytest.mark.parametrize("src,dst", _joints(G.S1) + _joints(G.S2), ids=lambda v: _id(v))
def test_trilinear_adjoint(dev, ext, src, dst):
    """The adjoint of the one-channel trilinear upsampling at the four tower joints against the float64 transpose of resample's
    interpolation matrices; e32: the same transpose applied in float32 by torch on the CPU."""
    B = 2
    gd = np.random.default_rng(21).standard_normal([B, 1] + list(dst)).astype(np.float32)

    def transpose(dtype):
        t = torch.from_numpy(gd).to(dtype)
        for ax in range(3):
            m = torch.from_numpy(_axis_weights(src[ax], dst[ax])).to(dtype)            # (n_out, n_in)
            t = torch.movedim(torch.tensordot(t, m, dims=([2 + ax], [0])), -1, 2 + ax)
        return t.double().numpy()
    g64, g32 = transpose(torch.float64), transpose(torch.float32)
    e32 = float(np.abs(g32 - g64).max() / np.abs(g64).max())
    got = ext.trilinear_upsample_backward(torch.from_numpy(gd).to(dev), list(src)).cpu().numpy()
    err = float(np.abs(got - g64).max() / np.abs(g64).max())
    print(f"\nCNN3D_ADJOINT {_id(src)} <- {_id(dst)} err {err:.3e} e32 {e32:.3e} ratio {err / e32:.2f}")
    assert got.shape == g64.shape and err <= FACTOR * e32


@pytest.fixture(scope="module")
def fluid_case():
    return G.fluidnet_case(G.S1)


@pytest.mark.parametrize("mode", ["fp32", "fp32_f2", "fp32_direct"])
def test_fluidnet_level_gradients(dev, ext, weights, fluid_case, mode):
    """loss = sum(w_p p) + sum(w_U U) on flags with an interior obstacle box: (p, U) has the inference FluidNet's bits, and the parameter
    gradients are the float64 chain's (div, unbiased-std scale, net, velocityUpdate, unscale, setWallBcs) under the native masks"""
    from fluidnet_cxx_amd import FluidNet, FluidNetTrain3D
    inp_np, w_p, w_U = fluid_case
    B, D, H, W = G.S1
    inp = torch.from_numpy(inp_np).to(dev)
    net = FluidNetTrain3D(_mconf(mode))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    net.to(dev)
    p, U = net(inp)
    assert p.requires_grad and U.requires_grad
    ((p * torch.from_numpy(w_p).to(dev)).sum() + (U * torch.from_numpy(w_U).to(dev)).sum()).backward()
    inf = FluidNet.from_weights(_mconf(mode), weights, dev)
    p_inf, U_inf = inf(inp)
    assert_bitexact(p.detach().cpu().numpy(), p_inf.cpu().numpy(), "p of FluidNetTrain3D and FluidNet")
    assert_bitexact(U.detach().cpu().numpy(), U_inf.cpu().numpy(), "U of FluidNetTrain3D and FluidNet")
    # the same forward through the extension, for the tape and the scale (deterministic: the same bits)
    p2, U2, tape, scale, flags2 = ext.fluidnet3d_forward_train(net.packed, inp, 1e-5, mode)
    assert_bitexact(p2.cpu().numpy(), p.detach().cpu().numpy(), "p of the two forwards")
    assert_bitexact(U2.cpu().numpy(), U.detach().cpu().numpy(), "U of the two forwards")
    assert_bitexact(flags2.cpu().numpy(), inp_np[:, 4:5], "flags channel")
    layout = ext.multiscale3d_tape_layout(B, D, H, W)
    tape_np = tape.cpu().numpy()
    x_net = G.tape_views(tape_np, layout, B)["in1"][:, 0:2].copy()      # resampling to the same size is the identity
    sc = scale.cpu().numpy()
    # the float64 chain's own scale and net input agree with the native ones to float32 rounding; it then takes the native ones
    with torch.no_grad():
        keep = {}
        G.fluidnet_forward(G.as_params(weights, requires_grad=False), inp_np, keep=keep)
    assert_close_rel(x_net, keep["in1"][:, 0:2].numpy(), 1e-5, "the net's input")
    e32, _ = G.fluidnet_e32(weights, inp_np, w_p, w_U, x_net=x_net, scale=sc)
    g64, (p64, U64), _ = G.fluidnet_gradients(weights, inp_np, w_p, w_U, masks=G.masks_from_tape(tape_np, layout, B), x_net=x_net, scale=sc)
    assert_close_rel(p.detach().cpu().numpy(), p64, 1e-5, "p against the float64 chain")
    assert_close_rel(U.detach().cpu().numpy(), U64, 1e-5, "U against the float64 chain")
    got = {k: v.grad.cpu().numpy() for k, v in net.named_parameters()}
    _check_zero_taps(got, G.S1, f"fluidnet {mode}")
    _check_grads(got, g64, e32, f"fluidnet {_id(G.S1)} {mode}")


def test_short_training_run(dev, weights):
    """8 steps of plain SGD at rate 1e-4 on mean((p - t)^2) at S1, natively and with the float64 model (free ReLU: the loss is continuous
    across a flip).  On the CPU the float64 loss goes 1.20512 -> 1.12257, falling at every step.  Bound on the final loss: 2 mean|p - t|
    1e-5 |p|max (float64 values of the last step) -- what the forward tolerance 1e-5 |ref|max allows the loss to move if every voxel
    erred the same way (the 2D test's bound)."""
    from fluidnet_cxx_amd import FluidNet, FluidNetTrain3D
    B, D, H, W = G.S1
    x = net_input(B, D, H, W, seed=3)
    t = np.random.default_rng(9).standard_normal((B, 1, D, H, W))
    lr, steps = 1e-4, 8
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
    net = FluidNetTrain3D(_mconf("fp32"))
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
    print("\nCNN3D_TRAIN_LOSS float64 " + " ".join(f"{v:.6f}" for v in ref))
    print("CNN3D_TRAIN_LOSS native  " + " ".join(f"{v:.6f}" for v in got))
    print(f"CNN3D_TRAIN_LOSS |final difference| {abs(got[-1] - ref[-1]):.3e} bound {bound:.3e}")
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


@pytest.mark.parametrize("fused", [True, False])
def test_simulate_under_no_grad_with_the_training_net(dev, weights, fused):
    """Three convnet steps of a 3D plume with a FluidNetTrain3D in train() mode under no_grad: the bits of the same steps through a
    FluidNet loaded from its state_dict."""
    from fluidnet_cxx_amd import FluidNet, FluidNetTrain3D, simulate
    from util import PLUME_CFG, plume_state
    mconf = dict(PLUME_CFG, **_mconf("fp32"))
    net = FluidNetTrain3D(mconf)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    net.to(dev).train()
    inf = FluidNet(mconf, dropout=False)
    inf.load_state_dict(net.state_dict())
    inf.to(dev)
    a = {k: torch.from_numpy(v).to(dev) for k, v in plume_state(24, D=12).items()}
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
    """packed and packed3d_t look alike and differ in size: a swapped pair is an error before anything is launched"""
    x = torch.zeros(1, 2, 8, 8, 8, device=dev)
    with pytest.raises(RuntimeError, match="swapped"):
        ext.multiscale3d_forward_train(images[1], x, "fp32")
    _, tape = ext.multiscale3d_forward_train(images[0], x, "fp32")
    with pytest.raises(RuntimeError, match="swapped"):
        ext.multiscale3d_backward(images[0], torch.zeros(1, 1, 8, 8, 8, device=dev), tape, "fp32")
    with pytest.raises(RuntimeError, match="swapped"):
        ext.fluidnet3d_forward_train(images[1], torch.zeros(1, 6, 8, 8, 8, device=dev), 1e-5, "fp32")


def test_out_of_scope_cases_raise(dev, ext, images):
    from fluidnet_cxx_amd import FluidNetTrain3D
    with pytest.raises(RuntimeError, match="3D only"):
        ext.multiscale3d_forward_train(images[0], torch.zeros(1, 2, 16, 16, device=dev), "fp32")
    with pytest.raises(RuntimeError, match="3D only"):
        ext.multiscale3d_forward_train(images[0], torch.zeros(1, 2, 1, 16, 16, device=dev), "fp32")
    with pytest.raises(RuntimeError, match="3D only"):
        ext.fluidnet3d_forward_train(images[0], torch.zeros(1, 5, 1, 16, 16, device=dev), 1e-5, "fp32")
    x = torch.zeros(1, 2, 8, 8, 8, device=dev)
    _, tape = ext.multiscale3d_forward_train(images[0], x, "fp32")
    with pytest.raises(RuntimeError, match="3D only"):
        ext.multiscale3d_backward(images[1], torch.zeros(1, 1, 16, 16, device=dev), tape, "fp32")
    for mode in ("bf16x6", "bf16x3"):
        with pytest.raises(RuntimeError, match="fp32 arithmetic only"):
            ext.multiscale3d_forward_train(images[0], x, mode)
        with pytest.raises(RuntimeError, match="fp32 arithmetic only"):
            ext.multiscale3d_backward(images[1], torch.zeros(1, 1, 8, 8, 8, device=dev), tape, mode)
    net = FluidNetTrain3D(_mconf("fp32")).to(dev)
    with pytest.raises(RuntimeError, match="requires_grad"):
        net(torch.zeros(1, 6, 8, 8, 8, device=dev, requires_grad=True))
    with pytest.raises(RuntimeError, match="requires_grad"):
        net.multiScale(torch.zeros(1, 2, 8, 8, 8, device=dev, requires_grad=True))
