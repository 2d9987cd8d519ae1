"""The 3D training loop on the GPU: the loss kernel against a float64 model (tests/train_reference.py), its composition with
FluidNetTrain3D, the online sampler, a short Adam run against a CPU model of the same loop, the long-term term, reproducibility and
resume, and the use of the checkpoint."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import poisson_reference as PR
import scene_reference as S3
import train_reference as T3
from util import assert_bitexact, random_state

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 8.0                                                 # the suite's rule (tests/test_training_gpu.py)
LAMBDAS = {"reference": (0.0, 1.0, 0.0, 0.0), "all_terms": (1.0, 1.0, 0.5, 0.5)}     # those of tests/test_training_gpu.py
# scene parameters scaled to the 16-cell grids of these tests
SCENE = dict(S3.DEFAULTS[3], wavelength=8.0, octaves=2)
# the short training run: K Adam iterations at rate LR on 16^3, B = 2 (see test_training_lowers_the_held_out_divergence)
K, LR = 24, 3e-4
CPU_BEGIN, CPU_END = 9.209267e-02, 1.686494e-03      # the CPU model's held-out divL2 before and after (see the test's docstring)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    from fluidnet_cxx_amd._ext import ext
    return ext


def T(a, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(dev)


def _mconf(**kw):
    from fluidnet_cxx_amd.training3d import MCONF3D_DEFAULTS
    return dict(MCONF3D_DEFAULTS, **kw)


# ---- the loss ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loss_case():
    """(B,D,H,W) = (2, 6, 10, 70) of util.random_state(boxes=True).  make_flags places its boxes from 12 cells per axis on only, so at
    H = 10 the state has none: one box is added here, so that obstacle cells inside the shell take part as the issue of the boxes asks."""
    B, D, H, W = 2, 6, 10, 70
    s = random_state(B, D, H, W, 0.5, seed=13, boxes=True)
    s["flags"][:, :, 2:4, 3:6, 20:41] = 2.0
    s["flags"][1, :, 4, 7, 66] = 2.0
    t = np.random.default_rng(17).standard_normal((B, 1, D, H, W)).astype(np.float32)
    return s, t


@pytest.mark.parametrize("lam", list(LAMBDAS))
def test_loss_against_float64(dev, ext, loss_case, lam):
    from fluidnet_cxx_amd import fluid
    from fluidnet_cxx_amd.training3d import fluidnet_loss3d
    s, t = loss_case
    B, _, D, H, W = s["p"].shape
    lams = LAMBDAS[lam]
    use_t = lams[0] != 0 or lams[2] != 0
    v64, gp64, gU64 = T3.loss_and_gradients(s["p"], s["U"], s["flags"], t, lams, torch.float64)
    v32, gp32, gU32 = T3.loss_and_gradients(s["p"], s["U"], s["flags"], t, lams, torch.float32)
    p = T(s["p"], dev).requires_grad_(True)
    U = T(s["U"], dev).requires_grad_(True)
    flags = T(s["flags"], dev)
    total, terms = fluidnet_loss3d(p, U, flags, T(t, dev) if use_t else None, lams)
    assert not terms.requires_grad and total.requires_grad
    total.backward()
    got = np.array(terms.cpu().tolist() + [float(total)], np.float64)
    live = [i for i in range(5) if (use_t or i in (1, 3, 4))]          # without a target the two pressure terms are reported as 0
    rel = lambda a: max(abs(a[i] - v64[i]) / abs(v64[i]) for i in live)
    e32_v, err_v = rel(v32), rel(got)
    print(f"\nTRAIN3D_LOSS_ERR {lam} value: native {err_v:.3e} torch-float32 {e32_v:.3e} ratio {err_v / max(e32_v, 1e-300):.2f}")
    if not use_t:
        assert got[0] == 0 and got[2] == 0
    gmax = lambda a: float(np.abs(a).max())
    e32_U, err_U = gmax(gU32 - gU64) / gmax(gU64), gmax(U.grad.cpu().numpy() - gU64) / gmax(gU64)
    print(f"TRAIN3D_LOSS_ERR {lam} grad_U: native {err_U:.3e} torch-float32 {e32_U:.3e} ratio {err_U / e32_U:.2f}")
    if use_t:
        e32_p, err_p = gmax(gp32 - gp64) / gmax(gp64), gmax(p.grad.cpu().numpy() - gp64) / gmax(gp64)
        print(f"TRAIN3D_LOSS_ERR {lam} grad_p: native {err_p:.3e} torch-float32 {e32_p:.3e} ratio {err_p / e32_p:.2f}")
    assert err_v <= FACTOR * e32_v
    assert err_U <= FACTOR * e32_U
    if use_t:
        assert err_p <= FACTOR * e32_p
    else:
        assert not np.any(p.grad.cpu().numpy()), "grad_p must be exactly 0 when both pressure lambdas are 0"
    # exactly 0 where the divergence is exactly 0: a face both of whose cells have div == 0
    div = fluid.velocityDivergence(U.detach(), flags).cpu().numpy()
    z = (div == 0)[:, 0]
    assert z.sum() > B * 2 * (D * H + D * (W - 2) + (H - 2) * (W - 2))
    g = U.grad.cpu().numpy()
    for a, ax in ((0, 3), (1, 2), (2, 1)):
        za = z.copy()
        lo, hi = [slice(None)] * 4, [slice(None)] * 4
        lo[ax], hi[ax] = slice(1, None), slice(0, -1)
        za[tuple(lo)] &= z[tuple(hi)]
        assert not np.any(g[:, a][za]) and np.any(g[:, a][~za]), a
    # the divergence the loss implies is velocityDivergence's, bit for bit: with divL1 alone the total is the mean of |div|, whose fp64
    # sum over the B D H W = 8400 cells the kernel forms from the very float32 values, so the host's fp64 sum of |velocityDivergence|
    # agrees to the rounding of 8400 fp64 additions (8400 * 2^-53 relative) and of the conversion of the mean to float32 (2^-24)
    l1 = ext.train_loss3d(p.detach(), U.detach(), flags, None, [0.0, 0.0, 0.0, 1.0], None, True)[0].cpu().numpy().astype(np.float64)
    want_l1 = np.abs(div.astype(np.float64)).sum() / div.size
    want_l2 = (div.astype(np.float64) ** 2).sum() / div.size
    assert np.float32(want_l1) == np.float32(l1[3]) or abs(l1[3] - want_l1) <= 2.0 ** -23 * want_l1
    assert abs(l1[1] - want_l2) <= 2.0 ** -23 * want_l2 and abs(l1[4] - want_l1) <= 2.0 ** -23 * want_l1
    if not use_t:
        # ... and cell by cell: with divL2 alone dL/d div is fl(fl(2 / N) * div), so grad_U must be the float32 differences of that
        # product formed from velocityDivergence's values, bit for bit (== : a -0 of the masked product equals the kernel's +0)
        gd = np.float32(2.0 / div.size) * div[:, 0]
        for a, ax in ((0, 3), (1, 2), (2, 1)):
            prev = np.zeros_like(gd)
            lo, hi = [slice(None)] * 4, [slice(None)] * 4
            lo[ax], hi[ax] = slice(1, None), slice(0, -1)
            prev[tuple(lo)] = gd[tuple(hi)]
            assert np.array_equal(g[:, a], gd - prev), f"grad_U component {a} from velocityDivergence's bits"
    # two calls, the same bits; a weight on the total scales the gradient through the kernel
    p2, U2 = p.detach().clone().requires_grad_(True), U.detach().clone().requires_grad_(True)
    total2, terms2 = fluidnet_loss3d(p2, U2, flags, T(t, dev) if use_t else None, lams)
    total2.backward()
    assert_bitexact(terms2.cpu().numpy(), terms.cpu().numpy(), "terms of a second call")
    assert_bitexact(total2.detach().cpu().numpy(), total.detach().cpu().numpy(), "total of a second call")
    assert_bitexact(U2.grad.cpu().numpy(), U.grad.cpu().numpy(), "grad_U of a second call")
    assert_bitexact(p2.grad.cpu().numpy(), p.grad.cpu().numpy(), "grad_p of a second call")
    terms5, gp3, gU3 = ext.train_loss3d(p.detach(), U.detach(), flags, T(t, dev) if use_t else None, list(lams),
                                        torch.full((1,), 0.5, device=dev), True)
    assert_bitexact(terms5[:4].cpu().numpy(), terms.cpu().numpy(), "terms of the fused call")
    assert_bitexact(gU3.cpu().numpy(), 0.5 * U.grad.cpu().numpy(), "grad_U under an upstream of 0.5")
    assert_bitexact(gp3.cpu().numpy(), 0.5 * p.grad.cpu().numpy(), "grad_p under an upstream of 0.5")
    with pytest.raises(RuntimeError, match="target_p is null"):
        ext.train_loss3d(p.detach(), U.detach(), flags, None, [1.0, 1.0, 0.0, 0.0], None, True)
    with pytest.raises(RuntimeError, match="3D only"):
        ext.train_loss3d(p.detach()[:, :, :1].contiguous(), U.detach()[:, :2, :1].contiguous(), flags[:, :, :1].contiguous(), None,
                         [0.0, 1.0, 0.0, 0.0], None, True)


def test_loss_composes_with_the_training_net(dev, ext):
    """fluidnet_loss3d(net(data)).backward() gives the parameter gradients of ((p * g_p).sum() + (U * g_U).sum()).backward() with
    (g_p, g_U) from ext.train_loss3d on the same outputs, bit for bit (the net's backward against float64: tests/test_cnn_train3d_gpu.py)"""
    import cnn_grad_reference as G3
    from fluidnet_cxx_amd import FluidNetTrain3D
    from fluidnet_cxx_amd.training import kaiming_init
    from fluidnet_cxx_amd.training3d import fluidnet_loss3d
    inp = G3.fluidnet_case((2, 8, 12, 16))[0]
    data = T(inp, dev)
    flags = data[:, 4:5].contiguous()
    lam = [1.0, 1.0, 0.5, 0.5]
    tp = T(np.random.default_rng(5).standard_normal((2, 1, 8, 12, 16)).astype(np.float32), dev)
    net = kaiming_init(FluidNetTrain3D(_mconf()), 3).to(dev).train()
    p, U = net(data)
    total, _ = fluidnet_loss3d(p, U, flags, tp, lam)
    total.backward()
    got = {k: v.grad.detach().cpu().numpy().copy() for k, v in net.named_parameters()}
    assert all(np.isfinite(g).all() for g in got.values()) and sum(bool(np.any(g)) for g in got.values()) == len(got)
    _, g_p, g_U = ext.train_loss3d(p.detach(), U.detach(), flags, tp, lam, torch.ones(1, device=dev), False)
    net.zero_grad()
    p2, U2 = net(data)
    ((p2 * g_p).sum() + (U2 * g_U).sum()).backward()
    for k, v in net.named_parameters():
        assert_bitexact(v.grad.detach().cpu().numpy(), got[k], k)


# ---- the sampler ------------------------------------------------------------------------------------------------------------------------
SAMPLER_SEED = 3


def _sampler(dev, seed=SAMPLER_SEED, B=4, dims=(16, 16, 24), **kw):
    from fluidnet_cxx_amd.training3d import SceneSampler3D
    return SceneSampler3D(_mconf(), B, dims[0], dims[1], dims[2], seed, dev, scene=SCENE, **kw)


def test_sampler_batches(dev, ext):
    """Every scene drawn here has one fluid component (the solver does not converge on sealed pockets): checked on the
    CPU with scene_reference.obstacles and scipy.ndimage.label for the ids 0 .. 47 of seed 3 at (16, 16, 24); the three calls draw the
    ids 0 .. 5."""
    from fluidnet_cxx_amd import fluid
    B, (D, H, W) = 4, (16, 16, 24)
    s = _sampler(dev, sceneLength=8, stride=1)
    assert s.age == [0, 2, 4, 6] and s.scene_id == list(range(B))
    for call in range(3):
        data, target = s.next()
        assert data.shape == (B, 6, D, H, W) and target.shape == (B, 5, D, H, W) and data.is_contiguous() and target.is_contiguous()
        d, t = data.cpu().numpy(), target.cpu().numpy()
        flags = d[:, 4:5]
        assert set(np.unique(flags)) <= {1.0, 2.0}
        assert_bitexact(flags, S3.obstacles(SAMPLER_SEED, s.scene_id, (D, H, W), **SCENE), "flags in data and of the numpy model")
        assert_bitexact(flags, s.bd["flags"].cpu().numpy(), "flags in data and in the scene")
        assert_bitexact(d[:, 5], t[:, 4], "density in data and target")
        assert_bitexact(t[:, 0:1], s.bd["p"].cpu().numpy(), "target p is the scene's p")
        assert_bitexact(t[:, 1:4], s.bd["U"].cpu().numpy(), "target U is the scene's U")
        assert d[:, 5].min() >= 0 and d[:, 5].max() <= 1 and d[:, 5].max() > 0
        div_in = fluid.velocityDivergence(data[:, 1:4].contiguous(), data[:, 4:5].contiguous()).cpu().numpy()
        assert np.abs(div_in).max() > 1e-3, "data's U must be divergent"
        # target: the float64 residual of the projection's p, as tests/test_pcg_gpu.py accepts it in 3D for pcgTol = 1e-5 (3e-5)
        p = t[:, 0:1].astype(np.float64)
        bproj = PR.project(flags, div_in, True)
        for b in range(B):
            r = bproj[b] - PR.apply(flags[b:b + 1], p[b:b + 1], True)[0]
            A, a = PR.matrix(flags[b, 0], True)
            act = a.reshape(r.shape)
            if PR.is_singular(A, a):
                r = np.where(act, r - r[act].mean(), 0.0)
            rel = np.linalg.norm(r) / np.linalg.norm(bproj[b])
            print(f"SAMPLER3D_RESIDUAL call {call} slot {b} scene {s.scene_id[b]} {rel:.2e}")
            assert rel <= 3e-5, (call, b, rel)
        div_out = fluid.velocityDivergence(target[:, 1:4].contiguous(), data[:, 4:5].contiguous()).cpu().numpy()
        assert np.linalg.norm(div_out) <= 1e-3 * np.linalg.norm(div_in)
    assert s.scene_id == [0, 1, 5, 4]


def test_redraw_replaces_exactly_the_due_slots(dev, ext):
    s = _sampler(dev, sceneLength=8, stride=1)
    s.next()                                                  # ages 2, 4, 6, 8
    assert s.age == [2, 4, 6, 8]
    before = {k: v.clone() for k, v in s.bd.items()}
    assert s.redraw_due() == [3] and s.scene_id == [0, 1, 2, 4] and s.age == [2, 4, 6, 0]
    flags4, U4, rho4 = s.draw([4])
    for k in before:
        assert_bitexact(s.bd[k][:3].cpu().numpy(), before[k][:3].cpu().numpy(), f"{k} of the slots that were not due")
    assert_bitexact(s.bd["flags"][3].cpu().numpy(), flags4[0].cpu().numpy(), "flags of the redrawn slot")
    assert_bitexact(s.bd["density"][3].cpu().numpy(), rho4[0].cpu().numpy(), "density of the redrawn slot")
    assert not torch.equal(s.bd["U"][3], before["U"][3])
    assert s.redraw_due() == []


def test_one_seed_gives_the_same_batches(dev):
    a, b = _sampler(dev, sceneLength=4, stride=1), _sampler(dev, sceneLength=4, stride=1)
    c = _sampler(dev, seed=4, sceneLength=4, stride=1)
    differs = False
    for call in range(4):                                     # every slot is redrawn at least once
        da, ta = a.next()
        db, tb = b.next()
        dc, _ = c.next()
        assert_bitexact(da.cpu().numpy(), db.cpu().numpy(), f"data of call {call}")
        assert_bitexact(ta.cpu().numpy(), tb.cpu().numpy(), f"target of call {call}")
        assert a.last_choice == b.last_choice
        differs |= not torch.equal(da, dc)
    assert differs and a.next_id >= 2 * a.B and a.scene_id == b.scene_id
    # the state travels through a checkpoint
    sd = a.state_dict()
    d = _sampler(dev, sceneLength=4, stride=1)
    d.load_state_dict(sd)
    assert_bitexact(d.next()[0].cpu().numpy(), a.next()[0].cpu().numpy(), "data after load_state_dict")
    choices = [a.choices(i) for i in range(64)]
    seen = {tuple(ch["gravityVec"][k] for k in ("x", "y", "z")) for ch in choices}
    assert seen == {(1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)}
    assert 5 <= sum(ch["buoyancyScale"] > 0 for ch in choices) <= 35 and all(ch["dt"] >= 0.02028 for ch in choices)


# ---- training ---------------------------------------------------------------------------------------------------------------------------
TCONF = dict(res=16, batch=2, seed=11, sceneLength=16, stride=1, evalEvery=0, evalBatches=2, scene=SCENE)


def test_training_lowers_the_held_out_divergence(dev, ext):
    """K = 24 Adam iterations at rate 3e-4 on 16 x 16 x 16, B = 2, divL2 only (no long-term term), from the trainer's seeded Kaiming
    weights: the native held-out divL2 must fall by at least half of the relative fall of a CPU model of the same loop.
    Choice of K and the rate, on the CPU alone: a float32 torch model of the loop (train_reference.adam_run: the net of
    cnn_grad_reference, torch Adam) on train_reference.cpu_batches (scenes of the numpy model with SCENE, the oracle's 3D
    operators, poisson_reference; seed 11, 24 training batches, 2 held-out batches of seed 11 ^ 0x5eed5eed).  Its held-out divL2 falls
    from 9.209267e-02 to 1.686494e-03 (x 0.018; a relative fall of 0.982, far above the quarter asked for), so the native run must lose
    at least 0.491 of its own.  Tried next to it: (24, 1e-3) x 0.007, (40, 1e-4) x 0.034, (40, 3e-4) x 0.010.  The factor one half is a
    margin for batches that differ from the CPU model's (the sampler advances its scenes through the solver; the CPU batches are one
    advection after the projection), not a measured tolerance.  Every scene of both seeds (ids 0 .. 47) has one fluid component."""
    from fluidnet_cxx_amd import FluidNetTrain3D
    from fluidnet_cxx_amd.training import kaiming_init
    from fluidnet_cxx_amd.training3d import evaluate3d, train3d
    mconf = _mconf(divLongTermLambda=0.0, lr=LR)
    run = train3d(mconf, dict(TCONF, iters=K), dev)
    lam = [0.0, 1.0, 0.0, 0.0]
    end = evaluate3d(run["net"], run["held_out"], lam)["divL2_out"]
    begin = evaluate3d(kaiming_init(FluidNetTrain3D(mconf), TCONF["seed"]).to(dev), run["held_out"], lam)["divL2_out"]
    cpu_fall = 1.0 - CPU_END / CPU_BEGIN
    print(f"\nTRAIN3D_HELD_OUT divL2: native {begin:.6e} -> {end:.6e} (x{end / begin:.3f}); CPU model {CPU_BEGIN:.6e} -> {CPU_END:.6e} "
          f"(x{CPU_END / CPU_BEGIN:.3f})")
    print(f"TRAIN3D_LOSSES first {run['history'][0]['loss']:.6e} last {run['history'][-1]['loss']:.6e}")
    assert cpu_fall >= 0.25, "the CPU model must lose at least a quarter of its held-out divL2"
    assert end < begin
    assert 1.0 - end / begin >= 0.5 * cpu_fall


def _state_bits(run):
    return {k: v.cpu().numpy() for k, v in run["checkpoint"]["state_dict"].items()}


LT_TCONF = dict(TCONF, D=12)                                # (12, 16, 16)


def test_long_term_term_and_reproducibility(dev):
    """divLongTermLambda = 1 for 3 iterations at (12, 16, 16), B = 2: finite losses, every parameter tensor moves, two runs with one seed
    end in the same bits"""
    from fluidnet_cxx_amd import FluidNetTrain3D
    from fluidnet_cxx_amd.training import kaiming_init
    from fluidnet_cxx_amd.training3d import train3d
    mconf = _mconf(longTermDivNumSteps=[2, 4], longTermDivProbability=0.5)
    tconf = dict(LT_TCONF, iters=3)
    a = train3d(mconf, tconf, dev)
    b = train3d(mconf, tconf, dev)
    rows = a["history"]
    assert len(rows) == 3 and all(np.isfinite(r["loss"]) and r["lt"] is not None and np.isfinite(r["lt"]) and r["lt"] > 0 for r in rows)
    start = kaiming_init(FluidNetTrain3D(mconf), tconf["seed"]).state_dict()
    sa, sb = _state_bits(a), _state_bits(b)
    for k in sa:
        assert not np.array_equal(sa[k], start[k].detach().numpy()), f"{k} did not move"
        assert_bitexact(sa[k], sb[k], f"{k} of two runs with one seed")
    assert [r["loss"] for r in rows] == [r["loss"] for r in b["history"]]


def test_resume_and_the_checkpoint_in_use(dev, tmp_path):
    """4 iterations equal 2 + resume + 2 bit for bit; FluidNet with the checkpoint has the training net's forward bits, drives two
    convnet steps of the 3D plume with the bits of the training class under no_grad, and the plume driver takes it as --weights3d"""
    from fluidnet_cxx_amd import FluidNet, simulate
    from fluidnet_cxx_amd.training3d import train3d
    from util import PLUME_CFG, plume_state
    mconf = _mconf(longTermDivNumSteps=[1, 2])
    whole = train3d(mconf, dict(LT_TCONF, iters=4, evalEvery=2), dev)
    f, g = str(tmp_path / "half.pth"), str(tmp_path / "net3d.pth")
    half = train3d(mconf, dict(LT_TCONF, iters=2, evalEvery=2), dev, out=f)
    ck = torch.load(f, map_location="cpu", weights_only=False)
    assert {"state_dict", "optimizer", "mconf", "it"} <= set(ck) and ck["it"] == 2
    rest = train3d(mconf, dict(LT_TCONF, iters=4, evalEvery=2), dev, resume=f, out=g)
    sa, sb = _state_bits(whole), _state_bits(rest)
    for k in sa:
        assert_bitexact(sb[k], sa[k], f"{k}: resumed against uninterrupted")
    assert [r["loss"] for r in rest["history"]] == [r["loss"] for r in whole["history"]]
    assert [r.get("val") for r in rest["history"]] == [r.get("val") for r in whole["history"]]
    assert not np.array_equal(_state_bits(half)["multiScale.final.bias"], sa["multiScale.final.bias"])
    # the checkpoint in use
    ck = torch.load(g, map_location="cpu", weights_only=False)
    inf = FluidNet(ck["mconf"], dropout=False)
    inf.load_state_dict(ck["state_dict"])
    inf.to(dev)
    data = rest["held_out"][0][0]
    with torch.no_grad():
        p, U = rest["net"](data)
    p2, U2 = inf(data)
    assert_bitexact(p2.cpu().numpy(), p.cpu().numpy(), "p of FluidNet with the checkpoint")
    assert_bitexact(U2.cpu().numpy(), U.cpu().numpy(), "U of FluidNet with the checkpoint")
    cfg = dict(PLUME_CFG, **ck["mconf"])
    cfg.update(dt=PLUME_CFG["dt"], buoyancyScale=PLUME_CFG["buoyancyScale"], gravityVec=PLUME_CFG["gravityVec"])
    states = []
    for net in (inf, rest["net"]):
        bd = {k: torch.from_numpy(v).to(dev) for k, v in plume_state(24, D=12).items()}
        with torch.no_grad():
            for _ in range(2):
                simulate(cfg, bd, net, "convnet")
        states.append(bd)
    for k in ("p", "U", "density"):
        assert bool(torch.isfinite(states[0][k]).all())
        assert_bitexact(states[0][k].cpu().numpy(), states[1][k].cpu().numpy(), f"{k} after two convnet steps: FluidNet against FluidNetTrain3D")
    assert float(states[0]["U"].abs().max()) > 0
    out = tmp_path / "plume3d"
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "plume.py"), "--res", "24", "--depth", "12", "--iters", "2", "--out-iter", "1",
                        "--method", "convnet", "--weights3d", g, "--folder", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "It = 0" in r.stdout and any(n.endswith(".png") or n.endswith(".vtk") or n.endswith(".pth") for n in os.listdir(out)), os.listdir(out)
