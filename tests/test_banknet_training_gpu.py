"""The trainer with the 'FluidNet' bank model on the GPU (training.train with mconf['model'] = 'FluidNet'): a short Adam run against a
float64 yardstick built from tests/banknet_grad_reference.py, the long-term term, reproducibility, resume, the use of the checkpoint,
and that a ScaleNet run is what it was.  64 x 64, B = 8, seed 11, sceneLength 16, stride 1, as tests/test_training_gpu.py."""
import hashlib
import os
import struct
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import banknet_grad_reference as BG
import train_reference as TR
from util import assert_bitexact

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 8.0                                                 # the suite's rule (tests/test_cnn_train_gpu.py)
K, LR = 40, 1e-4
TCONF = dict(res=64, batch=8, seed=11, sceneLength=16, stride=1, evalEvery=0, evalBatches=2)
# sha256 of a two-iteration ScaleNet train() (scalenet_digest below), recorded at the commit before the bank trainer
SCALENET_DIGEST = "d8d1b394caf467e755f5339281449d3b114d7cb54d7b1a65aba6438e9d94b3df"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _mconf(**kw):
    from fluidnet_cxx_amd.training import MCONF_DEFAULTS
    return dict(MCONF_DEFAULTS, model="FluidNet", **kw)


def _state_bits(run):
    return {k: v.cpu().numpy() for k, v in run["checkpoint"]["state_dict"].items()}


def bank_kaiming_weights(seed):
    """the trainer's initial bank weights (training.kaiming_init over FluidNetBankTrain) as name -> float32 array, without the extension"""
    from fluidnet_cxx_amd.weights import make_banknet_weights
    w = make_banknet_weights(0)
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    for k in BG.PARAM_NAMES:
        if k.endswith(".weight"):
            t = torch.empty(w[k].shape, dtype=torch.float32)
            torch.nn.init.kaiming_uniform_(t, generator=gen)
            w[k] = t.numpy()
    return w


def _held_out(params, batches):
    dtype = next(iter(params.values())).dtype
    with torch.no_grad():
        v = [float(TR.div_l2(BG.fluidnet_forward(params, d)[1], TR._flags_of(d, dtype))) for d in batches]
    return sum(v) / len(v)


def bank_adam_run(weights, batches, held_out, lr, dtype):
    """TR.adam_run over the bank net's chain: (held-out divL2 before, after, the final parameters)"""
    params = BG.as_params(weights, dtype)
    opt = torch.optim.Adam(list(params.values()), lr=lr)
    first = _held_out(params, held_out)
    for data in batches:
        opt.zero_grad()
        TR.div_l2(BG.fluidnet_forward(params, data)[1], TR._flags_of(data, dtype)).backward()
        opt.step()
    return first, _held_out(params, held_out), params


def test_bank_training_against_float64(dev):
    """K = 40 Adam iterations at rate 1e-4, divL2 only, from the seeded Kaiming weights: the native run; a float64 and a float32 leg on
    the CPU (torch Adam over banknet_grad_reference's chain) on the very batches the native run drew.
    Allowed: |native - f64| <= 8 (|f32 - f64| + delta_eval) in the final held-out divL2, where delta_eval = |evaluate(FluidNet bank
    inference net holding the float64 leg's final weights) - the float64 model's figure for those weights| is the rounding of the
    held-out evaluation itself, measured with the inference forward and the loss kernel and none of the training code.  The float32
    twin alone is too lucky a yardstick: on CPU-made batches it ended 2.8e-10 from float64.  The float64 run's held-out divL2 must fall
    to at most three quarters (on CPU-made batches of seed 11: 6.362e-3 -> 1.534e-3, x 0.241)."""
    from fluidnet_cxx_amd import FluidNet, FluidNetBankTrain
    from fluidnet_cxx_amd.training import SceneSampler, evaluate, kaiming_init, train
    mconf = _mconf(divLongTermLambda=0.0, lr=LR)
    tconf = dict(TCONF, iters=K)
    t0 = time.time()
    run = train(mconf, tconf, dev)
    lam = [0.0, 1.0, 0.0, 0.0]
    held = run["held_out"]
    native_end = evaluate(run["net"], held, lam)["divL2_out"]
    again = SceneSampler(mconf, tconf["batch"], 64, 64, tconf["seed"], dev, None, tconf["sceneLength"], tconf["stride"])
    batches = [again.next()[0].cpu().numpy() for _ in range(K)]
    assert_bitexact(again.bd["U"].cpu().numpy(), run["sampler"].bd["U"].cpu().numpy(), "the replayed sampler's state")
    held_np = [d.cpu().numpy() for d, _ in held]
    t1 = time.time()
    w0 = bank_kaiming_weights(tconf["seed"])
    start = kaiming_init(FluidNetBankTrain(mconf), tconf["seed"])
    for k, v in start.state_dict().items():
        assert_bitexact(v.numpy(), w0[k], f"initial {k}")
    b64, e64, p64 = bank_adam_run(w0, batches, held_np, LR, torch.float64)
    t2 = time.time()
    b32, e32, _ = bank_adam_run(w0, batches, held_np, LR, torch.float32)
    t3 = time.time()
    native_begin = evaluate(start.to(dev), held, lam)["divL2_out"]
    inf = FluidNet.from_weights(mconf, {k: v.detach().to(torch.float32) for k, v in p64.items()}, dev)
    w64 = {k: v.detach().to(torch.float32).double() for k, v in p64.items()}           # the figure for the weights the net holds
    delta_eval = abs(evaluate(inf, held, lam)["divL2_out"] - _held_out(w64, held_np))
    d_native, d_f32 = abs(native_end - e64), abs(e32 - e64)
    print(f"\nBANK_TRAIN_F64 held-out divL2: float64 {b64:.6e} -> {e64:.6e} (x{e64 / b64:.3f})  float32 {b32:.6e} -> {e32:.6e}  "
          f"native {native_begin:.6e} -> {native_end:.6e}")
    print(f"BANK_TRAIN_F64 |native - f64| {d_native:.3e}  |f32 - f64| {d_f32:.3e}  delta_eval {delta_eval:.3e}  ratio "
          f"{d_native / max(d_f32 + delta_eval, 1e-300):.2f}   time: native {t1 - t0:.1f} s, float64 {t2 - t1:.1f} s, float32 {t3 - t2:.1f} s")
    assert e64 < b64 and native_end < native_begin
    assert e64 <= 0.75 * b64, "the float64 run's held-out loss must fall by at least a quarter"
    assert d_native <= FACTOR * (d_f32 + delta_eval)


def test_long_term_term_and_reproducibility(dev):
    """divLongTermLambda = 1, longTermDivNumSteps = [2, 4], five iterations: finite losses, each of the twelve tensors moves, two runs
    with one seed end in the same bits, another seed does not"""
    from fluidnet_cxx_amd import FluidNetBankTrain
    from fluidnet_cxx_amd.training import kaiming_init, train
    mconf = _mconf(divLongTermLambda=1.0, longTermDivNumSteps=[2, 4], longTermDivProbability=0.5)
    tconf = dict(TCONF, iters=5)
    a = train(mconf, tconf, dev)
    b = train(mconf, tconf, dev)
    assert type(a["net"]).__name__ == "FluidNetBankTrain"
    rows = a["history"]
    assert len(rows) == 5 and all(np.isfinite(r["loss"]) and r["lt"] is not None and np.isfinite(r["lt"]) and r["lt"] > 0 for r in rows)
    start = kaiming_init(FluidNetBankTrain(mconf), tconf["seed"]).state_dict()
    sa, sb = _state_bits(a), _state_bits(b)
    assert list(sa) == BG.PARAM_NAMES
    for k in sa:
        assert not np.array_equal(sa[k], start[k].detach().numpy()), f"{k} did not move"
        assert_bitexact(sa[k], sb[k], f"{k} of two runs with one seed")
    assert [r["loss"] for r in rows] == [r["loss"] for r in b["history"]]
    c = train(mconf, dict(tconf, seed=12), dev)
    assert not np.array_equal(_state_bits(c)["convOut.weight"], sa["convOut.weight"])


def test_resume_continues_with_the_same_bits(dev, tmp_path):
    from fluidnet_cxx_amd.training import train
    mconf = _mconf(longTermDivNumSteps=[1, 2])
    whole = train(mconf, dict(TCONF, iters=6, evalEvery=2), dev)
    f = str(tmp_path / "half.pth")
    half = train(mconf, dict(TCONF, iters=3, evalEvery=2), dev, out=f)
    ck = torch.load(f, map_location="cpu", weights_only=False)
    assert {"state_dict", "optimizer", "mconf", "it"} <= set(ck) and ck["it"] == 3 and ck["mconf"]["model"] == "FluidNet"
    rest = train(mconf, dict(TCONF, iters=6, evalEvery=2), dev, resume=f)
    sa, sb = _state_bits(whole), _state_bits(rest)
    for k in sa:
        assert_bitexact(sb[k], sa[k], f"{k}: resumed against uninterrupted")
    assert [r["loss"] for r in rest["history"]] == [r["loss"] for r in whole["history"]]
    assert [r.get("val") for r in rest["history"]] == [r.get("val") for r in whole["history"]]
    assert not np.array_equal(_state_bits(half)["convOut.bias"], sa["convOut.bias"])


def test_the_checkpoint_in_use(dev, tmp_path):
    """FluidNet(ck['mconf']) with the checkpoint has the training net's forward bits; three convnet plume steps run; the plume driver
    takes it"""
    from fluidnet_cxx_amd import FluidNet, simulate
    from fluidnet_cxx_amd.training import train
    from util import PLUME_CFG, plume_state
    f = str(tmp_path / "net.pth")
    run = train(_mconf(longTermDivNumSteps=[1, 2]), dict(TCONF, iters=3), dev, out=f)
    ck = torch.load(f, map_location="cpu", weights_only=False)
    inf = FluidNet(ck["mconf"], dropout=False)
    assert inf.is_bank
    inf.load_state_dict(ck["state_dict"])
    inf.to(dev)
    data = run["held_out"][0][0]
    with torch.no_grad():
        p, U = run["net"](data)
    p2, U2 = inf(data)
    assert_bitexact(p2.cpu().numpy(), p.cpu().numpy(), "p of FluidNet with the checkpoint")
    assert_bitexact(U2.cpu().numpy(), U.cpu().numpy(), "U of FluidNet with the checkpoint")
    bd = {k: torch.from_numpy(v).to(dev) for k, v in plume_state(64).items()}
    cfg = dict(PLUME_CFG, **ck["mconf"])
    cfg.update(dt=PLUME_CFG["dt"], buoyancyScale=PLUME_CFG["buoyancyScale"], gravityVec=PLUME_CFG["gravityVec"])
    for _ in range(3):
        simulate(cfg, bd, inf, "convnet")
    assert all(bool(torch.isfinite(bd[k]).all()) for k in ("p", "U", "density")) and float(bd["U"].abs().max()) > 0
    out = tmp_path / "plume"
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "plume.py"), "--res", "64", "--iters", "2", "--out-iter", "1",
                        "--method", "convnet", "--weights", f, "--folder", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "It = 0" in r.stdout and any(n.endswith(".png") or n.endswith(".vtk") or n.endswith(".pth") for n in os.listdir(out)), os.listdir(out)


def scalenet_digest(dev):
    """sha256 over the final parameters (by name) and the two training losses of a two-iteration ScaleNet train()"""
    from fluidnet_cxx_amd.training import MCONF_DEFAULTS, train
    run = train(dict(MCONF_DEFAULTS, longTermDivNumSteps=[1, 2]), dict(TCONF, iters=2), dev)
    h = hashlib.sha256()
    sd = run["checkpoint"]["state_dict"]
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k].cpu().numpy()).tobytes())
    for r in run["history"]:
        h.update(struct.pack("<dd", r["loss"], r["lt"]))
    return h.hexdigest()


def test_scalenet_training_is_untouched(dev):
    assert scalenet_digest(dev) == SCALENET_DIGEST
