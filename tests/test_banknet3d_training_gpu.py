"""The trainer with the Conv3d bank net on the GPU (training3d.train_bank3d): a short Adam run against a float64 yardstick built from
tests/banknet3d_grad_reference.py.  16 x 16 x 16, B = 2, seed 11, sceneLength 16, stride 1 and the scenes of tests/test_training3d_gpu.py."""
import time

import numpy as np
import pytest
import torch

import banknet3d_grad_reference as BG
import train_reference as TR
from test_training3d_gpu import SCENE
from util import assert_bitexact

pytestmark = pytest.mark.gpu

FACTOR = 8.0                                                 # the suite's rule (tests/test_cnn_train_gpu.py)
K, LR = 24, 3e-4
TCONF = dict(res=16, batch=2, seed=11, sceneLength=16, stride=1, evalEvery=0, evalBatches=2, scene=SCENE)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def bank3d_kaiming_weights(seed):
    """the trainer's initial weights (training.kaiming_init over FluidNetBankTrain3D) as name -> float32 array, without the extension"""
    from fluidnet_cxx_amd.weights import make_banknet_weights
    w = make_banknet_weights(0, ndim=3)
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


def bank3d_adam_run(weights, batches, held_out, lr, dtype):
    """TR.adam_run over the Conv3d bank net's chain: (held-out divL2 before, after, the final parameters)"""
    params = BG.as_params(weights, dtype)
    opt = torch.optim.Adam(list(params.values()), lr=lr)
    first = _held_out(params, held_out)
    for data in batches:
        opt.zero_grad()
        TR.div_l2(BG.fluidnet_forward(params, data)[1], TR._flags_of(data, dtype)).backward()
        opt.step()
    return first, _held_out(params, held_out), params


def test_bank3d_training_against_float64(dev):
    """K = 24 Adam iterations at rate 3e-4, divL2 only, from the seeded Kaiming weights: the native run; a float64 and a float32 leg on
    the CPU (torch Adam over banknet3d_grad_reference's chain) on the very batches the native run drew.
    Allowed: |native - f64| <= 8 (|f32 - f64| + delta_eval) in the final held-out divL2, where delta_eval = |evaluate3d(FluidNet
    inference net holding the float64 leg's final weights) - the float64 model's figure for those weights| is the rounding of the
    held-out evaluation itself, measured with the inference forward and the loss kernel and none of the training code.  The float64
    run's held-out divL2 must fall to at most three quarters.
    Choice of K and the rate, on the CPU alone, on train_reference.cpu_batches (seed 11, 16^3, B = 2, SCENE; 2 held-out batches of seed
    11 ^ 0x5eed5eed), float64 leg: (24, 3e-4) 8.206571e-03 -> 8.245508e-04 (x 0.100), taken; (24, 1e-3) x 0.079, (40, 3e-4) x 0.087,
    (40, 1e-3) x 0.075.  The float32 leg ended 4.5e-08 from the float64 one at (24, 3e-4), 3.0e-09 at (24, 1e-3)."""
    from fluidnet_cxx_amd import FluidNet, FluidNetBankTrain3D
    from fluidnet_cxx_amd.training import kaiming_init
    from fluidnet_cxx_amd.training3d import MCONF3D_DEFAULTS, SceneSampler3D, evaluate3d, train_bank3d
    mconf = dict(MCONF3D_DEFAULTS, model="FluidNet3D", divLongTermLambda=0.0, lr=LR)
    tconf = dict(TCONF, iters=K)
    t0 = time.time()
    run = train_bank3d(mconf, tconf, dev)
    assert type(run["net"]).__name__ == "FluidNetBankTrain3D" and run["checkpoint"]["mconf"]["model"] == "FluidNet3D"
    lam = [0.0, 1.0, 0.0, 0.0]
    held = run["held_out"]
    native_end = evaluate3d(run["net"], held, lam)["divL2_out"]
    again = SceneSampler3D(mconf, tconf["batch"], 16, 16, 16, tconf["seed"], dev, SCENE, tconf["sceneLength"], tconf["stride"])
    batches = [again.next()[0].cpu().numpy() for _ in range(K)]
    assert_bitexact(again.bd["U"].cpu().numpy(), run["sampler"].bd["U"].cpu().numpy(), "the replayed sampler's state")
    held_np = [d.cpu().numpy() for d, _ in held]
    t1 = time.time()
    w0 = bank3d_kaiming_weights(tconf["seed"])
    start = kaiming_init(FluidNetBankTrain3D(mconf), tconf["seed"])
    for k, v in start.state_dict().items():
        assert_bitexact(v.numpy(), w0[k], f"initial {k}")
    b64, e64, p64 = bank3d_adam_run(w0, batches, held_np, LR, torch.float64)
    t2 = time.time()
    b32, e32, _ = bank3d_adam_run(w0, batches, held_np, LR, torch.float32)
    t3 = time.time()
    native_begin = evaluate3d(start.to(dev), held, lam)["divL2_out"]
    inf = FluidNet.from_weights(mconf, {k: v.detach().to(torch.float32) for k, v in p64.items()}, dev)
    w64 = {k: v.detach().to(torch.float32).double() for k, v in p64.items()}           # the figure for the weights the net holds
    delta_eval = abs(evaluate3d(inf, held, lam)["divL2_out"] - _held_out(w64, held_np))
    d_native, d_f32 = abs(native_end - e64), abs(e32 - e64)
    print(f"\nBANK3D_TRAIN_F64 held-out divL2: float64 {b64:.6e} -> {e64:.6e} (x{e64 / b64:.3f})  float32 {b32:.6e} -> {e32:.6e}  "
          f"native {native_begin:.6e} -> {native_end:.6e}")
    print(f"BANK3D_TRAIN_F64 |native - f64| {d_native:.3e}  |f32 - f64| {d_f32:.3e}  delta_eval {delta_eval:.3e}  ratio "
          f"{d_native / max(d_f32 + delta_eval, 1e-300):.2f}   time: native {t1 - t0:.1f} s, float64 {t2 - t1:.1f} s, float32 {t3 - t2:.1f} s")
    assert e64 < b64 and native_end < native_begin
    assert e64 <= 0.75 * b64, "the float64 run's held-out loss must fall by at least a quarter"
    assert d_native <= FACTOR * (d_f32 + delta_eval)
