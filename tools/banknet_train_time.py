#!/usr/bin/env python3
"""Training of the 'FluidNet' bank model next to the ScaleNet model, at 128^2, 1024^2 and 32 x 128^2 on a developed 2D plume, on one device:
  the training forward, the backward and both of the net alone (net.bank / net.multiScale through the extension's entry points), each
  captured once into a HIP graph of GRAPH_REPS calls and replayed, the cases of a grid alternating over ROUNDS rounds in one process;
  then one trainer iteration (training.train) with and without the long-term term for both models at 128^2, B = 64, as the wall-clock
  difference of a run of ITERS[1] and one of ITERS[0] iterations, alternating as well.
Reported: the mean and the spread (min .. max over the rounds) in us; for the bank net its rate against the algorithmic traffic of the tape,
written once by the forward and read once by the backward (121 floats a cell each way, 968 bytes); and the sanity condition, stated and
not asserted: bank forward + backward is faster than ScaleNet's.
python tools/banknet_train_time.py [--out FILE] [--quick]"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

import bench  # noqa: E402
from fluidnet_cxx_amd import FluidNetBankTrain, FluidNetTrain, fluid, simulate  # noqa: E402
from fluidnet_cxx_amd._ext import ext  # noqa: E402
from viscous_time import graph_of  # noqa: E402

ROUNDS = 5
GRAPH_REPS = 10
TAPE_BYTES_PER_CELL = 121 * 4      # one way
ITERS = (2, 10)


def timed(cases, reps):
    times = {k: [] for k in cases}
    for _ in range(ROUNDS):
        for k, g in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record(); torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / reps * 1e3)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small grids and a short warm-up: a rehearsal of the tool, not a measurement")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"training of the bank net ('FluidNet' model) and of the ScaleNet: HIP-graph replays of {GRAPH_REPS} calls, {ROUNDS} alternating rounds, "
        f"us per call (mean, min .. max); device {torch.cuda.get_device_name(0)}")
    for res, B in (((32, 1), (32, 4)) if a.quick else ((128, 1), (1024, 1), (128, 32))):
        w = dict(res=res, D=1, method="jacobi", iters=28, kind="plume", batch=B)
        m = bench.mconf_for(w)
        bd = bench.build_state(w, dev)
        for _ in range(5 if a.quick else 50):
            simulate(m, bd, None, "jacobi")
        torch.cuda.synchronize()
        cells = B * res * res
        x = torch.cat((fluid.velocityDivergence(bd["U"] / bd["U"].std(), bd["flags"]), fluid.flagsToOccupancy(bd["flags"])), 1)[:, :, 0].contiguous()
        gp = torch.randn((B, 1, res, res), device=dev)
        bank, scale = FluidNetBankTrain(dict(m, model="FluidNet")).to(dev), FluidNetTrain(m).to(dev)
        pk_b, pt_b = bank._packed(dev)
        pk_s, pt_s = scale._packed(dev)
        _, tape_b = ext.banknet_forward_train(pk_b, x, "fp32")
        _, tape_s = ext.multiscale_forward_train(pk_s, x, "fp32")

        def bank_both():
            _, t = ext.banknet_forward_train(pk_b, x, "fp32")
            ext.banknet_backward(pt_b, x, gp, t, "fp32")

        def scale_both():
            _, t = ext.multiscale_forward_train(pk_s, x, "fp32")
            ext.multiscale_backward(pt_s, gp, t, "fp32")

        cases = {
            "bank forward_train": lambda: ext.banknet_forward_train(pk_b, x, "fp32"),
            "bank backward": lambda: ext.banknet_backward(pt_b, x, gp, tape_b, "fp32"),
            "bank fwd + bwd": bank_both,
            "ScaleNet forward_train": lambda: ext.multiscale_forward_train(pk_s, x, "fp32"),
            "ScaleNet backward": lambda: ext.multiscale_backward(pt_s, gp, tape_s, "fp32"),
            "ScaleNet fwd + bwd": scale_both,
        }
        say()
        say(f"grid {B} x {res}^2")
        t = timed({k: graph_of(fn, GRAPH_REPS) for k, fn in cases.items()}, GRAPH_REPS)
        mean = {k: sum(v) / len(v) for k, v in t.items()}
        for k in cases:
            extra = ""
            if k.startswith("bank"):
                ways = 2 if k.endswith("bwd") else 1
                extra = f"  {cells * ways * TAPE_BYTES_PER_CELL / mean[k] * 1e-3:7.0f} GB/s of the tape's algorithmic traffic"
            say(f"  {k:24s} {mean[k]:9.1f} us ({min(t[k]):.1f} .. {max(t[k]):.1f}){extra}")
        ratio = mean["ScaleNet fwd + bwd"] / mean["bank fwd + bwd"]
        say(f"  ScaleNet fwd + bwd / bank fwd + bwd: {ratio:.2f} x  (sanity: the bank net is {'faster' if ratio > 1 else 'NOT faster'})")
        del bd, bank, scale, tape_b, tape_s, x, gp, cases
        torch.cuda.empty_cache()

    # one trainer iteration: wall clock of ITERS[1] iterations minus that of ITERS[0], per iteration
    from fluidnet_cxx_amd.training import MCONF_DEFAULTS, train
    say()
    res, B = (32, 4) if a.quick else (128, 64)
    say(f"one trainer iteration at {B} x {res}^2 (training.train, wall clock of {ITERS[1]} iterations minus {ITERS[0]}, per iteration), ms")
    runs = {(model, lt): dict(MCONF_DEFAULTS, model=model, divLongTermLambda=lt) for model in ("FluidNet", "ScaleNet") for lt in (1.0, 0.0)}
    wall = {k: [] for k in runs}

    def seconds(mconf, iters):
        torch.cuda.synchronize()
        t0 = time.time()
        train(mconf, dict(res=res, batch=B, iters=iters, seed=3, evalEvery=0, evalBatches=1), dev)
        torch.cuda.synchronize()
        return time.time() - t0

    for k, mconf in runs.items():
        seconds(mconf, ITERS[0])                  # warm-up
    for _ in range(2 if a.quick else 3):
        for k, mconf in runs.items():
            wall[k].append((seconds(mconf, ITERS[1]) - seconds(mconf, ITERS[0])) / (ITERS[1] - ITERS[0]) * 1e3)
    for (model, lt), v in wall.items():
        say(f"  {model:9s} {'with' if lt else 'without'} the long-term term {sum(v) / len(v):9.1f} ms ({min(v):.1f} .. {max(v):.1f})")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
