#!/usr/bin/env python3
"""The 'FluidNet' bank model next to the ScaleNet model on a developed 2D plume, at 128^2, 1024^2 and 32 x 128^2, on one device:
  the net alone (net.bank(x) / net.multiScale(x)) and the whole FluidNet.forward, each captured once into a HIP graph of GRAPH_REPS
  calls and replayed; then the 'convnet' step on the operator path (simulate(..., fused=False)) with either net and the native ScaleNet
  step, eager between device events, STEP_REPS steps a round.  The cases of a grid alternate over ROUNDS rounds in one process.
Reported: the mean and the spread (min .. max over the rounds) in us; for the bank net its rate against the model of DESIGN.md 24
(68 algorithmic bytes and 13 968 useful FLOP per cell); and the sanity condition: at 1024^2 the bank forward, with 1/35 of the ScaleNet's
FLOPs, must be faster than the ScaleNet forward of the same run (the tool exits non-zero otherwise).
python tools/banknet_time.py [--out FILE] [--quick]"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

import bench  # noqa: E402
from fluidnet_cxx_amd import FluidNet, simulate  # noqa: E402
from fluidnet_cxx_amd._ext import ext  # noqa: E402
from viscous_time import Eager, graph_of  # noqa: E402

ROUNDS = 5
GRAPH_REPS = 20
STEP_REPS = 10
BYTES_PER_CELL = 68        # x three times (24), the coarser results written (16 + 4) and read (16 + 4), p (4)
FLOP_PER_CELL = 13968      # 2 * (288 + 4608 * (1 + 1/4 + 1/16) + 648)


def timed(cases, reps):
    times = {k: [] for k in cases}
    for _ in range(ROUNDS):
        for k, g in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record(); torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / reps[k] * 1e3)
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

    say(f"bank net ('FluidNet' model) and ScaleNet: HIP-graph replays of {GRAPH_REPS} calls and the 'convnet' step (eager, {STEP_REPS} steps), "
        f"{ROUNDS} alternating rounds, us per call (mean, min .. max); device {torch.cuda.get_device_name(0)}")
    sane = True
    for res, B in (((32, 1), (32, 4)) if a.quick else ((128, 1), (1024, 1), (128, 32))):
        w = dict(res=res, D=1, method="jacobi", iters=28, kind="plume", batch=B)
        m = bench.mconf_for(w)
        bd = bench.build_state(w, dev)
        for _ in range(5 if a.quick else 50):
            simulate(m, bd, None, "jacobi")
        torch.cuda.synchronize()
        cells = B * res * res
        nets = {"bank": FluidNet(dict(m, model="FluidNet"), dropout=False).to(dev).eval(), "ScaleNet": FluidNet(m, dropout=False).to(dev).eval()}
        inp = torch.cat((bd["p"], bd["U"], bd["flags"], bd["density"]), 1).contiguous()
        # the net's own input: the divergence of the normalised velocity and the occupancy
        from fluidnet_cxx_amd import fluid
        x = torch.cat((fluid.velocityDivergence(bd["U"] / bd["U"].std(), bd["flags"]), fluid.flagsToOccupancy(bd["flags"])), 1)[:, :, 0].contiguous()
        say()
        say(f"grid {B} x {res}^2")
        cases = {
            "bank net": lambda: nets["bank"].bank(x),
            "bank forward": lambda: nets["bank"](inp),
            "ScaleNet net": lambda: nets["ScaleNet"].multiScale(x),
            "ScaleNet forward": lambda: nets["ScaleNet"](inp),
        }
        reps = {k: GRAPH_REPS for k in cases}
        t = timed({k: graph_of(fn, GRAPH_REPS) for k, fn in cases.items()}, reps)
        mean = {k: sum(v) / len(v) for k, v in t.items()}
        for k in cases:
            extra = ""
            if k == "bank net":
                extra = (f"  {cells * BYTES_PER_CELL / mean[k] * 1e-3:7.0f} GB/s algorithmic, "
                         f"{cells * FLOP_PER_CELL / mean[k] * 1e-6:6.2f} TFLOP/s useful")
            say(f"  {k:18s} {mean[k]:9.1f} us ({min(t[k]):.1f} .. {max(t[k]):.1f}){extra}")
        say(f"  ScaleNet forward / bank forward: {mean['ScaleNet forward'] / mean['bank forward']:.2f} x")
        if res == 1024 and not mean["bank forward"] < mean["ScaleNet forward"]:
            sane = False
            say("  DEFECT: the bank forward is not faster than the ScaleNet forward of the same run")
        steps = {}
        for name, net, fused in (("operator path, bank net", nets["bank"], False), ("operator path, ScaleNet", nets["ScaleNet"], False),
                                 ("native step, ScaleNet", nets["ScaleNet"], True)):
            st = {k: v.clone() for k, v in bd.items()}
            cfg = dict(m, model="FluidNet" if net.is_bank else "ScaleNet")
            steps[name] = Eager(lambda cfg=cfg, st=st, net=net, fused=fused: simulate(cfg, st, net, "convnet", fused=fused), STEP_REPS)
        reps = {k: STEP_REPS for k in steps}
        t = timed(steps, reps)
        for k in steps:
            say(f"  'convnet' step, {k:24s} {sum(t[k]) / len(t[k]):9.1f} us ({min(t[k]):.1f} .. {max(t[k]):.1f})")
        del bd, nets, steps, inp, x
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    sys.exit(0 if sane else 1)


if __name__ == "__main__":
    main()
