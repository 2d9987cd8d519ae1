#!/usr/bin/env python3
"""The Conv3d bank net ('FluidNet3D' model) next to the 3D ScaleNet on a developed 3D plume, at 4 x 64^3, 128^3 and 256^3, on one device:
  the net alone (net.bank(x) / net.multiScale(x)) and the whole FluidNet.forward, each captured once into a HIP graph of GRAPH_REPS
  calls and replayed; then the 'convnet' step on the operator path (simulate(..., fused=False)) with either net and the native ScaleNet
  step, eager between device events, STEP_REPS steps a round.  The cases of a grid alternate over ROUNDS rounds in one process.
Reported: the mean and the spread (min .. max over the rounds) in us; for the bank net its rate against the model of DESIGN.md 26
(34 560 useful FLOP per cell; 270 algorithmic bytes per cell); and the sanity condition: at every grid the bank net, with 1/38.7 of the
ScaleNet's FLOPs, must be faster than the ScaleNet net of the same run (the tool exits non-zero otherwise).
python tools/banknet3d_time.py [--out FILE] [--quick] [--grids 64x4,128,256]"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

import bench  # noqa: E402
from fluidnet_cxx_amd import FluidNet, simulate  # noqa: E402
from viscous_time import Eager, graph_of  # noqa: E402

ROUNDS = 5
FLOP_PER_CELL = 34560      # 2 * (864 + 13824 * (1 + 1/8 + 1/64) + 648)
# x read (8); a written and read, block.0's output written and read (4 * 64); at the two coarser levels a written and read, block.0's
# output written and read, block.2's written and read ((6 * 64) * (1/8 + 1/64)); p written (4): 322 bytes; the issue's round figure of
# "about 270" leaves the coarser levels' block.2 and the re-read halo out.  Reported against this count.
BYTES_PER_CELL = 8 + 256 + 384 * (1 / 8 + 1 / 64) + 4


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
    ap.add_argument("--grids", default="64x4,128,256", help="comma-separated RES or RESxBATCH (cubes)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    grids = [(16, 1), (16, 2)] if a.quick else [tuple(int(v) for v in (g.split("x") + ["1"])[:2]) for g in a.grids.split(",")]
    say(f"Conv3d bank net ('FluidNet3D' model) and 3D ScaleNet: HIP-graph replays and the 'convnet' step (eager), {ROUNDS} alternating rounds, "
        f"us per call (mean, min .. max); device {torch.cuda.get_device_name(0)}")
    sane = True
    for res, B in grids:
        big = res >= 256
        graph_reps, step_reps = (2, 2) if big else (10, 5)
        w = dict(res=res, D=res, method="jacobi", iters=28, kind="plume", batch=B)
        m = bench.mconf_for(w)
        bd = bench.build_state(w, dev)
        for _ in range(5 if a.quick else 30):
            simulate(m, bd, None, "jacobi")
        torch.cuda.synchronize()
        cells = B * res ** 3
        nets = {"bank": FluidNet(dict(m, model="FluidNet3D"), dropout=False).to(dev).eval(), "ScaleNet": FluidNet(m, dropout=False).to(dev).eval()}
        inp = torch.cat((bd["p"], bd["U"], bd["flags"], bd["density"]), 1).contiguous()
        # the net's own input: the divergence of the normalised velocity and the occupancy
        from fluidnet_cxx_amd import fluid
        x = torch.cat((fluid.velocityDivergence(bd["U"] / bd["U"].std(), bd["flags"]), fluid.flagsToOccupancy(bd["flags"])), 1).contiguous()
        say()
        say(f"grid {B} x {res}^3  (graphs of {graph_reps} calls, {step_reps} steps a round)")
        cases = {
            "bank net": lambda: nets["bank"].bank(x),
            "bank forward": lambda: nets["bank"](inp),
            "ScaleNet net": lambda: nets["ScaleNet"].multiScale(x),
            "ScaleNet forward": lambda: nets["ScaleNet"](inp),
        }
        reps = {k: graph_reps for k in cases}
        t = timed({k: graph_of(fn, graph_reps) for k, fn in cases.items()}, reps)
        mean = {k: sum(v) / len(v) for k, v in t.items()}
        for k in cases:
            extra = ""
            if k == "bank net":
                extra = (f"  {cells * BYTES_PER_CELL / mean[k] * 1e-3:7.0f} GB/s algorithmic, "
                         f"{cells * FLOP_PER_CELL / mean[k] * 1e-6:6.2f} TFLOP/s useful")
            say(f"  {k:18s} {mean[k]:9.1f} us ({min(t[k]):.1f} .. {max(t[k]):.1f}){extra}")
        say(f"  ScaleNet net / bank net: {mean['ScaleNet net'] / mean['bank net']:.2f} x;  "
            f"ScaleNet forward / bank forward: {mean['ScaleNet forward'] / mean['bank forward']:.2f} x")
        if not mean["bank net"] < mean["ScaleNet net"]:
            sane = False
            say("  DEFECT: the bank net is not faster than the ScaleNet net of the same run")
        del t
        torch.cuda.empty_cache()
        steps = {}
        for name, net, fused in (("operator path, bank net", nets["bank"], False), ("operator path, ScaleNet", nets["ScaleNet"], False),
                                 ("native step, ScaleNet", nets["ScaleNet"], True)):
            st = {k: v.clone() for k, v in bd.items()}
            cfg = dict(m, model="FluidNet3D" if net.is_bank else "ScaleNet")
            steps[name] = Eager(lambda cfg=cfg, st=st, net=net, fused=fused: simulate(cfg, st, net, "convnet", fused=fused), step_reps)
        reps = {k: step_reps for k in steps}
        t = timed(steps, reps)
        for k in steps:
            say(f"  'convnet' step, {k:24s} {sum(t[k]) / len(t[k]):9.1f} us ({min(t[k]):.1f} .. {max(t[k]):.1f})")
        del bd, nets, steps, inp, x
        from fluidnet_cxx_amd import _simulate
        _simulate.release_workspaces()
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    sys.exit(0 if sane else 1)


if __name__ == "__main__":
    main()
