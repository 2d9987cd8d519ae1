#!/usr/bin/env python3
"""Training of the Conv3d bank net ('FluidNet3D' model) next to the 3D ScaleNet on a developed 3D plume, at 4 x 64^3, 128^3 and 256^3, on
one device: the training forward, the backward and both of the net alone (the extension's banknet3d_* / multiscale3d_* entry points), each
captured once into a HIP graph of a few calls and replayed, the cases of a grid alternating over ROUNDS rounds in one process.
Reported: the mean and the spread (min .. max over the rounds) in us; for the bank net's backward its rate against the arithmetic of
DESIGN.md 28 (67 400 FLOP a voxel), for its forward against the 34 560 of DESIGN.md 26; and the sanity condition, stated and not asserted:
bank forward + backward is faster than the ScaleNet's of the same run.
python tools/banknet3d_train_time.py [--out FILE] [--quick] [--grids 64x4,128,256]"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

import bench  # noqa: E402
from fluidnet_cxx_amd import FluidNetBankTrain3D, FluidNetTrain3D, fluid, simulate  # noqa: E402
from fluidnet_cxx_amd._ext import ext  # noqa: E402
from viscous_time import graph_of  # noqa: E402

ROUNDS = 5
FWD_FLOP_PER_CELL = 34560
# input gradients 15 768 MAC, the bank weight gradients the same again, conv1 864, the tail about 1 300: 33 700 MAC
BWD_FLOP_PER_CELL = 2 * 33700


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
    ap.add_argument("--grids", default="64x4,128,256", help="comma-separated RES or RESxBATCH (cubes)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    grids = [(16, 1), (16, 2)] if a.quick else [tuple(int(v) for v in (g.split("x") + ["1"])[:2]) for g in a.grids.split(",")]
    say(f"training of the Conv3d bank net ('FluidNet3D' model) and of the 3D ScaleNet: HIP-graph replays, {ROUNDS} alternating rounds, "
        f"us per call (mean, min .. max); device {torch.cuda.get_device_name(0)}")
    for res, B in grids:
        reps = 2 if res >= 256 else 5
        w = dict(res=res, D=res, method="jacobi", iters=28, kind="plume", batch=B)
        m = bench.mconf_for(w)
        bd = bench.build_state(w, dev)
        for _ in range(5 if a.quick else 30):
            simulate(m, bd, None, "jacobi")
        torch.cuda.synchronize()
        cells = B * res ** 3
        x = torch.cat((fluid.velocityDivergence(bd["U"] / bd["U"].std(), bd["flags"]), fluid.flagsToOccupancy(bd["flags"])), 1).contiguous()
        gp = torch.randn((B, 1, res, res, res), device=dev)
        del bd
        from fluidnet_cxx_amd import _simulate
        _simulate.release_workspaces()
        torch.cuda.empty_cache()
        bank, scale = FluidNetBankTrain3D(dict(m, model="FluidNet3D")).to(dev), FluidNetTrain3D(m).to(dev)
        pk_b, pt_b = bank._packed(dev)
        pk_s, pt_s = scale._packed(dev)
        _, tape_b = ext.banknet3d_forward_train(pk_b, x, "fp32")
        _, tape_s = ext.multiscale3d_forward_train(pk_s, x, "fp32")

        def bank_both():
            _, t = ext.banknet3d_forward_train(pk_b, x, "fp32")
            ext.banknet3d_backward(pt_b, x, gp, t, "fp32")

        def scale_both():
            _, t = ext.multiscale3d_forward_train(pk_s, x, "fp32")
            ext.multiscale3d_backward(pt_s, gp, t, "fp32")

        cases = {
            "bank forward_train": lambda: ext.banknet3d_forward_train(pk_b, x, "fp32"),
            "bank backward": lambda: ext.banknet3d_backward(pt_b, x, gp, tape_b, "fp32"),
            "bank fwd + bwd": bank_both,
            "ScaleNet forward_train": lambda: ext.multiscale3d_forward_train(pk_s, x, "fp32"),
            "ScaleNet backward": lambda: ext.multiscale3d_backward(pt_s, gp, tape_s, "fp32"),
            "ScaleNet fwd + bwd": scale_both,
        }
        say()
        say(f"grid {B} x {res}^3  (graphs of {reps} calls)")
        t = timed({k: graph_of(fn, reps) for k, fn in cases.items()}, reps)
        mean = {k: sum(v) / len(v) for k, v in t.items()}
        for k in cases:
            extra = ""
            if k.startswith("bank"):
                flop = {"bank forward_train": FWD_FLOP_PER_CELL, "bank backward": BWD_FLOP_PER_CELL}.get(k, FWD_FLOP_PER_CELL + BWD_FLOP_PER_CELL)
                extra = f"  {cells * flop / mean[k] * 1e-6:6.2f} TFLOP/s useful"
            say(f"  {k:24s} {mean[k]:9.1f} us ({min(t[k]):.1f} .. {max(t[k]):.1f}){extra}")
        ratio = mean["ScaleNet fwd + bwd"] / mean["bank fwd + bwd"]
        say(f"  ScaleNet fwd + bwd / bank fwd + bwd: {ratio:.2f} x  (sanity: the bank net is {'faster' if ratio > 1 else 'NOT faster'})")
        del bank, scale, tape_b, tape_s, x, gp, cases, t
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
