#!/usr/bin/env python3
"""The 'FluidNet' bank net in the native step (fnx_simulate_step_net) on a developed plume, on one device, at 128^2 B = 64
and 1024^2 (2D: the step does not take the Conv3d bank net).  Per grid, the cases alternating over ROUNDS rounds in one process:
  the bank 'convnet' step native, on a workspace of its own with the static promises made (what the four-argument call arrives at
  from its third step on) -- eager, and as a HIP graph of the round's steps, replayed;
  the same step with fused=False (the operator path: code the native step does not touch, so it stands for the step before ABI 35);
  the bank whole forward and the ScaleNet whole forward, as replayed graphs;
  the native ScaleNet 'convnet' step, eager;
  'hybrid' with the bank net, native against fused=False, eager (its solve reads the residual on the host: not capturable).
Reported: the mean and the spread (min .. max over the rounds) in us a step, the glue of each native step over its net's whole forward,
and the sanity condition: at every grid the native bank step is no slower than the fused=False step of the same run beyond the two
spreads (the native step removes launches and passes and adds none; the tool exits non-zero otherwise).
python tools/bank_step_time.py [--out FILE] [--quick] [--grids 128x64,1024]"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

import bench  # noqa: E402
from fluidnet_cxx_amd import FluidNet, _simulate, simulate  # noqa: E402
from fluidnet_cxx_amd._ext import ext  # noqa: E402
from viscous_time import Eager, graph_of  # noqa: E402

ROUNDS = 5


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


class PromisedStep:
    """simulate() on a workspace of its own with the static promises of FnxStepParams.static_flags: nothing on the first call, 3 on the
    second, 7 from the third on -- what a capture after three warm-up calls bakes into the graph"""

    def __init__(self, cfg, st, net, method):
        B, D, H, W = (int(st["flags"].size(i)) for i in (0, 2, 3, 4))
        self.ws = torch.empty(ext.step_workspace_bytes(B, D, H, W, False), dtype=torch.uint8, device=st["flags"].device)
        self.cfg, self.st, self.net, self.method, self.calls = cfg, st, net, method, 0

    def __call__(self):
        bits = (0, 3, 7)[min(self.calls, 2)] | (8 if self.method == "hybrid" and self.calls else 0)     # 8: the kept PCG hierarchy
        simulate(self.cfg, self.st, self.net, self.method, workspace=self.ws, static_flags=bits)
        self.calls += 1


def parse_grid(s):
    """RES or RESxBATCH"""
    parts = s.split("x")
    return int(parts[0]), int(parts[1]) if len(parts) > 1 else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small grids and a short warm-up: a rehearsal of the tool, not a measurement")
    ap.add_argument("--grids", default="128x64,1024", help="comma-separated RES or RESxBATCH (squares)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    grids = [(32, 2), (64, 1)] if a.quick else [parse_grid(g) for g in a.grids.split(",")]
    say(f"bank nets in the native step: {ROUNDS} alternating rounds, us per step or call (mean, min .. max); device "
        f"{torch.cuda.get_device_name(0)}")
    sane = True
    for res, B in grids:
        reps = 5 if res >= 1024 else 10
        w = dict(res=res, D=1, method="jacobi", iters=28, kind="plume", batch=B)
        m = dict(bench.mconf_for(w), pcgTol=1e-5, pcgIter=30)
        bd = bench.build_state(w, dev)
        for _ in range(5 if a.quick else 30):
            simulate(m, bd, None, "jacobi")
        torch.cuda.synchronize()
        bconf = dict(m, model="FluidNet")
        bank, scale = FluidNet(bconf, dropout=False).to(dev).eval(), FluidNet(m, dropout=False).to(dev).eval()
        inp = torch.cat((bd["p"], bd["U"], bd["flags"], bd["density"]), 1).contiguous()
        say()
        say(f"grid {B} x {res}^2  ({reps} steps or calls a round)")

        def state():
            return {k: v.clone() for k, v in bd.items()}

        def step(cfg, net, method, fused):
            st = state()
            return lambda: simulate(cfg, st, net, method, fused=fused)

        cases = {
            "bank 'convnet' native, eager": Eager(PromisedStep(bconf, state(), bank, "convnet"), reps),
            "bank 'convnet' native, graph": graph_of(PromisedStep(bconf, state(), bank, "convnet"), reps),
            "bank 'convnet' fused=False": Eager(step(bconf, bank, "convnet", False), reps),
            "bank whole forward, graph": graph_of(lambda: bank(inp), reps),
            "ScaleNet 'convnet' native, eager": Eager(PromisedStep(m, state(), scale, "convnet"), reps),
            "ScaleNet whole forward, graph": graph_of(lambda: scale(inp), reps),
            "bank 'hybrid' native, eager": Eager(PromisedStep(bconf, state(), bank, "hybrid"), reps),
            "bank 'hybrid' fused=False": Eager(step(bconf, bank, "hybrid", False), reps),
        }
        t = timed(cases, reps)
        mean = {k: sum(v) / len(v) for k, v in t.items()}
        for k in cases:
            say(f"  {k:34s} {mean[k]:10.1f} us ({min(t[k]):.1f} .. {max(t[k]):.1f})")
        fwd, sfwd = mean["bank whole forward, graph"], mean["ScaleNet whole forward, graph"]
        eager, graph, ops = mean["bank 'convnet' native, eager"], mean["bank 'convnet' native, graph"], mean["bank 'convnet' fused=False"]
        sstep = mean["ScaleNet 'convnet' native, eager"]
        say(f"  glue of the native bank step over the bank forward:         eager {eager - fwd:8.1f} us, graph {graph - fwd:8.1f} us")
        say(f"  glue of the fused=False bank step over the bank forward:          {ops - fwd:8.1f} us")
        say(f"  glue of the native ScaleNet step over the ScaleNet forward: eager {sstep - sfwd:8.1f} us")
        for method in ("convnet", "hybrid"):
            nat, ops = f"bank '{method}' native, eager", f"bank '{method}' fused=False"
            say(f"  '{method}': fused=False / native = {mean[ops] / mean[nat]:.2f} x")
            # slower beyond the run's own spread: even the fastest native round is slower than the slowest operator-path round
            if min(t[nat]) > max(t[ops]):
                sane = False
                say(f"  DEFECT: the native bank '{method}' step is slower than the fused=False step of the same run")
        del cases, t, bd, bank, scale, inp
        _simulate.release_workspaces()
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    sys.exit(0 if sane else 1)


if __name__ == "__main__":
    main()
