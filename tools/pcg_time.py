#!/usr/bin/env python3
"""Time the converged pressure solve (fnx_pcg) on developed plume states.

    python tools/pcg_time.py [--sizes 128,1024,128x3,256x3] [--steps 4] [--reps 5] [--out profiles/r08/pcg_time.txt]

Per size: the plume state (tests/util.py plume_state) after `--steps` Jacobi-28 time steps, its divergence as the right-hand side.
  eager   : the solve at p_tol = 1e-5 as a user calls it (it reads the stop flag every 4 iterations), median of --reps solves timed with
            HIP events; iterations and the recurrence residual
  per-it  : the same solve with p_tol = 0 (fixed iterations, no host synchronisation) captured in HIP graphs of K1 and K2
            iterations, each replayed --reps times; (t(K2) - t(K1)) / (K2 - K1) is the time of one iteration, t(K1) - K1 * that
            the set-up (hierarchy build, right-hand side, first V-cycle, final mean shift)
One line per size on stdout and in --out.  Under `rocprofv3 --kernel-trace --stats` it gives the per-kernel split."""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from fluidnet_cxx_amd import fluid, simulate          # noqa: E402
from fluidnet_cxx_amd._ext import ext                 # noqa: E402
from util import PLUME_CFG, plume_state               # noqa: E402


def parse(size):
    if "x3" in size:
        n = int(size.split("x")[0])
        return n, n, True
    return int(size), 1, False


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,1024,128x3,256x3")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k1", type=int, default=8)
    ap.add_argument("--k2", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    dev = torch.device("cuda")
    lines = [f"# device: {ext.device_name()}; plume state after {a.steps} Jacobi-28 steps; median of {a.reps}"]
    print(lines[0], flush=True)
    for size in a.sizes.split(","):
        res, D, is3d = parse(size)
        st = plume_state(res, D=D)
        bd = {k: torch.from_numpy(v).to(dev) for k, v in st.items()}
        for _ in range(a.steps):
            simulate(PLUME_CFG, bd, None, "jacobi")
        flags = bd["flags"]
        div = fluid.velocityDivergence(bd["U"], flags)
        solve = lambda tol, it: ext.solve_linear_system_pcg(flags, div, is3d, tol, it, False, None)   # noqa: E731
        _, r, iters = solve(1e-5, 100)                     # warm-up, and the iteration count
        eager = timed(lambda: solve(1e-5, 100), a.reps)
        graphs = {}
        for k in (a.k1, a.k2):
            solve(0.0, k)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                solve(0.0, k)
            g.replay()
            graphs[k] = timed(g.replay, a.reps * 4)
        per_it = (graphs[a.k2] - graphs[a.k1]) / (a.k2 - a.k1)
        setup = graphs[a.k1] - a.k1 * per_it
        cells = int(flags.numel())
        line = (f"{size:>6}  cells {cells:>9}  iterations {iters[0]:>3} to 1e-5 (residual {float(r):.2e})  solve {eager:8.3f} ms  "
                f"per iteration {per_it:7.3f} ms  set-up {setup:6.3f} ms  ({per_it * 1e6 / cells:.2f} ns/cell/iteration)")
        print(line, flush=True)
        lines.append(line)
        del graphs, bd, flags, div
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
