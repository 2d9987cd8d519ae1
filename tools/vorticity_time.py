#!/usr/bin/env python3
"""Time the time step with and without vorticity confinement.

    python tools/vorticity_time.py [--sizes 256x3,1024] [--steps 4] [--reps 7] [--rounds 3] [--amp 0.5] [--out profiles/r10/vorticity_time.txt]

Per size (bench.py's plume3d_256_jacobi: 256^3, Jacobi-100; plume2d_1024_jacobi: 1024^2, Jacobi-28): the plume state
(tests/util.py plume_state) after `--steps` steps with the confinement on, then the whole step captured in two HIP graphs -- amplitude 0
and `--amp` -- on copies of that state.  The two graphs are replayed in alternation, `--rounds` rounds of `--reps` replays each, every
replay timed with HIP events; the line gives the median and the spread of the round medians for both and their difference, which is
the confinement's launches (the cut stage's extra pass included).  The operator on its own (fnx_add_vorticity_confinement on the
step's velocity field) and one Jacobi pass of the same session -- the bandwidth yardstick of the bytes-per-cell model -- follow.
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
    ap.add_argument("--sizes", default="256x3,1024")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--amp", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    dev = torch.device("cuda")
    lines = [f"# device: {ext.device_name()}; plume state after {a.steps} steps at amplitude {a.amp}; {a.rounds} alternating rounds of {a.reps} replays"]
    print(lines[0], flush=True)
    for size in a.sizes.split(","):
        res, D, is3d = parse(size)
        cfg = dict(PLUME_CFG, jacobiIter=100 if is3d else 28)
        on = dict(cfg, vorticityConfinementAmp=a.amp)
        bd = {k: torch.from_numpy(v).to(dev) for k, v in plume_state(res, D=D).items()}
        for _ in range(a.steps):
            simulate(on, bd, None, "jacobi")
        graphs, states = {}, {}
        for name, c in (("off", cfg), ("on", on)):
            st = {k: v.clone() for k, v in bd.items()}
            ws = torch.empty(ext.step_workspace_bytes(1, D, res, res, is3d), dtype=torch.uint8, device=dev)
            simulate(c, st, None, "jacobi", workspace=ws, static_flags=0)
            simulate(c, st, None, "jacobi", workspace=ws, static_flags=3)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                simulate(c, st, None, "jacobi", workspace=ws, static_flags=7)
            g.replay()
            graphs[name], states[name] = g, (st, ws)
        med = {"off": [], "on": []}
        for _ in range(a.rounds):
            for name in ("off", "on"):
                med[name].append(timed(graphs[name].replay, a.reps))
        off, on_ms = float(np.median(med["off"])), float(np.median(med["on"]))
        spread = lambda v: max(v) - min(v)           # noqa: E731
        # the operator alone, and one Jacobi pass (two sweeps in 3D) as the session's bandwidth yardstick
        U, flags = bd["U"], bd["flags"]
        ext.add_vorticity_confinement(U, flags, a.amp, None)
        op = timed(lambda: ext.add_vorticity_confinement(U, flags, a.amp, None), a.reps * 3)
        div = fluid.velocityDivergence(U, flags)
        p = torch.zeros_like(div)
        k = 2 if is3d else 1
        ext.jacobi_sweeps_(flags, div, p, is3d, k)
        jac = timed(lambda: ext.jacobi_sweeps_(flags, div, p, is3d, k), a.reps * 3)
        cells = int(flags.numel())
        line = (f"{size:>6}  cells {cells:>9}  step amp 0 {off:8.3f} ms (spread {spread(med['off']):.3f})  amp {a.amp} {on_ms:8.3f} ms "
                f"(spread {spread(med['on']):.3f})  difference {on_ms - off:7.3f} ms  operator alone {op:7.3f} ms "
                f"({op * 1e6 / cells:.3f} ns/cell, incl. its output allocation)  jacobi_sweeps x{k} {jac:7.3f} ms")
        print(line, flush=True)
        lines.append(line)
        del graphs, states, bd, U, flags, div, p
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
