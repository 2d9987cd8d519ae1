#!/usr/bin/env python3
"""The 3D viscous-flow operators on a developed plume, 128^3 and 256^3, on one device:
  addViscosity 3D (out of place, 28 algorithmic bytes a cell: three components and flags in, three components out),
  setWallBcsStick 3D (out of place, 32: three components, flags and flags_stick in, three components out),
  and in the same run the stand-alone 3D velocityUpdate (in place, 32: p, flags and three components in, three components out),
  the yardstick with the same access pattern minus the z neighbours;
  then the Jacobi-100 step with viscosity = 0 against viscosity > 0.  The native step has no 3D viscous stage, so the viscous step is
  the operator path (simulate(..., fused=False)); it is timed against the operator path with viscosity = 0, and the native step is
  given beside them.  These three are eager calls between device events (the operator path allocates its outputs, so it is not
  captured), STEP_REPS steps a round.
Each operator is captured once into a HIP graph of 200 calls and replayed; the cases of a grid alternate over ROUNDS rounds in one process.
Reported: the mean and the spread (min .. max over the rounds) in us, and for the operators GB/s of algorithmic bytes.
python tools/viscous_time.py [--out FILE] [--quick]"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

import bench  # noqa: E402
from fluidnet_cxx_amd import simulate  # noqa: E402
from fluidnet_cxx_amd._ext import ext  # noqa: E402

ROUNDS = 5
STEP_REPS = 10
BYTES = dict(addViscosity=28, setWallBcsStick=32, velocityUpdate=32)      # algorithmic bytes a cell
NU = 0.5                                                                  # NU * dt = 0.05 <= 1/6


def graph_of(fn, reps):
    """fn() `reps` times in one HIP graph (warmed up eagerly first)"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


class Eager:
    """fn() `reps` times, launched eagerly (warmed up first)"""

    def __init__(self, fn, reps):
        self.fn, self.reps = fn, reps
        for _ in range(3):
            fn()
        torch.cuda.synchronize()

    def replay(self):
        for _ in range(self.reps):
            self.fn()


def timed(graphs, reps):
    """us per call of every case, one figure per round, the cases alternating"""
    times = {k: [] for k in graphs}
    for _ in range(ROUNDS):
        for k, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record(); torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / reps[k] * 1e3)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="a small grid and a short warm-up: a rehearsal of the tool, not a measurement")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"3D viscous operators (HIP-graph replays of 200 calls) and the Jacobi-100 step (eager, {STEP_REPS} steps), {ROUNDS} alternating rounds, us per call "
        f"(mean, min .. max); device {torch.cuda.get_device_name(0)}")
    for res in ((24,) if a.quick else (128, 256)):
        w = dict(res=res, D=res, method="jacobi", iters=100, kind="plume")
        m = bench.mconf_for(w)
        bd = bench.build_state(w, dev)
        for _ in range(10 if a.quick else 100):
            simulate(m, bd, None, "jacobi")
        torch.cuda.synchronize()
        U, f, p = bd["U"], bd["flags"], bd["p"]
        cells = res ** 3
        stick = torch.where(f == 2.0, torch.full_like(f, 128.0), f)      # every wall no-slip
        out, Uv = torch.empty_like(U), U.clone()
        say()
        say(f"grid {res}^3, max CFL {float(U.abs().max()) * m['dt']:.3f}")
        ops = {
            "addViscosity": lambda: ext.add_viscosity_out(m["dt"], U, f, NU, out),
            "setWallBcsStick": lambda: ext.set_wall_bcs_stick_out(U, f, stick, out),
            "velocityUpdate": lambda: ext.velocity_update_(p, Uv, f, None),
        }
        reps = {k: 200 for k in ops}
        t = timed({k: graph_of(fn, reps[k]) for k, fn in ops.items()}, reps)
        rate = {}
        for k in ops:
            mean = sum(t[k]) / len(t[k])
            rate[k] = cells * BYTES[k] / mean * 1e-3
            say(f"  {k:16s} {mean:8.1f} us ({min(t[k]):.1f} .. {max(t[k]):.1f})  {BYTES[k]} B/cell  {rate[k]:7.0f} GB/s algorithmic")
        say(f"  addViscosity / velocityUpdate, rate of algorithmic bytes: {rate['addViscosity'] / rate['velocityUpdate']:.3f}")
        del out, Uv
        # the step: a copy of the state per case
        steps = {}
        for name, nu, fused in (("native step, viscosity=0", 0.0, True), ("operator path, viscosity=0", 0.0, False),
                                (f"operator path, viscosity={NU}", NU, False)):
            st = {k: v.clone() for k, v in bd.items()}
            cfg = dict(m, viscosity=nu)
            steps[name] = Eager(lambda cfg=cfg, st=st, fused=fused: simulate(cfg, st, None, "jacobi", fused=fused), STEP_REPS)
        reps = {k: STEP_REPS for k in steps}
        t = timed(steps, reps)
        mean = {k: sum(v) / len(v) for k, v in t.items()}
        for k in steps:
            say(f"  {k:28s} {mean[k]:9.1f} us ({min(t[k]):.1f} .. {max(t[k]):.1f})")
        _, k0, k1 = list(steps)
        say(f"  on the operator path viscosity adds {mean[k1] - mean[k0]:+.1f} us a step ({(mean[k1] / mean[k0] - 1) * 100:+.1f} %): the copy of U, "
            f"addViscosity, and the advection of a field that is not U")
        del bd, U, f, p, stick, steps
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
