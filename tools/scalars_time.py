#!/usr/bin/env python3
"""One fluid.advectScalars call of C channels against C calls of advectScalar (plan 'auto' and plan 'cells') on a developed plume:
1024^2, 128^3 and 256^3 (C <= 4), C in 1, 2, 4, 8.  Alternating rounds in one process; the mean and the spread (min .. max over the
rounds) per case, the ratio to the faster comparator, and whether the outputs are the same bits at the timed size.
python tools/scalars_time.py [--out FILE] [--quick]"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

import bench  # noqa: E402
from fluidnet_cxx_amd import simulate  # noqa: E402
from fluidnet_cxx_amd._ext import ext  # noqa: E402

M = "maccormackFluidNet"
ROUNDS, REPS = 5, 20


def developed_plume(res, D, dev, steps):
    """the warm-up of tools/advect_ab.py: the benchmark's plume after `steps` Jacobi steps"""
    w = dict(res=res, D=D, method="jacobi", iters=40, kind="plume")
    m = bench.mconf_for(w)
    bd = bench.build_state(w, dev)
    for _ in range(steps):
        simulate(m, bd, None, "jacobi")
    torch.cuda.synchronize()
    return m, bd


def timed(cases):
    for fn in cases.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(ROUNDS):
        for k, fn in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                fn()
            e1.record(); torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / REPS * 1e3)
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

    grids = [(1024, 1, (1, 2, 4, 8)), (128, 128, (1, 2, 4, 8)), (256, 256, (1, 2, 4))]
    if a.quick:
        grids = [(64, 1, (1, 2)), (24, 24, (1, 2))]
    say(f"advectScalars(C) vs C x advectScalar, MacCormack strength 0.6, {ROUNDS} alternating rounds of {REPS} calls, us per case "
        f"(mean, min .. max); device {torch.cuda.get_device_name(0)}")
    for res, D, Cs in grids:
        m, bd = developed_plume(res, D, dev, 10 if a.quick else 100)
        rho, U, f = bd["density"], bd["U"], bd["flags"]
        dt = m["dt"]
        say()
        say(f"grid {D} x {res} x {res}, max CFL {float(U.abs().max()) * dt:.3f}")
        for C in Cs:
            # channel c: the density shifted by c cells along x and scaled, so that the channels differ
            src = torch.cat([torch.roll(rho, c, 4) * (1.0 - 0.1 * c) for c in range(C)], 1).contiguous()
            one, per_a, per_c = torch.empty_like(src), torch.empty_like(src), torch.empty_like(src)
            ws = torch.empty(ext.advect_scalars_workspace_bytes(1, D, res, res, D > 1, C), dtype=torch.uint8, device=dev)
            views = [(src[:, c:c + 1], per_a[:, c:c + 1], per_c[:, c:c + 1]) for c in range(C)]   # B = 1: a channel is contiguous

            def loop(plan, which):
                for v in views:
                    ext.advect_scalar(dt, v[0], U, f, M, 1, False, 0.6, v[which], None, plan)

            cases = {
                "scalars": lambda: ext.advect_scalars(dt, src, U, f, M, 1, False, 0.6, ws, None, one),
                "loop auto": lambda: loop("auto", 1),
                "loop cells": lambda: loop("cells", 2),
            }
            t = timed(cases)
            mean = {k: sum(v) / len(v) for k, v in t.items()}
            best = min(("loop auto", "loop cells"), key=lambda k: mean[k])
            spread = max(max(v) - min(v) for v in t.values())
            same = all(torch.equal(one.view(torch.int32), x.view(torch.int32)) for x in (per_a, per_c))
            row = "  ".join(f"{k} {mean[k]:8.1f} ({min(t[k]):.1f} .. {max(t[k]):.1f})" for k in cases)
            say(f"  C={C}: {row}  | scalars / {best} = {mean['scalars'] / mean[best]:.3f}, spread {spread:.1f} us, "
                f"slower by {mean['scalars'] - mean[best]:+.1f} us, same bits: {same}")
            del src, one, per_a, per_c, ws, views
        del bd, rho, U, f
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
