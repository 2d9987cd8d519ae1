#!/usr/bin/env python3
"""The 3D step glue of the headline workload (plume 256^3, Jacobi-100) on the library that is in place -- for tools/ab_libs.sh run:

    python tools/stage_word_time.py [--res 256] [--steps 20]          # one line: replayed step, and the stage class by HIP events
    tools/gpu_kernel_stats.sh <tag> tools/stage_word_time.py --eager  # per-kernel averages of the same steps under rocprofv3

The state is bench.py's plume after a few developing steps; static_flags 0, 3, then 7, on a workspace of ext.step_workspace_bytes (in
3D: with room for the stage word map, so stage3d_kernel<.., WORD> and post_projection_kernel<true, false, WORD> run; on a build from
before the word the same calls run the float kernels).  `stage_us`: the event pairs of the stage class (the staging launch, the
post-projection launch and, in a step that builds it, the word) per eager step -- each pair makes its launch wait for the one before
it to drain, so it reads a little long; the A/B is between two builds timed the same way."""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--eager", action="store_true", help="eager steps only (for a profiler's kernel table)")
    a = ap.parse_args()
    import torch
    import bench
    from fluidnet_cxx_amd import simulate
    from fluidnet_cxx_amd._ext import ext
    dev = torch.device("cuda:0")
    w = dict(res=a.res, D=a.res, method="jacobi", iters=a.iters, kind="plume")
    m, bd = bench.mconf_for(w), bench.build_state(w, dev)
    ws = torch.empty(ext.step_workspace_bytes(1, a.res, a.res, a.res, True), dtype=torch.uint8, device=dev)
    seen = []

    def step():
        simulate(m, bd, None, "jacobi", workspace=ws, static_flags=(0, 3, 7)[min(len(seen), 2)])
        seen.append(1)

    for _ in range(5):
        step()
    torch.cuda.synchronize()
    if a.eager:
        for _ in range(a.steps):
            step()
        torch.cuda.synchronize()
        return
    ext.profile_enable(True)
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize()
    stage_ms, launches = ext.profile_read(bench.PROF["stage"])
    ext.profile_enable(False)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    for _ in range(5):
        g.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        g.replay()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / a.steps * 1e3
    print(f"{a.res}^3 Jacobi-{a.iters}: replayed step {ms:.4f} ms; stage class {stage_ms / a.steps * 1e3:.1f} us per step in {launches / a.steps:.1f} launches")


if __name__ == "__main__":
    main()
