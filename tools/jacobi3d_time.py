"""GPU experiment: time of one 3D Jacobi solve (us per 2-sweep pass) for a grid.
   python tools/jacobi3d_time.py D H W [iters]            the operator, mask build and launch gaps included
   python tools/jacobi3d_time.py D H W [iters] --graph    a replayed HIP graph of one solve of `iters` sweeps from zero with the mask kept,
                                                          once per tiling of the two-sweep march (ext.Geom(jacobi_x=60 / 64), where
                                                          the 64-column kernel can run), three alternating rounds of 10 replays after a warm-up round"""
import sys
import torch
sys.path.insert(0, ".")
from fluidnet_cxx_amd import fluid
args = [a for a in sys.argv[1:] if not a.startswith("--")]
D, H, W = (int(v) for v in args[:3])
iters = int(args[3]) if len(args) > 3 else 100
dev = torch.device("cuda")
flags = torch.zeros(1, 1, D, H, W, device=dev); fluid.emptyDomain(flags)
div = torch.randn(1, 1, D, H, W, device=dev)


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


if "--graph" in sys.argv:
    from fluidnet_cxx_amd._ext import ext
    ws = torch.empty(ext.jacobi_workspace_bytes(1, D, H, W, True), dtype=torch.uint8, device=dev)
    p = torch.zeros_like(div)
    ext.jacobi_sweeps_(flags, div, p, True, iters, workspace=ws, reuse_mask=False, from_zero=True)     # builds the mask
    graphs, out = {}, {}
    for x in ("60", "64"):
        geom = ext.Geom(jacobi_x=int(x))
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            ext.jacobi_sweeps_(flags, div, p, True, iters, workspace=ws, reuse_mask=True, geom=geom, from_zero=True)
            s.synchronize()
            graphs[x] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[x], stream=s):
                ext.jacobi_sweeps_(flags, div, p, True, iters, workspace=ws, reuse_mask=True, geom=geom, from_zero=True)
        graphs[x].replay(); torch.cuda.synchronize()
        out[x] = p.clone()
    print(f"{D}x{H}x{W} Jacobi-{iters}, graph replay: same bits under both tilings: {torch.equal(out['60'], out['64'])}")
    for x in ("60", "64"):                               # warm-up, not reported
        timed(graphs[x].replay, 10)
    for rnd in range(3):
        for x in ("60", "64"):
            graphs[x].replay(); torch.cuda.synchronize()
            us = timed(graphs[x].replay, 10)
            print(f"  round {rnd} tiling {x}: {us:9.1f} us per solve, {us / (iters / 2):7.2f} us per 2-sweep pass")
else:
    solve = lambda: fluid.solveLinearSystemJacobi(flags, div, True, 0.0, iters)  # noqa: E731
    for _ in range(3):
        solve()
    torch.cuda.synchronize()
    us = timed(solve, 5)
    print(f"{D}x{H}x{W} Jacobi-{iters}: {us:9.1f} us per solve, {us / (iters / 2):7.2f} us per 2-sweep pass (incl. mask build + launch gaps)")
