#!/usr/bin/env python3
"""Step time and CG iteration counts of the converged projections on the plume: 'pcg' (cold), 'pcg' with pcgWarmStart (from the
previous step's pressure) and 'hybrid' (from the net's pressure; the net's default weights, or --weights CKPT).

    python tools/hybrid_time.py [--res 1024] [--depth 1] [--configs pcg,pcg_warm,hybrid] [--develop 100] [--warmup 10] [--steps 100]
                                [--rounds 5] [--count-steps 8] [--weights CKPT] [--root TREE] [--out FILE]

Every configuration starts from the same developed plume (`--develop` 'pcg' steps) and keeps its own state.  Timing: device events
around blocks of steps / rounds steps, the configurations alternated block by block in this one process, after `--warmup` steps each.
Iteration counts: `--count-steps` further steps per configuration, each preceded by the solve of that step at the operator level
(the stages of simulate()'s operator path, then ext.solve_linear_system_pcg with the configuration's guess), which is bit for bit the
fused step's solve.  `--root TREE` imports the package from another checkout (a build of the parent commit, which knows 'pcg' only).
One JSON line on stdout (and appended to --out)."""
import argparse
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--depth", type=int, default=1)
    ap.add_argument("--configs", default="pcg,pcg_warm,hybrid")
    ap.add_argument("--develop", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--count-steps", type=int, default=8)
    ap.add_argument("--weights", default=None)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from fluidnet_cxx_amd import FluidNet, fluid, simulate
    from fluidnet_cxx_amd._ext import ext

    dev = torch.device("cuda")
    is3d = a.depth > 1
    conf = dict(dt=0.1, maccormackStrength=0.6, sampleOutsideFluid=False, buoyancyScale=0.25, gravityScale=0, viscosity=0,
                correctScalar=False, gravityVec=dict(x=0.0, y=-1.0, z=0.0), operatingDensity=0.0, pTol=0.0, jacobiIter=28,
                pcgTol=1e-5, pcgIter=50, normalizeInputThreshold=1e-5)
    shape = (1, 1, a.depth, a.res, a.res)
    flags = torch.zeros(shape, device=dev)
    fluid.emptyDomain(flags)
    base = dict(p=torch.zeros(shape, device=dev), U=torch.zeros((1, 3 if is3d else 2) + shape[2:], device=dev), flags=flags,
                density=torch.zeros(shape, device=dev))
    fluid.createPlumeBCs(base, 0.1, 2, 0.145)
    for _ in range(a.develop):
        simulate(conf, base, None, "pcg")

    names = [c for c in a.configs.split(",") if c]
    net = None
    if "hybrid" in names:
        mconf = dict(conf, is3D=is3d, inputDim=3 if is3d else 2)
        net = FluidNet(mconf, dropout=False)
        if a.weights:
            state = torch.load(a.weights, map_location="cpu", weights_only=False)
            net = FluidNet(state["mconf"], dropout=False)
            net.load_state_dict(state["state_dict"])
        net = net.to(dev).eval()
    runs = {}
    for name in names:
        method = "hybrid" if name == "hybrid" else "pcg"
        c = dict(conf, pcgWarmStart=True) if name == "pcg_warm" else conf
        runs[name] = dict(conf=c, method=method, net=net if name == "hybrid" else None, bd={k: v.clone() for k, v in base.items()},
                          ms=[], iters=[])
    for r in runs.values():
        for _ in range(a.warmup):
            simulate(r["conf"], r["bd"], r["net"], r["method"])
    torch.cuda.synchronize()
    block = max(a.steps // a.rounds, 1)
    for _ in range(a.rounds):
        for r in runs.values():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(block):
                simulate(r["conf"], r["bd"], r["net"], r["method"])
            e1.record()
            e1.synchronize()
            r["ms"].append(e0.elapsed_time(e1) / block)

    def guess_and_div(r):
        bd, c = r["bd"], r["conf"]
        p, U, fl = bd["p"], bd["U"].clone(), bd["flags"]
        tmp = dict(bd)
        rho = fluid.advectScalar(c["dt"], bd["density"], U, fl, method="maccormackFluidNet", boundary_width=1,
                                 sample_outside_fluid=c["sampleOutsideFluid"], maccormack_strength=c["maccormackStrength"])
        U = fluid.advectVelocity(dt=c["dt"], orig=U, U=U, flags=fl, method="maccormackFluidNet", boundary_width=1,
                                 maccormack_strength=c["maccormackStrength"])
        fluid.setConstVals(tmp, p, U, fl, rho)
        g = c["gravityVec"]
        U = fluid.addBuoyancy(U, fl, rho, [-c["buoyancyScale"] * g[k] for k in ("x", "y", "z")], c["operatingDensity"], c["dt"])
        U = fluid.setWallBcs(U, fl)
        fluid.setConstVals(tmp, p, U, fl, rho)
        div = fluid.velocityDivergence(U, fl)
        p0 = None
        if r["method"] == "hybrid":
            p0, _ = r["net"](torch.cat((p, U, fl, rho), 1))
        elif c.get("pcgWarmStart"):
            p0 = p
        return div, p0

    for r in runs.values():
        for _ in range(a.count_steps):
            div, p0 = guess_and_div(r)
            kw = {} if p0 is None else dict(p0=p0)
            r["iters"].append(ext.solve_linear_system_pcg(r["bd"]["flags"], div, is3d, conf["pcgTol"], conf["pcgIter"], False, None, **kw)[2][0])
            simulate(r["conf"], r["bd"], r["net"], r["method"])
    torch.cuda.synchronize()
    out = dict(label=a.label, res=a.res, depth=a.depth, develop=a.develop, warmup=a.warmup, steps_per_block=block, rounds=a.rounds,
               weights=a.weights or ("default" if net is not None else None), device=torch.cuda.get_device_name(0),
               configs={n: dict(ms_per_step_blocks=[round(x, 4) for x in r["ms"]], ms_per_step_median=round(sorted(r["ms"])[len(r["ms"]) // 2], 4),
                                ms_per_step_min=round(min(r["ms"]), 4), ms_per_step_max=round(max(r["ms"]), 4), cg_iterations=r["iters"])
                        for n, r in runs.items()})
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
