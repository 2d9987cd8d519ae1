#!/usr/bin/env python3
"""Time one training iteration (fluidnet_cxx_amd/training.py: train) stage by stage.

    python tools/train_time.py [--res 128] [--batches 64,16] [--warmup 3] [--iters 10] [--out profiles/r12/train_time.txt]
    python tools/train_time.py --trace-only --batches 16 --iters 3          # the loop alone, for rocprofv3 --kernel-trace --stats -- ...
    python tools/train_time.py --depth 64 --res 64 --batches 4 [--no-long-term]      # the 3D loop (fluidnet_cxx_amd/training3d.py)

The loop is train()'s iteration with device events between its stages, back to back after a warm-up, no host synchronisation inside an
iteration: sampler (next(): redraw, `stride` pcg steps, the operator-path step and its projection), forward (FluidNetTrain, the repack
of the weights the optimiser wrote included -- it is timed once more on its own), loss kernel (fnx_train_loss, terms), rollout (the
no-grad convnet steps and the second forward + loss), backward (both roots: the loss kernel's gradient, fnx_fluidnet_backward, autograd's
accumulation), optimiser (Adam).  The sampler's own stages are timed in a second pass, the redraw split into its scene kernels and the
wall BCs + pcg projection next to them.  Nothing is asserted: the figures are a record."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fluidnet_cxx_amd import FluidNetTrain, fluid, simulate      # noqa: E402
from fluidnet_cxx_amd._ext import ext                            # noqa: E402
from fluidnet_cxx_amd.training import (MCONF_DEFAULTS, SceneSampler, fluidnet_loss, host_uniform, kaiming_init, lambdas_of,      # noqa: E402
                                       _STREAM_TRAINER)

STAGES = ["sampler", "forward", "loss kernel", "rollout", "backward", "optimiser"]


def run(res, B, warmup, iters, dev, record=True, depth=None, long_term=True):
    seed = 0
    if depth is None:
        mconf = dict(MCONF_DEFAULTS)
        net = kaiming_init(FluidNetTrain(mconf), seed).to(dev).train()
        sampler = SceneSampler(mconf, B, res, res, seed, dev)
        loss_fn, raw_loss, nU = fluidnet_loss, ext.train_loss, 2
    else:
        from fluidnet_cxx_amd import FluidNetTrain3D
        from fluidnet_cxx_amd.training3d import MCONF3D_DEFAULTS, SceneSampler3D, fluidnet_loss3d
        mconf = dict(MCONF3D_DEFAULTS)
        net = kaiming_init(FluidNetTrain3D(mconf), seed).to(dev).train()
        sampler = SceneSampler3D(mconf, B, depth, res, res, seed, dev)
        loss_fn, raw_loss, nU = fluidnet_loss3d, ext.train_loss3d, 3
    opt = torch.optim.Adam(net.parameters(), lr=mconf["lr"])
    lam = lambdas_of(mconf)
    one, ltw = torch.ones((), device=dev), torch.full((), float(mconf["divLongTermLambda"]), device=dev)
    marks, steps_taken = [], []
    for it in range(warmup + iters):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(STAGES) + 1)]
        ev[0].record()
        data, target = sampler.next()
        ev[1].record()
        opt.zero_grad()
        flags = data[:, 1 + nU:2 + nU].contiguous()
        out_p, out_U = net(data)
        ev[2].record()
        total, _ = loss_fn(out_p, out_U, flags, None, lam)
        ev[3].record()
        n = int(mconf["longTermDivNumSteps"][1] if host_uniform(seed, it, _STREAM_TRAINER, 0) > mconf["longTermDivProbability"]
                else mconf["longTermDivNumSteps"][0]) if long_term else 0
        roots, weights = [total], [one]
        if long_term:
            bd = dict(p=out_p.detach().clone(), U=out_U.detach().clone(), flags=flags, density=data[:, 2 + nU:3 + nU].contiguous())
            conf = sampler.sim_conf(sampler.last_choice)
            with torch.no_grad():
                for _ in range(n):
                    simulate(conf, bd, net, "convnet")
            p_lt, U_lt = net(torch.cat((bd["p"], bd["U"], flags, bd["density"]), 1))
            total_lt, _ = loss_fn(p_lt, U_lt, flags, None, [0.0, 1.0, 0.0, 0.0])
            roots.append(total_lt)
            weights.append(ltw)
        ev[4].record()
        torch.autograd.backward(roots, weights)
        ev[5].record()
        opt.step()
        ev[6].record()
        if it >= warmup:
            marks.append(ev)
            steps_taken.append(n)
    torch.cuda.synchronize()
    if not record:
        return None
    per = [sum(m[i].elapsed_time(m[i + 1]) for m in marks) / len(marks) for i in range(len(STAGES))]
    whole = sum(marks[k][0].elapsed_time(marks[k][-1]) for k in range(len(marks))) / len(marks)
    # the repack on its own: what the first forward after an optimiser step does before it launches the net
    params = net.multiScale._ordered()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(10):
        blob = torch.cat([p.detach().reshape(-1) for p in params]).contiguous()
        ext.scalenet_pack(blob, depth is not None)
        (ext.scalenet_pack_t if depth is None else ext.scalenet3d_pack_t)(blob)
    b.record()
    torch.cuda.synchronize()
    repack = a.elapsed_time(b) / 10
    # the loss kernel with its gradient in one call (terms and both gradients)
    a.record()
    for _ in range(20):
        raw_loss(out_p.detach(), out_U.detach(), flags, None, lam, one.reshape(1), True)
    b.record()
    torch.cuda.synchronize()
    fused_loss = a.elapsed_time(b) / 20
    # the sampler's stages
    names = ["redraw (all slots)", f"{sampler.stride} pcg steps", "advection + buoyancy + wall BCs", "pcg projection",
             "of the redraw: the scene kernels", "of the redraw: wall BCs + pcg projection"]
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(7)]
    reps = 5
    acc = [0.0] * 6
    for _ in range(reps):
        conf = sampler.sim_conf(sampler.choices(0))
        evs[4].record()
        fl0, U0, _ = sampler.draw(list(range(B)))
        evs[5].record()
        fluid.setWallBcs(U0, fl0)
        sampler._project(U0, fl0)
        evs[6].record()
        evs[0].record()
        sampler._redraw(list(range(B)))
        evs[1].record()
        for _ in range(sampler.stride):
            simulate(conf, sampler.bd, None, "pcg")
        evs[2].record()
        U, fl, rho = sampler.bd["U"], sampler.bd["flags"], sampler.bd["density"]
        rho2 = fluid.advectScalar(conf["dt"], rho, U, fl, maccormack_strength=conf["maccormackStrength"])
        U2 = fluid.advectVelocity(dt=conf["dt"], orig=U, U=U, flags=fl, maccormack_strength=conf["maccormackStrength"])
        fluid.addBuoyancy(U2, fl, rho2, [0.0, 1.0, 0.0], 0.0, conf["dt"])
        fluid.setWallBcs(U2, fl)
        evs[3].record()
        sampler._project(U2, fl)
        last = torch.cuda.Event(enable_timing=True)
        last.record()
        torch.cuda.synchronize()
        spans = [(evs[0], evs[1]), (evs[1], evs[2]), (evs[2], evs[3]), (evs[3], last), (evs[4], evs[5]), (evs[5], evs[6])]
        for i, (a0, a1) in enumerate(spans):
            acc[i] += a0.elapsed_time(a1) / reps
    return dict(res=res, B=B, per=per, whole=whole, repack=repack, fused_loss=fused_loss, rollout_steps=sum(steps_taken) / len(steps_taken),
                sampler=list(zip(names, acc)), scene_length=sampler.sceneLength, stride=sampler.stride)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--batches", default="64,16")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--depth", type=int, default=None, metavar="N", help="time the 3D loop on N x res x res cells")
    ap.add_argument("--no-long-term", action="store_true", help="leave the long-term rollout out of the iteration")
    a = ap.parse_args(argv)
    dev = torch.device("cuda")
    grid = f"{a.res}^2" if a.depth is None else f"{a.depth} x {a.res} x {a.res}"
    lines = [f"training iteration at {grid}{' without the long-term term' if a.no_long_term else ''} on {ext.device_name()}: device events, "
             f"{a.iters} back-to-back iterations after {a.warmup} of warm-up; ms"]
    for B in [int(b) for b in a.batches.split(",")]:
        r = run(a.res, B, a.warmup, a.iters, dev, record=not a.trace_only, depth=a.depth, long_term=not a.no_long_term)
        if r is None:
            continue
        lines.append(f"B = {B}: iteration {r['whole']:.3f} ms (rollout steps per iteration {r['rollout_steps']:.1f})")
        for name, ms in zip(STAGES, r["per"]):
            lines.append(f"    {name:12s} {ms:9.3f}  {100 * ms / r['whole']:5.1f} %")
        lines.append(f"    repack (inside the first forward after an optimiser step) {r['repack']:.3f}")
        lines.append(f"    loss kernel, terms and both gradients in one call {r['fused_loss']:.3f}")
        lines.append(f"    sampler stages, timed apart (a redraw of ALL slots; next() redraws (stride + 1) / sceneLength = "
                     f"{(r['stride'] + 1) / r['scene_length']:.3f} of them per call on average):")
        for name, ms in r["sampler"]:
            lines.append(f"        {name:34s} {ms:9.3f}")
    text = "\n".join(lines)
    print(text)
    if a.out and not a.trace_only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
