#!/usr/bin/env python3
"""Train the 2D or the 3D pressure net on one GPU, with nothing downloaded -- what the reference's `pytorch/fluid_net_train.py` does with a
Mantaflow data set, on scenes generated while training (fluidnet_cxx_amd/training.py; with --depth fluidnet_cxx_amd/training3d.py).

    python examples/train.py [--res 128] [--batch 64] [--iters 1000] [--seed 0] [--out convModel.pth] [--lr 5e-5] [--eval-every 50]
                             [--no-long-term] [--resume CKPT] [--report FILE] [--depth N] [--model {ScaleNet,FluidNet,FluidNet3D}]

Writes a checkpoint {'state_dict', 'optimizer', 'mconf', 'it', ...} that `FluidNet.load_state_dict` takes and
`examples/plume.py --method convnet --weights` runs.  With --report the loss curve, the held-out ratio divL2(net's U) / divL2(U before
the projection) and the number of Jacobi sweeps that reach the same held-out divL2 on the same scenes go to FILE as text.

`--model FluidNet` trains the reference's 16-channel bank net (what its trainConfig.yaml ships; 2D, res a multiple of 4) instead of the
ScaleNet; `examples/plume.py` picks the net from the checkpoint's mconf.

`--depth N` (N >= 4) trains the 3D net on a N x res x res grid instead (the defaults become --res 64 --batch 4); its checkpoint goes to
`examples/plume.py --depth N --method convnet --weights3d`.  The report then has no Jacobi line.  `--depth N --model FluidNet3D` trains the
Conv3d 16-channel bank net there (N and res multiples of 4); the checkpoint's mconf carries the model, so the same plume command runs it."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fluidnet_cxx_amd.training import MCONF_DEFAULTS, evaluate, jacobi_divL2, jacobi_sweeps_to_reach, lambdas_of, train      # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=None, help="cells along x and y (default 128; 64 with --depth)")
    ap.add_argument("--batch", type=int, default=None, help="default 64 (trainConfig.yaml: batchSize); 4 with --depth")
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="convModel.pth")
    ap.add_argument("--lr", type=float, default=MCONF_DEFAULTS["lr"])
    ap.add_argument("--eval-every", type=int, default=50)
    ap.add_argument("--no-long-term", action="store_true", help="divLongTermLambda = 0 (the reference's default is 1)")
    ap.add_argument("--resume", default=None, metavar="CKPT")
    ap.add_argument("--report", default=None, metavar="FILE")
    ap.add_argument("--depth", type=int, default=None, metavar="N", help="train the 3D net on N x res x res cells (N >= 4)")
    ap.add_argument("--model", choices=("ScaleNet", "FluidNet", "FluidNet3D"), default="ScaleNet",
                    help="FluidNet: the 16-channel bank net (2D only); FluidNet3D: its Conv3d counterpart (with --depth)")
    a = ap.parse_args(argv)
    if a.depth is not None and a.model == "FluidNet":
        ap.error("--model FluidNet is 2D only (the reference asserts it); --depth trains the 3D ScaleNet, or the Conv3d bank net with "
                 "--model FluidNet3D")
    if a.depth is None and a.model == "FluidNet3D":
        ap.error("--model FluidNet3D is 3D only: give --depth N (without --depth, --model FluidNet trains the 2D bank net)")
    if a.depth is not None and a.depth < 4:
        ap.error("--depth must be at least 4 (the net's three scales need 4 planes); without --depth the 2D net is trained")
    is3d = a.depth is not None
    a.res = a.res if a.res is not None else (64 if is3d else 128)
    a.batch = a.batch if a.batch is not None else (4 if is3d else 64)
    return a


def main(argv=None):
    a = parse_args(argv)
    is3d = a.depth is not None
    if is3d:
        from fluidnet_cxx_amd.training3d import MCONF3D_DEFAULTS, evaluate3d, train3d, train_bank3d
    mconf = dict(MCONF3D_DEFAULTS if is3d else MCONF_DEFAULTS, lr=a.lr, model=a.model)
    if a.no_long_term:
        mconf["divLongTermLambda"] = 0.0
    tconf = dict(res=a.res, batch=a.batch, iters=a.iters, seed=a.seed, evalEvery=a.eval_every)
    t0 = time.time()
    if is3d:
        run = (train_bank3d if a.model == "FluidNet3D" else train3d)(mconf, dict(tconf, D=a.depth), torch.device("cuda"), out=a.out,
                                                                     resume=a.resume, log=print)
    else:
        run = train(mconf, tconf, torch.device("cuda"), out=a.out, resume=a.resume, log=print)
    torch.cuda.synchronize()
    seconds = time.time() - t0
    lam = lambdas_of(mconf)
    ev = (evaluate3d if is3d else evaluate)(run["net"], run["held_out"], lam)
    ratio = ev["divL2_out"] / ev["divL2_in"]
    sweeps = None if is3d else jacobi_sweeps_to_reach(run["held_out"], ev["divL2_out"])
    lines = [f"examples/train.py{f' --depth {a.depth}' if is3d else ''} {'' if a.model == 'ScaleNet' else f' --model {a.model}'} --res {a.res} --batch {a.batch} --iters {a.iters} --seed {a.seed} --lr {a.lr:g}"
             f"{' --no-long-term' if a.no_long_term else ''}: {seconds:.1f} s wall ({seconds / max(a.iters, 1) * 1e3:.1f} ms per iteration, "
             "sampler, evaluation and checkpoint included)",
             f"held-out ({len(run['held_out'])} batches of another seed): loss {ev['loss']:.4e}, divL2 of the net's U {ev['divL2_out']:.4e}, "
             f"divL2 of U before the projection {ev['divL2_in']:.4e}, ratio {ratio:.4e}",
             "Jacobi sweeps that reach the same held-out divL2: not searched in 3D" if is3d else
             f"Jacobi sweeps that reach the same held-out divL2 on the same scenes: {sweeps}"
             + ("" if sweeps is None else f" (divL2 {jacobi_divL2(run['held_out'], sweeps):.4e}; {max(sweeps - 1, 1)} sweeps: "
                                          f"{jacobi_divL2(run['held_out'], max(sweeps - 1, 1)):.4e})"),
             "it  loss  long-term  lr  [held-out loss  divL2 out / in]"]
    for r in run["history"]:
        if "val" in r or r["it"] % max(a.eval_every // 5, 1) == 0:
            lt = "-" if r["lt"] is None else f"{r['lt']:.4e}"
            val = f"  {r['val']:.4e}  {r['val_divL2_out'] / r['val_divL2_in']:.4e}" if "val" in r else ""
            lines.append(f"{r['it'] + 1:6d}  {r['loss']:.4e}  {lt}  {r['lr']:.3e}{val}")
    text = "\n".join(lines)
    print(text)
    print(f"checkpoint: {a.out}")
    if a.report:
        os.makedirs(os.path.dirname(os.path.abspath(a.report)), exist_ok=True)
        with open(a.report, "w") as f:
            f.write(text + "\n")
    return run


if __name__ == "__main__":
    main()
