#!/usr/bin/env python3
"""One SHA-256 per tensor of the training scenes and the training loss (2D and 3D) on seeded inputs, to compare two builds bit for bit:

    python tools/scene_digest.py [TREE] [--out FILE]

TREE is the checkout whose built package is imported (default: the one this file sits in).  Only extension functions are used, so any
two trees that have them can be compared: run the tool once per tree, each in a process of its own, and compare the outputs line by line.
Shapes: the 64 x 4 workgroup is crossed in x and in y, more than one plane and more than one sample; scene ids that are neither
consecutive nor ordered.  The loss runs terms only, gradients only and both in one call (its three kernels per dimension), once with all
four lambdas and a target pressure and once with the two divergence lambdas and none."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

CASES2D = [(3, 6, 70), (2, 37, 53)]                  # (B, H, W)
CASES3D = [(3, 5, 6, 70), (2, 9, 7, 33)]             # (B, D, H, W)
IDS = [1000003, 5, 2 ** 31 - 1]
SEED = 20263
OBSTACLES = (0, 4, -0.3, 0.3, 0.03, 0.12)            # n_min, n_max, centre_min, centre_max, size_min, size_max
TURBULENCE = (3, 11.3, 8.0, 1.0)                     # octaves, wavelength, amplitude, density_scale
LOSSES = [("all", True, [1.0, 1.0, 0.5, 0.5]), ("div", False, [0.0, 1.0, 0.0, 0.5])]      # (label, with target_p, lambdas)


def sid(shape):
    return "x".join(str(v) for v in shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("tree", nargs="?", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from fluidnet_cxx_amd._ext import ext
    dev = torch.device("cuda")
    lines = []

    def emit(label, t):
        torch.cuda.synchronize()
        line = f"{label} {hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()}"
        print(line, flush=True)
        lines.append(line)

    for shape in CASES2D + CASES3D:
        is3d = len(shape) == 4
        B, grid = shape[0], tuple(shape[1:])
        ids = torch.tensor(IDS[:B], dtype=torch.int64).to(torch.int32).to(dev)
        obstacles, turbulence, loss = ((ext.scene_obstacles3d, ext.scene_turbulence3d, ext.train_loss3d) if is3d else
                                       (ext.scene_obstacles, ext.scene_turbulence, ext.train_loss))
        flags = obstacles(ids, *grid, SEED, *OBSTACLES)
        U, rho = turbulence(ids, *grid, SEED, *TURBULENCE, True)
        for name, t in (("flags", flags), ("U", U), ("density", rho)):
            emit(f"scene {sid(shape)} {name}", t)
        # the loss on a field that is not divergence free, over the scene's obstacles
        rng = np.random.default_rng(sum(shape))
        noise = lambda like: torch.from_numpy(rng.standard_normal(tuple(like.shape)).astype(np.float32)).to(dev)
        out_U, out_p, target = U + 0.5 * noise(U), noise(rho), noise(rho)
        up = torch.full((1,), 0.75, device=dev)
        for label, with_t, lam in LOSSES:
            tp = target if with_t else None
            emit(f"loss {sid(shape)} {label} terms-only terms", loss(out_p, out_U, flags, tp, lam, None, True)[0])
            _, gp, gU = loss(out_p, out_U, flags, tp, lam, up, False)
            emit(f"loss {sid(shape)} {label} grads-only grad_p", gp)
            emit(f"loss {sid(shape)} {label} grads-only grad_U", gU)
            for name, t in zip(("terms", "grad_p", "grad_U"), loss(out_p, out_U, flags, tp, lam, up, True)):
                emit(f"loss {sid(shape)} {label} both {name}", t)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
