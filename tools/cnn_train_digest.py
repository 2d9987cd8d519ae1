#!/usr/bin/env python3
"""One SHA-256 per tensor of the native training path and of the inference forward (2D and 3D) on seeded inputs, to compare two builds
bit for bit:

    python tools/cnn_train_digest.py [TREE] [--out FILE]

TREE is the checkout whose built package is imported (default: the one this file sits in).  Only extension functions are used, so any
two trees that have them can be compared: run the tool once per tree, each in a process of its own, and compare the outputs line by line.
Shapes: W not a multiple of 32, H not a multiple of 4, B > 1, more than one split, the plain and the MFMA weight-gradient kernels and
the direct, F(2x2) and F(4x4) input-gradient launches.  Inference ("infer" lines): ext.multiscale_forward in all six precision modes on a
grid where every launcher falls back and on one past the F(2x2) / F(4x4) / bf16 fill thresholds, ext.fluidnet_forward, and the forward on
nested z-crops with and without trims."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

MODES = ("fp32", "fp32_f2", "fp32_direct")
CASES2D = [((2, 37, 53), MODES), ((3, 199, 215), MODES), ((2, 255, 508), MODES)]
CASES3D = [((2, 6, 10, 37), MODES), ((1, 9, 14, 70), ("fp32",))]
BIG3D = (2, 32, 64, 64)            # past the Winograd kernels' fill thresholds: backward at fp32 on an fp32_direct tape
ALL_MODES = ("fp32", "fp32_direct", "bf16x6", "bf16x3", "fp32_f4", "fp32_f2")
INFER2D = [((2, 37, 53), ALL_MODES), ((2, 255, 508), ALL_MODES)]
INFER3D = [((2, 6, 10, 37), ALL_MODES), (BIG3D, ("fp32",))]
CROP3D, CROP_TRIM = (1, 24, 12, 37), [8, 4, 4, 0]
FLUID, OBST = 1.0, 2.0


def sid(shape):
    return "x".join(str(v) for v in shape)


def fluid_input(shape, rng):
    """(B, 3 + nc, D, H, W) = [p, U, flags, density]: a closed domain with an obstacle box"""
    B, dims = shape[0], (1,) * (4 - len(shape)) + tuple(shape[1:])
    nc = len(shape) - 1
    D, H, W = dims
    flags = np.full((B, 1) + dims, FLUID, np.float32)
    if nc == 3:
        flags[:, :, 0] = OBST; flags[:, :, -1] = OBST
    flags[:, :, :, 0] = OBST; flags[:, :, :, -1] = OBST
    flags[:, :, :, :, 0] = OBST; flags[:, :, :, :, -1] = OBST
    flags[:, :, D // 3:D // 3 + 2, H // 3:H // 3 + 3, W // 3:W // 3 + 5] = OBST
    inp = np.zeros((B, 3 + nc) + dims, np.float32)
    inp[:, 1:1 + nc] = rng.standard_normal((B, nc) + dims).astype(np.float32) * 0.5
    inp[:, 1 + nc:2 + nc] = flags
    inp[:, 2 + nc] = rng.random((B,) + dims).astype(np.float32)
    return inp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("tree", nargs="?", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from fluidnet_cxx_amd._ext import ext
    from fluidnet_cxx_amd.model import blob_from_state_dict
    from fluidnet_cxx_amd.weights import make_scalenet_weights
    dev = torch.device("cuda")
    lines = []

    def emit(label, t):
        torch.cuda.synchronize()
        line = f"{label} {hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()}"
        print(line, flush=True)
        lines.append(line)

    def entries(tape, shape):
        """the tape's tensors without the alignment gaps between them (which nothing writes)"""
        layout = ext.multiscale3d_tape_layout(*shape) if len(shape) == 4 else ext.multiscale_tape_layout(*shape)
        return torch.cat([tape[e[1]:e[1] + shape[0] * int(np.prod(e[2:]))] for e in layout])

    def inputs(shape):
        rng = np.random.default_rng(sum(shape))
        x = rng.standard_normal((shape[0], 2) + tuple(shape[1:]), dtype=np.float32)
        x[:, 1] = x[:, 1] > 0.84                                            # a 20 % occupancy channel
        gp = rng.standard_normal((shape[0], 1) + tuple(shape[1:]), dtype=np.float32)
        return torch.from_numpy(x).to(dev), torch.from_numpy(gp).to(dev)

    for ndim, cases in ((2, CASES2D), (3, CASES3D)):
        is3d = ndim == 3
        blob = torch.from_numpy(blob_from_state_dict(make_scalenet_weights(0, ndim=ndim), ndim)).to(dev)
        packed = ext.scalenet_pack(blob, is3d)
        packed_t = (ext.scalenet3d_pack_t if is3d else ext.scalenet_pack_t)(blob)
        fwd = ext.multiscale3d_forward_train if is3d else ext.multiscale_forward_train
        bwd = ext.multiscale3d_backward if is3d else ext.multiscale_backward
        plain = ext.multiscale3d_backward_plain if is3d else ext.multiscale_backward_plain
        emit(f"{ndim}d packed_t", packed_t)
        for shape, modes in cases:
            x, gp = inputs(shape)
            for mode in modes:
                p, tape = fwd(packed, x, mode)
                emit(f"{sid(shape)} {mode} p", p)
                emit(f"{sid(shape)} {mode} tape", entries(tape, shape))
                emit(f"{sid(shape)} {mode} grad", bwd(packed_t, gp, tape, mode))
                if mode == "fp32":
                    emit(f"{sid(shape)} {mode} grad_plain", plain(packed_t, gp, tape, mode))
                del p, tape
        if is3d:
            x, gp = inputs(BIG3D)
            _, tape = fwd(packed, x, "fp32_direct")
            emit(f"{sid(BIG3D)} fp32 on an fp32_direct tape grad", bwd(packed_t, gp, tape, "fp32"))
            del tape
            D, H, W = CASES3D[1][0][1:]
            q, h = [int(n * 0.25) for n in (D, H, W)], [int(n * 0.5) for n in (D, H, W)]
            for src, dst in ((q, h), (h, [D, H, W])):
                gd = torch.from_numpy(np.random.default_rng(21).standard_normal([2, 1] + dst).astype(np.float32)).to(dev)
                emit(f"trilinear_upsample_backward {sid(src)} <- {sid(dst)}", ext.trilinear_upsample_backward(gd, src))
        # the FluidNet-level forward and backward
        shape = cases[0][0]
        rng = np.random.default_rng(13)
        inp = torch.from_numpy(fluid_input(shape, rng)).to(dev)
        p, U, tape, scale, flags = (ext.fluidnet3d_forward_train if is3d else ext.fluidnet_forward_train)(packed, inp, 1e-5, "fp32")
        w_p = torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(np.float32)).to(dev)
        w_U = torch.from_numpy(rng.standard_normal(tuple(U.shape)).astype(np.float32)).to(dev)
        grad = (ext.fluidnet3d_backward if is3d else ext.fluidnet_backward)(packed_t, flags, scale, w_p, w_U, tape, "fp32")
        for name, t in (("p", p), ("U", U), ("tape", entries(tape, shape)), ("scale", scale), ("flags", flags), ("grad", grad)):
            emit(f"fluidnet{ndim}d {sid(shape)} fp32 {name}", t)
        del p, U, tape, grad
        # the inference forward: every precision mode where every launcher falls back and past the fill thresholds, the whole
        # FluidNet.forward, and (3D) the forward on nested z-crops
        for ishape, modes in INFER3D if is3d else INFER2D:
            x, _ = inputs(ishape)
            for mode in modes:
                emit(f"infer {sid(ishape)} {mode} p", ext.multiscale_forward(packed, x, mode))
        for name, t in zip(("p", "U"), ext.fluidnet_forward(packed, inp, 1e-5, "fp32")):
            emit(f"infer fluidnet{ndim}d {sid(shape)} fp32 {name}", t)
        if is3d:
            x, _ = inputs(CROP3D)
            for trim in (CROP_TRIM, [0, 0, 0, 0]):
                emit(f"infer {sid(CROP3D)} fp32 trim {trim} p", ext.multiscale_forward(packed, x, "fp32", trim))
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
