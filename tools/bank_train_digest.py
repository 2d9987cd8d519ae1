#!/usr/bin/env python3
"""One SHA-256 per tensor of the bank net's native training path (2D and 3D) on seeded inputs, to compare two builds bit for bit:

    python tools/bank_train_digest.py [TREE] [--out FILE]

TREE is the checkout whose built package is imported (default: the one this file sits in).  Only extension functions are used, so any
two trees that have them can be compared: run the tool once per tree, each in a process of its own, and compare the outputs line by line.
Per dimension: packed_t; at every shape p, the tape's entries without the alignment gaps and the gradient blob; at one shape the
FluidNet-level p, U, scale, flags, tape and gradient, and the inference whole forward's p and U.  The weights are He-scaled, so that every level and every ReLU carries gradient.
Shapes: 2D (1,4,4) has fewer than 64 cells, so the tail backward's masked lanes run; (3,36,68) is a batch with partial tiles;
(2,132,260) has 1 074 units of 64 cells on 512 workgroups, so a workgroup takes several.  3D (1,4,4,4) and (2,4,36,68) are the smallest
and a thin batch; (2,32,64,64) has 4 096 units, above the cap.  In 3D, D H W is always a multiple of 64 (each a multiple of 4), so the
masked lanes of the tail kernel, which serves both dimensions, are only reachable in 2D."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

from cnn_train_digest import fluid_input, sid

SHAPES = {2: [(1, 4, 4), (3, 36, 68), (2, 132, 260)], 3: [(1, 4, 4, 4), (2, 4, 36, 68), (2, 32, 64, 64)]}
FLUID_SHAPE = {2: (3, 36, 68), 3: (2, 4, 36, 68)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("tree", nargs="?", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from fluidnet_cxx_amd._ext import ext
    from fluidnet_cxx_amd.model import _bank_keys, blob_from_state_dict
    from fluidnet_cxx_amd.weights import banknet_layers, make_banknet_weights
    dev = torch.device("cuda")
    lines = []

    def emit(label, t):
        torch.cuda.synchronize()
        line = f"{label} {hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()}"
        print(line, flush=True)
        lines.append(line)

    for ndim in (2, 3):
        sfx = "3d" if ndim == 3 else ""
        fn = lambda name: getattr(ext, name.replace("#", sfx))      # noqa: E731
        w = make_banknet_weights(0, ndim=ndim)
        for L in banknet_layers():
            w[L["name"] + ".weight"] = (w[L["name"] + ".weight"].astype(np.float64) * np.sqrt(6.0 if L["relu"] else 3.0)).astype(np.float32)
            w[L["name"] + ".bias"] = (w[L["name"] + ".bias"].astype(np.float64) * 0.1).astype(np.float32)
        blob = torch.from_numpy(blob_from_state_dict(w, keys=_bank_keys())).to(dev)
        packed, packed_t = fn("banknet#_pack")(blob), fn("banknet#_pack_t")(blob)
        emit(f"{ndim}d packed_t", packed_t)

        def entries(tape, shape):
            """the tape's tensors without the alignment gaps between them (which nothing writes)"""
            return torch.cat([tape[e[1]:e[1] + shape[0] * int(np.prod(e[2:]))] for e in fn("banknet#_tape_layout")(*shape)])

        for shape in SHAPES[ndim]:
            rng = np.random.default_rng(sum(shape))
            x = rng.standard_normal((shape[0], 2) + shape[1:], dtype=np.float32)
            x[:, 1] = x[:, 1] > 0.84                                            # a 20 % occupancy channel
            gp = rng.standard_normal((shape[0], 1) + shape[1:], dtype=np.float32)
            x, gp = torch.from_numpy(x).to(dev), torch.from_numpy(gp).to(dev)
            p, tape = fn("banknet#_forward_train")(packed, x, "fp32")
            emit(f"{sid(shape)} p", p)
            emit(f"{sid(shape)} tape", entries(tape, shape))
            emit(f"{sid(shape)} grad", fn("banknet#_backward")(packed_t, x, gp, tape, "fp32"))
            del p, tape
        shape = FLUID_SHAPE[ndim]
        rng = np.random.default_rng(13)
        inp = torch.from_numpy(fluid_input(shape, rng)).to(dev)
        p, U, tape, scale, flags = fn("fluidnet_bank#_forward_train")(packed, inp, 1e-5, "fp32")
        w_p = torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(np.float32)).to(dev)
        w_U = torch.from_numpy(rng.standard_normal(tuple(U.shape)).astype(np.float32)).to(dev)
        grad = fn("fluidnet_bank#_backward")(packed_t, flags, scale, w_p, w_U, tape, "fp32")
        for name, t in (("p", p), ("U", U), ("scale", scale), ("flags", flags), ("tape", entries(tape, shape)), ("grad", grad)):
            emit(f"fluidnet bank {ndim}d {sid(shape)} {name}", t)
        # the inference whole forward on the same input (ext.fluidnet_bank_forward / fluidnet_bank3d_forward)
        for name, t in zip(("p", "U"), fn("fluidnet_bank#_forward")(packed, inp, 1e-5, "fp32")):
            emit(f"fluidnet bank {ndim}d {sid(shape)} infer {name}", t)
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
