#!/usr/bin/env python3
"""Time the training path of the pressure net (2D and 3D) next to its inference forward.

    python tools/cnn_train_time.py [--cases 128x16,128x64,1024x1] [--cases3d 64x4,128x1] [--modes fp32_direct,fp32] [--reps 10]
                                   [--plain] [--out profiles/r09/cnn_train_time.txt]

Per case (resolution x batch) and mode: the inference forward (ext.multiscale_forward), the training forward (the same launches
into the tape + the 8-channel tensor), the backward (ext.multiscale_backward) and forward + backward, each as `--reps` back-to-back
calls between one pair of HIP events (no host synchronisation inside), median of 3 such runs; then the repacking of both weight
images, which a training step pays once per optimiser step.  --plain also times the backward with the plain weight-gradient
kernel for every layer (ext.multiscale_backward_plain), i.e. what the MFMA weight-gradient kernel replaces.
--cases3d (cube edge x batch; --cases3d "" leaves them out, as --cases "" leaves the 2D ones out) does the same for the 3D net through
ext.multiscale3d_forward_train / multiscale3d_backward(_plain).
One line per measurement on stdout and in --out.  Under `rocprofv3 --kernel-trace --stats` it gives the per-kernel split."""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from fluidnet_cxx_amd._ext import ext                                   # noqa: E402
from fluidnet_cxx_amd.model import blob_from_state_dict                 # noqa: E402
from fluidnet_cxx_amd.weights import make_scalenet_weights              # noqa: E402


def timed(fn, reps, runs=3):
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / reps)
    return float(np.median(ts))


def time_3d(a, dev, emit):
    """the 3D net: the same four measurements per case (cube edge x batch) and mode"""
    blob = torch.from_numpy(blob_from_state_dict(make_scalenet_weights(0, ndim=3), 3)).to(dev)
    packed, packed_t = ext.scalenet_pack(blob, True), ext.scalenet3d_pack_t(blob)
    for case in a.cases3d.split(","):
        res, B = (int(v) for v in case.split("x"))
        rng = np.random.default_rng(res + B)
        x = torch.from_numpy(rng.standard_normal((B, 2, res, res, res), dtype=np.float32)).to(dev)
        x[:, 1] = (x[:, 1] > 0.84).float()                                 # a 20 % occupancy channel
        gp = torch.from_numpy(rng.standard_normal((B, 1, res, res, res), dtype=np.float32)).to(dev)
        for mode in a.modes.split(","):
            _, tape = ext.multiscale3d_forward_train(packed, x, mode)
            ext.multiscale3d_backward(packed_t, gp, tape, mode)             # warm-up
            ext.multiscale_forward(packed, x, mode, [])
            torch.cuda.synchronize()
            inf = timed(lambda: ext.multiscale_forward(packed, x, mode, []), a.reps)
            fwd = timed(lambda: ext.multiscale3d_forward_train(packed, x, mode), a.reps)
            bwd = timed(lambda: ext.multiscale3d_backward(packed_t, gp, tape, mode), a.reps)
            both = timed(lambda: ext.multiscale3d_backward(packed_t, gp, ext.multiscale3d_forward_train(packed, x, mode)[1], mode), a.reps)
            line = (f"{res:>5}^3 B={B:<3} {mode:<12} inference forward {inf:8.3f}  training forward {fwd:8.3f}  backward {bwd:8.3f}  "
                    f"forward + backward {both:8.3f}  backward / inference forward {bwd / inf:5.2f}  tape {tape.numel() * 4 / 2**30:.2f} GiB")
            if a.plain:
                plain = timed(lambda: ext.multiscale3d_backward_plain(packed_t, gp, tape, mode), 1, runs=1)
                line += f"  backward with the plain weight gradient {plain:9.3f}"
            emit(line)
            del tape
            torch.cuda.empty_cache()
    pack = timed(lambda: (ext.scalenet_pack(blob, True), ext.scalenet3d_pack_t(blob)), a.reps)
    emit(f"repacking both 3D weight images (once per optimiser step) {pack:8.3f}")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="128x16,128x64,1024x1")
    ap.add_argument("--cases3d", default="64x4,128x1")
    ap.add_argument("--modes", default="fp32_direct,fp32")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    dev = torch.device("cuda")
    blob = torch.from_numpy(blob_from_state_dict(make_scalenet_weights(0))).to(dev)
    packed, packed_t = ext.scalenet_pack(blob, False), ext.scalenet_pack_t(blob)
    lines = [f"# device: {ext.device_name()}; {a.reps} back-to-back calls per event pair, median of 3; ms per call"]
    print(lines[0], flush=True)

    def emit(line):
        print(line, flush=True)
        lines.append(line)
    for case in [c for c in a.cases.split(",") if c]:
        res, B = (int(v) for v in case.split("x"))
        rng = np.random.default_rng(res + B)
        x = torch.from_numpy(rng.standard_normal((B, 2, res, res), dtype=np.float32)).to(dev)
        x[:, 1] = (x[:, 1] > 0.84).float()                                 # a 20 % occupancy channel
        gp = torch.from_numpy(rng.standard_normal((B, 1, res, res), dtype=np.float32)).to(dev)
        for mode in a.modes.split(","):
            _, tape = ext.multiscale_forward_train(packed, x, mode)
            ext.multiscale_backward(packed_t, gp, tape, mode)               # warm-up
            ext.multiscale_forward(packed, x, mode, [])
            torch.cuda.synchronize()
            inf = timed(lambda: ext.multiscale_forward(packed, x, mode, []), a.reps)
            fwd = timed(lambda: ext.multiscale_forward_train(packed, x, mode), a.reps)
            bwd = timed(lambda: ext.multiscale_backward(packed_t, gp, tape, mode), a.reps)
            both = timed(lambda: ext.multiscale_backward(packed_t, gp, ext.multiscale_forward_train(packed, x, mode)[1], mode), a.reps)
            line = (f"{res:>5}^2 B={B:<3} {mode:<12} inference forward {inf:8.3f}  training forward {fwd:8.3f}  backward {bwd:8.3f}  "
                    f"forward + backward {both:8.3f}  backward / inference forward {bwd / inf:5.2f}  tape {tape.numel() * 4 / 2**30:.2f} GiB")
            if a.plain:
                plain = timed(lambda: ext.multiscale_backward_plain(packed_t, gp, tape, mode), 1, runs=2)
                line += f"  backward with the plain weight gradient {plain:9.3f}"
            emit(line)
            del tape
            torch.cuda.empty_cache()
    if a.cases:
        pack = timed(lambda: (ext.scalenet_pack(blob, False), ext.scalenet_pack_t(blob)), a.reps)
        emit(f"repacking both weight images (once per optimiser step) {pack:8.3f}")
    if a.cases3d:
        time_3d(a, dev, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
