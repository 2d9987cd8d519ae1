#!/usr/bin/env python3
"""Time the volume rendering operator (fnx_render_volume) next to its traffic model.

    python tools/render_time.py [--sizes 256x256x256,256x512x512] [--calls 200] [--warmup 20] [--out profiles/r13/render_time.txt]

Sizes are DxHxW.  Per size the pairs (view, light): the headlight, one perpendicular light and the backlight for a view along each axis.
Each case is `--calls` back-to-back calls after `--warmup` calls, timed as one span between two device events; the time per call stands
next to the bytes the kernels have to move and the share of the 8 TB/s HBM peak those bytes in that time are:
  general pair  light pass: rho 4 + flags 4 in, L 4 out;  view pass: rho 4 + flags 4 + L 4 in  = 24 B per cell, plus the image
  headlight     one march: rho 4 + flags 4 in                                                =  8 B per cell, plus the image
The volume is a developed-plume stand-in (a smooth blob of density in emptyDomain flags with one box): the kernels' time does not depend
on the values.  One line per case on stdout and in --out.  Under `rocprofv3 --kernel-trace --stats` it gives the per-kernel split."""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from fluidnet_cxx_amd import fluid                    # noqa: E402
from fluidnet_cxx_amd._ext import ext                 # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s
CASES = (("-z", "-z", "headlight"), ("-z", "-y", "perpendicular"), ("-z", "+z", "backlight"),
         ("-y", "-y", "headlight"), ("-y", "+x", "perpendicular"), ("-y", "+y", "backlight"),
         ("+x", "+x", "headlight"), ("+x", "-y", "perpendicular"), ("+x", "-x", "backlight"))


def volume(D, H, W, dev):
    z, y, x = (torch.linspace(-1, 1, n, device=dev) for n in (D, H, W))
    r2 = z.view(D, 1, 1) ** 2 + (y.view(1, H, 1) + 0.3) ** 2 + x.view(1, 1, W) ** 2
    density = torch.exp(-4.0 * r2).view(1, 1, D, H, W).contiguous()
    flags = torch.zeros(1, 1, D, H, W, device=dev)
    fluid.emptyDomain(flags)
    flags[:, :, D // 3:D // 3 + D // 8, H // 2:H // 2 + H // 8, W // 4:W // 4 + W // 8] = float(fluid.CellType.TypeObstacle)
    return density, flags


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256x256x256,256x512x512")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    assert a.calls >= 1
    dev = torch.device("cuda")
    lines = [f"# device: {ext.device_name()}; {a.calls} back-to-back calls per case after {a.warmup}, one device-event span; "
             f"model: 24 B/cell (headlight 8 B/cell) + image, share of {HBM_PEAK / 1e12:.0f} TB/s"]
    print(lines[0], flush=True)
    for size in a.sizes.split(","):
        D, H, W = (int(v) for v in size.split("x"))
        density, flags = volume(D, H, W, dev)
        cells = D * H * W
        for view, light, kind in CASES:
            for _ in range(a.warmup):
                img = fluid.renderVolume(density, flags, view, light)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.calls):
                img = fluid.renderVolume(density, flags, view, light)
            t1.record()
            t1.synchronize()
            ms = t0.elapsed_time(t1) / a.calls
            nbytes = cells * (8 if view == light else 24) + img.numel() * 4
            share = nbytes / (ms * 1e-3) / HBM_PEAK
            line = (f"{size:>12}  view {view} light {light} {kind:<13}  {ms * 1e3:8.1f} us/call  model {nbytes / 1e6:7.1f} MB  "
                    f"{nbytes / (ms * 1e-3) / 1e12:5.2f} TB/s = {100 * share:4.1f} % of peak")
            print(line, flush=True)
            lines.append(line)
        del density, flags
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
