#!/usr/bin/env python3
"""One SHA-256 each of p, U and density after three native steps with the 2D 'FluidNet' bank net (fnx_simulate_step_net: 'convnet' and
'hybrid', static promises 0, 3, 7 on a workspace of its own) on a developed plume at 2 x 64^2 and 1 x 136^2, to compare two builds bit
for bit -- what tools/step_launch_cases.py, which runs the ScaleNet, does not reach:

    python tools/bank_step_digest.py TREE > out.txt

The state, the bank FluidNet and the static promises are built as tools/bank_step_time.py builds them (bench.build_state on a plume
warmed up by Jacobi steps, its PromisedStep's 0, 3, 7 and bit 8 for 'hybrid'): that tool times these steps, this one hashes what they
leave, so a change to how one of them sets a step up belongs in both.  TREE is the checkout whose built package is imported; run the tool once per tree, each in a process of its own, and compare line by line."""
import hashlib
import os
import sys
tree = os.path.abspath(sys.argv[1])
sys.path.insert(0, os.path.join(tree, "tools"))
sys.path.insert(0, tree)
import torch
import bench
from fluidnet_cxx_amd import FluidNet, simulate
from fluidnet_cxx_amd._ext import ext
import fluidnet_cxx_amd
assert os.path.dirname(os.path.dirname(os.path.abspath(fluidnet_cxx_amd.__file__))) == tree
dev = torch.device("cuda:0")
for res, B in ((64, 2), (136, 1)):
    w = dict(res=res, D=1, method="jacobi", iters=28, kind="plume", batch=B)
    m = dict(bench.mconf_for(w), pcgTol=1e-5, pcgIter=30)
    bd = bench.build_state(w, dev)
    for _ in range(5):
        simulate(m, bd, None, "jacobi")
    bconf = dict(m, model="FluidNet")
    bank = FluidNet(bconf, dropout=False).to(dev).eval()
    for method in ("convnet", "hybrid"):
        st = {k: v.clone() for k, v in bd.items()}
        ws = torch.empty(ext.step_workspace_bytes(B, 1, res, res, False), dtype=torch.uint8, device=dev)
        for call in range(3):
            bits = (0, 3, 7)[call] | (8 if method == "hybrid" and call else 0)
            simulate(bconf, st, bank, method, workspace=ws, static_flags=bits)
        torch.cuda.synchronize()
        for k in ("p", "U", "density"):
            print(f"bank {method} {B}x{res}^2 {k} {hashlib.sha256(st[k].detach().cpu().contiguous().numpy().tobytes()).hexdigest()}", flush=True)
