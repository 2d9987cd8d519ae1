#!/usr/bin/env python3
"""Generate tests/golden/banknet.npz from the REFERENCE's lib.FluidNet with mconf['model'] = 'FluidNet' (the 16-channel bank net).

Runs where tools/make_golden.py runs (the reference tree, no GPU) and uses that file's helpers; it writes no other golden.  The
fixture holds inputs and outputs only:

  fwd<i>_U, fwd<i>_flags                      the input of FluidNet.forward at tests/banknet_reference.GOLDEN_SHAPES[i] (p and density are
                                              zero: neither reaches the output)
  fwd<i>_p, fwd<i>_Uout                       what the reference's forward returns
  fwd<i>_net_x, fwd<i>_net_p                  the net alone: what conv1 received and convOut returned inside that forward
  flags, UBC, UBCInvMask, densityBC, densityBCInvMask, step<k>_{U,density,p}, steps
                                              the 64x64 plume and its state after k = 1, 2 lib.simulate(..., 'convnet') steps

all with tests/banknet_reference.propagating_bank_weights(): under default-scale weights the plume's p is its bias constant and
max|U| stays the inlet's, so a step golden would be blind to the net.  The tool asserts that the states are finite, that p varies
by at least 10 % of max|p| over the fluid cells, and that the same steps with the net replaced by the float64 model of
tests/banknet_reference.py stay within 2e-6 |ref|max of the reference's states (a fifth of the tests' tolerance); a step that
misses the last check is not recorded (`steps` holds how many are).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "tests")]
import make_golden as G  # noqa: E402

MODEL_TOL = 2e-6


def bank_net(torch, lib, mconf, weights):
    net = lib.FluidNet(mconf, dropout=False)
    sd = net.state_dict()
    for k, v in weights.items():
        assert sd[k].shape == tuple(v.shape), (k, sd[k].shape, v.shape)
        sd[k].copy_(torch.from_numpy(v))
    net.eval()
    return net


class NetTap:
    """Records what the bank net receives (conv1's input) and returns (convOut's output) inside FluidNet.forward; with `model` the
    output is replaced by model(x) -- the float64 model in the reference's place."""

    def __init__(self, net, model=None):
        self.x = self.p = None
        self.model = model
        self.handles = [net.conv1.register_forward_pre_hook(self._pre), net.convOut.register_forward_hook(self._post)]

    def _pre(self, module, args):
        self.x = args[0].detach().clone()

    def _post(self, module, args, out):
        if self.model is not None:
            out = self.model(self.x).to(out.dtype)
        self.p = out.detach().clone()
        return out

    def remove(self):
        for h in self.handles:
            h.remove()


def plume_steps(torch, lib, mconf, net, n):
    bd = G.plume_setup(torch, lib, 64)
    states = []
    with torch.no_grad():
        for _ in range(n):
            lib.simulate(mconf, bd, net, "convnet")
            states.append({k: bd[k].numpy().copy() for k in ("U", "density", "p")})
    return bd, states


def main():
    torch, lib, _ = G.import_reference()
    from banknet_reference import GOLDEN_SHAPES, banknet_forward64, propagating_bank_weights
    mconf = G.plume_mconf(torch)
    mconf["model"] = "FluidNet"
    w = propagating_bank_weights()
    net = bank_net(torch, lib, mconf, w)
    out = {}
    rng = np.random.default_rng(11)
    for i, (B, H, W) in enumerate(GOLDEN_SHAPES):
        flags = G.make_flags(rng, B, 1, H, W, boxes=H >= 16)
        U = (rng.standard_normal((B, 2, 1, H, W)) * 0.5).astype(np.float32)
        zero = np.zeros((B, 1, 1, H, W), np.float32)
        tap = NetTap(net)
        with torch.no_grad():
            p, Uo = net(G.t(np.concatenate([zero, U, flags, zero], 1), torch))
        tap.remove()
        out.update({f"fwd{i}_U": U, f"fwd{i}_flags": flags, f"fwd{i}_p": p.numpy().copy(), f"fwd{i}_Uout": Uo.numpy().copy(),
                    f"fwd{i}_net_x": tap.x.numpy().copy(), f"fwd{i}_net_p": tap.p.numpy().copy()})
        assert all(np.isfinite(out[f"fwd{i}_{k}"]).all() for k in ("p", "Uout", "net_p"))
        print(f"  forward {(B, H, W)}: |net p|max {np.abs(tap.p.numpy()).max():.4f}")

    bd, ref = plume_steps(torch, lib, mconf, net, 2)
    tap = NetTap(net, lambda x: banknet_forward64(w, x.numpy()))
    _, mod = plume_steps(torch, lib, mconf, net, 2)
    tap.remove()
    fluid = bd["flags"].numpy() == 1
    steps = 0
    for k in (1, 2):
        r, m = ref[k - 1], mod[k - 1]
        assert all(np.isfinite(v).all() for v in r.values()), f"step {k}: a state is not finite"
        pf = r["p"][fluid]
        var = (pf.max() - pf.min()) / np.abs(r["p"]).max()
        assert var >= 0.1, f"step {k}: p varies by {var:.3f} of max|p| over the fluid cells: the golden would be blind to the net"
        dev = max(np.abs(m[f] - r[f]).max() / np.abs(r[f]).max() for f in ("U", "density", "p"))
        print(f"  step {k}: |p|max {np.abs(r['p']).max():.4f}, |U|max {np.abs(r['U']).max():.4f}, p variation {var:.3f}, "
              f"float64 model within {dev:.2e} |ref|max")
        if dev > MODEL_TOL:
            assert k > 1, f"step 1: the float64 model is {dev:.2e} |ref|max from the reference (limit {MODEL_TOL})"
            print(f"  step {k} NOT recorded: the float64 model is {dev:.2e} |ref|max from the reference (limit {MODEL_TOL})")
            break
        steps = k
        for f in ("U", "density", "p"):
            out[f"step{k}_{f}"] = r[f]
    out["steps"] = np.int32(steps)
    for k in ("flags", "UBC", "UBCInvMask", "densityBC", "densityBCInvMask"):
        out[k] = bd[k].numpy().copy()
    path = os.path.join(G.OUT, "banknet.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote banknet.npz ({os.path.getsize(path) / 1024:.0f} kB, {steps} plume step(s))")


if __name__ == "__main__":
    main()
