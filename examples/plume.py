#!/usr/bin/env python3
"""The reference's `pytorch/plume.py` main loop on this backend -- what a driver looks like after the switch.

    python examples/plume.py [--res 128] [--iters 200] [--out-iter 50] [--method jacobi|pcg|convnet|hybrid] [--weights CKPT]
                             [--pcg-warm] [--vorticity AMP] [--viscosity NU] [--depth N] [--weights3d CKPT] [--render] [--dyes N]
                             [--obstacle sphere|box|PATH.obj] [--folder out] [--restart]

Same structure as the reference driver (plume.py:66-178 setup, :231-424 loop): build the batch, `createPlumeBCs`, optional
restart from `<folder>/restart.pth`, echo the configuration as YAML, then `simulate()` per iteration and, every `out-iter`
iterations, the PNG panels, the VTK cell data and the restart file.  Only the import line differs from a reference-side
driver: `lib` -> `fluidnet_cxx_amd`.  `--method convnet --weights CKPT` projects with a trained net: CKPT is what examples/train.py
writes ({'state_dict', 'mconf', ...}), loaded the way the reference driver loads convModel_lastEpoch_best.pth (plume.py:119-123).
The checkpoint's own mconf['model'] picks the net, so no option does: 'ScaleNet' is the MultiScale net on the native step, 'FluidNet'
(what the reference's trainConfig.yaml ships) is its 16-channel bank net, 2D only; simulate() runs either in the native step.
`--depth N` (N > 1) runs the 3D plume on a N x res x res grid (jacobi, pcg and --vorticity as in 2D); there `--method convnet` takes
`--weights3d CKPT`, a checkpoint of `examples/train.py --depth N` (the 3D net; a 2D checkpoint given by --weights is refused) or one whose
mconf['model'] is 'FluidNet3D', the Conv3d bank net (N and res multiples of 4; simulate() runs it operator by operator).  `--render` adds volume renderings of the density (output.save_render: from the front, lit from above, and from the side)
to every output event.  `--method hybrid` takes the same checkpoints as convnet and projects with the converged solve started from the
net's pressure; `--dyes N` (1..3) carries N passive dyes along (batch_dict['scalars'], fluid.advectScalars: all of them through one pair
of line traces): the inlet is cut into N equal sectors along x and dye n enters through sector n at concentration 1, so the output
event's scalars_<it>.png shows in red, green and blue where each sector's fluid goes; `--pcg-warm` starts the 'pcg' solve from the previous step's pressure (mconf['pcgWarmStart']).
`--viscosity NU` sets mconf['viscosity'] (the velocity advected is fluid.addViscosity of U) for any --depth; the explicit update is
stable for NU * dt <= 1/4 in 2D and <= 1/6 in 3D (dt is 0.1 here).  The native step has no 3D viscous stage, so with --depth > 1 the
viscous step runs operator by operator (simulate(..., fused=False)).
`--obstacle sphere|box|PATH.obj` (with --depth N) puts a body into the 3D plume's way, centred at (res/2, 0.45 res, depth/2): a sphere of
radius 0.12 res (fluid.createSphere), the cube of that half-width (fluid.createBox3D), or the closed triangle mesh of a Wavefront OBJ
file scaled so that its longest side is 0.3 res (fluid.load_obj, fluid.voxelizeMesh) -- all written into flags on the device."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fluidnet_cxx_amd import fluid, simulate, output, load_restart, FluidNet      # noqa: E402   (reference: `import lib, lib.fluid as fluid`)


RENDER_VIEWS = (("-z", "-y"), ("+x", "-y"))               # (view, light): from the front and from the side, lit from above


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out-iter", type=int, default=50)
    ap.add_argument("--method", default="jacobi", choices=["jacobi", "pcg", "convnet", "hybrid"])
    ap.add_argument("--weights", default=None, metavar="CKPT", help="checkpoint of examples/train.py (needed by --method convnet and hybrid)")
    ap.add_argument("--pcg-warm", action="store_true",
                    help="--method pcg: start each solve from the previous step's pressure (mconf['pcgWarmStart'])")
    ap.add_argument("--vorticity", type=float, default=0.0, metavar="AMP",
                    help="vorticity confinement amplitude (mconf['vorticityConfinementAmp'], no reference key; 0 = off)")
    ap.add_argument("--viscosity", type=float, default=0.0, metavar="NU",
                    help="kinematic viscosity (mconf['viscosity'], 2D and 3D; 0 = off).  The explicit update is stable for "
                         "NU * dt <= 1/6 in 3D and <= 1/4 in 2D (dt = 0.1); nothing checks it")
    ap.add_argument("--weights3d", default=None, metavar="CKPT",
                    help="checkpoint of examples/train.py --depth N (needed by --method convnet and hybrid with --depth > 1)")
    ap.add_argument("--depth", type=int, default=1, metavar="N", help="cells along z; 1 (default) is the 2D plume, N > 1 the 3D one")
    ap.add_argument("--render", action="store_true", help="write volume renderings (render_<view>_<it>.png) with every output event")
    ap.add_argument("--dyes", type=int, default=None, metavar="N",
                    help="carry N passive dyes (1..3), one per sector of the inlet along x (batch_dict['scalars']); default: none")
    ap.add_argument("--obstacle", default=None, metavar="sphere|box|PATH.obj",
                    help="a body in the 3D plume's way (needs --depth N): a sphere, a cube, or the closed mesh of an OBJ file")
    ap.add_argument("--folder", default="plume_out")
    ap.add_argument("--restart", action="store_true")
    return ap


def parse_args(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    uses_net = a.method in ("convnet", "hybrid")
    if a.pcg_warm and a.method != "pcg":
        ap.error("--pcg-warm is only read by --method pcg")
    if a.viscosity < 0:
        ap.error("--viscosity must not be negative")
    if a.dyes is not None and not 1 <= a.dyes <= 3:
        ap.error("--dyes must be 1, 2 or 3 (the channels of scalars_<it>.png)")
    if a.depth < 1 or a.depth == 2:
        ap.error("--depth must be 1 (2D) or at least 3")
    if a.obstacle is not None:
        if a.depth == 1:
            ap.error("--obstacle places a 3D body: it needs --depth N (N > 1)")
        if a.obstacle not in ("sphere", "box") and not a.obstacle.lower().endswith(".obj"):
            ap.error("--obstacle must be 'sphere', 'box' or the path of a .obj file")
    if a.depth > 1:
        if a.weights is not None:
            ap.error("--weights with --depth > 1: no 3D weights can be trained here by the 2D trainer this checkpoint comes from; "
                     "train the 3D net with examples/train.py --depth N and pass its checkpoint as --weights3d CKPT")
        if uses_net != (a.weights3d is not None):
            ap.error(f"--method {a.method if uses_net else 'convnet'} with --depth > 1 needs --weights3d CKPT, and --weights3d is only read by "
                     "--method convnet and hybrid")
        if uses_net and a.depth < 4:
            ap.error(f"--method {a.method} needs --depth of at least 4 (the net's three scales)")
        return a
    if a.weights3d is not None:
        ap.error("--weights3d is a 3D checkpoint: it needs --depth N (N > 1)")
    if uses_net != (a.weights is not None):
        ap.error(f"--method {a.method if uses_net else 'convnet'} needs --weights CKPT, and --weights is only read by --method convnet and hybrid")
    return a


def add_dyes(batch_dict, n):
    """n dyes on a batch createPlumeBCs has been through: scalars = 0, and channel c enters at concentration 1 through sector c of
    the inlet (n equal sectors along x of the cells where densityBC is set), under the density's mask"""
    dbc, mask = batch_dict["densityBC"], batch_dict["densityBCInvMask"]
    inlet = dbc[0, 0] != 0                                                # (D, H, W)
    xs = torch.nonzero(inlet.any(0).any(0)).flatten()
    x0, width = int(xs.min()), int(xs.max()) - int(xs.min()) + 1
    sector = ((torch.arange(dbc.size(4), device=dbc.device) - x0) * n).div(width, rounding_mode="floor")   # (W,)
    bc = torch.zeros((1, n) + tuple(dbc.shape[2:]), dtype=dbc.dtype, device=dbc.device)
    for c in range(n):
        bc[0, c] = (inlet & (sector == c)).to(dbc.dtype)
    batch_dict["scalars"] = torch.zeros_like(bc)
    batch_dict["scalarsBC"] = bc
    batch_dict["scalarsBCInvMask"] = mask.expand_as(bc).contiguous()


def add_obstacle(batch_dict, what, res, depth):
    """the body of --obstacle, centred at (res/2, 0.45 res, depth/2), written into batch_dict['flags'] on the device"""
    cx, cy, cz, r = res / 2, 0.45 * res, depth / 2, 0.12 * res
    if what == "sphere":
        fluid.createSphere(batch_dict, cx, cy, cz, r)
    elif what == "box":
        fluid.createBox3D(batch_dict, cx - r, cx + r, cy - r, cy + r, cz - r, cz + r)
    else:
        v, f = fluid.load_obj(what)
        if len(v) == 0 or len(f) == 0:
            sys.exit(f"plume.py: {what} holds no vertices or no faces")
        lo, hi = v.min(axis=0), v.max(axis=0)
        v = (v - (lo + hi) / 2) * (0.3 * res / float((hi - lo).max())) + (cx, cy, cz)
        dev = batch_dict["flags"].device
        # check=True: an open or broken mesh raises here, before the first step (the one synchronisation of the setup)
        fluid.voxelizeMesh(batch_dict, torch.from_numpy(v).float().to(dev), torch.from_numpy(f).to(dev))


def main(argv=None):
    a = parse_args(argv)
    cuda = torch.device("cuda")
    # plumeConfig.yaml:29-76 (the keys simulate() reads)
    simConf = dict(dt=0.1, maccormackStrength=0.6, sampleOutsideFluid=False, buoyancyScale=0.25, gravityScale=0, viscosity=0,
                   correctScalar=False, gravityVec=dict(x=0.0, y=-1.0, z=0.0), operatingDensity=0.0, pTol=0.0, jacobiIter=28,
                   simMethod=a.method, resX=a.res, resY=a.res, maxIter=a.iters, outputFolder=a.folder)
    if a.method in ("pcg", "hybrid"):                     # the converged solve (fluid.solveLinearSystemPCG), cold or from a guess
        simConf.update(pcgTol=1e-5, pcgIter=50, pcgWarmStart=bool(a.pcg_warm))
    if a.vorticity > 0:                                   # puts back the small-scale rotation the advection smooths away
        simConf.update(vorticityConfinementAmp=a.vorticity)
    if a.viscosity > 0:                                   # simulate.py:66-69: the velocity advected is addViscosity(U)
        simConf.update(viscosity=a.viscosity)
    net = None
    if a.method in ("convnet", "hybrid"):                 # plume.py:119-123
        state = torch.load(a.weights3d if a.depth > 1 else a.weights, map_location="cpu", weights_only=False)
        mconf = state["mconf"]
        assert bool(mconf.get("is3D", False)) == (a.depth > 1), "the checkpoint's net has another dimension than the grid"
        if mconf.get("model", "ScaleNet") == "FluidNet3D" and (a.depth % 4 or a.res % 4):
            sys.exit(f"plume.py: the checkpoint's net is the 'FluidNet3D' bank net, which adds three levels: --depth {a.depth} and --res {a.res} "
                     "must be multiples of 4")
        net = FluidNet(mconf, dropout=False)
        net = net.cuda()
        net.load_state_dict(state["state_dict"])
        net.eval()
        simConf.update(normalizeInputThreshold=mconf.get("normalizeInputThreshold", 1e-5))
    os.makedirs(a.folder, exist_ok=True)
    resX = resY = a.res
    resZ = a.depth
    # plume.py:131-163
    p = torch.zeros(1, 1, resZ, resY, resX, dtype=torch.float, device=cuda)
    U = torch.zeros(1, 3 if resZ > 1 else 2, resZ, resY, resX, dtype=torch.float, device=cuda)
    flags = torch.zeros(1, 1, resZ, resY, resX, dtype=torch.float, device=cuda)
    density = torch.zeros(1, 1, resZ, resY, resX, dtype=torch.float, device=cuda)
    fluid.emptyDomain(flags)
    batch_dict = dict(p=p, U=U, flags=flags, density=density)
    fluid.createPlumeBCs(batch_dict, 0.1, 2, 0.145)
    if a.obstacle is not None:                            # (a restart brings its flags, body included)
        add_obstacle(batch_dict, a.obstacle, a.res, a.depth)
    it = 0
    restart_file = os.path.join(a.folder, "restart.pth")
    if a.restart:                                         # plume.py:168-175
        assert os.path.isfile(restart_file), "Restart file does not exists."
        batch_dict, it = load_restart(restart_file, cuda)
        print("Restarting from checkpoint at it = " + str(it))
    if a.dyes and "scalars" not in batch_dict:
        add_dyes(batch_dict, a.dyes)
    output.echo_config(os.path.join(a.folder, "plumeConfig.yaml"), simConf)      # plume.py:176-178
    while it < a.iters:                                   # plume.py:231-424
        # (the native step has no 3D viscous stage: that one step runs operator by operator)
        simulate(simConf, batch_dict, net, a.method, fused=not (a.depth > 1 and a.viscosity > 0))
        if it % a.out_iter == 0:
            print("It = " + str(it))
            output.save_state(a.folder, it, batch_dict, render=RENDER_VIEWS if a.render else None)
        it += 1
    return batch_dict, it


if __name__ == "__main__":
    main()
