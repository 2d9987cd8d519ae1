"""Training of the 3D pressure net, end to end on the device: the 3D counterpart of fluidnet_cxx_amd/training.py.

    from fluidnet_cxx_amd.training3d import train3d, train_bank3d, SceneSampler3D, fluidnet_loss3d

The reference has no 3D training at all (its FluidNet is Conv2d only), so nothing here follows a reference file: the loop is the 2D one
(fluidnet_cxx_amd/training.py holds the bodies both share, in private bases) around `FluidNetTrain3D`, with scenes from fnx_scene_obstacles3d /
fnx_scene_turbulence3d and the loss from fnx_train_loss3d.  `SceneSampler3D` hands out data (B,6,D,H,W) = [p of the previous step, Ux,
Uy, Uz before the projection, flags, density] and target (B,5,D,H,W) = [p, U, density] of the converged ('pcg') projection, in the
library's default 3D semantics (no reference quirks).  The checkpoint has the 2D keys, so `FluidNet(ck["mconf"])` loads
`ck["state_dict"]` and `examples/plume.py --depth N --method convnet --weights3d` runs it.

3D only: a 2D grid (is3D false, or fewer than the 4 planes the net's three scales need) is refused before the device is touched;
fluidnet_cxx_amd.training trains the 2D net.
"""
import torch

from ._ext import ext
from .train import FluidNetBankTrain3D
from .train3d import FluidNetTrain3D
from .training import MCONF_DEFAULTS, TCONF_DEFAULTS, _Dim, _SceneSamplerBase, _evaluate, _loss_fn, _train

# up to four balls / boxes whose centres lie within 0.3 min(D, H, W) of the grid centre and whose radius / half extent is 0.03 .. 0.12
# min(D, H, W): from 20 cells per axis on they stay clear of the border shell.  The turbulence is scaled to grids of 64 cells.
SCENE3D_DEFAULTS = dict(n_min=0, n_max=4, centre_min=-0.3, centre_max=0.3, size_min=0.03, size_max=0.12, octaves=3, wavelength=16.0,
                        amplitude=4.0, density_scale=1.0)
MCONF3D_DEFAULTS = dict(MCONF_DEFAULTS, is3D=True, inputDim=3)
TCONF3D_DEFAULTS = dict(TCONF_DEFAULTS, res=64, batch=4)


def _refuse_2d(what, mconf=None, depth=None):
    if mconf is not None and not mconf.get("is3D", False):
        raise ValueError(f"fluidnet_cxx_amd.training3d.{what}: training here is 3D only (is3D is not set; training.py trains the 2D net)")
    if depth is not None and int(depth) < 4:
        raise ValueError(f"fluidnet_cxx_amd.training3d.{what}: training here is 3D only (depth {int(depth)}: the net's three scales need 4 planes)")


_LossFn3D = _loss_fn(ext.train_loss3d)


def fluidnet_loss3d(out_p, out_U, flags, target_p, lambdas):
    """training.fluidnet_loss for out_p (B,1,D,H,W), out_U (B,3,D,H,W): (total, terms), differentiable with respect to out_p and out_U
    through one kernel (fnx_train_loss3d); div = velocityDivergence(out_U, flags) on the 3D grid, bit for bit."""
    lam = [float(v) for v in lambdas]
    assert len(lam) == 4, "lambdas = (pL2Lambda, divL2Lambda, pL1Lambda, divL1Lambda)"
    _refuse_2d("fluidnet_loss3d", depth=flags.size(2) if flags.dim() == 5 else 1)
    if target_p is not None:
        target_p = target_p.contiguous()
    return _LossFn3D.apply(out_p, out_U, flags.contiguous(), target_p, lam)


class SceneSampler3D(_SceneSamplerBase):
    """B scenes of D x H x W cells advancing in lock step; ages, redraws, per-call choices and the state dict are those of
    training.SceneSampler.  A redraw: obstacles, turbulence and density from the 3D scene kernels, setWallBcs, one 'pcg' projection.
    next(): `stride` full 'pcg' steps, then 3D advection, buoyancy and setWallBcs on the operator path -> data (B,6,D,H,W), the 'pcg'
    projection -> target (B,5,D,H,W).  The gravity direction is one of +-x / +-y / +-z."""

    _IS3D = True

    def __init__(self, mconf, B, D, H, W, seed, device="cuda", scene=None, sceneLength=32, stride=2):
        mconf = dict(MCONF3D_DEFAULTS, **mconf)
        _refuse_2d("SceneSampler3D", mconf, D)
        self.D, self.H, self.W = int(D), int(H), int(W)
        self._init(mconf, B, seed, device, SCENE3D_DEFAULTS, scene, sceneLength, stride)

    def draw(self, ids):
        """(flags, U, density) of the scenes `ids`, as the kernels give them (no boundary condition applied)"""
        s = self.scene
        t = torch.tensor([int(i) for i in ids], dtype=torch.int32, device=self.device)
        flags = ext.scene_obstacles3d(t, self.D, self.H, self.W, self.seed, s["n_min"], s["n_max"], s["centre_min"], s["centre_max"],
                                      s["size_min"], s["size_max"])
        U, rho = ext.scene_turbulence3d(t, self.D, self.H, self.W, self.seed, s["octaves"], s["wavelength"], s["amplitude"],
                                        s["density_scale"], True)
        return flags, U, rho

    def _gravity(self, h):
        return ("x", "y", "z")[(h >> 1) % 3], float((h & 1) * 2 - 1)


_DIM3 = _Dim(3, FluidNetTrain3D, lambda mconf, B, dims, *rest: SceneSampler3D(mconf, B, dims[0], dims[1], dims[2], *rest), fluidnet_loss3d,
             ext.train_loss3d)
# the same with the Conv3d 16-channel bank net in the middle (mconf['model'] = 'FluidNet3D')
_DIM3_BANK = _Dim(3, FluidNetBankTrain3D, _DIM3.sampler, fluidnet_loss3d, ext.train_loss3d)


def evaluate3d(net, batches, lambdas):
    """training.evaluate on 3D batches: the held-out loss, divL2 of the net's U and divL2 of the U it was given"""
    return _evaluate(_DIM3, net, batches, lambdas)


def train3d(mconf=None, tconf=None, device="cuda", out=None, resume=None, log=None):
    """training.train for the 3D net.  mconf: MCONF3D_DEFAULTS; tconf: TCONF3D_DEFAULTS, the grid from 'res' or from 'D', 'H', 'W'.
    FluidNetTrain3D + kaiming_init + Adam + ReduceLROnPlateau, the long-term rollout with the net as the projection, a bit-exact resume
    and the checkpoint keys of the 2D run."""
    mconf = dict(MCONF3D_DEFAULTS, **(mconf or {}))
    tconf = dict(TCONF3D_DEFAULTS, **(tconf or {}))
    D, H, W = (int(tconf.get(k, tconf["res"])) for k in ("D", "H", "W"))
    _refuse_2d("train3d", mconf, D)
    if mconf.get("model", "ScaleNet") == "FluidNet3D":
        raise ValueError("train3d: training the 'FluidNet3D' model is not built into train3d, which trains the 3D ScaleNet; "
                         "train_bank3d trains the Conv3d bank net")
    return _train(_DIM3, mconf, tconf, (D, H, W), device, out, resume, log)


def train_bank3d(mconf=None, tconf=None, device="cuda", out=None, resume=None, log=None):
    """train3d for the Conv3d bank net: mconf['model'] is 'FluidNet3D' (set if absent), the net FluidNetBankTrain3D, D, H and W multiples
    of 4.  The checkpoint's mconf carries the model name, so FluidNet(ck["mconf"]) loads ck["state_dict"]."""
    mconf = dict(MCONF3D_DEFAULTS, **dict({"model": "FluidNet3D"}, **(mconf or {})))
    tconf = dict(TCONF3D_DEFAULTS, **(tconf or {}))
    D, H, W = (int(tconf.get(k, tconf["res"])) for k in ("D", "H", "W"))
    _refuse_2d("train_bank3d", mconf, D)
    return _train(_DIM3_BANK, mconf, tconf, (D, H, W), device, out, resume, log)
