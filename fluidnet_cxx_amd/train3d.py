"""Training of the 3D pressure net on the native backend: `FluidNetTrain3D`, the Conv3d counterpart of train.FluidNetTrain.

It is the same class body (train._FluidNetTrainBase) on the 3D entry points of the extension: a torch.nn.Module with the reference
FluidNet's parameter names in Conv3d shapes (`multiScale.convN_4.encode.0.weight` (32,2,3,3,3) ...), so state_dict() / load_state_dict()
exchange checkpoints with `FluidNet(mconf with is3D)`.  forward(input_) takes (B,6,D,H,W) = [p, Ux, Uy, Uz, flags, density] and returns
(p, U) attached to ONE autograd function whose backward is the native backward pass (fnx_fluidnet3d_backward); `net.multiScale(x)` is
differentiable in the same way.  Under torch.no_grad() or .eval() both run the inference launches, so simulate(..., net, 'convnet')
takes the net on a 3D grid as it takes FluidNet.

Scope: the 3D ScaleNet configuration `FluidNet` accepts (mconf['is3D'] true), precision modes fp32 / fp32_f4 / fp32_f2 / fp32_direct,
gradients with respect to the parameters.  2D (train.FluidNetTrain), the bf16 modes, dropout and a gradient with respect to input_ raise.
"""
from .train import _FluidNetTrainBase


class FluidNetTrain3D(_FluidNetTrainBase):
    """input_ (B,6,D,H,W) = [p, Ux, Uy, Uz, flags, density] -> (p, U), differentiable with respect to the net's 34 parameters."""

    _NDIM = 3

    def _check_dim(self, mconf):
        if not mconf.get("is3D", False):
            raise ValueError("fluidnet_cxx_amd.FluidNetTrain3D: this class trains the 3D net only (mconf['is3D'] must be true; "
                             "FluidNetTrain trains the 2D net)")
