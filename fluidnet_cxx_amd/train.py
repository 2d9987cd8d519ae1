"""Training of the 2D pressure net on the native backend (reference pytorch/fluid_net_train.py:270-285, 356-375).

`FluidNetTrain(mconf, dropout=False)` is a torch.nn.Module with the reference FluidNet's parameter names and shapes
(`multiScale.convN_4.encode.0.weight` ...), so state_dict() / load_state_dict() exchange checkpoints with `FluidNet` and with the
reference, and torch.optim.* / zero_grad() work on it.  forward(input_) returns (p, U) attached to ONE autograd function whose
backward is the native backward pass (fnx_fluidnet_backward); `net.multiScale(x)` is differentiable in the same way.  Under
torch.no_grad() or .eval() both run the inference launches.  Gradients come from the kernels: torch only carries the tensors.

`FluidNetBankTrain(mconf, dropout=False)` is the same for the reference's 16-channel bank net (mconf['model'] = 'FluidNet',
model.py:177-209; csrc/fnx_banknet_train.hip): the twelve parameters `conv1`, `convBank.block.0`, `convBank.block.2`, `conv2`, `conv3`,
`convOut`, and `net.bank(x)` where the ScaleNet has `net.multiScale(x)`.  Both nets share the autograd functions; an `_Api` names the
extension's entry points of each.

`FluidNetBankTrain3D` is that for the Conv3d bank net (mconf['model'] = 'FluidNet3D'; csrc/fnx_banknet3d_train.hip).

Scope: the 2D configurations `FluidNet` accepts, precision modes fp32 / fp32_f4 / fp32_f2 / fp32_direct, gradients with respect to
the parameters.  3D (but for FluidNetBankTrain3D and train3d.FluidNetTrain3D), the bf16 modes, dropout and a gradient with respect to
input_ raise.
"""
from collections import OrderedDict

import torch

from ._ext import ext
from .model import _BANK_UNUSED_PREFIXES, _UNUSED_PREFIXES, NET_EXT
from .weights import banknet_layers, make_banknet_weights, make_scalenet_weights, scalenet_layers

_TRAIN_MODES = ("fp32", "fp32_f4", "fp32_f2", "fp32_direct")


def _no_input_grad(t, what):
    if t.requires_grad:
        raise RuntimeError(f"fluidnet_cxx_amd.FluidNetTrain: {what}.requires_grad is set, but the native backward pass gives gradients "
                           "with respect to the parameters only (the training data is a leaf without grad in the reference too)")


def _split(blob, shapes):
    """the gradient blob (the layout of model.blob_from_state_dict) as one view per parameter"""
    grads, off = [], 0
    for shp in shapes:
        grads.append(blob[off:off + shp.numel()].view(shp))
        off += shp.numel()
    return grads


class _Api:
    """what differs between the 2D net, the 3D net and the two bank nets: the extension's entry points (model.NET_EXT's row) and the
    number of velocity components (only the dimension and the model are state, so a module that holds one copies and pickles as before)"""

    bank = False                         # (a class default: an _Api pickled before the bank net existed has no such attribute)

    def __init__(self, ndim, bank=False):
        self.ndim, self.nc, self.bank = ndim, ndim, bank

    @property
    def _row(self):
        return NET_EXT[self.bank, self.ndim]

    def _fn(self, op):
        return getattr(ext, self._row[op])

    def pack(self, blob):
        return self._fn("pack")(blob, *self._row["pack_args"]), self._fn("pack_t")(blob)

    def net_forward(self, packed, x, mode):
        """the inference launches of the net alone"""
        return self._fn("forward")(packed, x, mode, *self._row["forward_args"])

    def net_backward(self, packed_t, x, gp, tape, mode):
        """(the bank net's backward reads the net's input again: conv1's weight gradient)"""
        return self._fn("backward")(packed_t, *((x,) if self._row["backward_x"] else ()), gp, tape, mode)

    fluidnet_forward = property(lambda self: self._fn("whole_forward"))          # the inference launches of FluidNet.forward
    multiscale_forward_train = property(lambda self: self._fn("forward_train"))
    fluidnet_forward_train = property(lambda self: self._fn("whole_forward_train"))
    fluidnet_backward = property(lambda self: self._fn("whole_backward"))


class _MultiScaleFn(torch.autograd.Function):
    """x (B,2,H,W), (B,2,1,H,W) or, for the 3D net, (B,2,D,H,W) -> p; the parameters ride along so that autograd routes their gradients"""

    @staticmethod
    def forward(ctx, x, owner, *params):
        packed, ctx.packed_t = owner._packed(x.device)
        p, ctx.tape = owner._api.multiscale_forward_train(packed, x, owner.precision_mode)
        ctx.mode, ctx.shapes, ctx.api = owner.precision_mode, [q.shape for q in params], owner._api
        ctx.x = x if ctx.api._row["backward_x"] else None
        return p

    @staticmethod
    def backward(ctx, gp):
        blob = ctx.api.net_backward(ctx.packed_t, ctx.x, gp.contiguous(), ctx.tape, ctx.mode)
        return (None, None) + tuple(_split(blob, ctx.shapes))


class _FluidNetFn(torch.autograd.Function):
    """input_ (B,5,1,H,W) or, for the 3D net, (B,6,D,H,W) -> (p, U)   (model.py:76-227 around the taped net)"""

    @staticmethod
    def forward(ctx, input_, owner, *params):
        packed, ctx.packed_t = owner._packed(input_.device)
        p, U, ctx.tape, ctx.scale, ctx.flags = owner._api.fluidnet_forward_train(packed, input_, owner.threshold, owner.precision_mode)
        ctx.mode, ctx.shapes, ctx.api = owner.precision_mode, [q.shape for q in params], owner._api
        return p, U

    @staticmethod
    def backward(ctx, gp, gU):
        # a loss that leaves out one of the two outputs delivers None for it
        gp = ctx.flags.new_zeros(ctx.flags.shape) if gp is None else gp.contiguous()
        gU = ctx.flags.new_zeros((ctx.flags.size(0), ctx.api.nc) + tuple(ctx.flags.shape[2:])) if gU is None else gU.contiguous()
        blob = ctx.api.fluidnet_backward(ctx.packed_t, ctx.flags, ctx.scale, gp, gU, ctx.tape, ctx.mode)
        return (None, None) + tuple(_split(blob, ctx.shapes))


class _Conv(torch.nn.Module):
    """the parameters of one convolution, under the names torch.nn.Conv2d gives them"""

    def __init__(self, weight, bias):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.from_numpy(weight).clone())
        self.bias = torch.nn.Parameter(torch.from_numpy(bias).clone())


class _Holder(torch.nn.Module):
    pass


def _repack(owner, device):
    """(packed, packed_t) of owner._ordered() on `device`, cached in owner._key / owner._images: repacked on the device whenever a
    parameter was written (an optimiser step, load_state_dict, .to())"""
    params = owner._ordered()
    key = (str(device),) + tuple((p.data_ptr(), p._version) for p in params)
    if key != owner._key:
        blob = torch.cat([p.detach().reshape(-1) for p in params]).to(device=device, dtype=torch.float32).contiguous()
        owner._images = owner._api.pack(blob)
        owner._key = key
    return owner._images


class _MultiScaleTrain(torch.nn.Module):
    """x (B,2,H,W) -> p (B,1,H,W), or (B,2,D,H,W) -> (B,1,D,H,W) with ndim = 3   (multi_scale_net.py:118-127), differentiable with
    respect to the parameters"""

    def __init__(self, precision_mode, ndim=2):
        super().__init__()
        self.precision_mode = precision_mode
        self._api = _Api(ndim)
        w = make_scalenet_weights(0, ndim=ndim)
        for L in scalenet_layers(2, ndim):
            parts = L["name"].split(".")[1:]             # convN_4, encode, 0  |  final
            mod = self
            for part in parts[:-1]:
                if not hasattr(mod, part):
                    mod.add_module(part, _Holder())
                mod = getattr(mod, part)
            mod.add_module(parts[-1], _Conv(w[L["name"] + ".weight"], w[L["name"] + ".bias"]))
        self._key = None
        self._images = None

    def _ordered(self):
        """the 34 parameters in the blob's order (scalenet_layers(): weight, bias per convolution)"""
        named = dict(self.named_parameters())
        return [named[L["name"].split(".", 1)[1] + sfx] for L in scalenet_layers(2, self._api.ndim) for sfx in (".weight", ".bias")]

    def _packed(self, device):
        """(packed, packed_t) for the current parameter values on `device`"""
        return _repack(self, device)

    def forward(self, x):
        x = x.contiguous()
        if not (self.training and torch.is_grad_enabled()):
            return self._api.net_forward(self._packed(x.device)[0], x, self.precision_mode)
        _no_input_grad(x, "x")
        return _MultiScaleFn.apply(x, self, *self._ordered())


def _refuse_bank3d(mconf, name):
    if mconf.get("model", "ScaleNet") == "FluidNet3D":
        raise ValueError(f"{name}: training the 'FluidNet3D' model is not built into this class or trainer: FluidNetBankTrain3D(mconf) "
                         "is the Conv3d bank net's training module and training3d.train_bank3d its trainer")


class _FluidNetTrainBase(torch.nn.Module):
    """What FluidNetTrain (2D), FluidNetTrain3D, FluidNetBankTrain and FluidNetBankTrain3D share: everything but the dimension, which a subclass states in
    _NDIM, its check of mconf['is3D'] (_check_dim), and the net in the middle (_check_model, _build_net, _ordered, _packed)."""

    _NDIM = 2
    _UNUSED = _UNUSED_PREFIXES           # the reference's parameters this model's forward never reads, kept for state_dict()

    def _check_model(self, mconf, name):
        _refuse_bank3d(mconf, name)
        if mconf.get("model", "ScaleNet") != "ScaleNet":
            raise ValueError(f"{name}: only the ScaleNet variant is accelerated")

    def _build_net(self):
        self.multiScale = _MultiScaleTrain(self.precision_mode, self._NDIM)
        self._api = self.multiScale._api

    def _ordered(self):
        return self.multiScale._ordered()

    def _check_dim(self, mconf):
        raise NotImplementedError

    def __init__(self, mconf, dropout=False):
        super().__init__()
        name = f"fluidnet_cxx_amd.{type(self).__name__}"
        if dropout:
            raise ValueError(f"{name}: dropout=True is not supported (the reference's drivers build the ScaleNet "
                             "path with dropout=False)")
        self._check_model(mconf, name)
        ic = mconf.get("inputChannels", {"div": True, "pDiv": False, "UDiv": False})
        if not (ic.get("div", False) and not ic.get("pDiv", False) and not ic.get("UDiv", False)):
            raise ValueError(f"{name}: inputChannels must be {{div}} (convModel_mconf.pth)")
        if not (mconf.get("normalizeInput", True) and mconf.get("normalizeInputChan", "UDiv") == "UDiv"):
            raise ValueError(f"{name}: normalizeInput on 'UDiv' is the supported configuration")
        self._check_dim(mconf)
        self.precision_mode = str(mconf.get("precisionMode", "fp32"))
        if self.precision_mode not in _TRAIN_MODES:
            raise ValueError(f"{name}: training runs in fp32 arithmetic only (precisionMode one of {_TRAIN_MODES}), "
                             f"not '{self.precision_mode}'")
        self.mconf = mconf
        self.is3D = self._NDIM == 3
        self.inDims = mconf.get("inputDim", self._NDIM)
        self.threshold = float(mconf.get("normalizeInputThreshold", 1e-5))
        self._build_net()
        self._extra = OrderedDict()          # the reference's unused parameters (conv1.* ...), kept for state_dict()

    def _packed(self, device):
        return self.multiScale._packed(device)

    @property
    def packed(self):
        return self._packed(next(self.parameters()).device)[0]

    def packed_for(self, device):
        """The packed weight blob on `device` (what fnx_simulate_step takes as FnxState.net): simulate(..., net, 'convnet') and the
        z-slab driver ask a net for it, as they ask FluidNet."""
        return self._packed(device)[0]

    def step_net(self, device):
        """(kind, packed) for the native step, as FluidNet.step_net: the image of the CURRENT parameter values (_repack looks at every
        parameter's _version, so an optimiser step or load_state_dict is followed by a new image)."""
        if self._api.bank and self._NDIM == 3:
            raise RuntimeError(f"{type(self).__name__}.step_net: this net is the 'FluidNet3D' bank model, which the native step does not "
                               "take (simulate() runs it operator by operator)")
        return ("bank" if self._api.bank else "scalenet"), self._packed(device)[0]

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        if args:                                  # the deprecated positional form (destination, prefix, keep_vars)
            destination = args[0]
            prefix = args[1] if len(args) > 1 else prefix
            keep_vars = args[2] if len(args) > 2 else keep_vars
        # (a parent module passes its own `destination` and ignores the return value: the kept keys go into that dict)
        sd = super().state_dict(destination=destination, prefix=prefix, keep_vars=keep_vars)
        for k, v in self._extra.items():
            sd[prefix + k] = v
        return sd

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        """Like FluidNet.load_state_dict: every multiScale.* parameter must be present with the right shape; the reference FluidNet's
        parameters that the ScaleNet forward never reads are accepted and kept."""
        extra = OrderedDict((k, v) for k, v in state_dict.items() if k.startswith(self._UNUSED))
        own = OrderedDict((k, torch.as_tensor(v)) for k, v in state_dict.items() if not k.startswith(self._UNUSED))
        res = super().load_state_dict(own, strict=strict, **kwargs)
        self._extra = extra
        return res

    def forward(self, input_):
        input_ = input_.contiguous()
        if not (self.training and torch.is_grad_enabled()):
            p, U = self._api.fluidnet_forward(self._packed(input_.device)[0], input_, self.threshold, self.precision_mode)
            return p, U
        _no_input_grad(input_, "input_")
        return _FluidNetFn.apply(input_, self, *self._ordered())


class FluidNetTrain(_FluidNetTrainBase):
    """input_ (B,5,1,H,W) = [p, U, flags, density] -> (p, U), differentiable with respect to the net's parameters.

    What replaces `lib.FluidNet` in the reference's fluid_net_train.py; constructed, loaded and called the same way."""

    def _check_dim(self, mconf):
        if mconf.get("is3D", False):
            raise ValueError("fluidnet_cxx_amd.FluidNetTrain: training is 2D only (is3D=True; FluidNetTrain3D trains the 3D net)")


class FluidNetBankTrain(_FluidNetTrainBase):
    """FluidNetTrain for the reference's 16-channel bank net, mconf['model'] = 'FluidNet' (model.py:177-209): the twelve parameters
    conv1, convBank.block.0, convBank.block.2, conv2, conv3, convOut (.weight / .bias), a fresh net holding
    weights.make_banknet_weights(0).  load_state_dict requires the twelve tensors and keeps multiScale.* / scale.*, as FluidNet does for
    this model; `net.bank(x)`, x (B,2,H,W) -> p (B,1,H,W), is the net alone, differentiable like forward().  2D, H and W multiples of 4."""

    is_bank = True                       # step_net() hands the native step a bank image
    _UNUSED = _BANK_UNUSED_PREFIXES

    def _check_model(self, mconf, name):
        _refuse_bank3d(mconf, name)
        if mconf.get("model", "ScaleNet") != "FluidNet":
            raise ValueError(f"{name}: mconf['model'] must be 'FluidNet', the 16-channel bank net (FluidNetTrain trains the ScaleNet)")

    def _check_dim(self, mconf):
        if mconf.get("is3D", False):
            raise ValueError("fluidnet_cxx_amd.FluidNetBankTrain: the 'FluidNet' bank model is 2D only (the reference asserts it)")

    def _build_net(self):
        self._api = _Api(self._NDIM, bank=True)
        w = make_banknet_weights(0, ndim=self._NDIM)
        for L in banknet_layers():
            parts = L["name"].split(".")                  # conv1  |  convBank, block, 0
            mod = self
            for part in parts[:-1]:
                if not hasattr(mod, part):
                    mod.add_module(part, _Holder())
                mod = getattr(mod, part)
            mod.add_module(parts[-1], _Conv(w[L["name"] + ".weight"], w[L["name"] + ".bias"]))
        self._key = None
        self._images = None

    def _ordered(self):
        """the twelve parameters in the blob's order (banknet_layers(): weight, bias per convolution)"""
        named = dict(self.named_parameters())
        return [named[L["name"] + sfx] for L in banknet_layers() for sfx in (".weight", ".bias")]

    def _packed(self, device):
        return _repack(self, device)

    def _not_scalenet(self, what):
        raise RuntimeError(f"{type(self).__name__}.{what}: this net is the 'FluidNet' bank model; the z-slab drivers take the ScaleNet image only "
                           "(net.step_net(device) is what the native step takes; net.bank(x) and net(input) run the bank kernels)")

    @property
    def packed(self):
        self._not_scalenet("packed")

    def packed_for(self, device):
        self._not_scalenet("packed_for")

    def bank(self, x):
        x = x.contiguous()
        if not (self.training and torch.is_grad_enabled()):
            return self._api.net_forward(self._packed(x.device)[0], x, self.precision_mode)
        _no_input_grad(x, "x")
        return _MultiScaleFn.apply(x, self, *self._ordered())


class FluidNetBankTrain3D(FluidNetBankTrain):
    """FluidNetBankTrain for the Conv3d bank net, mconf['model'] = 'FluidNet3D' with is3D (csrc/fnx_banknet3d_train.hip): the same twelve
    parameter names with 5-D weights, a fresh net holding weights.make_banknet_weights(0, ndim=3); input_ (B,6,D,H,W) -> (p, U) and
    `net.bank(x)`, x (B,2,D,H,W) -> p (B,1,D,H,W).  D, H and W multiples of 4.  Its checkpoints load into FluidNet(mconf) and back."""

    _NDIM = 3

    def _check_model(self, mconf, name):
        if mconf.get("model", "ScaleNet") != "FluidNet3D":
            raise ValueError(f"{name}: mconf['model'] must be 'FluidNet3D', the Conv3d 16-channel bank net (FluidNetTrain3D trains the "
                             "3D ScaleNet, FluidNetBankTrain the 2D 'FluidNet' bank net)")

    def _check_dim(self, mconf):
        if not mconf.get("is3D", False):
            raise ValueError("fluidnet_cxx_amd.FluidNetBankTrain3D: the 'FluidNet3D' model is 3D only (is3D=False)")
