"""FluidNet / MultiScaleNet forward on MI355X (reference pytorch/lib/model.py:42-227,
pytorch/lib/multi_scale_net.py:100-127, ScaleNet configuration of convModel_mconf.pth).

Inference only.  `FluidNet` is constructed and loaded the way the reference drivers do it (plume.py:119-123):

    net = FluidNet(mconf, dropout=False)
    net = net.cuda()
    net.load_state_dict(state['state_dict'])
    net.eval()
    p, U = net(torch.cat((p, U, flags, density), 1))

Weights are torch-style state-dict entries (`multiScale.convN_4.encode.0.weight` ...).  They are repacked for the MFMA
kernels lazily, on the first forward on a given device (and again after `load_state_dict` / `.to()`).

mconf['model'] = 'FluidNet' selects the reference's other net (model.py:177-209), the 16-channel bank net of `conv1`, `convBank`,
`conv2`, `conv3` and `convOut`: `BankNet` / `net.bank(x)`, 2D, fp32 modes (csrc/fnx_banknet.hip).  mconf['model'] = 'FluidNet3D' (with
is3D) is that net with every module replaced by its 3D sibling, this project's own definition: `BankNet3D` (csrc/fnx_banknet3d.hip).
"""
from collections import OrderedDict

import numpy as np
import torch

from ._ext import ext
from .weights import banknet_layers, make_banknet_weights, make_scalenet_weights, scalenet_layers

# Parameters of the reference FluidNet that its ScaleNet forward never reads (model.py:59-72: conv1, convBank, conv2,
# conv3, convOut are only used by the 'FluidNet' variant).  A checkpoint of the reference carries them; load_state_dict
# keeps them verbatim so that state_dict() round-trips.
_UNUSED_PREFIXES = ("conv1.", "convBank.", "conv2.", "conv3.", "convOut.", "scale.")
# The other way round for the bank model (mconf['model'] = 'FluidNet', model.py:177-209): its forward reads those five modules and never
# the MultiScaleNet, whose parameters a reference checkpoint carries all the same.
_BANK_UNUSED_PREFIXES = ("multiScale.", "scale.")


# The four pressure nets' entry points in ext, by (bank, ndim): the one table of their names (train._Api, BankNet and FluidNet read it).
# The first three operations are inference, where the ScaleNet has one name for both dimensions and an argument more (pack_args: is3D;
# forward_args: no trim); the rest is training.  backward_x: the net's backward takes the net's input behind packed_t.
_NET_OPS = ("pack", "forward", "whole_forward", "pack_t", "forward_train", "backward", "whole_forward_train", "whole_backward")


def _net_row(names, pack_args=(), forward_args=(), backward_x=True):
    return dict(zip(_NET_OPS, names.split()), pack_args=pack_args, forward_args=forward_args, backward_x=backward_x)


NET_EXT = {
    (False, 2): _net_row("scalenet_pack multiscale_forward fluidnet_forward scalenet_pack_t multiscale_forward_train multiscale_backward "
                         "fluidnet_forward_train fluidnet_backward", (False,), ([],), False),
    (False, 3): _net_row("scalenet_pack multiscale_forward fluidnet_forward scalenet3d_pack_t multiscale3d_forward_train multiscale3d_backward "
                         "fluidnet3d_forward_train fluidnet3d_backward", (True,), ([],), False),
    (True, 2): _net_row("banknet_pack banknet_forward fluidnet_bank_forward banknet_pack_t banknet_forward_train banknet_backward "
                        "fluidnet_bank_forward_train fluidnet_bank_backward"),
    (True, 3): _net_row("banknet3d_pack banknet3d_forward fluidnet_bank3d_forward banknet3d_pack_t banknet3d_forward_train banknet3d_backward "
                        "fluidnet_bank3d_forward_train fluidnet_bank3d_backward"),
}


def _layer_keys(ndim):
    return [L["name"] + sfx for L in scalenet_layers(2, ndim) for sfx in (".weight", ".bias")]


def _bank_keys():
    return [L["name"] + sfx for L in banknet_layers() for sfx in (".weight", ".bias")]


def blob_from_state_dict(sd, ndim=2, keys=None):
    parts = []
    for k in (_layer_keys(ndim) if keys is None else keys):
        v = sd[k]
        v = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
        parts.append(np.ascontiguousarray(v, np.float32).ravel())
    return np.concatenate(parts)


class MultiScaleNet:
    """x (B,2,H,W) or (B,2,D,H,W) -> (B,1,...)   (multi_scale_net.py:118-127)"""

    def __init__(self, state_dict, device="cuda", is3D=False, precision_mode="fp32"):
        self.is3D = bool(is3D)
        # "fp32": exact-fp32 MFMA arithmetic, 3x3 layers in the Winograd domain where the launch fills the chip;
        # "fp32_direct": every convolution a direct sum over its taps (include/fluidnet_hip.h: FNX_PRECISION_*)
        # "bf16x6" (opt-in): the 64/128-output-channel Winograd layers as six bf16 MFMA products per fp32 product
        # "bf16x3" (opt-in): the same layers with the three products without a low piece (tolerance 1e-4 |ref|max)
        # "fp32_f4": the 64/128-output-channel 3x3(x3) layers in the Winograd F(4x4,3x3) domain, exact-fp32 MFMAs -- what "fp32" runs since
        # round 6; "fp32_f2": F(2x2) for every Winograd layer, the default of rounds 2-5
        self.precision_mode = precision_mode
        blob = torch.from_numpy(blob_from_state_dict(state_dict, 3 if is3D else 2)).to(device)
        self.packed = ext.scalenet_pack(blob, self.is3D)

    def __call__(self, x, trim=None):
        """trim (3D, the z-slab driver): nested z-crops -- [full-tower low, high, half-tower low, high] full-resolution planes
        (include/fluidnet_hip.h: fnx_multiscale_forward_crop); the result then holds planes [trim[0], D - trim[1])"""
        return ext.multiscale_forward(self.packed, x.contiguous(), self.precision_mode, list(trim) if trim is not None else [])


class BankNet:
    """x (B,2,H,W) -> (B,1,H,W): the 16-channel bank net of model.py:177-209 (fnx_banknet.hip).  H and W multiples of 4, fp32 modes.
    is3D: its Conv3d counterpart, x (B,2,D,H,W) -> (B,1,D,H,W) with D a multiple of 4 as well (fnx_banknet3d.hip)."""

    def __init__(self, state_dict, device="cuda", precision_mode="fp32", is3D=False):
        self.is3D = bool(is3D)
        self.precision_mode = precision_mode
        blob = torch.from_numpy(blob_from_state_dict(state_dict, keys=_bank_keys())).to(device)
        self.packed = self._fn("pack")(blob)

    def _fn(self, op):
        return getattr(ext, NET_EXT[True, 3 if self.is3D else 2][op])

    def __call__(self, x):
        return self._fn("forward")(self.packed, x.contiguous(), self.precision_mode)


class BankNet3D(BankNet):
    """The Conv3d bank net, mconf['model'] = 'FluidNet3D': BankNet with is3D."""

    def __init__(self, state_dict, device="cuda", precision_mode="fp32", is3D=True):
        super().__init__(state_dict, device, precision_mode, is3D)


# what differs between the three models of mconf['model'] besides NET_EXT's names: a fresh net's weights (seed, ndim) and the net alone
# (state_dict, device, precision_mode, is3D)
_MODELS = {
    "ScaleNet": dict(weights=make_scalenet_weights, net=MultiScaleNet),
    "FluidNet": dict(weights=make_banknet_weights, net=BankNet),
    "FluidNet3D": dict(weights=make_banknet_weights, net=BankNet3D),
}


class FluidNet:
    """input_ (B,5|6,D,H,W) = [p, U, flags, density] -> (p, U)   (model.py:76-227)

    `FluidNet(mconf, dropout=True)` like the reference (model.py:45); `dropout` only exists for signature
    compatibility -- every Dropout layer is the identity in eval mode, which is the only mode here (simulate.py:140).
    Supports the shipped configuration: model='ScaleNet', inputChannels={'div'}, normalizeInput on 'UDiv'.
    A freshly constructed net holds deterministic random-init weights of the reference architecture
    (weights.make_scalenet_weights(0)); `load_state_dict` replaces them.

    model='FluidNet' (what the reference's trainConfig.yaml ships) is the 16-channel bank net of model.py:177-209, 2D and fp32 modes
    only: a fresh net holds weights.make_banknet_weights(0), `load_state_dict` requires the twelve conv1 / convBank / conv2 / conv3 /
    convOut tensors and keeps multiScale.* and scale.*, `net.bank(x)` is the net alone, and `packed_for` raises -- the z-slab
    drivers and FluidNetTrain take the ScaleNet image only; `simulate()` runs such a net in the native step through `step_net`
    (fnx_simulate_step_net; 2D: the 'FluidNet3D' model below stays on the operator path), and train.FluidNetBankTrain is its
    counterpart with a native backward pass.

    model='FluidNet3D' (with is3D=True; not a reference model, which is 2D only) is the same net with every module replaced by its 3D
    sibling: a fresh net holds weights.make_banknet3d_weights(0), the twelve tensors have 5-D weights, `net.bank(x)` takes
    (B,2,D,H,W) with D, H and W multiples of 4, and everything else is as for 'FluidNet'.  Inference only: no trainer takes it."""

    def __init__(self, mconf, dropout=True):
        model = mconf.get("model", "ScaleNet")
        assert model in ("ScaleNet", "FluidNet", "FluidNet3D"), \
            "mconf['model'] must be 'ScaleNet' or 'FluidNet' (the 16-channel bank net) or 'FluidNet3D' (its Conv3d counterpart)"
        self.is_bank3d = model == "FluidNet3D"
        self.is_bank = model in ("FluidNet", "FluidNet3D")       # step_net() names the kind of image the native step gets
        assert not (model == "FluidNet" and mconf.get("is3D", False)), \
            "the 'FluidNet' bank model is 2D only (the reference asserts it); its Conv3d counterpart is model='FluidNet3D'"
        assert not (self.is_bank3d and not mconf.get("is3D", False)), "the 'FluidNet3D' bank model is 3D only (is3D=True); 'FluidNet' is the 2D net"
        ic = mconf.get("inputChannels", {"div": True, "pDiv": False, "UDiv": False})
        assert ic.get("div", False) and not ic.get("pDiv", False) and not ic.get("UDiv", False), \
            "inputChannels must be {div} (convModel_mconf.pth)"
        assert mconf.get("normalizeInput", True) and mconf.get("normalizeInputChan", "UDiv") == "UDiv"
        self.mconf = mconf
        self.dropout = dropout
        self.inDims = mconf.get("inputDim", 2)
        self.is3D = bool(mconf.get("is3D", False))
        self.threshold = float(mconf.get("normalizeInputThreshold", 1e-5))
        # not a reference key: "fp32" (default), "fp32_direct" (no Winograd), "bf16x6" or "bf16x3" (opt-in), see MultiScaleNet
        self.precision_mode = str(mconf.get("precisionMode", "fp32"))
        self.training = False
        self._ndim = 3 if self.is3D else 2
        self._model = _MODELS[model]         # (only names and classes: a FluidNet copies and pickles)
        init = self._model["weights"](0, ndim=self._ndim)
        self._params = OrderedDict((k, torch.from_numpy(v)) for k, v in init.items())
        self._want = _bank_keys() if self.is_bank else _layer_keys(self._ndim)
        self._unused = _BANK_UNUSED_PREFIXES if self.is_bank else _UNUSED_PREFIXES
        self._extra = OrderedDict()          # the reference's unused parameters, kept for state_dict()
        self._device = None                  # set by cuda()/to(); else the device of the first input
        self._ms = None                      # MultiScaleNet packed for `_ms_device`
        self._ms_device = None

    # ---- construction helpers -----------------------------------------------------------------------------------------
    @classmethod
    def from_weights(cls, mconf, weights, device="cuda", dropout=False):
        """Shortcut: a net holding `weights` (name -> array/tensor), packed on `device`."""
        net = cls(mconf, dropout)
        net.load_state_dict(weights)
        return net.to(device)

    # ---- the nn.Module surface the drivers use ------------------------------------------------------------------------
    def cuda(self, device=None):
        return self.to(torch.device("cuda", torch.cuda.current_device() if device is None else device))

    def to(self, device=None, *_, **__):
        if device is not None:
            self._device = torch.device(device)
            self._ensure_packed(self._device)
        return self

    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        assert not mode, "fluidnet_cxx_amd.FluidNet is inference-only (no backward pass)"
        return self

    def state_dict(self):
        sd = OrderedDict()
        for k, v in self._extra.items():
            sd[k] = v
        for k, v in self._params.items():
            sd[k] = v.to(self._device) if self._device is not None else v
        return sd

    def load_state_dict(self, state_dict, strict=True):
        """Like nn.Module.load_state_dict: every multiScale.* parameter (bank model: each of the twelve bank tensors) must be present
        with the right shape; the reference FluidNet's parameters that this model's forward never reads are accepted and kept."""
        want = self._want
        missing = [k for k in want if k not in state_dict]
        unexpected = [k for k in state_dict if k not in self._params and not k.startswith(self._unused)]
        if missing or (strict and unexpected):
            msg = "Error(s) in loading state_dict for FluidNet:"
            if missing:
                msg += "\n\tMissing key(s) in state_dict: " + ", ".join(f'"{k}"' for k in missing) + "."
            if strict and unexpected:
                msg += "\n\tUnexpected key(s) in state_dict: " + ", ".join(f'"{k}"' for k in unexpected) + "."
            raise RuntimeError(msg)
        new = OrderedDict()
        for k in want:
            v = state_dict[k]
            v = v.detach().to("cpu", torch.float32) if torch.is_tensor(v) else torch.from_numpy(np.asarray(v, np.float32))
            if tuple(v.shape) != tuple(self._params[k].shape):
                raise RuntimeError(f"Error(s) in loading state_dict for FluidNet:\n\tsize mismatch for {k}: copying a param "
                                   f"with shape {tuple(v.shape)} from checkpoint, the shape in current model is "
                                   f"{tuple(self._params[k].shape)}.")
            new[k] = v.contiguous().clone()
        self._params = new
        self._extra = OrderedDict((k, v) for k, v in state_dict.items() if k.startswith(self._unused))
        self._ms = None                      # repacked on the next forward / to()
        if self._device is not None:
            self._ensure_packed(self._device)

    # ---- forward ------------------------------------------------------------------------------------------------------
    def _ensure_packed(self, device):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._ms is None or self._ms_device != device:
            self._ms = self._model["net"](self._params, device, precision_mode=self.precision_mode, is3D=self.is3D)
            self._ms_device = device
        return self._ms

    def _not_scalenet(self, what):
        raise RuntimeError(f"FluidNet.{what}: this net is the '{self.mconf.get('model')}' bank model; the z-slab drivers and the trainers "
                           "take the ScaleNet image only (net.step_net(device) is what the native step takes; net.bank(x) and net(input) run the bank "
                           "kernels)")

    @property
    def multiScale(self):
        if self.is_bank:
            self._not_scalenet("multiScale")
        return self._ensure_packed(self._device if self._device is not None else "cuda")

    @property
    def bank(self):
        """The bank net alone, x (B,2,H,W) -> (B,1,H,W) ('FluidNet3D': (B,2,D,H,W) -> (B,1,D,H,W)): the counterpart of `multiScale`."""
        if not self.is_bank:
            raise RuntimeError("FluidNet.bank: this net is the ScaleNet model (net.multiScale(x))")
        return self._ensure_packed(self._device if self._device is not None else "cuda")

    @property
    def packed(self):
        return self.multiScale.packed

    def packed_for(self, device):
        """The packed weight blob on `device` (what fnx_simulate_step takes as FnxState.net)."""
        if self.is_bank:
            self._not_scalenet("packed_for")
        return self._ensure_packed(device).packed

    def step_net(self, device):
        """(kind, packed) for the native step (ext.simulate_step_'s net_kind and net, fnx_simulate_step_net): 'scalenet' or 'bank' and
        the image of that kind on `device`.  What simulate() asks a net for; `packed_for` stays the ScaleNet image alone.  The
        'FluidNet3D' model raises: the native step does not take the Conv3d bank net, simulate() runs it operator by operator."""
        if not self.is_bank:
            return "scalenet", self.packed_for(device)
        if self.is_bank3d:
            raise RuntimeError("FluidNet.step_net: this net is the 'FluidNet3D' bank model, which the native step does not take "
                               "(simulate() runs it operator by operator; net.bank(x) and net(input) run the bank kernels)")
        return "bank", self._ensure_packed(device).packed

    def __call__(self, input_):
        ms = self._ensure_packed(input_.device)
        p, U = getattr(ext, NET_EXT[self.is_bank, self._ndim]["whole_forward"])(ms.packed, input_.contiguous(), self.threshold, self.precision_mode)
        return p, U

    forward = __call__
