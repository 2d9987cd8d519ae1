"""One fluid time step -- drop-in for the reference's `lib.simulate` (pytorch/lib/simulate.py:28-171).

`simulate(mconf, batch_dict, net, sim_method)` keeps the reference's calling convention (in place on
batch_dict, same mconf keys).  Two execution modes:
  fused=True  (default): one call into the native `simulate_step_` (the whole step enqueued by C++, no
              Python between kernels);
  fused=False: operator by operator through the `fluid.*` surface in the reference's order (what the
              parity tests use to compare stage by stage).
fused=True still runs operator by operator where the native step has no form of the call: output_div=True, a 3D state with
flags_stick, a density BC without a 'density' key, and mconf['viscosity'] > 0 with a (dt, viscosity) pair whose double product the two
floats of FnxStepParams do not give (about a third of all pairs, dt = 0.1 with viscosity = 0.05 among them; the reference rounds the
product once, viscosity.py:64).  `workspace` and `static_flags` are then not used.  The same bits, more launches: until FnxStepParams
carries the product (an ABI change) such a viscous 2D run is slower than one with, say, viscosity = 0.02.
The net of 'convnet' and 'hybrid' in 2D is whichever model the net is: the layer asks `net.step_net(device)` for (kind, image) --
'scalenet', or 'bank' for the reference's 'FluidNet' bank model (mconf['model'] = 'FluidNet') -- and the native step runs that net
between the same launches (fnx_simulate_step_net): the static path, an explicit workspace and a HIP-graph capture work
with the bank net as with the ScaleNet, with the bits of the operator path.  A net without `step_net` is asked for
`packed_for(device)`, a ScaleNet image.  The training nets (train.FluidNetTrain, FluidNetBankTrain) hand out an image of their current
parameters; the native step records nothing for autograd, whatever the net's mode.  A net of the Conv3d bank model
(mconf['model'] = 'FluidNet3D') still runs operator by operator, whatever `fused`, `workspace` or `static_flags` say: both methods call
net(...), which runs the bank kernels of fnx_banknet3d.hip (the native step does not take that net yet).
The reference's own call -- `simulate(mconf, batch_dict, net, sim_method)`, four arguments (plume.py:237) -- gets the static
path by itself: the layer keeps one step workspace per (device, grid shape) and looks at `(data_ptr, _version, shape, stride)` of
`flags` and of the four BC arrays (torch bumps `_version` on every in-place write, and so do this package's own in-place
operators).  While they are the tensors of the previous call, unwritten, the step reuses what it derived from them (the 3D
solver's obstacle mask; the 1-byte class map of the BC stages, built on the second such call); any change -- a new tensor, an
in-place write, another shape -- drops back to deriving everything again for that call.  The cache holds a reference to the
five tensors of the previous call, so their addresses cannot be recycled while it trusts them; what it derived from EARLIER
flags (the mask of a Jacobi call, the hierarchy of a PCG call, some calls back) it drops as soon as a call sees other flags --
those tensors may be freed, and a new tensor at a freed one's address has its version and shape too -- so a swap back to them
derives again.  Identities are recorded only after the native call has returned: a call that raises (a refused argument, an
interrupt) leaves the cache with nothing, and the next call derives everything.  What torch's counter does not see: writes through
`.data`, a numpy / dlpack alias or a raw pointer -- after one of those call `forget_static_inputs()` (or pass `static_flags=0`).
`release_workspaces()` frees the cached workspaces (the CNN's is ~1 KB per cell; one per device, stream and grid shape, at most four).
A call captured in a HIP graph bakes the bits of capture time into the graph: replays do not look at the tensors again (and a graph
captured over a cached workspace must not be replayed after `release_workspaces()`; a FIRST call inside a capture keeps nothing).

Explicit control, as before: `workspace` (a uint8 tensor of ext.step_workspace_bytes) with `static_flags` = True / the C ABI's
bit set (FnxStepParams.static_flags): 1 = flags unchanged since the previous call on that workspace (the 3D Jacobi reuses its
obstacle mask), 2 = the four BC arrays unchanged (the BC stages then go by a 1-byte class map kept in the workspace), 4 = that
map was already built by an earlier call with bit 2 -- e.g. 0 for the first step, 3 for the second, 7 from the third on.
8 = ('pcg') the workspace holds the multigrid hierarchy of these flags, built by an earlier call (used only together with 1; the
automatic mode records it only after a call has succeeded).
`static_flags=None` (the default) with no `workspace` is the automatic mode above; with a caller's workspace it means 0.
sim_method 'pcg' (no reference counterpart) projects with the converged solve of fluid.solveLinearSystemPCG: mconf['pcgTol']
(default 1e-5) and mconf['pcgIter'] (default 50); the wall BCs and periodic patches as for 'jacobi'.  mconf['pcgWarmStart'] (default
off) starts that solve from batch_dict['p'], the previous step's pressure (a first step from p = 0 is the cold solve).
sim_method 'hybrid' is 'pcg' started from the net's pressure: p0, _ = net(cat(p, U, flags, density)) on the U the solve projects (the
net's velocity is discarded), then solveLinearSystemPCG(..., p0=p0) to pcgTol / pcgIter -- the net's speed-up with a checked residual.
mconf['vorticityConfinementAmp'] > 0 (no reference key either) adds fluid.addVorticityConfinement with that amplitude after
addGravity and before setWallBcs, for every method; whole grids only (a compute window or z-slab `geom` raises).
mconf['viscosity'] > 0 and batch_dict['flags_stick'] with 'convnet' in 3D (the reference's 3D branches cannot run; default semantics of
fluid.addViscosity / fluid.setWallBcsStick, so a `geom` with ref_quirks raises): the native step has no 3D viscous stage.  A 3D state
with flags_stick takes the operator path by itself; a 3D state with viscosity runs with fused=False and raises with fused=True.
Stable for viscosity * dt <= 1/4 (2D), 1/6 (3D).
batch_dict['scalars'] (no reference key; (B,C,D,H,W) fp32, C >= 1): passive scalars carried along with the step -- a second smoke
source, a dye, a temperature to look at.  They do not act on the flow.  At the top of the call, while U is still the old velocity (the
one the density is advected by), on the fused and the operator path alike:
  s = fluid.advectScalars(dt, scalars, U, flags) with the step's maccormackStrength and sampleOutsideFluid -- all channels through one
      pair of line traces, each with the bits advectScalar gives the density;
  mconf['correctScalar']: every channel gets the density's correction with the divergence of the old U;
  'scalarsBC' and 'scalarsBCInvMask' present ((B,C,D,H,W)): s = s * scalarsBCInvMask + scalarsBC, two roundings, once.  The density
      gets its setConstVals three times a step; for masks of 0 / 1 with scalarsBC == 0 wherever the mask is 1 -- what the drivers
      build -- one application gives the same bits as three (x*1 + 0 and x*0 + bc are fixed points of a second and a third one);
  batch_dict['scalars'] = s.
A channel that starts as a copy of the density with the density's BC arrays stays the density, bit for bit.  No 'density' key is needed,
and output_div=True runs the stage too.  The stage enqueues only, so a step with it stays capturable in a HIP graph; it is out of place,
so such a graph reads the tensor the key held at capture time and writes the one it holds afterwards (copy one into the other between
replays).  Whole single
domains only: with a compute window or z-slab `geom` and the key present the call raises.
`geom` (an `ext.Geom`, 3D only) selects the reference-quirk mode / a z-slab view for this call; it is per call, the
extension keeps no state.
"""
import ctypes

import torch

from . import fluid
from ._ext import ext


def setConstVals(batch_dict, p, U, flags, density):
    fluid.setConstVals(batch_dict, p, U, flags, density)


def _gravity(mconf, scale):
    gv = mconf["gravityVec"]
    return [float(gv["x"]), float(gv["y"]), float(gv["z"])], float(scale)


_BC_KEYS = ("UBC", "UBCInvMask", "densityBC", "densityBCInvMask")
_AUTO = {}            # (device index, stream, B, D, H, W, is3D) -> _AutoStep
_AUTO_MAX = 4         # grid shapes kept (least recently used goes first)


def _ident(t):
    """what identifies a tensor's CONTENT between two calls, or None when torch cannot say (inference tensors have no counter)"""
    if t is None:
        return ()
    try:
        return (t.data_ptr(), t._version, tuple(t.shape), t.stride())
    except RuntimeError:
        return None


class _AutoStep:
    """The step workspace of one grid shape + what it holds that was derived from flags / the BC arrays.

    A step is `bits, after = begin(...)`, the native call with those bits, `commit(after)`.  begin() forgets everything, so between the
    two the entry trusts nothing: a call that raises (a refusal, an interrupt) never reaches commit() and the next call sends 0 --
    whatever the failed one was about to build may be half written.  Only commit() records identities.
    An identity is trusted only while the entry holds its tensor (`held`: the five tensors of the previous call), because a freed
    tensor's address, version and shape can all come back with other contents.  flags_id and bc_id are those tensors' own.  mask_id and
    mg_id describe the flags a Jacobi / PCG call saw, which may be several calls back: they are dropped as soon as a call sees other
    flags (they are None or flags_id, never the identity of a tensor the entry no longer holds).  Keeping those older flags alive
    instead would pin a caller's freed tensors for the sake of one case, a swap back to them."""

    def __init__(self, nbytes, like):
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=like.device)
        self.forget()

    def forget(self):
        self.flags_id = self.bc_id = None     # identities at the previous call
        self.mask_id = None                   # flags identity the kept 3D obstacle mask was built from: None or flags_id
        self.cls_id = None                    # BC identity the kept class map was built from: None or bc_id
        self.mg_id = None                     # flags identity the kept PCG hierarchy was built from: None or flags_id
        self.held = None                      # the five tensors themselves: alive -> their addresses cannot be reused

    def begin(self, batch_dict, flags, is3D, jacobi, pcg=False):
        """(static_flags of this call, what commit() records once it has returned); the entry itself is left with nothing"""
        fid = _ident(flags)
        bcs = [batch_dict.get(k) for k in _BC_KEYS]
        bid = None if any(_ident(t) is None for t in bcs) else tuple(_ident(t) for t in bcs)
        same_flags = fid is not None and fid == self.flags_id
        mask_id = self.mask_id if same_flags else None          # other flags: what was derived from earlier ones is dropped
        mg_id = self.mg_id if same_flags else None
        bits = 0
        if same_flags and (not (is3D and jacobi) or mask_id == fid):
            bits |= 1                         # flags unchanged (and, where a mask is used, the kept one is theirs)
        cls_id = None
        if bid is not None and bid == self.bc_id:
            bits |= 2                         # BC arrays unchanged since the previous call: go by the class map ...
            if self.cls_id == bid:
                bits |= 4                     # ... which an earlier call already built
            cls_id = bid
        if pcg and (bits & 1) and mg_id == fid:
            bits |= 8                         # the kept hierarchy is that of these flags
        if pcg:
            mg_id = fid                       # this call leaves the hierarchy of these flags behind (built now, or reused)
        if is3D and jacobi:
            mask_id = fid                     # and this one the mask
        self.forget()
        return bits, (fid, bid, mask_id, cls_id, mg_id, (flags, bcs))

    def commit(self, after):
        """the call begin() gave the bits for has returned: the workspace holds what it built"""
        self.flags_id, self.bc_id, self.mask_id, self.cls_id, self.mg_id, self.held = after


def _auto_step(flags, is3D):
    """the cached step state of this (device, stream, grid shape), or None where the layer must not keep one: a first call inside a
    HIP-graph capture (its allocation would belong to the graph's private pool and die with the graph)"""
    dev = flags.device.index if flags.device.index is not None else torch.cuda.current_device()
    # per stream: two simulations of one shape on two streams must not share scratch memory, and a workspace is handed back to the
    # allocator on the stream it was used on
    key = (dev, torch.cuda.current_stream(dev).cuda_stream) + tuple(int(flags.size(i)) for i in (0, 2, 3, 4)) + (bool(is3D),)
    a = _AUTO.pop(key, None)
    if a is None:
        if torch.cuda.is_current_stream_capturing():
            return None
        while len(_AUTO) >= _AUTO_MAX:
            _AUTO.pop(next(iter(_AUTO)))
        a = _AutoStep(ext.step_workspace_bytes(key[2], key[3], key[4], key[5], key[6]), flags)
    _AUTO[key] = a                            # (re-inserted: most recently used last)
    return a


def forget_static_inputs():
    """the next simulate() call of every grid shape derives everything from flags / the BC arrays again (after a write torch's
    version counter cannot see: `.data`, a numpy / dlpack alias, a raw pointer)"""
    for a in _AUTO.values():
        a.forget()


def release_workspaces():
    """free the step workspaces the automatic mode keeps (one per grid shape seen, at most four)"""
    _AUTO.clear()


def _f32(x):
    return ctypes.c_float(x).value


def _step_has_the_viscous_coefficient(dt, viscosity):
    """The reference multiplies dt and viscosity as Python floats and rounds the product once (viscosity.py:64; fluid.addViscosity
    does the same).  FnxStepParams carries the two as floats and the native step multiplies those: for about a third of all pairs that
    coefficient is an ulp off (dt = 0.1 with viscosity = 0.05; not with the 0.02 of the goldens).  Such a step runs operator by operator
    -- the same kernels, the reference's bits."""
    return _f32(_f32(dt) * _f32(viscosity)) == _f32(dt * viscosity)


def _is_view(geom):
    return geom is not None and (geom.k_begin != 0 or geom.k_end != 0 or geom.z_offset != 0 or geom.D_global != 0)


def _scalars_stage(mconf, batch_dict, dt, U, flags, geom):
    """the passive scalars of batch_dict['scalars'] by the old U (module docstring)"""
    if _is_view(geom):
        raise ValueError("simulate(): batch_dict['scalars'] is single-domain only (no compute window or z-slab view through geom)")
    s = fluid.advectScalars(dt, batch_dict["scalars"], U, flags, method="maccormackFluidNet", boundary_width=1,
                            sample_outside_fluid=mconf["sampleOutsideFluid"], maccormack_strength=mconf["maccormackStrength"], geom=geom)
    if mconf.get("correctScalar", False):
        div = fluid.velocityDivergence(U, flags, geom=geom)
        for c in range(s.size(1)):                              # (the operator takes one field; a channel view is copied in and out)
            fluid.correctScalar(dt, s[:, c:c + 1], div, flags)
    if "scalarsBC" in batch_dict and "scalarsBCInvMask" in batch_dict:
        s = s * batch_dict["scalarsBCInvMask"] + batch_dict["scalarsBC"]
    batch_dict["scalars"] = s


def simulate(mconf, batch_dict, net, sim_method, output_div=False, fused=True, workspace=None, static_flags=None,
             geom=None):
    assert sim_method in ("convnet", "jacobi", "pcg", "hybrid"), "Simulation method not supported. Choose convnet, jacobi, pcg or hybrid."
    uses_net = sim_method in ("convnet", "hybrid")
    uses_pcg = sim_method in ("pcg", "hybrid")
    pcg_warm = sim_method == "pcg" and bool(mconf.get("pcgWarmStart", False))
    dt = float(mconf["dt"])
    maccormackStrength = mconf["maccormackStrength"]
    sampleOutsideFluid = mconf["sampleOutsideFluid"]
    buoyancyScale = mconf["buoyancyScale"]
    gravityScale = mconf.get("gravityScale", 0)
    viscosity = mconf.get("viscosity", 0)
    assert viscosity >= 0, "Viscosity must be positive"
    vorticityAmp = mconf.get("vorticityConfinementAmp", 0)      # no reference key: fluid.addVorticityConfinement after addGravity
    p, U, flags = batch_dict["p"], batch_dict["U"], batch_dict["flags"]
    has_density = "density" in batch_dict

    is3D = U.size(1) == 3
    if is3D and geom is not None and geom.ref_quirks and (viscosity > 0 or ("flags_stick" in batch_dict and sim_method == "convnet")):
        # neither operator takes a geom: in 3D the reference has no form of them that quirks could reproduce (fnx_add_viscosity and
        # fnx_set_wall_bcs_stick refuse FnxGrid.ref_quirks for the same reason)
        raise RuntimeError("simulate(): viscosity and flags_stick have no 3D form with ref_quirks (the reference's 3D branches cannot run)")
    # 3D viscosity: fluid.addViscosity takes 3D fields, so the operator path runs the viscous step; the native step has no 3D
    # viscous stage (fnx_simulate_step refuses it), and a call that asks for the native step is told so before anything is written
    if is3D and viscosity > 0 and fused and not output_div:
        raise RuntimeError("simulate(): mconf['viscosity'] is 2D only in the native step; in 3D pass fused=False (the operator path)")
    if "scalars" in batch_dict:                                 # before anything writes U: the scalars go by the old velocity
        _scalars_stage(mconf, batch_dict, dt, U, flags, geom)
    # the optional stages (viscosity, gravityScale, correctScalar, the periodic patches, flags_stick) are branches of the
    # native step (FnxStepParams / FnxState); what stays on the operator path: output_div (a training-time early return),
    # 3D states with flags_stick (the native step refuses them; fluid.setWallBcsStick takes 3D fields),
    # no 'density' key but a density BC: the reference applies setConstVals to its zeros (simulate.py:82-97), and
    # a (dt, viscosity) pair whose product the step's two floats do not give (_step_has_the_viscous_coefficient)
    # and a net of the Conv3d bank model: the native step takes the ScaleNet and the 2D bank net (FluidNet.step_net)
    simple = (not output_div and not (is3D and "flags_stick" in batch_dict)
              and not (uses_net and is3D and getattr(net, "is_bank", False))
              and (has_density or not ("densityBC" in batch_dict and "densityBCInvMask" in batch_dict))
              and (viscosity == 0 or _step_has_the_viscous_coefficient(dt, viscosity)))
    if fused and simple:
        periodic = 0
        if "periodic-x" in mconf and "periodic-y" in mconf:                     # simulate.py:121, :157
            periodic = 1 | (2 if mconf["periodic-x"] else 0) | (4 if mconf["periodic-y"] else 0)
        want_gvec = has_density and (buoyancyScale > 0 or gravityScale > 0)
        # gravityVec is only read when buoyancy is applied (simulate.py:99-105)
        gvec = _gravity(mconf, 1.0)[0] if want_gvec else [0.0, 0.0, 0.0]
        density = batch_dict["density"] if has_density else None
        # the net by its kind: ScaleNet or the 2D bank net ('bank'); a net without step_net hands out a ScaleNet image
        net_kind, packed = "scalenet", None
        if uses_net:
            net_kind, packed = net.step_net(U.device) if hasattr(net, "step_net") else ("scalenet", net.packed_for(U.device))
        auto = None
        if workspace is None and static_flags is None and flags.is_cuda and geom is None:
            # the reference's four-argument call: the layer's own workspace, static inputs detected (module docstring)
            auto = _auto_step(flags, is3D)
            if auto is not None:
                workspace = auto.workspace
                static_flags, kept = auto.begin(batch_dict, flags, is3D, sim_method == "jacobi", uses_pcg)
        if static_flags is None:
            static_flags = 0
        ext.simulate_step_(p, U, flags, density, batch_dict.get("UBC"), batch_dict.get("UBCInvMask"),
                           batch_dict.get("densityBC"), batch_dict.get("densityBCInvMask"), packed, dt,
                           float(maccormackStrength), bool(sampleOutsideFluid), float(buoyancyScale), gvec,
                           float(mconf.get("operatingDensity", 0.0)), float(mconf.get("pTol", 0.0)),
                           int(mconf.get("jacobiIter", 1)), sim_method,
                           float(mconf.get("normalizeInputThreshold", 1e-5)), workspace, int(static_flags), geom,
                           getattr(net, "precision_mode", "fp32") if uses_net else "fp32",
                           float(viscosity), float(gravityScale) if gravityScale > 0 else 0.0,
                           bool(mconf.get("correctScalar", False)) and has_density, periodic,
                           batch_dict.get("flags_stick") if sim_method == "convnet" else None,
                           pcg_tol=float(mconf.get("pcgTol", 1e-5)), pcg_iter=int(mconf.get("pcgIter", 50)),
                           vorticity_confinement=float(vorticityAmp) if vorticityAmp > 0 else 0.0, pcg_warm=pcg_warm,
                           net_kind=net_kind)
        if auto is not None:
            auto.commit(kept)                                   # only a call that returned: one that raised has left `auto` forgotten
        if not has_density:
            batch_dict["density"] = torch.zeros_like(flags)     # simulate.py:82-83
        return

    stick = "flags_stick" in batch_dict                          # simulate.py:61-64
    # ---- operator-by-operator path, reference order ----
    orig = U
    if viscosity > 0:                                           # simulate.py:66-69
        orig = U.clone()
        fluid.addViscosity(dt, orig, flags, viscosity)
    if has_density:
        density = fluid.advectScalar(dt, batch_dict["density"], U, flags, method="maccormackFluidNet",
                                     boundary_width=1, sample_outside_fluid=sampleOutsideFluid,
                                     maccormack_strength=maccormackStrength, geom=geom)
        if mconf.get("correctScalar", False):
            div = fluid.velocityDivergence(U, flags, geom=geom)
            fluid.correctScalar(dt, density, div, flags)
    else:
        density = torch.zeros_like(flags)
    U = fluid.advectVelocity(dt=dt, orig=orig, U=U, flags=flags, method="maccormackFluidNet", boundary_width=1,
                             maccormack_strength=maccormackStrength, geom=geom)
    setConstVals(batch_dict, p, U, flags, density)
    if has_density and buoyancyScale > 0:
        gvec, _ = _gravity(mconf, 1.0)
        gravity = (torch.tensor(gvec, dtype=torch.float32) * (-buoyancyScale)).tolist()
        U = fluid.addBuoyancy(U, flags, density, gravity, mconf["operatingDensity"], dt, geom=geom)
    if has_density and gravityScale > 0:                        # simulate.py:107-114 (inside the density branch)
        gvec, _ = _gravity(mconf, 1.0)
        gravity = (torch.tensor(gvec, dtype=torch.float32) * (-gravityScale)).tolist()
        U = fluid.addGravity(U, flags, gravity, dt, geom=geom)
    if vorticityAmp > 0:                                        # a body force like the two above; the projection removes its divergence
        U = fluid.addVorticityConfinement(U, flags, vorticityAmp, geom=geom)
    if output_div:
        return
    periodic = "periodic-x" in mconf and "periodic-y" in mconf

    def wall_bcs(U):
        if periodic:
            U_temp = U.clone()
        U = fluid.setWallBcs(U, flags, geom=geom)
        if periodic:
            if mconf["periodic-x"]:
                U[:, 1, :, :, 1] = U_temp[:, 1, :, :, U.size(4) - 1]
            if mconf["periodic-y"]:
                U[:, 0, :, 1] = U_temp[:, 0, :, U.size(3) - 1]
        return U

    if sim_method != "convnet":
        U = wall_bcs(U)
    elif stick:                                                  # simulate.py:129-130
        fluid.setWallBcsStick(U, flags, batch_dict["flags_stick"])
    setConstVals(batch_dict, p, U, flags, density)
    if sim_method == "convnet":
        data = torch.cat((p, U, flags, density), 1)
        p, U = net(data)
        if stick:                                                # simulate.py:165-166
            fluid.setWallBcsStick(U, flags, batch_dict["flags_stick"])
    else:
        div = fluid.velocityDivergence(U, flags, geom=geom)
        is3D = U.size(2) > 1
        if uses_pcg:
            p0 = p if pcg_warm else None
            if sim_method == "hybrid":                           # the net's pressure of the U being projected; its velocity is not used
                p0, _ = net(torch.cat((p, U, flags, density), 1))
            p, residual = fluid.solveLinearSystemPCG(flags=flags, div=div, is_3d=is3D, p_tol=mconf.get("pcgTol", 1e-5),
                                                     max_iter=mconf.get("pcgIter", 50), geom=geom, p0=p0)
        else:
            p, residual = fluid.solveLinearSystemJacobi(flags=flags, div=div, is_3d=is3D, p_tol=mconf["pTol"],
                                                        max_iter=mconf["jacobiIter"], geom=geom)
        fluid.velocityUpdate(pressure=p, U=U, flags=flags, geom=geom)
        U = wall_bcs(U)
    setConstVals(batch_dict, p, U, flags, density)
    batch_dict["U"] = U
    batch_dict["density"] = density
    batch_dict["p"] = p
