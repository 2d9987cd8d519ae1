"""Operator wrappers with the reference's Python signatures.

Each function cites the reference function it replaces; argument checks mirror the reference's asserts
(AssertionError for shape errors raised on the Python side, RuntimeError from the native side).

The 3D-capable operators take one extra keyword-only argument the reference does not have: `geom`, an
`ext.Geom(ref_quirks=..., z_offset=..., D_global=..., k_begin=..., k_end=...)` (see `Geom` in `fluid/__init__.py`).
It is per call -- the extension keeps no mutable state.
"""
import torch

from .._ext import ext


def _check_advection_method(method):
    # cpp/advection.py:4-7
    assert method in ("eulerFluidNet", "maccormackFluidNet"), \
        "Error: Advection method not supported. Options are: maccormackFluidNet, eulerFluidNet"


def _check5(*ts):
    for t in ts:
        assert t.dim() == 5, "Dimension mismatch"
        assert t.is_contiguous(), "Input is not contiguous"


def getDx(self):
    """lib/fluid/grid.py:3-6"""
    return 1.0 / max(self.size(2), self.size(3), self.size(4))


def getCentered(self):
    """lib/fluid/grid.py:7-32: MAC velocity (B,2|3,D,H,W) -> cell-centred (B,3,D,H,W), 0 on the last column/row/plane."""
    assert self.dim() == 5, "Dimension mismatch"
    return ext.get_centered(self.contiguous())


def advectScalar(dt, src, U, flags, method="maccormackFluidNet", boundary_width=1, sample_outside_fluid=False,
                 maccormack_strength=0.75, *, geom=None, plan="auto"):
    """cpp/advection.py:14-66 -> pybind advect_scalar (cpp/fluids_init.cpp:265-382). 3D is supported here.
    `plan` ('auto' | 'tiles' | 'cells'): the kernel family (same bits; 'auto' = LDS tiles in 3D and on 2D grids of >= 1.5 M cells)."""
    _check_advection_method(method)
    _check5(src, U, flags)
    assert flags.size(1) == 1, "flags is not scalar"
    is3D = U.size(1) == 3
    if not is3D:
        assert flags.size(2) == 1, "2D velocity field but zdepth > 1"
        assert U.size(1) == 2, "2D velocity field must have only 2 channels"
    assert U.size(0) == flags.size(0) and U.shape[2:] == flags.shape[2:], "Size mismatch"
    return ext.advect_scalar(float(dt), src, U, flags, method, int(boundary_width), bool(sample_outside_fluid),
                             float(maccormack_strength), None, geom, plan)


def advectScalars(dt, src, U, flags, method="maccormackFluidNet", boundary_width=1, sample_outside_fluid=False,
                  maccormack_strength=0.75, *, geom=None):
    """Passive scalar transport (no reference counterpart; include/fluidnet_hip.h: fnx_advect_scalars): src (B,C,D,H,W), C >= 1, every
    channel advected by U through ONE forward and ONE backward line trace.  Returns a new (B,C,D,H,W) tensor whose channel c has the
    bits of advectScalar(dt, src[:, c:c+1], ...), whatever that call's `plan`.  Whole single domains only: a compute window or z-slab
    view through `geom` raises ("single-domain only"); geom.ref_quirks is honoured.
    One field (C == 1) has nothing to share a trace with and is handed to advectScalar, whose tile kernels are the faster there
    (1.15x to 1.28x; same bits, so the dispatch cannot be seen); ext.advect_scalars itself takes any C >= 1."""
    _check_advection_method(method)
    _check5(src, U, flags)
    assert flags.size(1) == 1, "flags is not scalar"
    assert src.size(1) >= 1, "src has no channel"
    is3D = U.size(1) == 3
    if not is3D:
        assert flags.size(2) == 1, "2D velocity field but zdepth > 1"
        assert U.size(1) == 2, "2D velocity field must have only 2 channels"
    assert U.size(0) == flags.size(0) and U.shape[2:] == flags.shape[2:], "Size mismatch"
    assert src.size(0) == flags.size(0) and src.shape[2:] == flags.shape[2:], "Size mismatch"
    if src.size(1) == 1:
        assert geom is None or not (geom.k_begin or geom.k_end or geom.z_offset or geom.D_global), \
            "advect_scalars: no compute window or z-slab view (single-domain only)"
        return ext.advect_scalar(float(dt), src, U, flags, method, int(boundary_width), bool(sample_outside_fluid),
                                 float(maccormack_strength), None, geom, "auto")
    return ext.advect_scalars(float(dt), src, U, flags, method, int(boundary_width), bool(sample_outside_fluid),
                              float(maccormack_strength), None, geom)


def advectVelocity(dt, orig, U, flags, method="maccormackFluidNet", boundary_width=1, maccormack_strength=0.75, *,
                   geom=None, plan="auto"):
    """cpp/advection.py:68-118 -> pybind advect_vel (cpp/fluids_init.cpp:656-807).  `plan` as in advectScalar (tiles exist for
    self-advection, `orig is U`, which is what simulate.py:93 passes unless viscosity > 0)."""
    _check_advection_method(method)
    _check5(orig, U, flags)
    assert flags.size(1) == 1, "flags is not scalar"
    is3D = U.size(1) == 3
    if not is3D:
        assert flags.size(2) == 1, "2D velocity field but zdepth > 1"
        assert orig.size(1) == 2 and U.size(1) == 2, "2D velocity field must have only 2 channels"
    assert U.shape == orig.shape and U.size(0) == flags.size(0) and U.shape[2:] == flags.shape[2:], "Size mismatch"
    return ext.advect_vel(float(dt), orig, U, flags, method, int(boundary_width), float(maccormack_strength), None, geom, plan)


def correctScalar(dt, src, div, flags):
    """cpp/advection.py:9-12 (off in all shipped configs): src += dt*0.5*src*div on fluid cells, in place.
    The reference's statement is plain tensor arithmetic, so it takes strided views and broadcastable `div` / `flags`; here those are
    brought to the native operator's form (5-D contiguous fp32, one shape) and the result is copied back into `src`'s own storage."""
    for t, name in ((src, "src"), (div, "div"), (flags, "flags")):
        assert t.is_cuda, "fluidnet_cxx_amd has no CPU path: tensors must be on the GPU"
        assert t.dtype == torch.float32, f"{name} must be float32"
    assert src.dim() == 5, "Dimension mismatch"
    shape = src.shape
    assert torch.broadcast_shapes(shape, div.shape, flags.shape) == shape, "Size mismatch"       # (src is written in place: it sets the shape)
    work = src if src.is_contiguous() else src.contiguous()
    ext.correct_scalar_(float(dt), work, div.expand(shape).contiguous(), flags.expand(shape).contiguous())
    if work is not src:
        src.copy_(work)


def solveLinearSystemJacobi(flags, div, is_3d=False, p_tol=1e-5, max_iter=1000, verbose=False, *, geom=None):
    """cpp/solve_linear_sys.py:4-40 -> pybind solve_linear_system (cpp/fluids_init.cpp:809-1004).
    Returns (p, residual) with residual a 0-dim tensor, like the reference."""
    _check5(div, flags)
    assert flags.size(1) == 1, "flags is not scalar"
    assert div.shape == flags.shape, "Size mismatch"
    p, res = ext.solve_linear_system(flags, div, bool(is_3d), float(p_tol), int(max_iter), bool(verbose), geom)
    return p, res


def solveLinearSystemPCG(flags, div, is_3d=False, p_tol=1e-5, max_iter=50, verbose=False, *, geom=None, p0=None):
    """The converged pressure solve (no reference counterpart): the pressure the Jacobi solve tends to with infinitely many sweeps, by
    multigrid-preconditioned conjugate gradients (fnx_pcg).  Stops per sample at ||div - A p|| <= p_tol ||div|| (div projected onto
    mean zero over the fluid cells of a closed domain, p then has mean zero there); p_tol <= 0 runs exactly max_iter iterations.
    `p0`: a starting guess of div's shape (fnx_pcg_from) -- a net's pressure, the previous step's.  The solve starts from a0 p0 with
    the line-search scale a0 = (p0 . div) / (p0 . A p0), so the guess's magnitude and (on a closed domain) its mean do not matter and
    the start is never worse than the cold one; a sample whose guess is zero or not finite runs the cold solve bit for bit.  With a
    guess max_iter may be 0: the scaled guess is returned.
    Returns (p, residual) like solveLinearSystemJacobi, residual the largest relative residual of the batch (0-dim tensor)."""
    _check5(div, flags)
    assert flags.size(1) == 1, "flags is not scalar"
    if p0 is not None:
        _check5(p0, flags)
    p, res, _ = ext.solve_linear_system_pcg(flags, div, bool(is_3d), float(p_tol), int(max_iter), bool(verbose), geom, p0)
    return p, res


# ---- autograd: the reference's operators are chains of differentiable ATen ops, and its training graph goes through
# velocityUpdate -> setWallBcs -> velocityDivergence (model.py:190-227, fluid_net_train.py:366).  Here each operator is one
# native launch, so its adjoint is one too (fnx_velocity_divergence_backward, fnx_velocity_update_backward; setWallBcs is
# its own adjoint).  The in-place operators stay in place (`mark_dirty`), like the reference's slice assignments.
class _DivergenceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, U, flags, geom):
        ctx.save_for_backward(flags)
        ctx.geom, ctx.is3d = geom, U.size(1) == 3
        return ext.velocity_divergence(U, flags, geom)

    @staticmethod
    def backward(ctx, g):
        (flags,) = ctx.saved_tensors
        return ext.velocity_divergence_backward(g.contiguous(), flags, ctx.is3d, ctx.geom), None, None


class _VelocityUpdateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pressure, U, flags, geom):
        ctx.save_for_backward(flags)
        ctx.geom = geom
        ext.velocity_update_(pressure, U, flags, geom)
        ctx.mark_dirty(U)
        return U

    @staticmethod
    def backward(ctx, g):
        (flags,) = ctx.saved_tensors
        gU, gp = ext.velocity_update_backward(g.contiguous(), flags, ctx.geom)
        return gp, gU, None, None


class _SetWallBcsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, U, flags, geom):
        ctx.save_for_backward(flags)
        ctx.geom = geom
        ext.set_wall_bcs_(U, flags, geom)
        ctx.mark_dirty(U)
        return U

    @staticmethod
    def backward(ctx, g):
        (flags,) = ctx.saved_tensors
        g = g.contiguous().clone()
        ext.set_wall_bcs_(g, flags, ctx.geom)              # zeroing a flag-dependent set of entries is its own adjoint
        return g, None, None


def _needs_grad(*ts, geom=None):
    need = torch.is_grad_enabled() and any(t.requires_grad for t in ts)
    # the adjoint entry points cover whole fields; a windowed forward (planes outside [k_begin, k_end) left as they were)
    # has no matching backward
    assert not (need and geom is not None and (geom.k_begin != 0 or geom.k_end != 0)), \
        "autograd through an operator with a compute window (Geom.k_begin / k_end) is not supported"
    return need


def velocityDivergence(U, flags, *, geom=None):
    """lib/fluid/velocity_divergence.py:4-74 (differentiable w.r.t. U)"""
    _check5(U, flags)
    assert flags.size(1) == 1, "flags is not scalar"
    if _needs_grad(U, geom=geom):
        return _DivergenceFn.apply(U, flags, geom)
    return ext.velocity_divergence(U, flags, geom)


def velocityUpdate(pressure, U, flags, *, geom=None):
    """lib/fluid/velocity_update.py:6-162 -- in place on U, returns None (differentiable w.r.t. pressure and U)."""
    _check5(pressure, U, flags)
    assert flags.size(1) == 1, "flags is not scalar"
    assert pressure.shape == flags.shape, "size mismatch"
    if _needs_grad(pressure, U, geom=geom):
        _VelocityUpdateFn.apply(pressure, U, flags, geom)
        return
    ext.velocity_update_(pressure, U, flags, geom)


def addBuoyancy(U, flags, density, gravity, rho_star, dt, *, geom=None):
    """lib/fluid/source_terms.py:6-116 -- in place on U, returns U.  gravity: 3 floats (tensor or sequence)."""
    _check5(U, flags, density)
    assert flags.size(1) == 1, "flags is not scalar"
    g = gravity.detach().cpu().tolist() if torch.is_tensor(gravity) else [float(x) for x in gravity]
    assert len(g) == 3, "Gravity must be a 3D vector (even in 2D)"
    ext.add_buoyancy_(U, flags, density, g, float(rho_star), float(dt), geom)
    return U


def addGravity(U, flags, gravity, dt, *, geom=None):
    """lib/fluid/source_terms.py:122-219 -- in place on U, returns U."""
    _check5(U, flags)
    assert flags.size(1) == 1, "flags is not scalar"
    g = gravity.detach().cpu().tolist() if torch.is_tensor(gravity) else [float(x) for x in gravity]
    assert len(g) == 3, "Gravity must be a 3D vector (even in 2D)"
    ext.add_gravity_(U, flags, g, float(dt), geom)
    return U


def addViscosity(dt, U, flags, viscosity):
    """lib/fluid/viscosity.py:7-70 -- in place on U.  One explicit step of the viscous term on the MAC faces whose two cells are
    fluid: U += (dt * viscosity) * (sum of the 2 nd face neighbours - 2 nd U), other interior faces are zeroed, the border is kept.
    2D gives the reference's bits (its fourth neighbour is (i-1, j-1)).  3D, where the reference's branch cannot run, is the same
    rule with the axis as a variable (include/fluidnet_hip.h: fnx_add_viscosity; tests/viscous_model_nd.py states it).
    The explicit update is stable for dt * viscosity <= 1 / (2 nd): 1/4 in 2D, 1/6 in 3D.  Nothing checks that, as in the reference."""
    _check5(U, flags)
    assert flags.size(1) == 1, "flags is not scalar"
    ext.add_viscosity_(float(dt), U, flags, float(viscosity))


def addVorticityConfinement(U, flags, strength, *, geom=None):
    """Vorticity confinement (no runnable reference counterpart; include/fluidnet_hip.h: fnx_add_vorticity_confinement) -- in place
    on U, returns U.  F = (grad|w| / |grad|w||) x w * strength from the curl w of the cell-centred velocity, averaged onto the MAC
    faces addGravity writes.  Whole grids only: a compute window or z-slab view through `geom` raises.  strength 0 leaves U alone."""
    _check5(U, flags)
    assert flags.size(1) == 1, "flags is not scalar"
    ext.add_vorticity_confinement_(U, flags, float(strength), geom)
    return U


RENDER_DIRECTIONS = ("+x", "-x", "+y", "-y", "+z", "-z")     # the way rays / light travel; the codes of FnxRenderParams


def renderVolume(density, flags, view="-z", light="-y", *, absorption=None, light_absorption=None, ambient=0.25, albedo_smoke=1.0,
                 albedo_obstacle=0.5, bnd=1):
    """Volume rendering (no reference counterpart; include/fluidnet_hip.h: fnx_render_volume): density (B,1,D,H,W) with the obstacles
    of flags -> (B,2,R,Cc) float32, channel 0 the radiance towards the viewer, channel 1 the transmittance left for a background.
    Orthographic along `view`, single scattering with self-shadowing from `light`; both are one of '+x' '-x' '+y' '-y' '+z' '-z', the
    way the rays or the light TRAVEL (x = W, y = H, z = D), and independent of each other.  Rows and columns are the two axes the
    view does not travel along, in (z, y, x) order, index 0 = coordinate 0.  `absorption` / `light_absorption`: extinction per cell
    of density 1 along the view / the light (default 16 / cells along that axis).  Cells within `bnd` of a domain face count as empty
    (emptyDomain's wall would hide everything).  Neither input is written."""
    _check5(density, flags)
    assert flags.size(1) == 1, "flags is not scalar"
    assert density.shape == flags.shape, "size mismatch"
    assert density.dtype == torch.float32 and flags.dtype == torch.float32, "density and flags must be float32"
    assert density.is_cuda and flags.is_cuda, "density and flags must be on the GPU"
    assert view in RENDER_DIRECTIONS and light in RENDER_DIRECTIONS, "view / light must be one of " + " ".join(RENDER_DIRECTIONS)
    assert int(bnd) >= 0, "bnd < 0"
    v, l = RENDER_DIRECTIONS.index(view), RENDER_DIRECTIONS.index(light)
    cells = lambda d: density.size(4 - (d >> 1))                          # noqa: E731   (x: W, y: H, z: D)
    k_view = 16.0 / cells(v) if absorption is None else float(absorption)
    k_light = 16.0 / cells(l) if light_absorption is None else float(light_absorption)
    return ext.render_volume(density, flags, v, l, k_view, k_light, float(ambient), float(albedo_smoke), float(albedo_obstacle), int(bnd))


def setWallBcs(U, flags, *, geom=None):
    """lib/fluid/set_wall_bcs.py:4-86 -- in place on U, returns U (differentiable w.r.t. U)."""
    _check5(U, flags)
    assert flags.size(1) == 1, "flags is not a scalar"
    if _needs_grad(U, geom=geom):
        return _SetWallBcsFn.apply(U, flags, geom)
    ext.set_wall_bcs_(U, flags, geom)
    return U


def setWallBcsStick(U, flags, flags_stick):
    """lib/fluid/set_wall_bcs_stick.py:5-157 -- no-slip walls, in place on U.  `flags_stick` is a copy of flags
    with the no-slip obstacle cells set to CellType.TypeStick (cylinder.py:76).  The reference function raises
    NameError as shipped; in 2D this is its body with the three unbound names bound (include/fluidnet_hip.h).
    In 3D, where the reference's branch cannot run, a stick cell's tangential components become minus the mean of its fluid
    neighbours' across the transverse axes, and a component normal to a fluid/obstacle face stays 0 (fnx_set_wall_bcs_stick;
    tests/viscous_model_nd.py states it)."""
    _check5(U, flags)
    assert flags.dim() == 5 and flags_stick.dim() == 5, "Dimension mismatch"
    assert flags.size(1) == 1, "flags is not a scalar"
    assert flags_stick.size(1) == 1, "flags is not a scalar"
    assert flags_stick.is_contiguous(), "Input is not contiguous"
    if U.size(1) == 3:          # the extension's in-place entry point is the reference's, 2D; the 3D operator is out of place
        U.copy_(ext.set_wall_bcs_stick_out(U, flags, flags_stick, torch.empty_like(U)))
        return
    ext.set_wall_bcs_stick_(U, flags, flags_stick)


def flagsToOccupancy(flags):
    """lib/fluid/flags_to_occupancy.py:6-19"""
    return ext.flags_to_occupancy(flags)


def setConstVals(batch_dict, p, U, flags, density):
    """lib/simulate.py:4-26 (same side effects on batch_dict: stores clones)."""
    has_u = ("UBCInvMask" in batch_dict) and ("UBC" in batch_dict)
    has_r = ("densityBCInvMask" in batch_dict) and ("densityBC" in batch_dict)
    if not (has_u or has_r):
        return
    ext.set_const_vals_(U, batch_dict["UBC"] if has_u else None, batch_dict["UBCInvMask"] if has_u else None,
                        density if has_r else None, batch_dict["densityBC"] if has_r else None,
                        batch_dict["densityBCInvMask"] if has_r else None)
    if has_u:
        batch_dict["U"] = U.clone()
    if has_r:
        batch_dict["density"] = density.clone()
