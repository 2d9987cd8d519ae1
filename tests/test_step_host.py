"""The host side of the time step without a GPU: the workspace sizes callers allocate by, every refusal of fnx_simulate_step,
fnx_pre_projection and fnx_post_projection that is made before the first launch (on dummy host pointers that nothing may read), in
its order, and the pure functions of csrc/fnx_step_plan.h -- the workspace layout, the stage's plan and the step's -- called from a
host-only program.  The expected sizes were recorded from the library before that header existed; the expected offsets and plans are
what that code did for the same cases (ws_step's sum and the Carver in fnx_simulate_step, the conditions scattered over
fnx_pre_projection and fnx_simulate_step), worked out from it.

Not here: the convnet branch's `unknown precision_mode` refusal, which comes after the staging launches and so needs a device."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from fluidnet_cxx_amd import build
from test_pcg_warm_host import _structs
from util import FnxGrid as _FnxGrid

REPO = os.path.dirname(build.HERE)
vp, ci, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
Prm, St = _structs()


def _enum(name):
    return int(re.search(name + r" = (\d+)", open(os.path.join(REPO, "include", "fluidnet_hip.h")).read()).group(1))


OP_JACOBI, OP_STEP, OP_FLUIDNET, OP_ADVECT_STEP = (_enum("FNX_OP_" + n) for n in ("JACOBI", "STEP", "FLUIDNET", "ADVECT_STEP"))
EINVAL, EWORKSPACE = _enum("FNX_EINVAL"), _enum("FNX_EWORKSPACE")
G2D, G3D = (2, 1, 40, 70), (1, 9, 20, 66)

# shape -> (fnx_workspace_bytes(FNX_OP_STEP), (FNX_OP_FLUIDNET)); (1, 1, 3, 3) is the smallest grid there is
WS_BYTES = {
    (2, 1, 40, 70): (6133760, 5951488),
    (1, 1, 3, 3): (101888, 27392),
    (1, 9, 20, 66): (12868352, 12538112),
    (1, 16, 33, 130): (74259968, 72371712),
    (1, 6, 21, 66): (9014528, 8782592),
}
# shape -> what goes into step_layout (the 3D neighbour mask's bytes, the PCG hierarchy's, the tail) and the offsets that come out.
# Every region is rounded up to 256 bytes.  The hierarchy: 2 bytes per cell, then 16 per cell of every coarser level (each axis halved,
# rounded up, until none is above 4).  (2, 1, 40, 70): 22400 bytes per scalar field -> 22528, 44800 per velocity -> 44800.
LAYOUT = {
    (2, 1, 40, 70): dict(mask=0, kept=41984, tail_need=5951488,
                         at=dict(rho2=0, U2=22528, div=67328, mask=-1, cls=89856, pcg_kept=95488, orig=137472, tail=182272)),
    (1, 1, 3, 3): dict(mask=0, kept=256, tail_need=100352,
                       at=dict(rho2=0, U2=256, div=512, mask=-1, cls=768, pcg_kept=1024, orig=1280, tail=1536)),
    (1, 9, 20, 66): dict(mask=24320, kept=56064, tail_need=12538112,
                         at=dict(rho2=0, U2=47616, div=190208, mask=237824, cls=262144, pcg_kept=274176, orig=-1, tail=330240)),
    (1, 16, 33, 130): dict(mask=144128, kept=302080, tail_need=72371712,
                           at=dict(rho2=0, U2=274688, div=1098496, mask=1373184, cls=1517312, pcg_kept=1586176, orig=-1, tail=1888256)),
    (1, 6, 21, 66): dict(mask=18432, kept=38656, tail_need=8782592,
                         at=dict(rho2=0, U2=33280, div=133120, mask=166400, cls=184832, pcg_kept=193280, orig=-1, tail=231936)),
}
REGIONS = ("rho2", "U2", "div", "mask", "cls", "pcg_kept", "orig", "tail")


def _grid(B, D, H, W, **kw):
    return _FnxGrid(B=B, D=D, H=H, W=W, is3D=int(D > 1), **kw)


@pytest.fixture(scope="module")
def lib():
    build.build_all()
    lib = ctypes.CDLL(build.LIB)
    lib.fnx_last_error.restype = ctypes.c_char_p
    G = ctypes.POINTER(_FnxGrid)
    lib.fnx_workspace_bytes.restype = lib.fnx_pcg_workspace_bytes.restype = sz
    lib.fnx_workspace_bytes.argtypes = [G, ci]
    lib.fnx_pcg_workspace_bytes.argtypes = [G]
    lib.fnx_simulate_step.argtypes = [G, ctypes.POINTER(Prm), ctypes.POINTER(St), vp, sz, vp]
    lib.fnx_pre_projection.argtypes = [G, ctypes.POINTER(Prm), ctypes.POINTER(St), vp, vp, vp, vp]
    lib.fnx_post_projection.argtypes = [G, ctypes.POINTER(St), vp]
    return lib


def _ws(lib, g, op):
    return lib.fnx_workspace_bytes(ctypes.byref(g), op)


@pytest.mark.parametrize("shape", list(WS_BYTES))
def test_workspace_bytes(lib, shape):
    g = _grid(*shape)
    assert (_ws(lib, g, OP_STEP), _ws(lib, g, OP_FLUIDNET)) == WS_BYTES[shape]
    if g.is3D:   # neither a compute window nor a z-slab view changes what a call needs
        for view in (dict(k_begin=2, k_end=5), dict(z_offset=3, D_global=shape[1] + 7)):
            gv = _grid(*shape, **view)
            assert (_ws(lib, gv, OP_STEP), _ws(lib, gv, OP_FLUIDNET)) == WS_BYTES[shape]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
BUF = {n: ctypes.cast(ctypes.create_string_buffer(64), vp).value for n in ("p", "U", "flags", "density", "net", "stick", "ws", "U_adv", "rho_adv", "div")}


def _state(**kw):
    return St(**dict(dict(p=BUF["p"], U=BUF["U"], flags=BUF["flags"]), **kw))


def _step(lib, g, prm, st, ws=BUF["ws"], ws_bytes=None):
    """(return code, fnx_last_error()); the workspace is a dummy of the size the step asks for unless told otherwise"""
    ws_bytes = _ws(lib, g, OP_STEP) if ws_bytes is None else ws_bytes
    rc = lib.fnx_simulate_step(ctypes.byref(g), ctypes.byref(prm) if prm else None, ctypes.byref(st) if st else None, ws, ws_bytes, None)
    return rc, lib.fnx_last_error().decode()


METHOD = "Simulation method not supported. Choose convnet, jacobi, pcg or hybrid."
PCG_ITER = "At least 1 iteration of the solver is needed (pcg_iter < 1)"
PCG_VIEW = "simulate_step: the PCG solve takes no compute window or z-slab view (single domain only)"
CONFINE_VIEW = "simulate_step: vorticity confinement takes no compute window or z-slab view (single domain only)"
NAN = float("nan")


def test_simulate_step_refusals_in_order(lib):
    """each refusal with its code and text, together with failures that come later in the order: the earlier one is reported"""
    g2, g3 = _grid(*G2D), _grid(*G3D)
    views = (_grid(*G3D, k_begin=2, k_end=5), _grid(*G3D, z_offset=3, D_global=16))
    st, net = _state(), _state(net=BUF["net"])
    # 1. the grid, ahead of a NULL state
    assert _step(lib, _FnxGrid(B=1, D=1, H=2, W=40), None, None, ws_bytes=0) == (EINVAL, "Dimension mismatch: B=1 D=1 H=2 W=40")
    assert _step(lib, _FnxGrid(B=1, D=2, H=20, W=40, is3D=1), Prm(method=7), None, ws_bytes=0) == (EINVAL, "3D domain needs D >= 3")
    # 2. NULL state, ahead of the method
    for bad in (None, _state(p=None), _state(U=None), _state(flags=None)):
        assert _step(lib, g2, Prm(method=7), bad, ws_bytes=0) == (EINVAL, "simulate_step: NULL state")
    assert _step(lib, g2, None, st, ws_bytes=0) == (EINVAL, "simulate_step: NULL state")
    # 3. the method, ahead of pcg_iter
    for method in (-1, 5):
        assert _step(lib, g2, Prm(method=method, pcg_iter=0), st, ws_bytes=0) == (EINVAL, METHOD)
    # 4. pcg_iter, ahead of the PCG view
    for method in (2, 3, 4):
        for v in views:
            assert _step(lib, v, Prm(method=method, pcg_iter=0), st, ws_bytes=0) == (EINVAL, PCG_ITER)
    # 5. PCG on a view, ahead of the confinement on a view and of the missing weights
    for method in (2, 3, 4):
        for v in views:
            assert _step(lib, v, Prm(method=method, pcg_iter=3, vorticity_confinement=0.5), st, ws_bytes=0) == (EINVAL, PCG_VIEW)
    # 6. confinement on a view, ahead of the convnet's missing weights
    for method in (0, 1):
        for v in views:
            assert _step(lib, v, Prm(method=method, vorticity_confinement=0.5), st, ws_bytes=0) == (EINVAL, CONFINE_VIEW)
    # 7. / 8. no weights, ahead of the precision mode and the workspace
    assert _step(lib, g2, Prm(method=1, precision_mode=99), st, ws_bytes=0) == (EINVAL, "simulate_step: convnet method needs packed weights")
    assert _step(lib, g2, Prm(method=3, pcg_iter=3, precision_mode=99), st, ws_bytes=0) == (EINVAL, "simulate_step: hybrid method needs packed weights")
    # 9. the hybrid's precision mode, ahead of the workspace
    for mode in (-1, 6, 99):
        assert _step(lib, g2, Prm(method=3, pcg_iter=3, precision_mode=mode), net, ws_bytes=0) == (EINVAL, f"simulate_step: unknown precision_mode {mode}")
    # 10. the workspace, with both sizes, ahead of the viscosity
    for g in (g2, g3, views[0]):
        need = _ws(lib, g, OP_STEP)
        for method in (0, 1, 2, 3, 4):
            if g is views[0] and method >= 2:
                continue
            prm = Prm(method=method, pcg_iter=3, viscosity=-1.0)
            assert _step(lib, g, prm, net, ws_bytes=need - 1) == (EWORKSPACE, f"simulate_step: workspace too small ({need - 1} < {need})")
            assert _step(lib, g, prm, net, ws_bytes=0) == (EWORKSPACE, f"simulate_step: workspace too small (0 < {need})")
            assert _step(lib, g, prm, net, ws=None) == (EWORKSPACE, f"simulate_step: workspace too small ({need} < {need})")
    # 11. negative viscosity, ahead of the NaN confinement
    for g in (g2, g3):
        assert _step(lib, g, Prm(viscosity=-1.0, vorticity_confinement=NAN), st) == (EINVAL, "Viscosity must be positive")
    # 12. NaN confinement, ahead of the 3D viscosity
    assert _step(lib, g3, Prm(viscosity=0.1, vorticity_confinement=NAN), st) == (EINVAL, "simulate_step: vorticity_confinement is NaN")
    assert _step(lib, g2, Prm(method=1, vorticity_confinement=NAN), net) == (EINVAL, "simulate_step: vorticity_confinement is NaN")
    # 13. viscosity in 3D, ahead of flags_stick in 3D
    stick = _state(net=BUF["net"], flags_stick=BUF["stick"])
    assert _step(lib, g3, Prm(method=1, viscosity=0.1), stick) == (EINVAL, "simulate_step: viscosity is 2D only (reference viscosity.py:5)")
    # 14. flags_stick in 3D: the convnet only (the other methods ignore it and would go on to launch: not called here)
    assert _step(lib, g3, Prm(method=1, precision_mode=99), stick) == (EINVAL, "simulate_step: flags_stick is 2D only (set_wall_bcs_stick.py:85-86)")


def test_stage_refusals(lib):
    """fnx_pre_projection: grid, NULL state, rho_adv without a density, aliasing, confinement on a view; fnx_post_projection: grid, NULL state"""
    g3 = _grid(*G3D)
    view = _grid(*G3D, k_begin=2, k_end=5)

    def pre(g, prm, st, U_adv=BUF["U_adv"], rho_adv=None):
        rc = lib.fnx_pre_projection(ctypes.byref(g), ctypes.byref(prm) if prm else None, ctypes.byref(st) if st else None, U_adv, rho_adv,
                                    BUF["div"], None)
        return rc, lib.fnx_last_error().decode()

    def post(g, st):
        return lib.fnx_post_projection(ctypes.byref(g), ctypes.byref(st) if st else None, None), lib.fnx_last_error().decode()

    rho = _state(density=BUF["density"])
    assert pre(_FnxGrid(B=1, D=1, H=2, W=40), None, None) == (EINVAL, "Dimension mismatch: B=1 D=1 H=2 W=40")
    for prm, st, U_adv in ((None, _state(), BUF["U_adv"]), (Prm(), None, BUF["U_adv"]), (Prm(), _state(U=None), BUF["U_adv"]),
                           (Prm(), _state(flags=None), BUF["U_adv"]), (Prm(), _state(), None)):
        assert pre(g3, prm, st, U_adv, rho_adv=BUF["rho_adv"]) == (EINVAL, "pre_projection: NULL state")
    # rho_adv without a density, ahead of the aliasing
    assert pre(g3, Prm(), _state(), U_adv=BUF["U"], rho_adv=BUF["rho_adv"]) == (EINVAL, "pre_projection: rho_adv given but state has no density")
    alias = "pre_projection: the advected fields must not alias the state"
    confine = Prm(vorticity_confinement=0.5)
    assert pre(view, confine, rho, U_adv=BUF["U"]) == (EINVAL, alias)
    assert pre(view, confine, rho, rho_adv=BUF["density"]) == (EINVAL, alias)
    for v in (view, _grid(*G3D, z_offset=3, D_global=16)):
        for method in (0, 1, 2):
            assert pre(v, Prm(method=method, vorticity_confinement=0.5), rho, rho_adv=BUF["rho_adv"]) == \
                (EINVAL, "pre_projection: vorticity confinement takes no compute window or z-slab view (single domain only)")
    assert post(_FnxGrid(B=1, D=1, H=2, W=40), None) == (EINVAL, "Dimension mismatch: B=1 D=1 H=2 W=40")
    for st in (None, _state(p=None), _state(U=None), _state(flags=None)):
        assert post(g3, st) == (EINVAL, "post_projection: NULL state")


# ---- the pure functions, from a host-only program ---------------------------------------------------------------------------------------
PROGRAM = r'''
#include "fnx_step_plan.h"
using namespace fnx;
// out: the offsets of rho2, U2, div, mask, cls, pcg_kept, orig, tail (-1: none), tail_bytes, bytes
extern "C" void layout(size_t cells, size_t nc, int is3d, size_t mask_bytes, size_t kept_bytes, size_t tail_need, char* base, long* out) {
  const StepLayout L = step_layout(cells, nc, is3d != 0, mask_bytes, kept_bytes, tail_need, base);
  const void* at[8] = {L.rho2, L.U2, L.div, L.mask, L.cls, L.pcg_kept, L.orig, L.tail};
  for (int r = 0; r < 8; ++r) out[r] = at[r] ? (const char*)at[r] - base : -1;
  out[8] = (long)L.tail_bytes; out[9] = (long)L.bytes;
}
static void stage_out(const StagePlan& s, int* f, float* x) {
  const int v[8] = {s.buoy, s.grav, s.wall, s.periodic, s.px, s.py, s.second_bcs, s.confine};
  for (int q = 0; q < 8; ++q) f[q] = v[q];
  for (int a = 0; a < 3; ++a) { x[a] = s.s[a]; x[3 + a] = s.g[a]; }
  x[6] = s.rho_star; x[7] = s.amp;
}
extern "C" void stage(const FnxStepParams* prm, int has_rho, int has_stick, int* f, float* x) {
  stage_out(stage_plan(prm, has_rho != 0, has_stick != 0), f, x);
}
extern "C" void step(const FnxStepParams* prm, int has_rho, int has_stick, int has_bc, int* f, float* x) {
  const StepPlan p = step_plan(prm, has_rho != 0, has_stick != 0, has_bc != 0);
  stage_out(p.stage, f, x);
  const int v[9] = {p.viscous, (int)p.advect, p.correct_scalar, (int)p.class_map, (int)p.projection, p.solve, p.pcg_rebuild, p.reuse_mask,
                    (int)p.tail};
  for (int q = 0; q < 9; ++q) f[8 + q] = v[q];
}
'''
STAGE_FIELDS = ("buoy", "grav", "wall", "periodic", "px", "py", "second_bcs", "confine")
STEP_FIELDS = ("viscous", "advect", "correct_scalar", "class_map", "projection", "solve", "pcg_rebuild", "reuse_mask", "tail")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("step_plan")
    cpp, so = str(d / "plan.cpp"), str(d / "libplan.so")
    open(cpp, "w").write(PROGRAM)
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-fPIC", "-shared", "-I", build.CSRC, cpp, "-o", so],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    plan = ctypes.CDLL(so)
    plan.layout.argtypes = [sz, sz, ci, sz, sz, sz, vp, vp]
    plan.stage.argtypes = [ctypes.POINTER(Prm), ci, ci, vp, vp]
    plan.step.argtypes = [ctypes.POINTER(Prm), ci, ci, ci, vp, vp]
    return plan


@pytest.mark.parametrize("shape", list(LAYOUT))
def test_step_layout(lib, plan, shape):
    """offsets to the byte, the size alone without a base, the size the library reports, and a tail that holds each of its users"""
    B, D, H, W = shape
    want, g = LAYOUT[shape], _grid(*shape)
    cells, nc = B * D * H * W, 3 if D > 1 else 2
    base = ctypes.create_string_buffer(16)
    out = (ctypes.c_long * 10)()
    plan.layout(cells, nc, int(D > 1), want["mask"], want["kept"], want["tail_need"], ctypes.cast(base, vp), out)
    assert dict(zip(REGIONS, out)) == want["at"]
    assert (out[8], out[9]) == (want["tail_need"], WS_BYTES[shape][0]) and out[9] == _ws(lib, g, OP_STEP)
    plan.layout(cells, nc, int(D > 1), want["mask"], want["kept"], want["tail_need"], None, out)
    assert tuple(out) == (-1,) * 8 + (want["tail_need"], WS_BYTES[shape][0])
    users = dict(advect=_ws(lib, g, OP_ADVECT_STEP), jacobi=_ws(lib, g, OP_JACOBI), net=_ws(lib, g, OP_FLUIDNET),
                 pcg=lib.fnx_pcg_workspace_bytes(ctypes.byref(g)) - want["kept"], periodic=B * D * (H + W) * 4)
    assert all(n > 0 for n in users.values())
    assert {k: n for k, n in users.items() if want["tail_need"] < n} == {}
    assert want["tail_need"] == max(users.values())


GRAVITY = (0.3, -0.7, 1.1)          # three different components, none of them a sum of a few powers of two
F32 = np.float32


def _strengths(scale, dt):
    """(gravity_vec * -scale) * dt in fp32, in that order"""
    ns = -F32(scale)
    return [(F32(c) * ns) * F32(dt) for c in GRAVITY]


def _bits(values):
    return [int(np.asarray(v, dtype=np.float32).view(np.uint32)) for v in values]


def _model(method, rho, stick, bc, static_flags, periodic, viscosity, confine, gravity_scale, buoyancy_scale, correct_scalar, dt):
    """the decisions as the code before fnx_step_plan.h made them, each where it stood"""
    wall = method != 1                                                       # fnx_pre_projection
    stage = dict(buoy=rho and buoyancy_scale > 0, grav=rho and gravity_scale > 0, wall=wall, periodic=wall and bool(periodic & 1),
                 px=bool(periodic & 2), py=bool(periodic & 4), second_bcs=not (method == 1 and stick), confine=confine > 0)
    zeros = [F32(0)] * 3
    x = (_strengths(buoyancy_scale, dt) if stage["buoy"] else zeros) + (_strengths(gravity_scale, dt) if stage["grav"] else zeros)
    viscous = viscosity > 0                                                  # fnx_simulate_step
    use_stick = method == 1 and stick
    step = dict(viscous=viscous, advect=2 if not rho else (1 if viscous else 0), correct_scalar=rho and correct_scalar,
                class_map=0 if not (static_flags & 2 and bc) else (2 if static_flags & 4 else 1),
                projection={0: 0, 2: 1, 3: 2, 4: 3, 1: 5 if use_stick else 4}[method], solve=method != 1,
                pcg_rebuild=(static_flags & 9) != 9, reuse_mask=bool(static_flags & 1),
                tail=(2 if use_stick else 3) if method == 1 else (1 if periodic & 1 else 0))
    return stage, x, step


def test_stage_and_step_plan(plan):
    """every field of both plans over the cross product of what they depend on; the strengths to the bit"""
    f, x = (ci * 17)(), (ctypes.c_float * 8)()
    dt, rho_star = 0.1, 0.37
    n = 0
    for method, rho, ubc, rbc, static_flags, periodic, viscosity, stick, confine, gravity_scale in itertools.product(
            (0, 1, 2, 3, 4), (False, True), (False, True), (False, True), (0, 1, 3, 7, 9, 15), (0, 1, 3, 5, 7), (0.0, 0.05), (False, True),
            (0.0, 0.7), (0.0, 1.3)):
        # the buoyancy and correctScalar go with the parity of the case number, so that both values meet every other choice
        buoyancy_scale, correct_scalar = (2.3, 0.0)[n & 1], (n >> 1) & 1
        n += 1
        prm = Prm(dt=dt, buoyancy_scale=buoyancy_scale, gravity_vec=GRAVITY, operating_density=rho_star, method=method,
                  static_flags=static_flags, viscosity=viscosity, gravity_scale=gravity_scale, correct_scalar=correct_scalar,
                  periodic=periodic, vorticity_confinement=confine)
        stage, strengths, step = _model(method, rho, stick, ubc or rbc, static_flags, periodic, viscosity, confine, gravity_scale,
                                        buoyancy_scale, bool(correct_scalar), dt)
        case = (method, rho, ubc, rbc, static_flags, periodic, viscosity, stick, confine, gravity_scale, buoyancy_scale, correct_scalar)
        want_x = _bits(strengths + [F32(rho_star), F32(confine)])
        plan.stage(ctypes.byref(prm), rho, stick, f, x)
        assert dict(zip(STAGE_FIELDS, f[:8])) == {k: int(v) for k, v in stage.items()}, case
        assert _bits(x) == want_x, case
        plan.step(ctypes.byref(prm), rho, stick, ubc or rbc, f, x)
        assert dict(zip(STAGE_FIELDS, f[:8])) == {k: int(v) for k, v in stage.items()}, case
        assert dict(zip(STEP_FIELDS, f[8:])) == {k: int(v) for k, v in step.items()}, case
        assert _bits(x) == want_x, case
    assert n == 19200


def test_strengths_written_out(plan):
    """one case by hand: gravity (0.3, -0.7, 1.1), buoyancy scale 2.3, gravity scale 1.3, dt 0.1 -- the fp32 products (g * -scale) * dt"""
    f, x = (ci * 17)(), (ctypes.c_float * 8)()
    prm = Prm(dt=0.1, buoyancy_scale=2.3, gravity_vec=GRAVITY, gravity_scale=1.3)
    plan.stage(ctypes.byref(prm), 1, 0, f, x)
    assert _bits(x[:6]) == [0xbd8d4fdf, 0x3e24dd2f, 0xbe818937, 0xbd1fbe77, 0x3dba5e35, 0xbe126e97]
    plan.stage(ctypes.byref(prm), 0, 0, f, x)            # no density: neither force
    assert list(f[:2]) == [0, 0] and _bits(x[:6]) == [0] * 6
