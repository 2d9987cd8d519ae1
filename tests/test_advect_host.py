"""The advection entry points of the C ABI without a GPU: the workspace sizes callers allocate by, and the refusals, which are all made
before the first launch (on dummy host pointers that nothing may read)."""
import ctypes
import os
import re

import pytest

from fluidnet_cxx_amd import build

REPO = os.path.dirname(build.HERE)
vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float


class _FnxGrid(ctypes.Structure):
    _fields_ = [(n, ci) for n in ("B", "D", "H", "W", "is3D", "ref_quirks", "z_offset", "D_global", "k_begin", "k_end")]


def _grid(B, D, H, W, **kw):
    return _FnxGrid(B=B, D=D, H=H, W=W, is3D=int(D > 1), **kw)


def _enum(name):
    return int(re.search(name + r" = (\d+)", open(os.path.join(REPO, "include", "fluidnet_hip.h")).read()).group(1))


OP_SCALAR, OP_VEL, OP_STEP, OP_ADVECT_STEP = (_enum(n) for n in ("FNX_OP_ADVECT_SCALAR", "FNX_OP_ADVECT_VEL", "FNX_OP_STEP", "FNX_OP_ADVECT_STEP"))
EINVAL, EMETHOD, EWORKSPACE = _enum("FNX_EINVAL"), _enum("FNX_EMETHOD"), _enum("FNX_EWORKSPACE")
MACCORMACK, EULER = _enum("FNX_ADVECT_MACCORMACK"), _enum("FNX_ADVECT_EULER")
PLANS = [_enum("FNX_ADVECT_PLAN_" + n) for n in ("AUTO", "TILES", "CELLS", "TILES_SPLIT")]

GRIDS = [(2, 1, 40, 70), (1, 9, 20, 66), (1, 16, 33, 130)]
# fnx_workspace_bytes of the build before the workspace layout became one function (fields and bitmaps, each rounded up to 256 bytes)
WS_BYTES = {
    (2, 1, 40, 70): {OP_SCALAR: 50176, OP_VEL: 49920, OP_ADVECT_STEP: 94976, OP_STEP: 6133760},
    (1, 9, 20, 66): {OP_SCALAR: 201984, OP_VEL: 154112, OP_ADVECT_STEP: 344576, OP_STEP: 12868352},
    (1, 16, 33, 130): {OP_SCALAR: 1149184, OP_VEL: 874496, OP_ADVECT_STEP: 1972992, OP_STEP: 74259968},
}


@pytest.fixture(scope="module")
def lib():
    build.build_all()
    lib = ctypes.CDLL(build.LIB)
    lib.fnx_last_error.restype = ctypes.c_char_p
    lib.fnx_workspace_bytes.restype = ctypes.c_size_t
    lib.fnx_workspace_bytes.argtypes = [ctypes.POINTER(_FnxGrid), ci]
    G, tail = ctypes.POINTER(_FnxGrid), [ci, vp, ctypes.c_size_t, vp]          # plan, ws, ws_bytes, stream
    lib.fnx_advect_scalar_plan.argtypes = [G, cf, vp, vp, vp, vp, ci, ci, ci, cf] + tail
    lib.fnx_advect_vel_plan.argtypes = [G, cf, vp, vp, vp, vp, ci, ci, cf] + tail
    lib.fnx_advect_step_plan.argtypes = [G, cf, vp, vp, vp, vp, vp, ci, cf] + tail
    return lib


@pytest.mark.parametrize("shape", GRIDS)
def test_workspace_bytes(lib, shape):
    g = _grid(*shape)
    assert {op: lib.fnx_workspace_bytes(ctypes.byref(g), op) for op in WS_BYTES[shape]} == WS_BYTES[shape]
    # neither a compute window nor a z-slab view changes what a call needs: the fields are indexed like the arrays
    if g.is3D:
        for view in (dict(k_begin=2, k_end=5), dict(z_offset=3, D_global=shape[1] + 7)):
            gv = _grid(*shape, **view)
            assert {op: lib.fnx_workspace_bytes(ctypes.byref(gv), op) for op in WS_BYTES[shape]} == WS_BYTES[shape]


class _Calls:
    """the three entry points on dummy pointers: call(name, **changes) -> (return code, fnx_last_error())"""

    def __init__(self, lib, g):
        self.lib, self.g = lib, g
        self.p = {n: ctypes.cast(ctypes.create_string_buffer(64), vp) for n in ("rho", "U", "orig", "flags", "rho_dst", "U_dst", "ws")}
        self.op = dict(advect_scalar=OP_SCALAR, advect_vel=OP_VEL, advect_step=OP_ADVECT_STEP)

    def need(self, name):
        return self.lib.fnx_workspace_bytes(ctypes.byref(self.g), self.op[name])

    def __call__(self, name, method=None, bnd=1, plan=0, ws_bytes=None, **ptrs):
        p = dict(self.p, **ptrs)
        method = MACCORMACK if method is None else method
        ws_bytes = self.need(name) if ws_bytes is None else ws_bytes
        g, tail = ctypes.byref(self.g), (plan, p["ws"], ws_bytes, None)
        if name == "advect_scalar":
            rc = self.lib.fnx_advect_scalar_plan(g, 0.1, p["rho"], p["U"], p["flags"], p["rho_dst"], method, bnd, 0, 0.6, *tail)
        elif name == "advect_vel":
            rc = self.lib.fnx_advect_vel_plan(g, 0.1, p["orig"], p["U"], p["flags"], p["U_dst"], method, bnd, 0.6, *tail)
        else:
            rc = self.lib.fnx_advect_step_plan(g, 0.1, p["rho"], p["U"], p["flags"], p["rho_dst"], p["U_dst"], 0, 0.6, *tail)
        return rc, self.lib.fnx_last_error().decode()


ENTRIES = ["advect_scalar", "advect_vel", "advect_step"]


@pytest.mark.parametrize("shape", GRIDS[:2])
@pytest.mark.parametrize("name", ENTRIES)
def test_workspace_refusal(lib, shape, name):
    """one byte short (or no workspace at all): FNX_EWORKSPACE, the entry point's name and the size fnx_workspace_bytes gives, under every
    plan -- the plan changes the kernels, never the layout"""
    call = _Calls(lib, _grid(*shape))
    need = call.need(name)
    assert need == WS_BYTES[shape][call.op[name]]
    for plan in PLANS:
        assert call(name, plan=plan, ws_bytes=need - 1) == (EWORKSPACE, f"{name}: workspace too small ({need - 1} < {need})")
    assert call(name, ws=None) == (EWORKSPACE, f"{name}: workspace too small ({need} < {need})")
    if name == "advect_vel":                               # the viscous step's call (orig is not U) needs the same
        assert call(name, orig=call.p["U"], ws_bytes=need - 1) == (EWORKSPACE, f"{name}: workspace too small ({need - 1} < {need})")


@pytest.mark.parametrize("shape", GRIDS[:2])
@pytest.mark.parametrize("name", ENTRIES)
def test_argument_refusals(lib, shape, name):
    """code and text of each refusal, and their order: grid, plan, NULL tensor, aliasing, method, boundary width, workspace"""
    call = _Calls(lib, _grid(*shape))
    short = dict(ws_bytes=call.need(name) - 1)             # every call below would also be refused for its workspace: the check made first wins
    for plan in (-1, 4):
        assert call(name, plan=plan, rho=None, U=None, **short) == (EINVAL, f"{name}: unknown plan {plan}")
    mine = dict(advect_scalar=("rho", "U", "flags", "rho_dst"), advect_vel=("orig", "U", "flags", "U_dst"),
                advect_step=("rho", "U", "flags", "rho_dst", "U_dst"))[name]
    for ptr in mine:
        assert call(name, **{ptr: None}, **short) == (EINVAL, f"{name}: NULL tensor")
    p = call.p
    if name == "advect_scalar":
        assert call(name, rho_dst=p["rho"], method=7, **short) == (EINVAL, "advect_scalar: dst must not alias src")
    elif name == "advect_vel":
        assert call(name, U_dst=p["orig"], method=7, **short) == (EINVAL, "advect_vel: dst must not alias orig or U")
        assert call(name, U_dst=p["U"], method=7, **short) == (EINVAL, "advect_vel: dst must not alias orig or U")
    else:
        assert call(name, rho_dst=p["rho"], **short) == (EINVAL, "advect_step: dst must not alias the inputs")
        assert call(name, U_dst=p["U"], **short) == (EINVAL, "advect_step: dst must not alias the inputs")
        return                                             # the pair is MacCormack with boundary width 1 by definition
    for method in (-1, 2):
        assert call(name, method=method, bnd=0, **short) == (EMETHOD, "Advection method not supported")
    text = {"advect_scalar": "advect_scalar: only boundary_width == 1 is supported (the reference's MAC sampling strips exactly one border cell)",
            "advect_vel": "advect_vel: only boundary_width == 1 is supported"}[name]
    for bnd in (0, 2):
        for method in (EULER, MACCORMACK):
            assert call(name, method=method, bnd=bnd, **short) == (EINVAL, text)


def test_bad_grid_is_refused_first(lib):
    for name in ENTRIES:
        rc, text = _Calls(lib, _FnxGrid(B=1, D=1, H=2, W=40))(name, plan=9, ws_bytes=0)
        assert rc == EINVAL and text == "Dimension mismatch: B=1 D=1 H=2 W=40"
