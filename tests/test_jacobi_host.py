"""The host side of the Jacobi solve without a GPU: the workspace sizes callers allocate by, every refusal of the C entry points (all made
before the first launch, on dummy host pointers that nothing may read), and the pure functions of csrc/fnx_jacobi_plan.h -- the launch
schedule, the tile geometry, the mask layout, the plan of a two-sweep launch and the mirror predicate -- called from a host-only
program with 256 compute units.  The expected values are written out: they are what the code before these functions existed did for the
same cases (two copies of the schedule loop, the plan inside launch_jacobi3d_x2), worked out by hand from it."""
import ctypes
import os
import re
import subprocess

import pytest

from fluidnet_cxx_amd import build

REPO = os.path.dirname(build.HERE)
vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float


class _FnxGrid(ctypes.Structure):
    _fields_ = [(n, ci) for n in ("B", "D", "H", "W", "is3D", "ref_quirks", "z_offset", "D_global", "k_begin", "k_end")]


class _FnxPlaneMirror(ctypes.Structure):
    _fields_ = [("out", vp * 2 * 2), ("slot_select", vp * 2), ("k_first", ci * 2), ("planes", ci), ("sample_stride", ctypes.c_size_t),
                ("start_clock", vp)]


def _grid(B, D, H, W, **kw):
    return _FnxGrid(B=B, D=D, H=H, W=W, is3D=int(D > 1), **kw)


def _enum(name):
    return int(re.search(name + r" = (\d+)", open(os.path.join(REPO, "include", "fluidnet_hip.h")).read()).group(1))


OP_JACOBI, OP_STEP = _enum("FNX_OP_JACOBI"), _enum("FNX_OP_STEP")
EINVAL, EWORKSPACE = _enum("FNX_EINVAL"), _enum("FNX_EWORKSPACE")

# fnx_workspace_bytes of the build before the mask layout became one function; (1, 6, 21, 66): H is no multiple of 4
WS_BYTES = {
    (2, 1, 40, 70): {OP_JACOBI: 30976, OP_STEP: 6133760},
    (1, 9, 20, 66): {OP_JACOBI: 76288, OP_STEP: 12868352},
    (1, 16, 33, 130): {OP_JACOBI: 423168, OP_STEP: 74259968},
    (1, 6, 21, 66): {OP_JACOBI: 56064, OP_STEP: 9014528},
}
G2D, G3D, G3D_ODD = (2, 1, 40, 70), (1, 9, 20, 66), (1, 6, 21, 66)


@pytest.fixture(scope="module")
def lib():
    build.build_all()
    lib = ctypes.CDLL(build.LIB)
    lib.fnx_last_error.restype = ctypes.c_char_p
    lib.fnx_workspace_bytes.restype = ctypes.c_size_t
    G, sz = ctypes.POINTER(_FnxGrid), ctypes.c_size_t
    lib.fnx_workspace_bytes.argtypes = [G, ci]
    lib.fnx_jacobi.argtypes = [G, vp, vp, vp, vp, cf, ci, vp, vp, sz, vp]
    lib.fnx_jacobi_sweeps_ex.argtypes = [G, vp, vp, vp, ci, vp, sz, ci, vp]
    lib.fnx_jacobi_pass_layout.argtypes = [G, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp, sz, ci, vp]
    lib.fnx_jacobi_pass_mirror.argtypes = [G, vp, vp, vp, vp, ci, ci, ci, ci, ctypes.POINTER(_FnxPlaneMirror), vp, sz, ci, vp]
    lib.fnx_jacobi_quad_ok.argtypes = [G]
    lib.fnx_jacobi_pass_mirror_ok.argtypes = [G, ci, ci, ci]
    return lib


@pytest.mark.parametrize("shape", list(WS_BYTES))
def test_workspace_bytes(lib, shape):
    g = _grid(*shape)
    assert {op: lib.fnx_workspace_bytes(ctypes.byref(g), op) for op in WS_BYTES[shape]} == WS_BYTES[shape]
    if g.is3D:   # neither a compute window nor a z-slab view changes what a call needs
        for view in (dict(k_begin=2, k_end=5), dict(z_offset=3, D_global=shape[1] + 7)):
            gv = _grid(*shape, **view)
            assert {op: lib.fnx_workspace_bytes(ctypes.byref(gv), op) for op in WS_BYTES[shape]} == WS_BYTES[shape]


class _Calls:
    """the four entry points on dummy pointers: call(name, **changes) -> (return code, fnx_last_error())"""

    def __init__(self, lib, g):
        self.lib, self.g = lib, g
        self.p = {n: ctypes.cast(ctypes.create_string_buffer(64), vp) for n in ("flags", "div", "p", "p_in", "residual", "ws", "m00", "m01", "m10", "m11", "sel")}
        self.need = lib.fnx_workspace_bytes(ctypes.byref(g), OP_JACOBI)

    def mirror(self, planes=1, out=("m00", None, "m10", None), sel=(None, None)):
        m = _FnxPlaneMirror(planes=planes, sample_stride=4096)
        for r in range(2):
            for q in range(2):
                m.out[r][q] = self.p[out[2 * r + q]] if out[2 * r + q] else None
            m.slot_select[r] = self.p[sel[r]] if sel[r] else None
        return m

    def __call__(self, name, n=2, kb=0, ke=0, kb2=-1, layout=0, reuse=0, ws_bytes=None, mirror="default", **ptrs):
        p = dict(self.p, **ptrs)
        ws_bytes = self.need if ws_bytes is None else ws_bytes
        g = ctypes.byref(self.g)
        if name == "solve":
            rc = self.lib.fnx_jacobi(g, p["flags"], p["div"], p["p"], p["residual"], 0.0, n, None, p["ws"], ws_bytes, None)
        elif name == "sweeps":
            rc = self.lib.fnx_jacobi_sweeps_ex(g, p["flags"], p["div"], p["p"], n, p["ws"], ws_bytes, reuse, None)
        elif name == "pass":
            rc = self.lib.fnx_jacobi_pass_layout(g, p["flags"], p["div"], p["p_in"], p["p"], n, kb, ke, kb2, layout, p["ws"], ws_bytes, reuse, None)
        else:
            m = self.mirror() if mirror == "default" else mirror
            rc = self.lib.fnx_jacobi_pass_mirror(g, p["flags"], p["div"], p["p_in"], p["p"], kb, ke, kb2, layout, ctypes.byref(m) if m else None,
                                                 p["ws"], ws_bytes, reuse, None)
        return rc, self.lib.fnx_last_error().decode()


NAMES = dict(solve="solve_linear_system", sweeps="jacobi_sweeps")
NAMES["pass"], NAMES["mirror"] = "jacobi_pass", "jacobi_pass_mirror"
MAXITER = "At least 1 iteration is needed (maxIter < 1)"


@pytest.mark.parametrize("shape", [G2D, G3D, G3D_ODD])
@pytest.mark.parametrize("name", ["solve", "sweeps", "pass", "mirror"])
def test_workspace_refusal(lib, shape, name):
    """one byte short, or no workspace at all: FNX_EWORKSPACE under the entry point's name with the size fnx_workspace_bytes gives -- whether
    or not the call would reuse the mask, since it is refused before the mask is built"""
    if shape == G2D and name in ("pass", "mirror"):
        return                                             # 3D only: refused before the workspace is looked at (test_refusals_pass)
    call = _Calls(lib, _grid(*shape))
    need = call.need
    assert need == WS_BYTES[shape][OP_JACOBI]
    args = dict(kb=2, ke=4) if name == "mirror" else {}
    for reuse in (0, 1):
        assert call(name, ws_bytes=need - 1, reuse=reuse, **args) == (EWORKSPACE, f"{NAMES[name]}: workspace too small ({need - 1} < {need})")
    assert call(name, ws=None, **args) == (EWORKSPACE, f"{NAMES[name]}: workspace too small ({need} < {need})")
    assert call(name, ws=None, ws_bytes=0, **args) == (EWORKSPACE, f"{NAMES[name]}: workspace too small (0 < {need})")


@pytest.mark.parametrize("shape", [G2D, G3D])
def test_refusals_solve_and_sweeps(lib, shape):
    """order: grid, NULL tensor, iteration count, workspace (then, for the solve, the launch limit); each with the later ones failing too"""
    call = _Calls(lib, _grid(*shape))
    short = dict(ws_bytes=call.need - 1)
    for name in ("solve", "sweeps"):
        for ptr in ("flags", "div", "p"):
            assert call(name, n=0, **{ptr: None}, **short) == (EINVAL, f"{NAMES[name]}: NULL tensor")
        for n in (0, -3):
            assert call(name, n=n, **short) == (EINVAL, MAXITER)
            assert call(name, n=n, ws=None) == (EINVAL, MAXITER)
        bad = _Calls(lib, _FnxGrid(B=1, D=1, H=2, W=40))
        assert bad(name, n=0, flags=None, ws_bytes=0) == (EINVAL, "Dimension mismatch: B=1 D=1 H=2 W=40")
    assert call("solve", n=10 ** 6, **short) == (EWORKSPACE, f"solve_linear_system: workspace too small ({call.need - 1} < {call.need})")


def test_solve_launch_limit_2d(lib):
    """(2, 1, 40, 70) runs launches of up to 28 sweeps (every tile has a compute unit to itself), and a call at most 1022 launches: 28616 fused
    sweeps.  The sweep that a caller who wants the residual gets on its own does not count."""
    call = _Calls(lib, _grid(*G2D))
    text = "solve_linear_system: max_iter too large for one call (%d)"
    assert call("solve", n=28617, residual=None) == (EINVAL, text % 28617)
    assert call("solve", n=28618) == (EINVAL, text % 28618)
    for n in (10 ** 6, 2 * 10 ** 9):
        assert call("solve", n=n, residual=None) == (EINVAL, text % n)
        assert call("solve", n=n) == (EINVAL, text % n)


def test_refusals_pass(lib):
    """fnx_jacobi_pass_layout; order: grid, layout range, what a layout needs, NULL or aliased, 3D only, nsweeps, plane range, second range,
    workspace"""
    call, odd, flat = _Calls(lib, _grid(*G3D)), _Calls(lib, _grid(*G3D_ODD)), _Calls(lib, _grid(*G2D))
    short = dict(ws_bytes=call.need - 1)
    D = G3D[1]
    assert _Calls(lib, _FnxGrid(B=1, D=2, H=20, W=40, is3D=1))("pass", layout=7, flags=None) == (EINVAL, "3D domain needs D >= 3")
    for layout in (-1, 4):
        assert call("pass", layout=layout, n=1, flags=None, kb=-1, **short) == (EINVAL, "jacobi_pass: layout must be 0..3")
    needs = "jacobi_pass: the row-quad layout needs a two-sweep pass on a grid fnx_jacobi_quad_ok accepts"
    for layout in (1, 2, 3):
        assert call("pass", layout=layout, n=1, flags=None, **short) == (EINVAL, needs)      # a one-sweep pass
        assert odd("pass", layout=layout, n=2, flags=None, ws_bytes=0) == (EINVAL, needs)    # H % 4 != 0
        assert flat("pass", layout=layout, n=2, flags=None, ws_bytes=0) == (EINVAL, needs)   # 2D
    for layout in (0, 3):
        for ptr in ("flags", "div", "p"):
            assert call("pass", layout=layout, **{ptr: None}, kb=-1, **short) == (EINVAL, "jacobi_pass: NULL or aliased tensor")
        assert call("pass", layout=layout, p_in=call.p["p"], kb=-1, **short) == (EINVAL, "jacobi_pass: NULL or aliased tensor")
    assert flat("pass", n=3, kb=-1, ws_bytes=0) == (EINVAL, "jacobi_pass: 3D only (2D uses fnx_jacobi_sweeps)")
    for n in (0, 3):
        assert call("pass", n=n, kb=-1, **short) == (EINVAL, "jacobi_pass: nsweeps must be 1 or 2")
    for n in (1, 2):
        for kb, ke in ((-1, 3), (0, D + 1), (4, 4), (5, 2)):
            assert call("pass", n=n, kb=kb, ke=ke, kb2=D, **short) == (EINVAL, "jacobi_pass: bad plane range")
        # the second range of (ke - kb) planes: none without a first, inside the grid, disjoint from the first on either side
        for kb, ke, kb2 in ((0, 0, 3), (3, 0, 5), (1, 4, D - 2), (2, 5, 4), (2, 5, 0), (2, 5, 2)):
            assert call("pass", n=n, kb=kb, ke=ke, kb2=kb2, **short) == (EINVAL, "jacobi_pass: bad or overlapping second plane range")
        for kb, ke, kb2 in ((1, 4, D - 3), (2, 5, 5), (3, 5, 1), (3, 0, -1)):     # accepted ranges: the workspace is next
            assert call("pass", n=n, kb=kb, ke=ke, kb2=kb2, **short)[0] == EWORKSPACE
    assert call("pass", n=2, layout=3, p_in=None, **short)[0] == EWORKSPACE          # a pass from zero is one


def test_refusals_mirror(lib):
    """fnx_jacobi_pass_mirror; order: grid, NULL / aliased / 2D, plane range, second range, whether the launch can mirror, the mirror,
    workspace"""
    call, odd, flat = _Calls(lib, _grid(*G3D)), _Calls(lib, _grid(*G3D_ODD)), _Calls(lib, _grid(*G2D))
    short = dict(ws_bytes=call.need - 1)
    D = G3D[1]
    assert _Calls(lib, _FnxGrid(B=1, D=2, H=20, W=40, is3D=1))("mirror", flags=None) == (EINVAL, "3D domain needs D >= 3")
    null = "jacobi_pass_mirror: NULL or aliased argument"
    for ptr in ("flags", "div", "p", "p_in"):
        assert call("mirror", kb=-1, **{ptr: None}, **short) == (EINVAL, null)
    assert call("mirror", kb=-1, p_in=call.p["p"], **short) == (EINVAL, null)
    assert call("mirror", kb=-1, mirror=None, **short) == (EINVAL, null)
    assert flat("mirror", kb=-1, ws_bytes=0) == (EINVAL, null)
    for kb, ke in ((-1, 3), (0, D + 1), (4, 4), (5, 2), (0, 0), (3, 0)):          # no "all planes" here
        assert call("mirror", kb=kb, ke=ke, kb2=D, layout=1, **short) == (EINVAL, "jacobi_pass_mirror: bad plane range")
    for kb, ke, kb2 in ((1, 4, D - 2), (2, 5, 4), (2, 5, 0), (2, 5, 2)):
        assert call("mirror", kb=kb, ke=ke, kb2=kb2, layout=1, **short) == (EINVAL, "jacobi_pass_mirror: bad or overlapping second plane range")
    cannot = "jacobi_pass_mirror: this launch cannot mirror its output (fnx_jacobi_pass_mirror_ok)"
    bad_mirror = call.mirror(planes=0)
    for layout in (1, 2, -1, 4):
        assert call("mirror", kb=2, ke=4, layout=layout, mirror=bad_mirror, **short) == (EINVAL, cannot)
    assert odd("mirror", kb=2, ke=4, layout=3, mirror=bad_mirror, ws_bytes=0) == (EINVAL, cannot)       # row quads need H % 4 == 0
    big = _Calls(lib, _grid(1, 40, 700, 1030))                                   # 3150 tiles: one range has its resident set, two have not
    assert big("mirror", kb=2, ke=4, kb2=9, mirror=bad_mirror, ws_bytes=0) == (EINVAL, cannot)
    assert big("mirror", kb=2, ke=4, mirror=bad_mirror, ws_bytes=0) == (EINVAL, "jacobi_pass_mirror: bad mirror")
    for layout in (0, 3):
        for kb2, m in ((-1, call.mirror(planes=0)), (-1, call.mirror(out=(None, "m01", "m10", "m11"))),
                       (-1, call.mirror(sel=("sel", None))),                       # a slot to choose and no second slot
                       (6, call.mirror(out=("m00", None, None, "m11"))), (6, call.mirror(sel=(None, "sel")))):
            assert call("mirror", kb=2, ke=4, kb2=kb2, layout=layout, mirror=m, **short) == (EINVAL, "jacobi_pass_mirror: bad mirror")
        # the same mirrors where nothing asks for their missing parts: the workspace is next
        for kb2, m in ((-1, call.mirror(out=("m00", None, None, None))), (-1, call.mirror(out=("m00", "m01", None, None), sel=("sel", "sel"))),
                       (6, call.mirror(out=("m00", "m01", "m10", "m11"), sel=("sel", "sel")))):
            assert call("mirror", kb=2, ke=4, kb2=kb2, layout=layout, mirror=m, **short)[0] == EWORKSPACE


def test_quad_ok_and_mirror_ok(lib):
    """the two predicates of the C ABI (no device: 256 compute units, 4096 wave slots)"""
    def quad(g):
        return lib.fnx_jacobi_quad_ok(ctypes.byref(g))

    def mirror(shape, planes, two, layout, **kw):
        return lib.fnx_jacobi_pass_mirror_ok(ctypes.byref(_grid(*shape, **kw)), planes, two, layout)

    assert [quad(_grid(*s)) for s in (G3D, (1, 12, 24, 66), G3D_ODD, (1, 9, 22, 66), G2D)] == [1, 1, 0, 0, 0]
    assert quad(_FnxGrid(B=1, D=2, H=20, W=40, is3D=1)) == 0 and quad(_grid(*G3D, k_begin=2, k_end=5)) == 1
    assert [mirror(G3D, 3, two, lay) for two in (0, 1) for lay in (0, 1, 2, 3)] == [1, 0, 0, 1, 1, 0, 0, 1]
    assert mirror(G3D_ODD, 3, 0, 3) == 1                    # whether the grid can hold row quads is fnx_jacobi_quad_ok's to say
    assert [mirror(G3D, n, 0, 0) for n in (-1, 0, 1)] == [0, 0, 1]
    assert mirror(G2D, 1, 0, 0) == 0 and mirror((1, 2, 20, 40), 1, 0, 0) == 0
    # one resident set: 54 tiles; 2048 tiles twice = the 4096 slots, 2064 twice do not fit; 4080 once, 4097 not
    assert [mirror((1, 40, 70, 130), 6, two, 3) for two in (0, 1)] == [1, 1]
    assert [mirror((1, 8, 512, 960), 4, two, 0) for two in (0, 1)] == [1, 1]
    assert [mirror((1, 8, 513, 960), 4, two, 0) for two in (0, 1)] == [1, 0]
    assert [mirror((1, 40, 700, 1030), 9, two, 3) for two in (0, 1)] == [1, 0]
    assert [mirror(s, 9, 0, 0) for s in ((1, 40, 960, 1020), (1, 40, 964, 1020), (1, 40, 1040, 1030))] == [1, 0, 0]
    # 32-bit offsets: (planes + 4) * H * W below 0x3fffffff; 960 x 1020 is 979200 cells a plane
    assert [mirror((1, 1100, 960, 1020), n, 0, 0) for n in (1092, 1093)] == [1, 0]


# ---- the pure functions, from a host-only program -------------------------------------------------------------------------------------
PROGRAM = r'''
struct GridDims { int B, D, H, W, HW, DHW; };
#include "fnx_jacobi_plan.h"
using namespace fnx;
static GridDims dims(const int* s) { return GridDims{s[0], s[1], s[2], s[3], s[2] * s[3], s[1] * s[2] * s[3]}; }
// out: n, kmax, then (sweeps, lay) per launch; returns the solve's first buffer with and without residual in bits 1 and 0
extern "C" int schedule(const int* s, int is3d, int nsweeps, int cus, int* out, int cap) {
  const JacobiSchedule sch = jacobi_schedule(dims(s), is3d != 0, nsweeps, cus);
  out[0] = sch.n; out[1] = sch.kmax;
  for (int l = 0; l < sch.n && 2 * l + 3 < cap; ++l) { out[2 + 2 * l] = sch.at(l).sweeps; out[3 + 2 * l] = sch.at(l).lay; }
  return jacobi_solve_first_buffer(sch, true) * 2 + jacobi_solve_first_buffer(sch, false);
}
extern "C" void tiles(const int* s, int cus, long* out) {
  const Jacobi3dTiles t = jacobi3d_tiles(dims(s));
  out[0] = t.nxt; out[1] = t.nyt; out[2] = t.ntiles; out[3] = t.kwords; out[4] = jacobi3d_wave_slots(cus);
}
extern "C" void mask_layout(const int* s, char* base, long* out) {
  const JacobiMaskLayout m = jacobi3d_mask_layout(dims(s), base);
  out[0] = base ? (char*)m.rows - base : (m.rows ? -1 : 0); out[1] = base ? (char*)m.quads - base : (m.quads ? -1 : 0);
  out[2] = base ? (char*)m.same - base : (m.same ? -1 : 0); out[3] = (long)m.bytes;
}
extern "C" void x2_plan(const int* s, int np, int two, int from_zero, int lay, int cus, long* out) {
  const Jacobi3dX2Plan p = jacobi3d_x2_plan(dims(s), np, two != 0, from_zero != 0, lay, cus);
  out[0] = p.zchunk; out[1] = p.split; out[2] = (long)p.G; out[3] = p.serial; out[4] = p.lay;
  out[5] = jacobi3d_mirror_ok(dims(s), np, two != 0, from_zero != 0, lay, cus);
}
'''
CUS = 256


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("jacobi_plan")
    cpp, so = str(d / "plan.cpp"), str(d / "libplan.so")
    open(cpp, "w").write(PROGRAM)
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-fPIC", "-shared", "-I", build.CSRC, cpp, "-o", so],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    return ctypes.CDLL(so)


def _shape(s):
    return (ci * 4)(*s)


def _schedule(plan, shape, n):
    """(launches as (sweeps, lay), first buffer of a solve without residual, with residual): 0 = p, 1 = the workspace's"""
    out = (ci * 2048)()
    first = plan.schedule(_shape(shape), int(shape[1] > 1), n, CUS, out, 2048)
    return [(out[2 + 2 * l], out[3 + 2 * l]) for l in range(out[0])], first & 1, first >> 1


def _solve(plan, shape, max_iter, residual):
    """what fnx_jacobi(max_iter) launches: [(sweeps, lay, the buffer written)]"""
    launches, first, first_res = _schedule(plan, shape, max_iter - 1 if residual else max_iter)
    first = first_res if residual else first
    got = [(k, lay, "p tmp".split()[(first + l) & 1]) for l, (k, lay) in enumerate(launches)]
    return got + [(1, 0, "p")] if residual else got


def _sweeps_ex(plan, shape, n):
    """what fnx_jacobi_sweeps_ex(n) launches, from zero or not: it starts at the workspace's buffer (an odd count is copied back)"""
    return [(k, lay, "p tmp".split()[(1 + l) & 1]) for l, (k, lay) in enumerate(_schedule(plan, shape, n)[0])]


def _pingpong(sizes, last="p", lays=None):
    bufs = ["p" if (len(sizes) - 1 - l) % 2 == 0 else "tmp" for l in range(len(sizes))]
    if last == "tmp":
        bufs = ["tmp" if b == "p" else "p" for b in bufs]
    return list(zip(sizes, lays or [0] * len(sizes), bufs))


# launch sizes of a run of n sweeps.  (2, 1, 40, 70): up to 8 sweeps in launches of at most 7; above, its 90 tiles at K = 28 all have a
# compute unit, so the fewest launches of at most 28, dealt evenly.  (1, 1, 515, 509): the deepest launch whose tiles fit 256 units is
# K = 15 (34-wide windows: 15 x 16 tiles)
SIZES_2D = {
    (2, 1, 40, 70): {1: [1], 2: [2], 6: [6], 7: [7], 8: [7, 1], 9: [9], 15: [15], 16: [16], 27: [27], 28: [28], 36: [18, 18], 37: [19, 18],
                     99: [25, 25, 25, 24], 100: [25] * 4},
    (1, 1, 515, 509): {1: [1], 2: [2], 6: [6], 7: [7], 8: [7, 1], 9: [9], 15: [15], 16: [8, 8], 27: [14, 13], 28: [14, 14], 36: [12, 12, 12],
                       37: [13, 13, 11], 99: [15] * 6 + [9], 100: [15] * 6 + [10]},
}


@pytest.mark.parametrize("shape", list(SIZES_2D))
def test_schedule_2d(plan, shape):
    for n in (1, 2, 7, 8, 9, 16, 28, 37, 100):
        sizes = SIZES_2D[shape][n]
        assert _solve(plan, shape, n, False) == _pingpong(sizes), n                       # the last launch writes p
        assert _sweeps_ex(plan, shape, n) == _pingpong(sizes, "p" if len(sizes) % 2 == 0 else "tmp"), n   # the first writes the workspace's
        # with the residual: n - 1 sweeps fused, ending in the workspace's buffer, then one sweep into p
        fused = SIZES_2D[shape][n - 1] if n > 1 else []
        assert _solve(plan, shape, n, True) == _pingpong(fused, "tmp") + [(1, 0, "p")], n
    assert _schedule(plan, shape, 0)[0] == []


def test_schedule_3d(plan):
    """pairs of sweeps and one single for an odd count; where H % 4 == 0 consecutive pairs hand each other the row-quad layout: the first
    writes it (lay 2), those between read and write it (3), the last pair reads it and writes rows (1)"""
    quad, odd = (1, 12, 24, 66), (1, 6, 21, 66)
    lays = {1: [0], 2: [0], 3: [0, 0], 7: [2, 3, 1, 0], 10: [2, 3, 3, 3, 1], 6: [2, 3, 1], 9: [2, 3, 3, 1, 0]}
    sizes = {n: [2] * (n // 2) + [1] * (n % 2) for n in lays}
    for n in (1, 2, 3, 7, 10):
        for shape in (quad, odd):
            ly = lays[n] if shape == quad else [0] * len(lays[n])
            assert _solve(plan, shape, n, False) == _pingpong(sizes[n], "p", ly), (shape, n)
            assert _sweeps_ex(plan, shape, n) == _pingpong(sizes[n], "p" if len(sizes[n]) % 2 == 0 else "tmp", ly), (shape, n)
            fused = _pingpong(sizes[n - 1], "tmp", lays[n - 1] if shape == quad else None) if n > 1 else []
            assert _solve(plan, shape, n, True) == fused + [(1, 0, "p")], (shape, n)


def test_tiles_and_mask_layout(plan):
    """60 columns by 4 rows; the three regions of the mask allocation, each rounded up to 256 bytes, to the byte"""
    want = {(1, 12, 24, 66): ((2, 6, 12, 1), (0, 19200, 38400, 38656)), (1, 6, 21, 66): ((2, 6, 12, 1), (0, 8448, 18176, 18432)),
            (1, 40, 70, 130): ((3, 18, 54, 2), (0, 364032, 738560, 739072)), (2, 33, 61, 121): ((3, 16, 96, 2), (0, 487168, 998400, 999168)),
            (1, 40, 1040, 1030): ((18, 260, 4680, 2), (0, 42848000, 85696000, 85733632))}
    for shape, (t, m) in want.items():
        out = (ctypes.c_long * 5)()
        plan.tiles(_shape(shape), CUS, out)
        assert tuple(out) == t + (4096,), shape
        base = ctypes.create_string_buffer(16)
        for b in (base, None):
            plan.mask_layout(_shape(shape), b, out)
            assert tuple(out)[:4] == (m if b else (0, 0, 0, m[3])), shape


def _x2(plan, shape, np_, two=0, from_zero=0, lay=0):
    out = (ctypes.c_long * 6)()
    plan.x2_plan(_shape(shape), np_, two, from_zero, lay, CUS, out)
    return dict(zip(("zchunk", "split", "G", "serial", "lay", "mirror_ok"), out))


def test_x2_plan(plan):
    small, mid, wide, huge = (1, 12, 24, 66), (1, 40, 70, 130), (1, 40, 700, 1030), (1, 40, 1040, 1030)
    P = lambda zchunk, split, G, serial, lay, mirror_ok: dict(zchunk=zchunk, split=split, G=G, serial=serial, lay=lay, mirror_ok=mirror_ok)   # noqa: E731
    # one range in a small grid: 12 tiles, 341 chunks a tile would fit, so chunks of zmin = 2 planes; G rounded up to 8
    assert _x2(plan, small, 12) == P(2, 0, 72, 0, 0, 1)
    assert _x2(plan, small, 3, lay=1) == P(2, 0, 24, 0, 1, 0)
    assert _x2(plan, small, 1, lay=3) == P(2, 0, 16, 0, 3, 1)
    # from zero: no input, bit 0 of lay is dropped; never mirrored
    assert _x2(plan, small, 12, from_zero=1, lay=3) == P(2, 0, 72, 0, 2, 0)
    assert _x2(plan, small, 12, from_zero=1, lay=1) == P(2, 0, 72, 0, 0, 0)
    assert _x2(plan, small, 12, from_zero=1, lay=0) == P(2, 0, 72, 0, 0, 0)
    # two ranges share the resident set: 54 tiles, 75 chunks a tile, 37 for each range
    assert _x2(plan, mid, 6, two=1, lay=3) == P(2, 0, 328, 0, 3, 1)
    assert _x2(plan, mid, 40, lay=3) == P(2, 0, 1080, 0, 3, 1)
    assert _x2(plan, mid, 38, two=1) == P(2, 0, 2056, 0, 0, 1)
    assert _x2(plan, mid, 300, two=1) == P(9, 0, 3672, 0, 0, 1)
    assert _x2(plan, mid, 300) == P(4, 0, 4056, 0, 0, 1)
    # more tiles (4680) than slots (4096): SPLIT, G = tiles * planes / 8 capped at the slots, a multiple of 8 and at least 8
    assert _x2(plan, huge, 40, lay=3) == P(0, 1, 4096, 0, 3, 0)
    assert _x2(plan, huge, 7) == P(0, 1, 4088, 0, 0, 0)
    assert _x2(plan, (1, 3, 16, 61441), 3) == P(0, 1, 1536, 0, 0, 0)
    # two ranges that do not fit at once: two launches, each planned as one range
    assert _x2(plan, huge, 7, two=1) == P(0, 1, 4088, 1, 0, 0)
    assert _x2(plan, wide, 9, two=1, lay=3) == P(9, 0, 3152, 1, 3, 0)
    assert _x2(plan, wide, 9, lay=3) == P(9, 0, 3152, 0, 3, 1)
    # 32-bit offsets: a split segment may span the whole range, so from (planes + 4) * H * W >= 0x3fffffff chunks of 64 planes instead
    limit = (1, 16, 8192, 8192)
    assert _x2(plan, limit, 11) == P(0, 1, 4096, 0, 0, 0)
    assert _x2(plan, limit, 12) == P(64, 0, 280576, 0, 0, 0)
    assert _x2(plan, limit, 12, two=1) == P(64, 0, 280576, 1, 0, 0)


def test_mirror_ok(plan):
    """true and false on either side of each condition: not from zero, lay 0 or 3, at least one plane, one resident set for all ranges, 32-bit
    offsets"""
    ok = lambda *a, **k: _x2(plan, *a, **k)["mirror_ok"]   # noqa: E731
    small = (1, 12, 24, 66)
    assert [ok(small, 4, lay=lay) for lay in (0, 1, 2, 3)] == [1, 0, 0, 1]
    assert [ok(small, 4, from_zero=fz, lay=0) for fz in (0, 1)] == [1, 0]
    assert [ok(small, n) for n in (0, 1)] == [0, 1]
    assert [ok((1, 8, 512, 960), 4, two=two) for two in (0, 1)] == [1, 1]           # 2048 tiles: twice is the 4096 slots
    assert [ok((1, 8, 513, 960), 4, two=two) for two in (0, 1)] == [1, 0]           # 2064 tiles
    assert [ok(s, 9) for s in ((1, 40, 960, 1020), (1, 40, 964, 1020))] == [1, 0]   # 4080 and 4097 tiles
    assert [ok((1, 1100, 960, 1020), n) for n in (1092, 1093)] == [1, 0]            # 1096 * 979200 < 0x3fffffff <= 1097 * 979200
