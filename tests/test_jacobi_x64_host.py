"""The rule that picks the tiling of a 3D two-sweep Jacobi launch and the plan of the 64-column tiling (csrc/fnx_jacobi_plan.h:
jacobi3d_x64_ok, jacobi3d_x64_pick, jacobi3d_x64_plan), called from a host-only program with 256 compute units (4096 wave slots).
No GPU."""
import ctypes
import subprocess

import pytest

from fluidnet_cxx_amd import build

PROGRAM = r'''
struct GridDims { int B, D, H, W, HW, DHW; };
#include "fnx_jacobi_plan.h"
using namespace fnx;
static GridDims dims(const int* s) { return GridDims{s[0], s[1], s[2], s[3], s[2] * s[3], s[1] * s[2] * s[3]}; }
extern "C" int pick(const int* s, int np, int two, int mirror, int request, int cus) {
  return jacobi3d_x64_pick(dims(s), np, two != 0, mirror != 0, request, cus);
}
extern "C" int ok(const int* s, int np, int two, int mirror, int cus) { return jacobi3d_x64_ok(dims(s), np, two != 0, mirror != 0, cus); }
extern "C" void plan64(const int* s, int np, int from_zero, int lay, int cus, long* out) {
  const Jacobi3dX64Plan p = jacobi3d_x64_plan(dims(s), np, from_zero != 0, lay, cus);
  out[0] = p.nw; out[1] = p.zchunk; out[2] = (long)p.G; out[3] = p.lay; out[4] = jacobi3d_x64_slots(p.nw, cus);
}
extern "C" void plan60(const int* s, int np, int cus, long* out) {
  const Jacobi3dX2Plan p = jacobi3d_x2_plan(dims(s), np, false, false, 3, cus);
  out[0] = jacobi3d_tiles(dims(s)).nxt; out[1] = p.zchunk; out[2] = (long)p.G; out[3] = p.split;
}
extern "C" int margin() { return X64_MARGIN_PCT; }
extern "C" int minchunk() { return X64_MIN_CHUNK; }
extern "C" int maxw() { return X64_MAXW; }
'''
CUS = 256
AUTO, X60, X64 = 0, 1, 2
ci = ctypes.c_int


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("jacobi_x64_plan")
    cpp, so = str(d / "plan.cpp"), str(d / "libplan.so")
    open(cpp, "w").write(PROGRAM)
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-fPIC", "-shared", "-I", build.CSRC, cpp, "-o", so],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    return ctypes.CDLL(so)


def _s(shape):
    return (ci * 4)(*shape)


def _pick(plan, shape, request=AUTO, np_=None, two=0, mirror=0):
    return plan.pick(_s(shape), shape[1] if np_ is None else np_, two, mirror, request, CUS)


def _plan64(plan, shape, from_zero=0, lay=3):
    out = (ctypes.c_long * 5)()
    plan.plan64(_s(shape), shape[1], from_zero, lay, CUS, out)
    return dict(nw=out[0], zchunk=out[1], G=out[2], lay=out[3], slots=out[4])


def _steps(plan, shape):
    """(wave-steps of the 60-column launch, of the 64-column launch): waves x (chunk + 2 lead-in steps)"""
    B, D, H, W = shape
    out = (ctypes.c_long * 4)()
    plan.plan60(_s(shape), D, CUS, out)
    w60 = out[0] * (H // 4) * B * -(-D // out[1]) * (out[1] + 2)
    p = _plan64(plan, shape)
    return w60, (H // 4) * B * -(-D // p["zchunk"]) * p["nw"] * (p["zchunk"] + 2)


# 256 planes of 256 (257) rows.  W: (60-column tiles, 64-column waves, chosen): chosen where the launch issues at least 19 % fewer
# wave-steps in chunks of at least 8 planes.  60, 67, 130, 300: as many waves a row either way.  64: half the waves, but 4096
# one-wave workgroups march 4 planes each.  128: 4096 x 10 against 3840 x 15 wave-steps.  256: 4096 x 18 against 3840 x 24, 20 %.
# 512: 4096 x 34 against 4032 x 39, 11 %.  1024: 16 waves a row do not fit a workgroup.
TABLE = {60: (1, 1, 0), 64: (2, 1, 0), 67: (2, 2, 0), 128: (3, 2, 1), 130: (3, 3, 0), 256: (5, 4, 1), 300: (5, 5, 0), 512: (9, 8, 0),
         1024: (18, 16, 0)}


def test_truth_table(plan):
    assert plan.margin() == 19 and plan.minchunk() == 8 and plan.maxw() == 8
    for W, (n60, n64, chosen) in TABLE.items():
        for H in (256, 257):
            shape = (1, 256, H, W)
            out = (ctypes.c_long * 4)()
            plan.plan60(_s(shape), 256, CUS, out)
            assert out[0] == n60 and (W + 63) // 64 == n64
            quad = H % 4 == 0
            assert _pick(plan, shape) == (chosen if quad else 0), (W, H)
            # forced: 60 never; 64 wherever the kernel can run (H % 4 == 0, at most 8 waves a row)
            assert _pick(plan, shape, X60) == 0
            assert _pick(plan, shape, X64) == (1 if quad and n64 <= 8 else 0), (W, H)
            assert plan.ok(_s(shape), 256, 0, 0, CUS) == (1 if quad and n64 <= 8 else 0)
    assert _steps(plan, (1, 256, 256, 128)) == (3840 * 15, 4096 * 10) and _steps(plan, (1, 256, 256, 256)) == (3840 * 24, 4096 * 18)
    assert _steps(plan, (1, 256, 256, 512)) == (4032 * 39, 4096 * 34)
    # the measured shapes (docs/history/r34_jacobi_x64.md): taken 256^3, 256 x 256 x 128, 512 x 128 x 128; left 128^3 (chunks of 2),
    # 64 x 512 x 512 (11 %), 128 x 128 x 256 (13 %), 64 x 64 x 256 (chunks of 2), 128 x 256 x 256 and 256 x 128 x 256 (18 %)
    taken = {(256, 256, 256): 1, (256, 256, 128): 1, (512, 128, 128): 1, (128, 128, 128): 0, (64, 512, 512): 0, (128, 128, 256): 0,
             (64, 64, 256): 0, (128, 256, 256): 0, (256, 128, 256): 0}
    assert {k: _pick(plan, (1,) + k) for k in taken} == taken


@pytest.mark.parametrize("shape", [(1, 256, 256, 256), (1, 64, 512, 512), (1, 128, 128, 128), (1, 192, 192, 192), (2, 24, 12, 192), (2, 3, 8, 67)])
def test_chunks_and_grid_fit_the_resident_set(plan, shape):
    B, D, H, W = shape
    p = _plan64(plan, shape)
    groups = B * H // 4
    assert p["nw"] == (W + 63) // 64 and p["slots"] == 256 * (16 // p["nw"])      # whole workgroups: 5 of three waves a compute unit
    nchunks = -(-D // p["zchunk"])
    assert p["zchunk"] >= 2 and groups * nchunks <= p["slots"]                    # every (row group, chunk) workgroup is resident
    assert p["G"] % 8 == 0 and groups * nchunks <= p["G"] < groups * nchunks + 8  # padded to the 8 XCDs
    if shape == (1, 256, 256, 256):       # 64 row groups x 4 waves: 16 chunks of 16 planes (60 columns: 320 tiles, 12 chunks of 22)
        assert (p["nw"], p["zchunk"], p["G"]) == (4, 16, 1024)
        out = (ctypes.c_long * 4)()
        plan.plan60(_s(shape), D, CUS, out)
        assert (out[0], out[1], out[2], out[3]) == (5, 22, 3840, 0)
    if shape == (1, 64, 512, 512):
        assert (p["nw"], p["zchunk"], p["G"]) == (8, 16, 512)
    if shape == (1, 192, 192, 192):       # 48 row groups, 1280 workgroups of three waves resident: 26 chunks -> 8 planes, 24 chunks
        assert (p["nw"], p["zchunk"], p["G"]) == (3, 8, 1152)
    # a pass from zero reads no input layout
    assert _plan64(plan, shape, from_zero=1, lay=3)["lay"] == 2 and _plan64(plan, shape, lay=1)["lay"] == 1


def test_refused_cases_keep_the_60_column_kernel(plan):
    shape = (1, 256, 256, 256)
    for request in (AUTO, X64):
        assert _pick(plan, shape, request) == 1
        assert _pick(plan, shape, request, two=1) == 0                    # two plane ranges in a launch
        assert _pick(plan, shape, request, mirror=1) == 0                 # MIR: the mirrored stores of the z-slab driver
        assert _pick(plan, shape, request, np_=100) == 0                  # a plane range
        assert _pick(plan, (1, 256, 254, 256), request) == 0              # H % 4 != 0: no row quads
        # SPLIT territory: more waves than one resident set holds (513 row groups x 8 waves > 4096)
        assert _pick(plan, (1, 8, 2052, 512), request) == 0 and _pick(plan, (1, 8, 2048, 512), X64) == 1
        assert _pick(plan, (1, 8, 64, 576), request) == 0                 # 9 waves a row
