"""The 3D stage word (csrc/fnx_stage_word.h) without a GPU: the header of pure functions that stage_word_kernel, stage3d_kernel<.., WORD>
and post_projection_kernel<true, false, WORD> share, compiled into a host-only library.  A model written here -- the float kernels'
neighbour convention and their float comparisons -- says what every predicate the kernels take from a word must be; the header's
encode / decode are checked against it.  Then when the step uses the word (stage_word_plan of fnx_step_plan.h) and what the workspace
that has room for it takes (fnx_workspace_bytes FNX_OP_STEP_STATIC)."""
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
vp, ci, cu, cf, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_float, ctypes.c_size_t
Prm, _ = _structs()

PROGRAM = r'''
#include "fnx_stage_word.h"
#include "fnx_step_plan.h"
using namespace fnx;
extern "C" unsigned word_at(const float* flags, const unsigned char* cls, int W, int H, int D, int i, int j, int k) {
  return stage_word_at(flags, cls, W, H, D, i, j, k);
}
// out: per flag (cell, -x, -y, -z, +x, +y, +z) the three predicates on its code: 21 ints; then class, ident without / with the +1 side
extern "C" void decode(unsigned w, int* out) {
  unsigned c[7] = {stage_word_cell(w)};
  for (int a = 0; a < 3; ++a) { c[1 + a] = stage_word_minus(w, a); c[4 + a] = stage_word_plus(w, a); }
  using K = FlagConst<unsigned>;
  for (int q = 0; q < 7; ++q) { out[3 * q] = c[q] == K::fluid; out[3 * q + 1] = c[q] == K::obst; out[3 * q + 2] = c[q] == K::empty; }
  out[21] = (int)stage_word_class(w); out[22] = stage_word_ident(w, false); out[23] = stage_word_ident(w, true);
}
extern "C" void float_predicates(float f, int* out) {
  using K = FlagConst<float>;
  out[0] = f == K::fluid; out[1] = f == K::obst; out[2] = f == K::empty;
}
extern "C" unsigned flag_code(float f) { return stage_flag_code(f); }
// 0 none, 1 build, 2 reuse; spare: the bytes the workspace has beyond the step's layout
extern "C" int word_plan(const FnxStepParams* prm, int is3d, int has_bc, size_t cells, size_t layout_bytes, size_t ws_bytes) {
  StepLayout L{};
  L.bytes = layout_bytes;
  return (int)stage_word_plan(prm, is3d != 0, step_plan(prm, true, false, has_bc != 0).class_map, L, cells, ws_bytes);
}
extern "C" size_t word_offset(size_t layout_bytes) { StepLayout L{}; L.bytes = layout_bytes; return stage_word_offset(L); }
'''

FLAG_VALUES = np.array([1.0, 2.0, 4.0, 0.0, 8.0, 3.5, np.nan, -1.0, 3.0], np.float32)   # the issue's six, and NaN, -1, 3 (a code, not a flag)


@pytest.fixture(scope="module")
def word(tmp_path_factory):
    d = tmp_path_factory.mktemp("stage_word")
    cpp, so = str(d / "word.cpp"), str(d / "libword.so")
    open(cpp, "w").write(PROGRAM)
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-I", build.CSRC, cpp, "-o", so],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    lib = ctypes.CDLL(so)
    lib.word_at.restype = lib.flag_code.restype = cu
    lib.word_at.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci]
    lib.decode.argtypes = [cu, vp]
    lib.float_predicates.argtypes = [cf, vp]
    lib.flag_code.argtypes = [cf]
    lib.word_plan.argtypes = [ctypes.POINTER(Prm), ci, ci, sz, sz, sz]
    lib.word_offset.restype, lib.word_offset.argtypes = sz, [sz]
    return lib


def _preds(f):
    """what the float kernels compute of a flag value"""
    return [int(f == np.float32(1.0)), int(f == np.float32(2.0)), int(f == np.float32(4.0))]


def test_flag_codes_and_predicates(word):
    """1 / 2 / 4 get their codes, everything else 0; the predicates on the value are the float comparisons, those on the code agree"""
    out = (ci * 3)()
    for f in FLAG_VALUES.tolist() + [-0.0, 1.0000001, float("inf"), 2.5, 16.0, 128.0]:
        code = word.flag_code(f)
        assert code == {1.0: 1, 2.0: 2, 4.0: 3}.get(f, 0), f
        word.float_predicates(f, out)
        assert list(out) == _preds(np.float32(f)), f
        assert [int(code == c) for c in (1, 2, 3)] == _preds(np.float32(f)), f


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_every_cell_of_a_small_grid(word, seed):
    """W x H x D = 5 x 4 x 3 (and the axes swapped round), every cell -- all faces, edges and corners, so each of the six missing
    neighbours occurs with each other -- with random flag values and class bytes: decode(word) gives, for the cell and its six
    neighbours under the float kernels' convention, the three flag predicates, the cell's class and `ident` with and without the +1 side"""
    rng = np.random.default_rng(seed)
    out = (ci * 24)()
    for W, H, D in ((5, 4, 3), (3, 5, 4), (4, 3, 5)):
        flags = rng.choice(FLAG_VALUES, size=(D, H, W)).astype(np.float32)
        cls = rng.choice(np.array([0, 1, 2, 3, 3, 3], np.uint8), size=(D, H, W))
        seen_ident = set()
        for k, j, i in itertools.product(range(D), range(H), range(W)):
            w = word.word_at(flags.ctypes.data, cls.ctypes.data, W, H, D, i, j, k)
            assert w < (1 << 22)
            # the float kernels: off[a] = 0 where the -1 neighbour does not exist (the cell itself); a missing +1 neighbour is never
            # used, and is loaded from the cell itself as well
            minus = [(k, j, i - 1 if i > 0 else i), (k, j - 1 if j > 0 else j, i), (k - 1 if k > 0 else k, j, i)]
            plus = [(k, j, i + 1 if i + 1 < W else i), (k, j + 1 if j + 1 < H else j, i), (k + 1 if k + 1 < D else k, j, i)]
            want = _preds(flags[k, j, i])
            for q in minus + plus:
                want += _preds(flags[q])
            mine = cls[k, j, i] == 3 and all(cls[q] & 2 for q in minus)
            want += [int(cls[k, j, i]), int(mine), int(mine and all(cls[q] == 3 for q in plus))]
            word.decode(w, out)
            assert list(out) == want, (W, H, D, i, j, k, hex(w))
            seen_ident.add((want[22], want[23]))
        assert seen_ident == {(0, 0), (1, 0), (1, 1)}       # the class bytes make all three outcomes


def test_class_bits_do_not_leak(word):
    """each input moves its own bits only: one flag or one class byte changed at a time on an interior cell"""
    W, H, D = 3, 3, 3
    flags = np.full((D, H, W), 1.0, np.float32)
    cls = np.full((D, H, W), 3, np.uint8)
    base = word.word_at(flags.ctypes.data, cls.ctypes.data, W, H, D, 1, 1, 1)
    assert base == 0b111_111_11_010101_010101_01
    cells = [(1, 1, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 2), (1, 2, 1), (2, 1, 1)]      # (k, j, i): cell, -x -y -z, +x +y +z
    for n, q in enumerate(cells):
        f = flags.copy(); f[q] = 4.0
        assert word.word_at(f.ctypes.data, cls.ctypes.data, W, H, D, 1, 1, 1) ^ base == (0b01 ^ 0b11) << (2 * n)
        for c, bits in ((2, (0b01 << 14, 0, 1)), (1, (0b10 << 14, 1, 1)), (0, (0b11 << 14, 1, 1))):
            cc = cls.copy(); cc[q] = c
            delta = bits[0] if n == 0 else (bits[1] << (16 + n - 1) if n < 4 else bits[2] << (19 + n - 4))
            assert word.word_at(flags.ctypes.data, cc.ctypes.data, W, H, D, 1, 1, 1) ^ base == delta, (q, c)


def test_stage_word_plan(word):
    """3D only, with the class map only, and with room behind the layout only; rebuilt unless bits 0 and 2 are both promised"""
    cells, layout = 11880, 12868352 + 3           # (an unaligned layout size: the map starts on the next 256 bytes)
    at = word.word_offset(layout)
    assert at == 12868608 and word.word_offset(at) == at
    enough = at + 4 * cells
    for static_flags, is3d, has_bc, ws_bytes in itertools.product(range(16), (0, 1), (0, 1), (layout, enough - 1, enough, enough + 999)):
        prm = Prm(static_flags=static_flags)
        got = word.word_plan(ctypes.byref(prm), is3d, has_bc, cells, layout, ws_bytes)
        uses = is3d and has_bc and (static_flags & 2) and ws_bytes >= enough
        want = 0 if not uses else (2 if (static_flags & 5) == 5 else 1)
        assert got == want, (static_flags, is3d, has_bc, ws_bytes)
    # the issue's stale case by name: the BC promise and the built map (6) without the flags promise builds the word again
    assert word.word_plan(ctypes.byref(Prm(static_flags=6)), 1, 1, cells, layout, enough) == 1
    assert word.word_plan(ctypes.byref(Prm(static_flags=7)), 1, 1, cells, layout, enough) == 2
    assert word.word_plan(ctypes.byref(Prm(static_flags=3)), 1, 1, cells, layout, enough) == 1


def test_workspace_with_the_word_map():
    """FNX_OP_STEP_STATIC = FNX_OP_STEP rounded up to 256 bytes + 4 bytes per cell (rounded up) in 3D, FNX_OP_STEP itself in 2D; a window or a
    z-slab view changes neither"""
    build.build_all()
    lib = ctypes.CDLL(build.LIB)
    lib.fnx_workspace_bytes.restype = sz
    lib.fnx_workspace_bytes.argtypes = [ctypes.POINTER(_FnxGrid), ci]
    hdr = open(os.path.join(REPO, "include", "fluidnet_hip.h")).read()
    op_step, op_static = (int(re.search(n + r" = (\d+)", hdr).group(1)) for n in ("FNX_OP_STEP", "FNX_OP_STEP_STATIC"))

    def al(n):
        return (n + 255) // 256 * 256

    for B, D, H, W in ((2, 1, 40, 70), (1, 1, 3, 3), (1, 9, 20, 66), (1, 16, 33, 130), (2, 6, 21, 66), (1, 3, 3, 3)):
        views = [{}] + ([dict(k_begin=1, k_end=2), dict(z_offset=3, D_global=D + 7)] if D > 1 else [])
        for view in views:
            g = _FnxGrid(B=B, D=D, H=H, W=W, is3D=int(D > 1), **view)
            step, static = lib.fnx_workspace_bytes(ctypes.byref(g), op_step), lib.fnx_workspace_bytes(ctypes.byref(g), op_static)
            assert step > 0 and static == (al(step) + al(4 * B * D * H * W) if D > 1 else step), (B, D, H, W, view)
