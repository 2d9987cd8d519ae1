"""The kernel source of fnx_render.hip, compiled for the HOST and run with emulated threads, against the numpy model -- without a GPU.

The unit's kernels are plain C++ apart from the HIP keywords, so this test takes the text of the unit from its anonymous namespace on,
defines the keywords away (`__shared__` becomes `static`: workgroups run one after the other), turns each `<<<grid, block>>>` launch into
a loop over workgroups whose threads are std::threads meeting at a std::barrier for `__syncthreads()`, and compiles it with g++ and
`-ffp-contract=off`.  What runs is the indexing, the tile hand-over, the border rule and the arithmetic of the device code; what it
cannot show is the device compiler's code or the hardware.  The result must be the model's, bit for bit; the image and the light
workspace start as NaN, so a value that is never written shows."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import render_reference as rr
from fluidnet_cxx_amd import build

f32 = np.float32
PRELUDE = r'''
#include <barrier>
#include <thread>
#include <vector>
#include <cstdio>
#include <cstddef>
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
thread_local dim3 threadIdx, blockIdx;
static std::barrier<>* g_bar;
#define __syncthreads() g_bar->arrive_and_wait()
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
#define __shared__ static
#define FNX_OBST 2.0f
typedef int hipStream_t;
struct GridDims { int B, D, H, W, HW, DHW; };
namespace fnx { struct RenderConsts { float k_view, k_light, ambient, one_minus_ambient, albedo_smoke, albedo_obstacle; int bnd; }; }
template <class F> void launch_emu(dim3 grid, int nthreads, F fn) {
  for (unsigned by = 0; by < grid.y; ++by) for (unsigned bx = 0; bx < grid.x; ++bx) {
    if (nthreads == 256) {   // no barriers in that kernel: threads one after the other
      for (int t = 0; t < nthreads; ++t) { threadIdx = dim3(t); blockIdx = dim3(bx, by); fn(); }
    } else {
      std::barrier<> bar(nthreads); g_bar = &bar;
      std::vector<std::thread> th;
      for (int t = 0; t < nthreads; ++t) th.emplace_back([&, t] { threadIdx = dim3(t); blockIdx = dim3(bx, by); fn(); });
      for (auto& x : th) x.join();
    }
  }
}
'''
ENTRY = r'''extern "C" void emu_render(int B, int D, int H, int W, int view, int light, float kv, float kl, float amb, float oma, float as, float ao, int bnd,
                           const float* density, const float* flags, float* Lws, float* image) {
  GridDims g{B, D, H, W, H * W, D * H * W};
  fnx::RenderConsts c{kv, kl, amb, oma, as, ao, bnd};
  fnx::launch_render_volume(g, view, light, c, density, flags, Lws, image, 0);
}
'''


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    src = open(os.path.join(build.CSRC, "fnx_render.hip")).read()
    body = src[src.index("namespace {"):]
    body, n = re.subn(r"(\w+<MODE>)<<<(\w+), (\w+), 0, s>>>\((.*)\);", r"launch_emu(\2, \3, [&] { \1(\4); });", body)
    assert n == 3, "the three launches of launch_pass"
    d = tmp_path_factory.mktemp("render_emu")
    cpp, so = str(d / "emu.cpp"), str(d / "libemu.so")
    open(cpp, "w").write(PRELUDE + body + ENTRY)
    p = subprocess.run(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", cpp, "-o", so],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    lib = ctypes.CDLL(so)
    fp = ctypes.POINTER(ctypes.c_float)
    lib.emu_render.argtypes = [ctypes.c_int] * 6 + [ctypes.c_float] * 6 + [ctypes.c_int] + [fp] * 4

    def render(d, f, view, light, kv, kl, bnd=1, ambient=0.25, albedo_smoke=1.0, albedo_obstacle=0.5):
        B, D, H, W = d.shape
        img = np.full((B, 2) + rr.image_shape(d.shape, view), np.nan, f32)
        L = np.full(d.shape, np.nan, f32)
        d2, f2 = d.copy(), f.copy()
        ptr = lambda a: a.ctypes.data_as(fp)                        # noqa: E731
        lib.emu_render(B, D, H, W, rr.DIRECTIONS.index(view), rr.DIRECTIONS.index(light), kv, kl, ambient, f32(1) - f32(ambient),
                       albedo_smoke, albedo_obstacle, bnd, ptr(d2), ptr(f2), ptr(L), ptr(img))
        assert np.array_equal(d2, d) and np.array_equal(f2, f), "an input was written"
        return img
    return render


def _case(shape, seed=0):
    rng = np.random.default_rng(seed)
    d = rng.uniform(-0.2, 1.3, shape).astype(f32)
    d[rng.random(shape) < 0.5] = 0
    f = np.ones(shape, f32)
    f[:, :, 0] = f[:, :, -1] = f[:, :, :, 0] = f[:, :, :, -1] = rr.TYPE_OBSTACLE
    if shape[1] > 1:
        f[:, 0] = f[:, -1] = rr.TYPE_OBSTACLE
    f[rng.random(shape) < 0.03] = rr.TYPE_OBSTACLE
    return d, f


PAIRS8 = (("+x", "-y"), ("-x", "+z"), ("+y", "-x"), ("-y", "+z"), ("+z", "+x"), ("-z", "-y"), ("-x", "-x"), ("+y", "-y"))


# partial and several 64-wide tiles along x, partial row blocks, more than one batch of 16 cells along y and z, and the 2D grid
@pytest.mark.parametrize("shape,pairs", [((2, 5, 7, 9), tuple(itertools.product(rr.DIRECTIONS, rr.DIRECTIONS))),
                                         ((1, 18, 35, 70), PAIRS8 + (("+y", "+y"), ("-z", "-z"))), ((2, 1, 37, 53), PAIRS8)],
                         ids=["2x5x7x9-all36", "18x35x70", "2d-2x37x53"])
def test_host_build_of_the_kernels_gives_the_models_bits(emu, shape, pairs):
    d, f = _case(shape)
    for (view, light), (kv, kl) in itertools.product(pairs, ((1.5, 2.5), (0.04, 0.03))):      # saturating and thin smoke
        for bnd in ((1, 0, 2) if (view, light) in PAIRS8[:3] else (1,)):
            got = emu(d, f, view, light, kv, kl, bnd=bnd)
            want = rr.render(d, f, view, light, k_view=kv, k_light=kl, bnd=bnd)
            bad = got.view(np.uint32) != want.view(np.uint32)
            assert not bad.any(), (shape, view, light, kv, kl, bnd, int(bad.sum()), tuple(np.argwhere(bad)[0]))
