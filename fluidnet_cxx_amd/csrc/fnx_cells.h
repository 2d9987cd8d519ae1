// The one-thread-per-cell launch idiom of the plane-parallel kernels (fnx_advect.hip, fnx_scalars.hip, fnx_stencils.hip, fnx_step.hip),
// and the dispatch of run-time choices to template arguments that their launchers share.
#pragma once
#include <hip/hip_runtime.h>
#include "fnx_device.h"

// 64x4 blocks, x fastest: a wave reads / writes 256 contiguous bytes per field row.  blockIdx.z walks the B * KN plane slices of the
// compute window (the whole domain is the window K0 = 0, KN = D, make_dims).
constexpr int BX = 64, BY = 4;

struct CellId { int b, k, j, i; bool valid; };

template <bool IS3D>
__device__ __forceinline__ CellId cell_id(const GridDims& g) {
  CellId c;
  c.i = blockIdx.x * BX + threadIdx.x;
  c.j = blockIdx.y * BY + threadIdx.y;
  const int bk = blockIdx.z;
  c.b = IS3D ? bk / g.KN : bk;
  c.k = IS3D ? g.K0 + (bk - c.b * g.KN) : 0;
  c.valid = (c.i < g.W) & (c.j < g.H);
  return c;
}

inline dim3 cell_grid(const GridDims& g) { return dim3((g.W + BX - 1) / BX, (g.H + BY - 1) / BY, g.B * g.KN); }

// run-time choices -> template arguments: `k` is a generic lambda that receives the choice as an IC<> constant
template <int V> struct IC { static constexpr int value = V; };
template <class K> void with_flag(bool b, K k) { if (b) k(IC<1>{}); else k(IC<0>{}); }
// k(IS3D, QUIRKS, SAMPLE_OUTSIDE) of an advection.  Quirks mode exists in 3D only: <2D, quirks> is never instantiated.
template <class K> void with_semantics(bool is3d, bool quirks, bool sample_outside, K k) {
  with_flag(is3d, [&](auto is3d_) {
    with_flag(is3d && quirks, [&](auto quirks_) {
      if constexpr (decltype(is3d_)::value || !decltype(quirks_)::value)
        with_flag(sample_outside, [&](auto outside_) { k(is3d_, quirks_, outside_); });
    });
  });
}
