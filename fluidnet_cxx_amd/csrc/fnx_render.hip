// Volume rendering for gfx950: a density grid with its obstacles -> an image.  Axis-aligned, orthographic, single scattering with
// self-shadowing from an axis-aligned light.  tests/render_reference.py is the same statement in numpy; the kernels give its bits.
//
// Per cell (fp32 add/sub/mul/compare only, no contraction, these parentheses):
//   rho = min(max(density, 0), 1);  obs = flags == TypeObstacle;  within bnd cells of a domain face: not an obstacle, rho = 0
//   (a 2D grid has no z faces)
//   light pass, along the light's travel:  L[cell] = Lin (1 before the first cell);  then Lin = obs ? 0 : Lin * (1 - min(k_light rho, 1))
//   view pass, along the view's travel, T = 1, C = 0:  s = ambient + one_minus_ambient * L[cell]
//     obs:   C = C + T * (albedo_obstacle * s);  T = 0
//     else:  a = min(k_view rho, 1);  C = C + (T * a) * (albedo_smoke * s);  T = T * (1 - a)
//   image channel 0 = C, channel 1 = T
//
// Both passes are marches of one column per thread with the running values (Lin; T, C) in registers, so a column's arithmetic is
// serial and in cell order whatever the axis -- which is what makes the result independent of the axis, bit for bit.
//   march along y or z (render_march_kernel): threads over the flattened (outer, x) columns, lanes over x.  Every step of a wave reads
//     64 consecutive floats of rho, flags (and L), and writes 64 consecutive floats of L; the image rows are the columns.
//   march along x (render_march_x_kernel): the march axis is the contiguous one, so a thread per row would stride by W.  One wave owns
//     64 rows ((z, y) flattened) and walks x in tiles of 64: it loads the tile with lanes over x (one 256-byte run per row) into LDS
//     as one value per cell (-1 for an obstacle, else rho), marches it with lanes over the rows reading LDS[row][x] -- rows are 65
//     floats apart, an odd stride, so the 32 lanes of a ds_read_b32 group fall on 32 different banks -- and carries Lin / T / C to the
//     next tile in registers.  The light pass puts L back into the tile in place and stores it with lanes over x again; the image
//     of an x view is indexed by the row, so its stores are consecutive over the lanes as they are.
// Three modes each: LIGHT (writes L), VIEW (reads L, writes the image) and HEAD (view == light: Lin rides along in a register, no L
// in memory).  16.6 KiB of LDS per array and tile (two arrays in VIEW), no atomics, no scratch; density and flags are only read.
#include "fnx_device.h"
#include "fnx_kernels.h"

namespace {

enum { MODE_LIGHT = 0, MODE_VIEW = 1, MODE_HEAD = 2 };

constexpr int XT = 64;   // x per tile of the x march
constexpr int XR = 64;   // rows per tile = threads per block: one wave
constexpr int MB = 256;  // threads per block of the y / z march
constexpr int NB = 16;   // cells whose loads are in flight together (y / z march: per thread; x march: rows per lane)

using fnx::RenderConsts;

// one value per cell: -1 marks an obstacle, anything else is the clamped density
__device__ __forceinline__ float cell_value(float d, float f) {
  float r = d < 0.f ? 0.f : d;
  r = r > 1.f ? 1.f : r;
  return f == FNX_OBST ? -1.f : r;
}

__device__ __forceinline__ float sat_mul(float k, float rho) {
  const float a = k * rho;
  return a > 1.f ? 1.f : a;
}

__device__ __forceinline__ void light_after(const RenderConsts& c, float e, float& Lin) {
  if (e < 0.f) Lin = 0.f;
  else Lin = Lin * (1.f - sat_mul(c.k_light, e));
}

__device__ __forceinline__ void view_cell(const RenderConsts& c, float e, float Lc, float& T, float& C) {
  const float s = c.ambient + c.one_minus_ambient * Lc;
  if (e < 0.f) {
    C = C + T * (c.albedo_obstacle * s);
    T = 0.f;
  } else {
    const float a = sat_mul(c.k_view, e);
    C = C + (T * a) * (c.albedo_smoke * s);
    T = T * (1.f - a);
  }
}

// March along y or z.  Column c of sample blockIdx.y: q = c / W, x = c % W, first cell q * qstride + x, cells `stride` apart, n of them.
// bq / bm: the border width on the q axis and on the march axis (0 where that axis is the z axis of a 2D grid); c.bnd is that of x.
template <int MODE>
__global__ __launch_bounds__(MB) void render_march_kernel(int ncol, int W, int Q, int qstride, int stride, int n, int DHW, bool neg, int bq,
                                                         int bm, RenderConsts c, const float* __restrict__ density,
                                                         const float* __restrict__ flags, float* __restrict__ Lws, float* __restrict__ image) {
  const int col = (int)blockIdx.x * MB + (int)threadIdx.x;
  if (col >= ncol) return;
  const int b = (int)blockIdx.y;
  const int q = col / W, x = col - q * W;
  const bool colborder = x < c.bnd || x >= W - c.bnd || q < bq || q >= Q - bq;
  const size_t sample = (size_t)b * DHW;
  const float* rp = density + sample + (size_t)q * qstride + x;
  const float* fp = flags + sample + (size_t)q * qstride + x;
  float* lp = MODE == MODE_HEAD ? nullptr : Lws + sample + (size_t)q * qstride + x;
  float Lin = 1.f, T = 1.f, C = 0.f;
  auto cell = [&](int k, float d, float f, float Lc) {
    float e = cell_value(d, f);
    if (colborder || k < bm || k >= n - bm) e = 0.f;
    if (MODE == MODE_LIGHT) { lp[(size_t)k * stride] = Lin; light_after(c, e, Lin); }
    if (MODE == MODE_VIEW) view_cell(c, e, Lc, T, C);
    if (MODE == MODE_HEAD) { view_cell(c, e, Lin, T, C); light_after(c, e, Lin); }
  };
  // the loads of NB cells are issued together, ahead of the serial chain that consumes them: a column's march is one thread, so the
  // bytes in flight per wave are what hides the memory latency
  int s = 0;
  for (; s + NB <= n; s += NB) {
    float d[NB], f[NB], l[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const size_t o = (size_t)(neg ? n - 1 - (s + u) : s + u) * stride;
      d[u] = rp[o]; f[u] = fp[o];
      l[u] = MODE == MODE_VIEW ? lp[o] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) cell(neg ? n - 1 - (s + u) : s + u, d[u], f[u], l[u]);
  }
  for (; s < n; ++s) {
    const int k = neg ? n - 1 - s : s;
    const size_t o = (size_t)k * stride;
    cell(k, rp[o], fp[o], MODE == MODE_VIEW ? lp[o] : 0.f);
  }
  if (MODE != MODE_LIGHT) {
    float* ip = image + (size_t)b * 2 * ncol;
    ip[col] = C;
    ip[ncol + col] = T;
  }
}

// March along x.  Block blockIdx.x owns rows [r0, r0 + XR) of the D*H rows of sample blockIdx.y.  by / bz: the border width on y and z.
template <int MODE>
__global__ __launch_bounds__(XR) void render_march_x_kernel(int nrows, int H, int W, int D, bool neg, int by, int bz, RenderConsts c,
                                                           const float* __restrict__ density, const float* __restrict__ flags,
                                                           float* __restrict__ Lws, float* __restrict__ image) {
  __shared__ float E[XR][XT + 1];
  __shared__ float LL[MODE == MODE_VIEW ? XR : 1][XT + 1];
  const int lane = (int)threadIdx.x;
  const int b = (int)blockIdx.y;
  const int r0 = (int)blockIdx.x * XR;
  const int nr = nrows - r0 < XR ? nrows - r0 : XR;          // rows of this block (block-uniform)
  const int row = r0 + lane;
  const bool mine = lane < nr;
  const int z = row / H, y = row - z * H;
  const bool rowborder = y < by || y >= H - by || z < bz || z >= D - bz;
  const size_t sample = (size_t)b * nrows * W;
  const float* rp = density + sample + (size_t)r0 * W;
  const float* fp = flags + sample + (size_t)r0 * W;
  float* lp = MODE == MODE_HEAD ? nullptr : Lws + sample + (size_t)r0 * W;
  const int ntile = (W + XT - 1) / XT;
  float Lin = 1.f, T = 1.f, C = 0.f;
  for (int tt = 0; tt < ntile; ++tt) {
    const int x0 = (neg ? ntile - 1 - tt : tt) * XT;
    const int xw = W - x0 < XT ? W - x0 : XT;                // cells of this tile along x (block-uniform)
    // the tile, lanes over x
    if (lane < xw) {
      int i = 0;
      for (; i + NB <= nr; i += NB) {
        float d[NB], f[NB], l[NB];
#pragma unroll
        for (int u = 0; u < NB; ++u) {
          const size_t o = (size_t)(i + u) * W + x0 + lane;
          d[u] = rp[o]; f[u] = fp[o];
          l[u] = MODE == MODE_VIEW ? lp[o] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < NB; ++u) {
          E[i + u][lane] = cell_value(d[u], f[u]);
          if (MODE == MODE_VIEW) LL[i + u][lane] = l[u];
        }
      }
      for (; i < nr; ++i) {
        const size_t o = (size_t)i * W + x0 + lane;
        E[i][lane] = cell_value(rp[o], fp[o]);
        if (MODE == MODE_VIEW) LL[i][lane] = lp[o];
      }
    }
    __syncthreads();
    // the march, lanes over the rows
    if (mine) {
#pragma unroll 8
      for (int j = 0; j < xw; ++j) {
        const int jj = neg ? xw - 1 - j : j;
        const int x = x0 + jj;
        float e = E[lane][jj];
        if (rowborder || x < c.bnd || x >= W - c.bnd) e = 0.f;
        if (MODE == MODE_LIGHT) { E[lane][jj] = Lin; light_after(c, e, Lin); }
        if (MODE == MODE_VIEW) view_cell(c, e, LL[lane][jj], T, C);
        if (MODE == MODE_HEAD) { view_cell(c, e, Lin, T, C); light_after(c, e, Lin); }
      }
    }
    __syncthreads();
    if (MODE == MODE_LIGHT) {
      if (lane < xw) {
#pragma unroll 8
        for (int i = 0; i < nr; ++i) lp[(size_t)i * W + x0 + lane] = E[i][lane];
      }
      __syncthreads();
    }
  }
  if (MODE != MODE_LIGHT && mine) {
    float* ip = image + (size_t)b * 2 * nrows;
    ip[row] = C;
    ip[nrows + row] = T;
  }
}

template <int MODE>
void launch_pass(const GridDims& g, int dir, const RenderConsts& c, const float* density, const float* flags, float* Lws, float* image,
                 hipStream_t s) {
  const int axis = dir >> 1;                 // 0: x, 1: y, 2: z
  const bool neg = dir & 1;
  const int bz = g.D > 1 ? c.bnd : 0;        // a 2D grid has no z faces
  if (axis == 0) {
    const int nrows = g.D * g.H;
    const dim3 grid((nrows + XR - 1) / XR, g.B);
    render_march_x_kernel<MODE><<<grid, XR, 0, s>>>(nrows, g.H, g.W, g.D, neg, c.bnd, bz, c, density, flags, Lws, image);
  } else if (axis == 1) {                    // columns (z, x), cells W apart
    const int ncol = g.D * g.W;
    const dim3 grid((ncol + MB - 1) / MB, g.B);
    render_march_kernel<MODE><<<grid, MB, 0, s>>>(ncol, g.W, g.D, g.HW, g.W, g.H, g.DHW, neg, bz, c.bnd, c, density, flags, Lws, image);
  } else {                                   // columns (y, x), cells HW apart
    const int ncol = g.HW;
    const dim3 grid((ncol + MB - 1) / MB, g.B);
    render_march_kernel<MODE><<<grid, MB, 0, s>>>(ncol, g.W, g.H, g.W, g.HW, g.D, g.DHW, neg, c.bnd, bz, c, density, flags, Lws, image);
  }
}

}  // namespace

namespace fnx {

void launch_render_volume(const GridDims& g, int view_dir, int light_dir, const RenderConsts& c, const float* density, const float* flags,
                          float* Lws, float* image, hipStream_t s) {
  if (view_dir == light_dir) {
    launch_pass<MODE_HEAD>(g, view_dir, c, density, flags, nullptr, image, s);
    return;
  }
  launch_pass<MODE_LIGHT>(g, light_dir, c, density, flags, Lws, nullptr, s);
  launch_pass<MODE_VIEW>(g, view_dir, c, density, flags, Lws, image, s);
}

}  // namespace fnx
