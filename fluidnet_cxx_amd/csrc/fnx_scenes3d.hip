// Training scenes and the training loss in 3D for gfx950 (ABI 26): fnx_scene_obstacles3d, fnx_scene_turbulence3d, fnx_train_loss3d.
//
// The hash is that of the 2D unit (fnx_scene_common.h).  A lattice value at the integer point (lx, ly, lz) of octave o of a noise
// whose stream base is s0 is addressed by
//   key     = scene_key(seed, scene, (lz << 8) | (s0 + o))         the plane goes into the stream word, above its low byte
//   counter = ly * 65536 + lx                                        as in 2D
// which is injective for 0 <= lx, ly < 65536 and 0 <= lz < 2^24: the grids accepted here (every axis <= 32768) stay inside it.
// Stream bases (low byte of the stream word): 80 = the obstacle primitives (counter 16 * primitive + draw: 0 = ball / box, 1..3 = the
// centre's offsets along x, y, z, 4..6 = the radius resp. the half extents along x, y, z; counter 0xffff0000 = their number),
// 96 + o = psi_x, 112 + o = psi_y, 128 + o = psi_z, 144 + o = the density.  The 2D kernels use 0, 16 + o and 32 + o, the samplers 64
// and 65.
//
// Arithmetic of the scene kernels: integer operations, fp32 add / subtract / multiply / compare and int <-> float conversion only,
// compiled without contraction, each expression in the order written here; tests/scene_reference_3d.py is the same statement in numpy
// and the kernels are bit-identical to it.
//
// One thread per cell, the plane from the grid's z (blockIdx.z = b * D + k).  The turbulence thread evaluates its nine potential values
// itself: the kernel runs once per scene next to a converged pressure solve, so nothing is carried between planes.
//
// The loss is fnx_train_loss on (B,1,D,H,W) / (B,3,D,H,W): the divergence of a cell has the bits of divergence_kernel<true>
// (fnx_stencils.hip), the gradient with respect to U is formed per face from the recomputed divergences of the face's two cells.
#include "fnx_scene_common.h"

namespace {

constexpr unsigned STREAM_OBST3 = 80u, STREAM_PSIX = 96u, STREAM_PSIY = 112u, STREAM_PSIZ = 128u, STREAM_RHO3 = 144u,
                   COUNT_CTR3 = 0xffff0000u;

// ---- obstacles ----------------------------------------------------------------------------------------------------------------
struct Prim3 { float cx, cy, cz, a2, b2, c2; int box; };

__global__ __launch_bounds__(BX* BY) void scene_obstacles3d_kernel(GridDims g, FnxSceneParams prm, const int* __restrict__ ids,
                                                                   float* __restrict__ flags) {
  __shared__ Prim3 prims[FNX_SCENE_MAX_PRIMITIVES];
  __shared__ int nprim;
  const int b = blockIdx.z / g.D, k = blockIdx.z - b * g.D, t = threadIdx.y * BX + threadIdx.x;
  const unsigned key = scene_key(prm.seed, (unsigned)ids[b], STREAM_OBST3);
  const int span = prm.n_max - prm.n_min + 1;
  int n = prm.n_min + (int)(uniform01(key, COUNT_CTR3) * (float)span);
  if (n > prm.n_max) n = prm.n_max;
  if (t == 0) nprim = n;
  if (t < n) {
    const int hw = g.H < g.W ? g.H : g.W;
    const float m = (float)(g.D < hw ? g.D : hw);
    const unsigned c = 16u * (unsigned)t;
    Prim3 q;
    q.box = (int)(mix32(key ^ c) >> 31);
    const float ox = prm.centre_min + uniform01(key, c + 1u) * (prm.centre_max - prm.centre_min);
    const float oy = prm.centre_min + uniform01(key, c + 2u) * (prm.centre_max - prm.centre_min);
    const float oz = prm.centre_min + uniform01(key, c + 3u) * (prm.centre_max - prm.centre_min);
    q.cx = 0.5f * (float)(g.W - 1) + ox * m;
    q.cy = 0.5f * (float)(g.H - 1) + oy * m;
    q.cz = 0.5f * (float)(g.D - 1) + oz * m;
    const float ra = (prm.size_min + uniform01(key, c + 4u) * (prm.size_max - prm.size_min)) * m;
    const float rb = (prm.size_min + uniform01(key, c + 5u) * (prm.size_max - prm.size_min)) * m;
    const float rc = (prm.size_min + uniform01(key, c + 6u) * (prm.size_max - prm.size_min)) * m;
    q.a2 = ra * ra; q.b2 = rb * rb; q.c2 = rc * rc;
    prims[t] = q;
  }
  __syncthreads();
  const int i = blockIdx.x * BX + threadIdx.x, j = blockIdx.y * BY + threadIdx.y;
  if (i >= g.W || j >= g.H) return;
  bool obst = (i < 1) | (i > g.W - 2) | (j < 1) | (j > g.H - 2) | (k < 1) | (k > g.D - 2);      // emptyDomain, boundary width 1
  const float x = (float)i, y = (float)j, z = (float)k;
  for (int q = 0; q < nprim; ++q) {
    const Prim3 P = prims[q];
    const float dx = x - P.cx, dy = y - P.cy, dz = z - P.cz;
    const float dx2 = dx * dx, dy2 = dy * dy, dz2 = dz * dz;
    // a ball of radius a, or the box of half extents (a, b, c): squared distances, no square root
    const bool in = P.box ? ((dx2 <= P.a2) & (dy2 <= P.b2) & (dz2 <= P.c2)) : ((dx2 + dy2) + dz2 <= P.a2);
    obst = obst | in;
  }
  flags[(size_t)b * g.DHW + (size_t)k * g.HW + (size_t)j * g.W + i] = obst ? FNX_OBST : FNX_FLUID;
}

// ---- lattice value noise ------------------------------------------------------------------------------------------------------
// the 2D kernel's sum over octaves with a trilinear smoothstep blend of the eight lattice values around the point: along x, then y,
// then z
__device__ __forceinline__ float lattice3(unsigned key, int lx, int ly) {
  return 2.0f * uniform01(key, (unsigned)ly * 65536u + (unsigned)lx) - 1.0f;
}
__device__ __forceinline__ float smooth3(float t) { return (t * t) * (3.0f - 2.0f * t); }

__device__ __forceinline__ float plane_blend(unsigned key, int lx, int ly, float sx, float sy) {
  const float v00 = lattice3(key, lx, ly), v10 = lattice3(key, lx + 1, ly);
  const float v01 = lattice3(key, lx, ly + 1), v11 = lattice3(key, lx + 1, ly + 1);
  const float a = v00 + sx * (v10 - v00), c = v01 + sx * (v11 - v01);
  return a + sy * (c - a);
}

__device__ float fractal_noise3(unsigned seed, unsigned scene, unsigned stream0, int octaves, float f0, int i, int j, int k) {
  float acc = 0.f, gain = 1.f, f = f0;
  for (int o = 0; o < octaves; ++o) {
    const float x = (float)i * f, y = (float)j * f, z = (float)k * f;
    const int lx = (int)x, ly = (int)y, lz = (int)z;
    const float sx = smooth3(x - (float)lx), sy = smooth3(y - (float)ly), sz = smooth3(z - (float)lz);
    const unsigned s = stream0 + (unsigned)o;
    const float lo = plane_blend(scene_key(seed, scene, ((unsigned)lz << 8) | s), lx, ly, sx, sy);
    const float hi = plane_blend(scene_key(seed, scene, ((unsigned)(lz + 1) << 8) | s), lx, ly, sx, sy);
    acc = acc + gain * (lo + sz * (hi - lo));
    gain = gain * 0.5f; f = f * 2.0f;
  }
  return acc;
}

__global__ __launch_bounds__(BX* BY) void scene_turbulence3d_kernel(GridDims g, FnxSceneParams prm, float f0,
                                                                    const int* __restrict__ ids, float* __restrict__ U,
                                                                    float* __restrict__ density) {
  const int i = blockIdx.x * BX + threadIdx.x, j = blockIdx.y * BY + threadIdx.y;
  const int b = blockIdx.z / g.D, k = blockIdx.z - b * g.D;
  if (i >= g.W || j >= g.H) return;
  const unsigned scene = (unsigned)ids[b];
  // psi_a sits on the cell edges along axis a; (i, j, k) names the edge that starts at the cell's low corner.  Every thread evaluates
  // an edge value by the same expression, so the twelve differences around a cell cancel up to their own rounding.
  auto psi = [&](unsigned s0, int ii, int jj, int kk) { return prm.amplitude * fractal_noise3(prm.seed, scene, s0, prm.octaves, f0, ii, jj, kk); };
  const float x0 = psi(STREAM_PSIX, i, j, k), xj = psi(STREAM_PSIX, i, j + 1, k), xk = psi(STREAM_PSIX, i, j, k + 1);
  const float y0 = psi(STREAM_PSIY, i, j, k), yi = psi(STREAM_PSIY, i + 1, j, k), yk = psi(STREAM_PSIY, i, j, k + 1);
  const float z0 = psi(STREAM_PSIZ, i, j, k), zi = psi(STREAM_PSIZ, i + 1, j, k), zj = psi(STREAM_PSIZ, i, j + 1, k);
  const size_t o = (size_t)k * g.HW + (size_t)j * g.W + i;
  float* u = U + (size_t)b * 3 * g.DHW + o;
  u[0] = (zj - z0) - (yk - y0);
  u[g.DHW] = (xk - x0) - (zi - z0);
  u[(size_t)2 * g.DHW] = (yi - y0) - (xj - x0);
  if (density) {
    float r = prm.density_scale * fractal_noise3(prm.seed, scene, STREAM_RHO3, prm.octaves, f0, i, j, k);
    r = r < 0.f ? 0.f : (r > 1.f ? 1.f : r);
    density[(size_t)b * g.DHW + o] = r;
  }
}

// ---- the loss -----------------------------------------------------------------------------------------------------------------
// the divergence of cell (i, j, k) with the bits of divergence_kernel<true> (fnx_stencils.hip); u, fl: channel 0 / flags of the
// sample.  The +1, +W and +HW reads happen for non-border cells only.
__device__ __forceinline__ float cell_div3(const GridDims& g, const float* __restrict__ u, const float* __restrict__ fl, int i, int j, int k) {
  if ((i < 1) | (i > g.W - 2) | (j < 1) | (j > g.H - 2) | (k < 1) | (k > g.D - 2)) return 0.f;
  const size_t o = (size_t)k * g.HW + (size_t)j * g.W + i;
  if (fl[o] == FNX_OBST) return 0.f;
  const float* v = u + g.DHW;
  const float* w = u + (size_t)2 * g.DHW;
  const float d = ((u[o] - u[o + 1]) + v[o]) - v[o + g.W];
  return d + (w[o] - w[o + g.HW]);
}

template <bool SUMS, bool GRADS>
__global__ __launch_bounds__(BX* BY) void train_loss3d_kernel(GridDims g, const float* __restrict__ out_p, const float* __restrict__ out_U,
                                                              const float* __restrict__ flags, const float* __restrict__ target_p,
                                                              LossCoef kc, const float* __restrict__ upstream,
                                                              double* __restrict__ partial, float* __restrict__ grad_p,
                                                              float* __restrict__ grad_U) {
  const int i = blockIdx.x * BX + threadIdx.x, j = blockIdx.y * BY + threadIdx.y;
  const int b = blockIdx.z / g.D, k = blockIdx.z - b * g.D;
  const bool valid = i < g.W && j < g.H;
  double s[4] = {0.0, 0.0, 0.0, 0.0};              // (p - t)^2, div^2, |p - t|, |div|
  if (valid) {
    const size_t o = (size_t)k * g.HW + (size_t)j * g.W + i;
    const float* u = out_U + (size_t)b * 3 * g.DHW;
    const float* fl = flags + (size_t)b * g.DHW;
    const float d = cell_div3(g, u, fl, i, j, k);
    const float e = target_p ? out_p[(size_t)b * g.DHW + o] - target_p[(size_t)b * g.DHW + o] : 0.f;
    if (SUMS) {
      s[0] = (double)e * (double)e; s[1] = (double)d * (double)d;
      s[2] = (double)(e < 0.f ? -e : e); s[3] = (double)(d < 0.f ? -d : d);
    }
    if (GRADS) {
      const float up = upstream[0];
      // dL/d div of a cell; 0 wherever div is exactly 0 (border shell, obstacles: sign(0) = 0)
      auto gd = [&](float v) { return (kc.d2 * v + kc.d1 * sign_of(v)) * up; };
      const float own = gd(d);
      const float gx = i >= 1 ? gd(cell_div3(g, u, fl, i - 1, j, k)) : 0.f;
      const float gy = j >= 1 ? gd(cell_div3(g, u, fl, i, j - 1, k)) : 0.f;
      const float gz = k >= 1 ? gd(cell_div3(g, u, fl, i, j, k - 1)) : 0.f;
      float* gu = grad_U + (size_t)b * 3 * g.DHW + o;
      gu[0] = own - gx;                             // the stencil of divergence_bwd_kernel<true>
      gu[g.DHW] = own - gy;
      gu[(size_t)2 * g.DHW] = own - gz;
      // exactly 0 when both pressure lambdas are 0
      grad_p[(size_t)b * g.DHW + o] = (kc.p2 != 0.f || kc.p1 != 0.f) ? (kc.p2 * e + kc.p1 * sign_of(e)) * up : 0.f;
    }
  }
  if (SUMS) {
    __shared__ double red[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) s[q] += __shfl_down(s[q], off, 64);
    }
    const int t = threadIdx.y * BX + threadIdx.x;
    if ((t & 63) == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) red[t >> 6][q] = s[q];
    }
    __syncthreads();
    if (t < 4) {
      const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
      partial[blk * 4 + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
    }
  }
}

inline dim3 cells3(const FnxGrid* g) { return dim3((g->W + BX - 1) / BX, (g->H + BY - 1) / BY, g->B * g->D); }
inline size_t loss_blocks3(const FnxGrid* g) { const dim3 c = cells3(g); return (size_t)c.x * c.y * c.z; }

// The checks the 3D scene and loss entry points share, before any device call.
int check_scene_grid3(const char* fn, const FnxGrid* g, bool args) {
  if (!g || !args) return fnx::set_error(FNX_EINVAL, "%s: null argument", fn);
  if (!g->is3D || g->D < 4)
    return fnx::set_error(FNX_EINVAL, "%s: this entry point is 3D only (is3D = %d, D = %d; the net's three scales need 4 planes)", fn, g->is3D, g->D);
  if (g->B < 1 || g->H < 4 || g->W < 4) return fnx::set_error(FNX_EINVAL, "%s: at least 4 cells per axis are needed (B %d, D %d, H %d, W %d)", fn, g->B, g->D, g->H, g->W);
  if (g->D > 32768 || g->H > 32768 || g->W > 32768)
    return fnx::set_error(FNX_EINVAL, "%s: D, H, W <= 32768 (the noise lattice is addressed with 16 bits along x and y and the plane in the stream word)", fn);
  if ((long long)g->B * g->D > 65535) return fnx::set_error(FNX_EINVAL, "%s: B * D <= 65535 (B %d, D %d: the planes of the batch are a launch dimension)", fn, g->B, g->D);
  if ((long long)g->D * g->H * g->W > 2147483647LL)
    return fnx::set_error(FNX_EINVAL, "%s: D * H * W < 2^31 cells per sample (D %d, H %d, W %d)", fn, g->D, g->H, g->W);
  return FNX_OK;
}

}  // namespace

extern "C" {

int fnx_scene_obstacles3d(const FnxGrid* g, const FnxSceneParams* prm, const int* scene_ids, float* flags, void* stream) {
  if (int rc = check_scene_grid3(__func__, g, prm && scene_ids && flags)) return rc;
  if (int rc = check_scene_params(__func__, prm, true)) return rc;
  scene_obstacles3d_kernel<<<cells3(g), dim3(BX, BY), 0, (hipStream_t)stream>>>(make_dims(g->B, g->D, g->H, g->W), *prm, scene_ids, flags);
  return scene_status(__func__);
}

int fnx_scene_turbulence3d(const FnxGrid* g, const FnxSceneParams* prm, const int* scene_ids, float* U, float* density, void* stream) {
  if (int rc = check_scene_grid3(__func__, g, prm && scene_ids && U)) return rc;
  if (int rc = check_scene_params(__func__, prm, false)) return rc;
  const float f0 = 1.0f / prm->wavelength;          // (a correctly rounded fp32 division on the host)
  scene_turbulence3d_kernel<<<cells3(g), dim3(BX, BY), 0, (hipStream_t)stream>>>(make_dims(g->B, g->D, g->H, g->W), *prm, f0, scene_ids, U, density);
  return scene_status(__func__);
}

size_t fnx_train_loss3d_ws_bytes(const FnxGrid* g) {
  if (check_scene_grid3(__func__, g, true)) return 0;
  return loss_blocks3(g) * 4 * sizeof(double);
}

int fnx_train_loss3d(const FnxGrid* g, const float* out_p, const float* out_U, const float* flags, const float* target_p,
                     const float lambdas[4], const float* upstream, float* terms, float* grad_p, float* grad_U, void* ws, size_t ws_bytes,
                     void* stream) {
  if (int rc = check_scene_grid3(__func__, g, out_p && out_U && flags && lambdas)) return rc;
  if (!target_p && (lambdas[0] != 0.f || lambdas[2] != 0.f))
    return fnx::set_error(FNX_EINVAL, "%s: target_p is null but a pressure term is on (pL2Lambda %g, pL1Lambda %g)", __func__, lambdas[0], lambdas[2]);
  const bool sums = terms != nullptr, grads = grad_p || grad_U;
  if (!sums && !grads) return fnx::set_error(FNX_EINVAL, "%s: null argument (neither terms nor gradients are asked for)", __func__);
  if (grads && !(grad_p && grad_U && upstream)) return fnx::set_error(FNX_EINVAL, "%s: null argument (the gradients need grad_p, grad_U and upstream)", __func__);
  if (sums && !ws) return fnx::set_error(FNX_EINVAL, "%s: null argument (the terms need the workspace)", __func__);
  if (sums && ws_bytes < fnx_train_loss3d_ws_bytes(g)) return fnx::set_error(FNX_EWORKSPACE, "%s: workspace of %zu bytes is too small", __func__, ws_bytes);
  const GridDims d = make_dims(g->B, g->D, g->H, g->W);
  const double n = (double)g->B * g->D * g->H * g->W;
  LossCoef k;
  k.p2 = (float)(2.0 * lambdas[0] / n); k.p1 = (float)(lambdas[2] / n);
  k.d2 = (float)(2.0 * lambdas[1] / n); k.d1 = (float)(lambdas[3] / n);
  hipStream_t s = (hipStream_t)stream;
  double* partial = (double*)ws;
  const dim3 grid = cells3(g), block(BX, BY);
  if (sums && grads) train_loss3d_kernel<true, true><<<grid, block, 0, s>>>(d, out_p, out_U, flags, target_p, k, upstream, partial, grad_p, grad_U);
  else if (sums) train_loss3d_kernel<true, false><<<grid, block, 0, s>>>(d, out_p, out_U, flags, target_p, k, upstream, partial, grad_p, grad_U);
  else train_loss3d_kernel<false, true><<<grid, block, 0, s>>>(d, out_p, out_U, flags, target_p, k, upstream, partial, grad_p, grad_U);
  if (sums) train_loss_finish_kernel<<<1, 256, 0, s>>>(loss_blocks3(g), n, partial, lambdas[0], lambdas[1], lambdas[2], lambdas[3], terms);
  return scene_status(__func__);
}

}  // extern "C"
