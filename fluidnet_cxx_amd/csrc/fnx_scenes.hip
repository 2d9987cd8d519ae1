// Training scenes and the training loss for gfx950, in 2D (ABI 23: fnx_scene_obstacles, fnx_scene_turbulence, fnx_train_loss) and in 3D
// (ABI 26: the same names with a 3d suffix).  One unit: the kernels are templates on the dimension over a grid {D, H, W} with D = 1 in 2D.
//
// Randomness is counter based: no state, no atomics.  A 32-bit word is a function of (seed, scene_id, stream, counter) alone,
//   mix(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16      (the "lowbias32" integer finaliser)
//   hash(seed, scene, stream, counter) = mix(mix(mix(mix(seed + 0x9e3779b9) ^ scene) ^ stream) ^ counter)
//   uniform = (hash >> 8) * 2^-24 in [0, 1)
// so a scene's bits depend on (seed, scene_id, the grid) and the parameters only -- not on its batch slot, the batch size or the launch.
// A lattice value at the integer point (lx, ly, lz) of octave o of a noise whose stream base is s0 is addressed by
//   key     = scene_key(seed, scene, (lz << 8) | (s0 + o))         the plane goes into the stream word, above its low byte (2D: lz = 0)
//   counter = ly * 65536 + lx
// which is injective for 0 <= lx, ly < 65536 and 0 <= lz < 2^24: the grids accepted here (every axis <= 32768) stay inside it.
// Stream bases (low byte of the stream word), per dimension in Streams<IS3D>:
//   2D   0 = the obstacle primitives (counter 8 * primitive + draw: 0 = disc / box, 1..2 = the centre's offsets along x, y, 3..4 = the
//        radius resp. the half extents), 16 + o = the potential, 32 + o = the density
//   3D   80 = the obstacle primitives (counter 16 * primitive + draw: 0 = ball / box, 1..3 = the offsets along x, y, z, 4..6 = the radius
//        resp. the half extents), 96 + o = psi_x, 112 + o = psi_y, 128 + o = psi_z, 144 + o = the density
// Counter 0xffff0000 of the obstacle stream is the number of primitives.  The samplers use 64 and 65.
//
// Arithmetic of the scene kernels: integer operations, fp32 add / subtract / multiply / compare and int <-> float conversion only,
// compiled without contraction, each expression in the order written here; tests/scene_reference.py and tests/scene_reference_3d.py are
// the same statement in numpy and the kernels are bit-identical to them.
//
// One thread per cell, the plane from the grid's z (blockIdx.z = b * D + k).  The 3D turbulence thread evaluates its nine potential
// values itself: the kernel runs once per scene next to a converged pressure solve, so nothing is carried between planes.
//
// The loss (fluid_net_train.py:276-285) is tolerance-checked: one launch computes the four terms' fp64 partial sums per workgroup
// and both gradients, a one-workgroup launch adds the partials in index order.  The divergence of a cell has the bits of
// fnx_velocity_divergence; the gradient with respect to U is formed per face from the divergences of the face's two cells, which the
// thread recomputes (nothing is stored in between).
#include <stdio.h>
#include "fnx_device.h"
#include "fnx_kernels.h"
#include "../../include/fluidnet_hip.h"

namespace {

constexpr int BX = 64, BY = 4;

__host__ __device__ __forceinline__ unsigned mix32(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
__host__ __device__ __forceinline__ unsigned scene_key(unsigned seed, unsigned scene, unsigned stream) {
  return mix32(mix32(mix32(seed + 0x9e3779b9u) ^ scene) ^ stream);
}
__host__ __device__ __forceinline__ float uniform01(unsigned key, unsigned ctr) {
  return (float)(int)(mix32(key ^ ctr) >> 8) * 5.9604644775390625e-8f;      // 2^-24
}

template <bool IS3D> struct Streams;
template <> struct Streams<false> { static constexpr unsigned OBST = 0u, PRIM_STRIDE = 8u, PSI = 16u, RHO = 32u; };
template <> struct Streams<true> { static constexpr unsigned OBST = 80u, PRIM_STRIDE = 16u, PSIX = 96u, PSIY = 112u, PSIZ = 128u, RHO = 144u; };
constexpr unsigned COUNT_CTR = 0xffff0000u;

// the sample and the plane of a workgroup: blockIdx.z = b * D + k
template <bool IS3D> __device__ __forceinline__ void plane_of(const GridDims& g, int& b, int& k) {
  if constexpr (IS3D) { b = blockIdx.z / g.D; k = blockIdx.z - b * g.D; }
  else { b = blockIdx.z; k = 0; }
}
// a cell of the one-cell border of the domain (emptyDomain, boundary width 1)
template <bool IS3D> __device__ __forceinline__ bool on_border(const GridDims& g, int i, int j, int k) {
  const bool ring = (i < 1) | (i > g.W - 2) | (j < 1) | (j > g.H - 2);
  if constexpr (IS3D) return ring | (k < 1) | (k > g.D - 2);
  else return ring;
}

// ---- obstacles ----------------------------------------------------------------------------------------------------------------
struct Prim { float c[3], r2[3]; int box; };      // centre and squared radius resp. half extents along x, y, z (2D: no z)

template <bool IS3D>
__global__ __launch_bounds__(BX* BY) void scene_obstacles_kernel(GridDims g, FnxSceneParams prm, const int* __restrict__ ids,
                                                                 float* __restrict__ flags) {
  constexpr int NA = IS3D ? 3 : 2;
  __shared__ Prim prims[FNX_SCENE_MAX_PRIMITIVES];
  __shared__ int nprim;
  int b, k;
  plane_of<IS3D>(g, b, k);
  const int t = threadIdx.y * BX + threadIdx.x;
  const unsigned key = scene_key(prm.seed, (unsigned)ids[b], Streams<IS3D>::OBST);
  const int span = prm.n_max - prm.n_min + 1;
  int n = prm.n_min + (int)(uniform01(key, COUNT_CTR) * (float)span);
  if (n > prm.n_max) n = prm.n_max;
  if (t == 0) nprim = n;
  if (t < n) {
    const int ext[3] = {g.W, g.H, g.D};
    int mi = g.H < g.W ? g.H : g.W;                 // the scale: min(H, W) in 2D, min(D, H, W) in 3D
    if constexpr (IS3D) mi = g.D < mi ? g.D : mi;
    const float m = (float)mi;
    const unsigned c = Streams<IS3D>::PRIM_STRIDE * (unsigned)t;
    Prim q;
    q.box = (int)(mix32(key ^ c) >> 31);
#pragma unroll
    for (int a = 0; a < NA; ++a) {                  // draws 1 .. NA: the centre's offsets, NA + 1 .. 2 NA: the sizes
      const float off = prm.centre_min + uniform01(key, c + 1u + a) * (prm.centre_max - prm.centre_min);
      q.c[a] = 0.5f * (float)(ext[a] - 1) + off * m;
      const float r = (prm.size_min + uniform01(key, c + 1u + NA + a) * (prm.size_max - prm.size_min)) * m;
      q.r2[a] = r * r;
    }
    prims[t] = q;
  }
  __syncthreads();
  const int i = blockIdx.x * BX + threadIdx.x, j = blockIdx.y * BY + threadIdx.y;
  if (i >= g.W || j >= g.H) return;
  bool obst = on_border<IS3D>(g, i, j, k);
  const float pos[3] = {(float)i, (float)j, (float)k};
  for (int q = 0; q < nprim; ++q) {
    const Prim P = prims[q];
    float d2[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) { const float d = pos[a] - P.c[a]; d2[a] = d * d; }
    // a disc (ball) of radius r[0], or the box of half extents r: squared distances, no square root
    bool inbox = (d2[0] <= P.r2[0]) & (d2[1] <= P.r2[1]);
    float dist2 = d2[0] + d2[1];
    if constexpr (IS3D) { inbox = inbox & (d2[2] <= P.r2[2]); dist2 = dist2 + d2[2]; }
    obst = obst | (P.box ? inbox : (dist2 <= P.r2[0]));
  }
  flags[(size_t)b * g.DHW + (size_t)k * g.HW + (size_t)j * g.W + i] = obst ? FNX_OBST : FNX_FLUID;
}

// ---- lattice value noise ------------------------------------------------------------------------------------------------------
// sum over octaves of gain_o * noise_o(x f_o, y f_o[, z f_o]): f_o = f_0 2^o, gain_o = 2^-o; a lattice value is 2 uniform - 1, the
// four (3D: eight) around a point are blended with the smoothstep s(t) = t t (3 - 2 t): along x, then y, then z
__device__ __forceinline__ float lattice(unsigned key, int lx, int ly) {
  return 2.0f * uniform01(key, (unsigned)ly * 65536u + (unsigned)lx) - 1.0f;
}
__device__ __forceinline__ float smooth(float t) { return (t * t) * (3.0f - 2.0f * t); }

__device__ __forceinline__ float plane_blend(unsigned key, int lx, int ly, float sx, float sy) {
  const float v00 = lattice(key, lx, ly), v10 = lattice(key, lx + 1, ly);
  const float v01 = lattice(key, lx, ly + 1), v11 = lattice(key, lx + 1, ly + 1);
  const float a = v00 + sx * (v10 - v00), c = v01 + sx * (v11 - v01);
  return a + sy * (c - a);
}

template <bool IS3D>
__device__ float fractal_noise(unsigned seed, unsigned scene, unsigned stream0, int octaves, float f0, int i, int j, int k) {
  float acc = 0.f, gain = 1.f, f = f0;
  for (int o = 0; o < octaves; ++o) {
    const float x = (float)i * f, y = (float)j * f;
    const int lx = (int)x, ly = (int)y;
    const float sx = smooth(x - (float)lx), sy = smooth(y - (float)ly);
    const unsigned s = stream0 + (unsigned)o;
    float v;
    if constexpr (IS3D) {
      const float z = (float)k * f;
      const int lz = (int)z;
      const float sz = smooth(z - (float)lz);
      const float lo = plane_blend(scene_key(seed, scene, ((unsigned)lz << 8) | s), lx, ly, sx, sy);
      const float hi = plane_blend(scene_key(seed, scene, ((unsigned)(lz + 1) << 8) | s), lx, ly, sx, sy);
      v = lo + sz * (hi - lo);
    } else {
      v = plane_blend(scene_key(seed, scene, s), lx, ly, sx, sy);
    }
    acc = acc + gain * v;
    gain = gain * 0.5f; f = f * 2.0f;
  }
  return acc;
}

template <bool IS3D>
__global__ __launch_bounds__(BX* BY) void scene_turbulence_kernel(GridDims g, FnxSceneParams prm, float f0,
                                                                  const int* __restrict__ ids, float* __restrict__ U,
                                                                  float* __restrict__ density) {
  using S = Streams<IS3D>;
  const int i = blockIdx.x * BX + threadIdx.x, j = blockIdx.y * BY + threadIdx.y;
  int b, k;
  plane_of<IS3D>(g, b, k);
  if (i >= g.W || j >= g.H) return;
  const unsigned scene = (unsigned)ids[b];
  auto noise = [&](unsigned s0, int ii, int jj, int kk) { return fractal_noise<IS3D>(prm.seed, scene, s0, prm.octaves, f0, ii, jj, kk); };
  auto psi = [&](unsigned s0, int ii, int jj, int kk) { return prm.amplitude * noise(s0, ii, jj, kk); };
  const size_t o = (size_t)k * g.HW + (size_t)j * g.W + i;
  float* u = U + (size_t)b * (IS3D ? 3 : 2) * g.DHW + o;
  // Every thread evaluates a value of the potential by the same expression, so the differences around a cell cancel up to their own
  // rounding.
  if constexpr (IS3D) {
    // the curl of a vector potential: psi_a sits on the cell edges along axis a; (i, j, k) names the edge that starts at the cell's
    // low corner
    const float x0 = psi(S::PSIX, i, j, k), xj = psi(S::PSIX, i, j + 1, k), xk = psi(S::PSIX, i, j, k + 1);
    const float y0 = psi(S::PSIY, i, j, k), yi = psi(S::PSIY, i + 1, j, k), yk = psi(S::PSIY, i, j, k + 1);
    const float z0 = psi(S::PSIZ, i, j, k), zi = psi(S::PSIZ, i + 1, j, k), zj = psi(S::PSIZ, i, j + 1, k);
    u[0] = (zj - z0) - (yk - y0);
    u[g.DHW] = (xk - x0) - (zi - z0);
    u[(size_t)2 * g.DHW] = (yi - y0) - (xj - x0);
  } else {
    // the curl of a stream function on the grid nodes (i, j), (i, j + 1), (i + 1, j)
    const float p00 = psi(S::PSI, i, j, 0), p01 = psi(S::PSI, i, j + 1, 0), p10 = psi(S::PSI, i + 1, j, 0);
    u[0] = p01 - p00;
    u[g.DHW] = 0.f - (p10 - p00);
  }
  if (density) {
    float r = prm.density_scale * noise(S::RHO, i, j, k);
    r = r < 0.f ? 0.f : (r > 1.f ? 1.f : r);
    density[(size_t)b * g.DHW + o] = r;
  }
}

// ---- the loss -----------------------------------------------------------------------------------------------------------------
struct LossCoef { float p2, p1, d2, d1; };     // 2 lambda / N resp. lambda / N of the four terms (the gradient's factors)

__device__ __forceinline__ float sign_of(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// the divergence of cell (i, j, k) with the bits of divergence_kernel<IS3D> (fnx_stencils.hip); u, fl: channel 0 / flags of the
// sample.  The +1, +W and +HW reads happen for non-border cells only.
template <bool IS3D>
__device__ __forceinline__ float cell_div(const GridDims& g, const float* __restrict__ u, const float* __restrict__ fl, int i, int j, int k) {
  if (on_border<IS3D>(g, i, j, k)) return 0.f;
  const size_t o = (size_t)k * g.HW + (size_t)j * g.W + i;
  if (fl[o] == FNX_OBST) return 0.f;
  const float* v = u + g.DHW;
  const float d = ((u[o] - u[o + 1]) + v[o]) - v[o + g.W];
  if constexpr (IS3D) {
    const float* w = u + (size_t)2 * g.DHW;
    return d + (w[o] - w[o + g.HW]);
  } else {
    return d;
  }
}

template <bool IS3D, bool SUMS, bool GRADS>
__global__ __launch_bounds__(BX* BY) void train_loss_kernel(GridDims g, const float* __restrict__ out_p, const float* __restrict__ out_U,
                                                            const float* __restrict__ flags, const float* __restrict__ target_p,
                                                            LossCoef kc, const float* __restrict__ upstream,
                                                            double* __restrict__ partial, float* __restrict__ grad_p,
                                                            float* __restrict__ grad_U) {
  constexpr int NA = IS3D ? 3 : 2;
  const int i = blockIdx.x * BX + threadIdx.x, j = blockIdx.y * BY + threadIdx.y;
  int b, k;
  plane_of<IS3D>(g, b, k);
  const bool valid = i < g.W && j < g.H;
  double s[4] = {0.0, 0.0, 0.0, 0.0};              // (p - t)^2, div^2, |p - t|, |div|
  if (valid) {
    const size_t o = (size_t)k * g.HW + (size_t)j * g.W + i;
    const float* u = out_U + (size_t)b * NA * g.DHW;
    const float* fl = flags + (size_t)b * g.DHW;
    const float d = cell_div<IS3D>(g, u, fl, i, j, k);
    const float e = target_p ? out_p[(size_t)b * g.DHW + o] - target_p[(size_t)b * g.DHW + o] : 0.f;
    if (SUMS) {
      s[0] = (double)e * (double)e; s[1] = (double)d * (double)d;
      s[2] = (double)(e < 0.f ? -e : e); s[3] = (double)(d < 0.f ? -d : d);
    }
    if (GRADS) {
      const float up = upstream[0];
      // dL/d div of a cell; 0 wherever div is exactly 0 (border, obstacles: sign(0) = 0)
      auto gd = [&](float v) { return (kc.d2 * v + kc.d1 * sign_of(v)) * up; };
      const float own = gd(d);
      const float gx = i >= 1 ? gd(cell_div<IS3D>(g, u, fl, i - 1, j, k)) : 0.f;
      const float gy = j >= 1 ? gd(cell_div<IS3D>(g, u, fl, i, j - 1, k)) : 0.f;
      const float gz = IS3D && k >= 1 ? gd(cell_div<IS3D>(g, u, fl, i, j, k - 1)) : 0.f;
      float* gu = grad_U + (size_t)b * NA * g.DHW + o;
      gu[0] = own - gx;                             // the stencil of divergence_bwd_kernel<IS3D>
      gu[g.DHW] = own - gy;
      if constexpr (IS3D) gu[(size_t)2 * g.DHW] = own - gz;
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

// terms[q] = sum of the partials in index order / N;  terms[4] = sum_q lambda_q terms[q]
__global__ __launch_bounds__(256) void train_loss_finish_kernel(size_t nblk, double n, const double* __restrict__ partial, float l0,
                                                                float l1, float l2, float l3, float* __restrict__ terms) {
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (size_t q = threadIdx.x; q < nblk; q += 256) {
#pragma unroll
    for (int c = 0; c < 4; ++c) s[c] += partial[q * 4 + c];
  }
  __shared__ double red[4][4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s[c] += __shfl_down(s[c], off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) red[threadIdx.x >> 6][c] = s[c];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double m[4];
    for (int c = 0; c < 4; ++c) m[c] = ((red[0][c] + red[1][c]) + (red[2][c] + red[3][c])) / n;
    for (int c = 0; c < 4; ++c) terms[c] = (float)m[c];
    terms[4] = (float)((((double)l0 * m[0] + (double)l1 * m[1]) + (double)l2 * m[2]) + (double)l3 * m[3]);
  }
}

// ---- the host side --------------------------------------------------------------------------------------------------------------
// one workgroup per 64 x 4 cells of a plane; the checks below have made D = 1 in 2D
inline dim3 cells(const FnxGrid* g) { return dim3((g->W + BX - 1) / BX, (g->H + BY - 1) / BY, g->B * g->D); }
inline size_t loss_blocks(const FnxGrid* g) { const dim3 c = cells(g); return (size_t)c.x * c.y * c.z; }
inline GridDims dims(const FnxGrid* g) { return make_dims(g->B, g->D, g->H, g->W); }

// The checks the scene and loss entry points of a dimension share, before any device call.
int check_scene_grid(const char* fn, const FnxGrid* g, bool is3d, bool args) {
  if (!g || !args) return fnx::set_error(FNX_EINVAL, "%s: null argument", fn);
  if (!is3d) {
    if (g->is3D || g->D != 1) return fnx::set_error(FNX_EINVAL, "%s: training scenes and the training loss are 2D only (is3D = %d, D = %d)", fn, g->is3D, g->D);
    if (g->B < 1 || g->H < 4 || g->W < 4) return fnx::set_error(FNX_EINVAL, "%s: at least 4 cells per axis are needed (B %d, H %d, W %d)", fn, g->B, g->H, g->W);
    if (g->H > 32768 || g->W > 32768 || g->B > 65535)
      return fnx::set_error(FNX_EINVAL, "%s: H, W <= 32768 and B <= 65535 (the noise lattice is addressed with 16 bits per axis; B is a launch dimension)", fn);
    return FNX_OK;
  }
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

int check_scene_params(const char* fn, const FnxSceneParams* p, bool obstacles) {
  if (obstacles) {
    if (p->n_max > FNX_SCENE_MAX_PRIMITIVES)
      return fnx::set_error(FNX_EINVAL, "%s: n_max %d is above the cap of %d primitives per scene", fn, p->n_max, FNX_SCENE_MAX_PRIMITIVES);
    if (p->n_min < 0 || p->n_min > p->n_max) return fnx::set_error(FNX_EINVAL, "%s: inverted range: n_min %d, n_max %d", fn, p->n_min, p->n_max);
    if (!(p->centre_min <= p->centre_max)) return fnx::set_error(FNX_EINVAL, "%s: inverted range: centre_min %g, centre_max %g", fn, p->centre_min, p->centre_max);
    if (!(p->size_min >= 0.f && p->size_min <= p->size_max)) return fnx::set_error(FNX_EINVAL, "%s: inverted range: size_min %g, size_max %g (0 <= min <= max)", fn, p->size_min, p->size_max);
  } else {
    if (p->octaves < 1 || p->octaves > FNX_SCENE_MAX_OCTAVES) return fnx::set_error(FNX_EINVAL, "%s: octaves %d outside 1 .. %d", fn, p->octaves, FNX_SCENE_MAX_OCTAVES);
    if (!(p->wavelength >= (float)(1 << (p->octaves - 1))))
      return fnx::set_error(FNX_EINVAL, "%s: wavelength %g cells is below 2^(octaves - 1) = %d (the finest octave needs a lattice of at least one cell)", fn,
                            p->wavelength, 1 << (p->octaves - 1));
    if (!(p->amplitude == p->amplitude) || !(p->density_scale == p->density_scale)) return fnx::set_error(FNX_EINVAL, "%s: amplitude or density_scale is NaN", fn);
  }
  return FNX_OK;
}

int scene_status(const char* fn) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? FNX_OK : fnx::set_error(FNX_EHIP, "%s: HIP error in a launch: %s", fn, hipGetErrorString(e));
}

// The bodies of the entry points; fn is the caller's name, which the error texts carry.
template <bool IS3D>
int scene_obstacles(const char* fn, const FnxGrid* g, const FnxSceneParams* prm, const int* scene_ids, float* flags, void* stream) {
  if (int rc = check_scene_grid(fn, g, IS3D, prm && scene_ids && flags)) return rc;
  if (int rc = check_scene_params(fn, prm, true)) return rc;
  scene_obstacles_kernel<IS3D><<<cells(g), dim3(BX, BY), 0, (hipStream_t)stream>>>(dims(g), *prm, scene_ids, flags);
  return scene_status(fn);
}

template <bool IS3D>
int scene_turbulence(const char* fn, const FnxGrid* g, const FnxSceneParams* prm, const int* scene_ids, float* U, float* density, void* stream) {
  if (int rc = check_scene_grid(fn, g, IS3D, prm && scene_ids && U)) return rc;
  if (int rc = check_scene_params(fn, prm, false)) return rc;
  const float f0 = 1.0f / prm->wavelength;          // (a correctly rounded fp32 division on the host)
  scene_turbulence_kernel<IS3D><<<cells(g), dim3(BX, BY), 0, (hipStream_t)stream>>>(dims(g), *prm, f0, scene_ids, U, density);
  return scene_status(fn);
}

size_t loss_ws_bytes(const char* fn, const FnxGrid* g, bool is3d) {
  if (check_scene_grid(fn, g, is3d, true)) return 0;
  return loss_blocks(g) * 4 * sizeof(double);
}

template <bool IS3D>
int train_loss(const char* fn, const FnxGrid* g, const float* out_p, const float* out_U, const float* flags, const float* target_p,
               const float lambdas[4], const float* upstream, float* terms, float* grad_p, float* grad_U, void* ws, size_t ws_bytes,
               void* stream) {
  if (int rc = check_scene_grid(fn, g, IS3D, out_p && out_U && flags && lambdas)) return rc;
  if (!target_p && (lambdas[0] != 0.f || lambdas[2] != 0.f))      // (without a pressure term a null target_p reports both as 0)
    return fnx::set_error(FNX_EINVAL, "%s: target_p is null but a pressure term is on (pL2Lambda %g, pL1Lambda %g)", fn, lambdas[0], lambdas[2]);
  const bool sums = terms != nullptr, grads = grad_p || grad_U;
  if (!sums && !grads) return fnx::set_error(FNX_EINVAL, "%s: null argument (neither terms nor gradients are asked for)", fn);
  if (grads && !(grad_p && grad_U && upstream)) return fnx::set_error(FNX_EINVAL, "%s: null argument (the gradients need grad_p, grad_U and upstream)", fn);
  if (sums && !ws) return fnx::set_error(FNX_EINVAL, "%s: null argument (the terms need the workspace)", fn);
  if (sums && ws_bytes < loss_blocks(g) * 4 * sizeof(double)) return fnx::set_error(FNX_EWORKSPACE, "%s: workspace of %zu bytes is too small", fn, ws_bytes);
  const GridDims d = dims(g);
  const double n = (double)g->B * g->D * g->H * g->W;
  LossCoef k;
  k.p2 = (float)(2.0 * lambdas[0] / n); k.p1 = (float)(lambdas[2] / n);
  k.d2 = (float)(2.0 * lambdas[1] / n); k.d1 = (float)(lambdas[3] / n);
  hipStream_t s = (hipStream_t)stream;
  double* partial = (double*)ws;
  const dim3 grid = cells(g), block(BX, BY);
  if (sums && grads) train_loss_kernel<IS3D, true, true><<<grid, block, 0, s>>>(d, out_p, out_U, flags, target_p, k, upstream, partial, grad_p, grad_U);
  else if (sums) train_loss_kernel<IS3D, true, false><<<grid, block, 0, s>>>(d, out_p, out_U, flags, target_p, k, upstream, partial, grad_p, grad_U);
  else train_loss_kernel<IS3D, false, true><<<grid, block, 0, s>>>(d, out_p, out_U, flags, target_p, k, upstream, partial, grad_p, grad_U);
  if (sums) train_loss_finish_kernel<<<1, 256, 0, s>>>(loss_blocks(g), n, partial, lambdas[0], lambdas[1], lambdas[2], lambdas[3], terms);
  return scene_status(fn);
}

}  // namespace

extern "C" {

int fnx_scene_obstacles(const FnxGrid* g, const FnxSceneParams* prm, const int* scene_ids, float* flags, void* stream) {
  return scene_obstacles<false>(__func__, g, prm, scene_ids, flags, stream);
}
int fnx_scene_obstacles3d(const FnxGrid* g, const FnxSceneParams* prm, const int* scene_ids, float* flags, void* stream) {
  return scene_obstacles<true>(__func__, g, prm, scene_ids, flags, stream);
}

int fnx_scene_turbulence(const FnxGrid* g, const FnxSceneParams* prm, const int* scene_ids, float* U, float* density, void* stream) {
  return scene_turbulence<false>(__func__, g, prm, scene_ids, U, density, stream);
}
int fnx_scene_turbulence3d(const FnxGrid* g, const FnxSceneParams* prm, const int* scene_ids, float* U, float* density, void* stream) {
  return scene_turbulence<true>(__func__, g, prm, scene_ids, U, density, stream);
}

size_t fnx_train_loss_ws_bytes(const FnxGrid* g) { return loss_ws_bytes(__func__, g, false); }
size_t fnx_train_loss3d_ws_bytes(const FnxGrid* g) { return loss_ws_bytes(__func__, g, true); }

int fnx_train_loss(const FnxGrid* g, const float* out_p, const float* out_U, const float* flags, const float* target_p,
                   const float lambdas[4], const float* upstream, float* terms, float* grad_p, float* grad_U, void* ws, size_t ws_bytes,
                   void* stream) {
  return train_loss<false>(__func__, g, out_p, out_U, flags, target_p, lambdas, upstream, terms, grad_p, grad_U, ws, ws_bytes, stream);
}
int fnx_train_loss3d(const FnxGrid* g, const float* out_p, const float* out_U, const float* flags, const float* target_p,
                     const float lambdas[4], const float* upstream, float* terms, float* grad_p, float* grad_U, void* ws, size_t ws_bytes,
                     void* stream) {
  return train_loss<true>(__func__, g, out_p, out_U, flags, target_p, lambdas, upstream, terms, grad_p, grad_U, ws, ws_bytes, stream);
}

}  // extern "C"
