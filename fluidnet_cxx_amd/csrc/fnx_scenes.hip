// Training scenes and the training loss for gfx950 (ABI 23): fnx_scene_obstacles, fnx_scene_turbulence, fnx_train_loss.
//
// Randomness is counter based: no state, no atomics.  A 32-bit word is a function of (seed, scene_id, stream, counter) alone,
//   mix(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16      (the "lowbias32" integer finaliser)
//   hash(seed, scene, stream, counter) = mix(mix(mix(mix(seed + 0x9e3779b9) ^ scene) ^ stream) ^ counter)
//   uniform = (hash >> 8) * 2^-24 in [0, 1)
// so a scene's bits depend on (seed, scene_id, H, W) and the parameters only -- not on its batch slot, the batch size or the launch.
// Streams: 0 = the obstacle primitives (counter 8 * primitive + draw; counter 0xffff0000 = their number), 16 + octave = the lattice
// of the potential's octave, 32 + octave = the lattice of the density's octave (counter = lattice y * 65536 + lattice x).
//
// Arithmetic: integer operations, fp32 add / subtract / multiply / compare and int <-> float conversion only, compiled without
// contraction, each expression in the order written here; tests/scene_reference.py is the same statement in numpy and the kernels
// are bit-identical to it.
//
// The loss (fluid_net_train.py:276-285) is tolerance-checked: one launch computes the four terms' fp64 partial sums per workgroup
// and both gradients, a one-workgroup launch adds the partials in index order.  The divergence of a cell has the bits of
// fnx_velocity_divergence; the gradient with respect to U is formed per face from the divergences of the face's two cells, which the
// thread recomputes (nothing is stored in between).
#include "fnx_scene_common.h"      // the hash, the loss's coefficients and finish, the parameter checks (shared with fnx_scenes3d.hip)

namespace {

constexpr unsigned STREAM_OBST = 0u, STREAM_PSI = 16u, STREAM_RHO = 32u, COUNT_CTR = 0xffff0000u;

// ---- obstacles ----------------------------------------------------------------------------------------------------------------
struct Prim { float cx, cy, a2, b2; int box; };

__global__ __launch_bounds__(BX* BY) void scene_obstacles_kernel(GridDims g, FnxSceneParams prm, const int* __restrict__ ids,
                                                                 float* __restrict__ flags) {
  __shared__ Prim prims[FNX_SCENE_MAX_PRIMITIVES];
  __shared__ int nprim;
  const int b = blockIdx.z, t = threadIdx.y * BX + threadIdx.x;
  const unsigned key = scene_key(prm.seed, (unsigned)ids[b], STREAM_OBST);
  const int span = prm.n_max - prm.n_min + 1;
  int n = prm.n_min + (int)(uniform01(key, COUNT_CTR) * (float)span);
  if (n > prm.n_max) n = prm.n_max;
  if (t == 0) nprim = n;
  if (t < n) {
    const float m = (float)(g.H < g.W ? g.H : g.W);
    const unsigned c = 8u * (unsigned)t;
    Prim q;
    q.box = (int)(mix32(key ^ c) >> 31);
    const float ox = prm.centre_min + uniform01(key, c + 1u) * (prm.centre_max - prm.centre_min);
    const float oy = prm.centre_min + uniform01(key, c + 2u) * (prm.centre_max - prm.centre_min);
    q.cx = 0.5f * (float)(g.W - 1) + ox * m;
    q.cy = 0.5f * (float)(g.H - 1) + oy * m;
    const float ra = (prm.size_min + uniform01(key, c + 3u) * (prm.size_max - prm.size_min)) * m;
    const float rb = (prm.size_min + uniform01(key, c + 4u) * (prm.size_max - prm.size_min)) * m;
    q.a2 = ra * ra; q.b2 = rb * rb;
    prims[t] = q;
  }
  __syncthreads();
  const int i = blockIdx.x * BX + threadIdx.x, j = blockIdx.y * BY + threadIdx.y;
  if (i >= g.W || j >= g.H) return;
  bool obst = (i < 1) | (i > g.W - 2) | (j < 1) | (j > g.H - 2);          // emptyDomain, boundary width 1
  const float x = (float)i, y = (float)j;
  for (int q = 0; q < nprim; ++q) {
    const Prim P = prims[q];
    const float dx = x - P.cx, dy = y - P.cy;
    const float dx2 = dx * dx, dy2 = dy * dy;
    // a disc of radius a, or the box of half extents (a, b): squared distances, no square root
    const bool in = P.box ? ((dx2 <= P.a2) & (dy2 <= P.b2)) : (dx2 + dy2 <= P.a2);
    obst = obst | in;
  }
  flags[(size_t)b * g.HW + (size_t)j * g.W + i] = obst ? FNX_OBST : FNX_FLUID;
}

// ---- lattice value noise ------------------------------------------------------------------------------------------------------
// sum over octaves of gain_o * noise_o(x f_o, y f_o): f_o = f_0 2^o, gain_o = 2^-o; a lattice value is 2 uniform - 1, the four
// around a point are blended with the smoothstep s(t) = t t (3 - 2 t)
__device__ __forceinline__ float lattice(unsigned key, int lx, int ly) {
  return 2.0f * uniform01(key, (unsigned)ly * 65536u + (unsigned)lx) - 1.0f;
}
__device__ __forceinline__ float smooth(float t) { return (t * t) * (3.0f - 2.0f * t); }

__device__ float fractal_noise(unsigned seed, unsigned scene, unsigned stream0, int octaves, float f0, int i, int j) {
  float acc = 0.f, gain = 1.f, f = f0;
  for (int o = 0; o < octaves; ++o) {
    const unsigned key = scene_key(seed, scene, stream0 + (unsigned)o);
    const float x = (float)i * f, y = (float)j * f;
    const int lx = (int)x, ly = (int)y;
    const float sx = smooth(x - (float)lx), sy = smooth(y - (float)ly);
    const float v00 = lattice(key, lx, ly), v10 = lattice(key, lx + 1, ly);
    const float v01 = lattice(key, lx, ly + 1), v11 = lattice(key, lx + 1, ly + 1);
    const float a = v00 + sx * (v10 - v00), c = v01 + sx * (v11 - v01);
    acc = acc + gain * (a + sy * (c - a));
    gain = gain * 0.5f; f = f * 2.0f;
  }
  return acc;
}

__global__ __launch_bounds__(BX* BY) void scene_turbulence_kernel(GridDims g, FnxSceneParams prm, float f0,
                                                                  const int* __restrict__ ids, float* __restrict__ U,
                                                                  float* __restrict__ density) {
  const int i = blockIdx.x * BX + threadIdx.x, j = blockIdx.y * BY + threadIdx.y, b = blockIdx.z;
  if (i >= g.W || j >= g.H) return;
  const unsigned scene = (unsigned)ids[b];
  // the potential on the grid nodes (i, j), (i, j + 1), (i + 1, j): every thread evaluates a node by the same expression, so the
  // four differences around a cell cancel up to their own rounding
  const float p00 = prm.amplitude * fractal_noise(prm.seed, scene, STREAM_PSI, prm.octaves, f0, i, j);
  const float p01 = prm.amplitude * fractal_noise(prm.seed, scene, STREAM_PSI, prm.octaves, f0, i, j + 1);
  const float p10 = prm.amplitude * fractal_noise(prm.seed, scene, STREAM_PSI, prm.octaves, f0, i + 1, j);
  const size_t o = (size_t)j * g.W + i;
  float* u = U + (size_t)b * 2 * g.HW + o;
  u[0] = p01 - p00;
  u[g.HW] = 0.f - (p10 - p00);
  if (density) {
    float r = prm.density_scale * fractal_noise(prm.seed, scene, STREAM_RHO, prm.octaves, f0, i, j);
    r = r < 0.f ? 0.f : (r > 1.f ? 1.f : r);
    density[(size_t)b * g.HW + o] = r;
  }
}

// ---- the loss -----------------------------------------------------------------------------------------------------------------
// the divergence of cell (i, j) with the bits of divergence_kernel (fnx_stencils.hip); u, fl: channel 0 / flags of the sample
__device__ __forceinline__ float cell_div(const GridDims& g, const float* __restrict__ u, const float* __restrict__ fl, int i, int j) {
  if ((i < 1) | (i > g.W - 2) | (j < 1) | (j > g.H - 2)) return 0.f;
  const size_t o = (size_t)j * g.W + i;
  if (fl[o] == FNX_OBST) return 0.f;
  return ((u[o] - u[o + 1]) + u[g.HW + o]) - u[(size_t)g.HW + o + g.W];
}

template <bool SUMS, bool GRADS>
__global__ __launch_bounds__(BX* BY) void train_loss_kernel(GridDims g, const float* __restrict__ out_p, const float* __restrict__ out_U,
                                                            const float* __restrict__ flags, const float* __restrict__ target_p,
                                                            LossCoef k, const float* __restrict__ upstream,
                                                            double* __restrict__ partial, float* __restrict__ grad_p,
                                                            float* __restrict__ grad_U) {
  const int i = blockIdx.x * BX + threadIdx.x, j = blockIdx.y * BY + threadIdx.y, b = blockIdx.z;
  const bool valid = i < g.W && j < g.H;
  double s[4] = {0.0, 0.0, 0.0, 0.0};              // (p - t)^2, div^2, |p - t|, |div|
  if (valid) {
    const size_t o = (size_t)j * g.W + i;
    const float* u = out_U + (size_t)b * 2 * g.HW;
    const float* fl = flags + (size_t)b * g.HW;
    const float d = cell_div(g, u, fl, i, j);
    const float e = target_p ? out_p[(size_t)b * g.HW + o] - target_p[(size_t)b * g.HW + o] : 0.f;
    if (SUMS) {
      s[0] = (double)e * (double)e; s[1] = (double)d * (double)d;
      s[2] = (double)(e < 0.f ? -e : e); s[3] = (double)(d < 0.f ? -d : d);
    }
    if (GRADS) {
      const float up = upstream[0];
      // dL/d div of a cell; 0 wherever div is exactly 0 (border ring, obstacles: sign(0) = 0)
      auto gd = [&](float v) { return (k.d2 * v + k.d1 * sign_of(v)) * up; };
      const float own = gd(d);
      const float gx = i >= 1 ? gd(cell_div(g, u, fl, i - 1, j)) : 0.f;
      const float gy = j >= 1 ? gd(cell_div(g, u, fl, i, j - 1)) : 0.f;
      float* gu = grad_U + (size_t)b * 2 * g.HW + o;
      gu[0] = own - gx;                             // the stencil of divergence_bwd_kernel
      gu[g.HW] = own - gy;
      // exactly 0 when both pressure lambdas are 0
      grad_p[(size_t)b * g.HW + o] = (k.p2 != 0.f || k.p1 != 0.f) ? (k.p2 * e + k.p1 * sign_of(e)) * up : 0.f;
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

inline dim3 cells(const FnxGrid* g) { return dim3((g->W + BX - 1) / BX, (g->H + BY - 1) / BY, g->B); }
inline size_t loss_blocks(const FnxGrid* g) { const dim3 c = cells(g); return (size_t)c.x * c.y * c.z; }

// The checks the scene and loss entry points share, before any device call.
int check_scene_grid(const char* fn, const FnxGrid* g, bool args) {
  if (!g || !args) return fnx::set_error(FNX_EINVAL, "%s: null argument", fn);
  if (g->is3D || g->D != 1) return fnx::set_error(FNX_EINVAL, "%s: training scenes and the training loss are 2D only (is3D = %d, D = %d)", fn, g->is3D, g->D);
  if (g->B < 1 || g->H < 4 || g->W < 4) return fnx::set_error(FNX_EINVAL, "%s: at least 4 cells per axis are needed (B %d, H %d, W %d)", fn, g->B, g->H, g->W);
  if (g->H > 32768 || g->W > 32768 || g->B > 65535)
    return fnx::set_error(FNX_EINVAL, "%s: H, W <= 32768 and B <= 65535 (the noise lattice is addressed with 16 bits per axis; B is a launch dimension)", fn);
  return FNX_OK;
}

}  // namespace

extern "C" {

int fnx_scene_obstacles(const FnxGrid* g, const FnxSceneParams* prm, const int* scene_ids, float* flags, void* stream) {
  if (int rc = check_scene_grid(__func__, g, prm && scene_ids && flags)) return rc;
  if (int rc = check_scene_params(__func__, prm, true)) return rc;
  scene_obstacles_kernel<<<cells(g), dim3(BX, BY), 0, (hipStream_t)stream>>>(make_dims(g->B, 1, g->H, g->W), *prm, scene_ids, flags);
  return scene_status(__func__);
}

int fnx_scene_turbulence(const FnxGrid* g, const FnxSceneParams* prm, const int* scene_ids, float* U, float* density, void* stream) {
  if (int rc = check_scene_grid(__func__, g, prm && scene_ids && U)) return rc;
  if (int rc = check_scene_params(__func__, prm, false)) return rc;
  const float f0 = 1.0f / prm->wavelength;          // (a correctly rounded fp32 division on the host)
  scene_turbulence_kernel<<<cells(g), dim3(BX, BY), 0, (hipStream_t)stream>>>(make_dims(g->B, 1, g->H, g->W), *prm, f0, scene_ids, U, density);
  return scene_status(__func__);
}

size_t fnx_train_loss_ws_bytes(const FnxGrid* g) {
  if (check_scene_grid(__func__, g, true)) return 0;
  return loss_blocks(g) * 4 * sizeof(double);
}

int fnx_train_loss(const FnxGrid* g, const float* out_p, const float* out_U, const float* flags, const float* target_p,
                   const float lambdas[4], const float* upstream, float* terms, float* grad_p, float* grad_U, void* ws, size_t ws_bytes,
                   void* stream) {
  if (int rc = check_scene_grid(__func__, g, out_p && out_U && flags && lambdas)) return rc;
  if (!target_p && (lambdas[0] != 0.f || lambdas[2] != 0.f))
    return fnx::set_error(FNX_EINVAL, "%s: target_p is null but a pressure term is on (pL2Lambda %g, pL1Lambda %g)", __func__, lambdas[0], lambdas[2]);
  const bool sums = terms != nullptr, grads = grad_p || grad_U;
  if (!sums && !grads) return fnx::set_error(FNX_EINVAL, "%s: null argument (neither terms nor gradients are asked for)", __func__);
  if (grads && !(grad_p && grad_U && upstream)) return fnx::set_error(FNX_EINVAL, "%s: null argument (the gradients need grad_p, grad_U and upstream)", __func__);
  if (sums && !ws) return fnx::set_error(FNX_EINVAL, "%s: null argument (the terms need the workspace)", __func__);
  if (sums && ws_bytes < fnx_train_loss_ws_bytes(g)) return fnx::set_error(FNX_EWORKSPACE, "%s: workspace of %zu bytes is too small", __func__, ws_bytes);
  const GridDims d = make_dims(g->B, 1, g->H, g->W);
  const double n = (double)g->B * g->H * g->W;
  const float* tp = target_p;                        // null: the two pressure terms are reported as 0
  LossCoef k;
  k.p2 = (float)(2.0 * lambdas[0] / n); k.p1 = (float)(lambdas[2] / n);
  k.d2 = (float)(2.0 * lambdas[1] / n); k.d1 = (float)(lambdas[3] / n);
  hipStream_t s = (hipStream_t)stream;
  double* partial = (double*)ws;
  const dim3 grid = cells(g), block(BX, BY);
  if (sums && grads) train_loss_kernel<true, true><<<grid, block, 0, s>>>(d, out_p, out_U, flags, tp, k, upstream, partial, grad_p, grad_U);
  else if (sums) train_loss_kernel<true, false><<<grid, block, 0, s>>>(d, out_p, out_U, flags, tp, k, upstream, partial, grad_p, grad_U);
  else train_loss_kernel<false, true><<<grid, block, 0, s>>>(d, out_p, out_U, flags, tp, k, upstream, partial, grad_p, grad_U);
  if (sums) train_loss_finish_kernel<<<1, 256, 0, s>>>(loss_blocks(g), n, partial, lambdas[0], lambdas[1], lambdas[2], lambdas[3], terms);
  return scene_status(__func__);
}

}  // extern "C"
