// Multigrid-preconditioned conjugate gradients for the pressure system of the Jacobi solve (ABI 20: fnx_pcg,
// fnx_poisson_apply, fnx_pcg_precondition, FnxStepParams.method 2).
//
// Operator: the fixed point of fnx_jacobi (cpp/fluids_init.cpp:858-994).  On an active cell (neither border nor obstacle)
//   (denom - n_sub) p_i - sum_{active nbr j} p_j = div_i
// denom 4 (2D) / 6 (3D); n_sub counts the obstacle neighbours the Jacobi replaces by p_i (Neumann) -- in 3D quirks mode
// the z obstacle neighbours are not replaced and contribute 0; a non-obstacle border neighbour
// contributes 0 (Dirichlet).  Every other cell is not a degree of freedom and gets p = 0.
//
// Hierarchy (built once per flags): level 0 is a 16-bit code per cell (the neighbour structure); level l+1 aggregates
// 2x2(x2) cells of level l (odd sizes leave a remainder aggregate of one cell per axis) and holds the Galerkin operator
// P^T A P of piecewise-constant P as (diag, w_-x, w_-y, w_-z) per cell: a face weight counts the coupled fine pairs across
// the coarse face, so every entry is an integer, exact in fp32.  Coarsening stops once every axis has <= 4 cells.
// Preconditioner M^-1: one V-cycle -- two damped-Jacobi sweeps (omega 2/3) from zero, residual restricted by R = P^T, the
// next level, correction prolongated by P and scaled by 1.8, two sweeps again; the coarsest level gets 16 sweeps from zero.
// Same sweeps before and after and R = P^T: M^-1 is one fixed symmetric linear map.  The levels of at most 4096 cells per
// sample run as ONE launch of one workgroup per sample (barriers between the phases) instead of ~6 launches per level.
// CG: per sample, zero initial guess, alpha / beta / norms on the device, every dot product as fp64 partial sums per
// workgroup added in a fixed order by one workgroup (no atomics): the same bits run to run.
// Warm start (ABI 27: fnx_pcg_from, FnxStepParams.method 3 and 4): with a guess x0, d = x0 on the degrees of freedom and 0 elsewhere,
// and the solve starts from x = a0 d, a0 = (d.b) / (d.A d) -- one steepest-descent step along d.  a0 = 0 is among the candidates, so
// in the energy norm the start is never worse than x = 0 whatever the guess's magnitude; A d, d.b (b has mean zero there) and d.A d
// do not see a constant added to d on a singular sample, so d needs no mean removal.  r0 = b - a0 (A d - mean(A d)) is the true fp32
// residual, and CG goes on from it exactly as from r0 = b.  A sample whose d.A d is not > 0 or whose dot products are not finite (a
// zero, NaN or Inf guess) is held out of that step and runs the cold solve bit for bit.  Without a guess nothing is added or changed.
#include "fnx_device.h"
#include "fnx_kernels.h"
#include "../../include/fluidnet_hip.h"
#include <stdio.h>
#include <vector>

namespace fnx {
namespace {

constexpr int kMaxLevels = 16;
constexpr int kSmallCells = 4096;     // levels at most this big (per sample) run in the one-workgroup launch
constexpr int kSmallThreads = 1024;
constexpr int kCoarsestSweeps = 16;   // even: the last sweep writes x
constexpr int kRed = 256;             // threads of the reduction and finalize launches
constexpr int kMaxBlk = 4096;         // workgroups per sample of a reduction launch (fixed by the grid: deterministic); 1024 left the
                                      // 256^3 direction kernel at 16 waves per CU and 5.5x its bandwidth time
constexpr int kNQ = 3;                // quantities per partial-sum slot
constexpr int kCheckEvery = 4;        // pcg_tol > 0: iterations between two host reads of the stop flag
constexpr float kOmega = 2.f / 3.f;
constexpr float kCorr = 1.8f;

// level-0 code bits
enum : unsigned {
  C_DOF = 1u, C_XM = 2u, C_XP = 4u, C_YM = 8u, C_YP = 16u, C_ZM = 32u, C_ZP = 64u,  // coupled to the active -x .. +z neighbour
  C_NSUB_SHIFT = 7u,                                                                   // 3 bits: Neumann (substituted) neighbours
  C_DIR = 1u << 10                                                                     // has a Dirichlet neighbour (row sum > 0)
};

struct LevelDev {
  int D, H, W, N;                 // per-sample dims of the level
  const unsigned short* code;     // level 0: per-cell code, else null
  const float4* op;               // levels >= 1: (diag, w_-x, w_-y, w_-z); diag < 0 marks a cell without fine degrees of freedom
  float* x; float* b; float* t;   // iterate, right-hand side, ping-pong partner (B * N floats each)
  float denom;
};
struct LevelSet { LevelDev lv[kMaxLevels]; int L; };

struct PcgScalars {
  double n, bnorm, rz, mean, xmean;
  float alpha, beta, mAp, zmean, relres, best;
  int singular, done, iters, converged;
};
struct PcgGlobal { float res; int all_done; };

enum { FIN_INIT = 0, FIN_BNORM, FIN_RZ0, FIN_ALPHA, FIN_CHECK, FIN_BETA, FIN_XMEAN, FIN_GUESS, FIN_START };
constexpr int kHeld = 2;              // PcgScalars.done between FIN_GUESS and FIN_START: the guess was rejected, the line-search step skips the sample

// ---- the operator ------------------------------------------------------------------------------------

__device__ __forceinline__ bool is_border_cell(const GridDims& g, bool is3d, int i, int j, int k) {
  return i == 0 || i == g.W - 1 || j == 0 || j == g.H - 1 || (is3d && (k == 0 || k == g.D - 1));
}

// level-0 code of cell (i, j, k) of one sample (`f`: that sample's flags)
__device__ __forceinline__ unsigned cell_code(const GridDims& g, bool is3d, bool quirks, const float* f, int i, int j, int k) {
  const int c = k * g.HW + j * g.W + i;
  if (is_border_cell(g, is3d, i, j, k) || f[c] == FNX_OBST) return 0u;
  unsigned m = C_DOF, nsub = 0;
  bool dir = false;
  auto nb = [&](int q, int ni, int nj, int nk, bool zdir, unsigned bit) {
    if (f[q] == FNX_OBST) {
      if (zdir && quirks) dir = true;              // Q13: p of the obstacle (0) instead of p_i
      else ++nsub;
    } else if (is_border_cell(g, is3d, ni, nj, nk)) {
      dir = true;                                  // border cells are held at 0
    } else {
      m |= bit;
    }
  };
  nb(c - 1, i - 1, j, k, false, C_XM);
  nb(c + 1, i + 1, j, k, false, C_XP);
  nb(c - g.W, i, j - 1, k, false, C_YM);
  nb(c + g.W, i, j + 1, k, false, C_YP);
  if (is3d) {
    nb(c - g.HW, i, j, k - 1, true, C_ZM);
    nb(c + g.HW, i, j, k + 1, true, C_ZP);
  }
  return m | (nsub << C_NSUB_SHIFT) | (dir ? (unsigned)C_DIR : 0u);
}

struct St { float d, xm, xp, ym, yp, zm, zp; bool dof; };

__device__ __forceinline__ St code_stencil(unsigned m, float denom) {
  St s;
  s.dof = (m & C_DOF) != 0;
  s.d = s.dof ? denom - (float)((m >> C_NSUB_SHIFT) & 7u) : 0.f;
  s.xm = (m & C_XM) ? 1.f : 0.f; s.xp = (m & C_XP) ? 1.f : 0.f;
  s.ym = (m & C_YM) ? 1.f : 0.f; s.yp = (m & C_YP) ? 1.f : 0.f;
  s.zm = (m & C_ZM) ? 1.f : 0.f; s.zp = (m & C_ZP) ? 1.f : 0.f;
  return s;
}

__device__ __forceinline__ St stencil_at(const LevelDev& L, size_t base, int c, int i, int j, int k) {
  if (L.code) return code_stencil(L.code[base + c], L.denom);
  St s;
  const float4 o = L.op[base + c];
  s.dof = o.x >= 0.f; s.d = fmaxf(o.x, 0.f);
  s.xm = o.y; s.ym = o.z; s.zm = o.w;
  s.xp = i + 1 < L.W ? L.op[base + c + 1].y : 0.f;
  s.yp = j + 1 < L.H ? L.op[base + c + L.W].z : 0.f;
  s.zp = k + 1 < L.D ? L.op[base + c + (size_t)L.H * L.W].w : 0.f;
  return s;
}

__device__ __forceinline__ bool dof_at(const LevelDev& L, size_t base, int c) {
  return L.code ? (L.code[base + c] & C_DOF) != 0 : L.op[base + c].x >= 0.f;
}

// (A x)_c; x is the sample's vector.  A weight is only non-zero towards an existing neighbour.
__device__ __forceinline__ float apply_st(const St& s, const float* x, int c, int W, int HW) {
  if (!s.dof) return 0.f;
  float y = s.d * x[c];
  if (s.xm != 0.f) y -= s.xm * x[c - 1];
  if (s.xp != 0.f) y -= s.xp * x[c + 1];
  if (s.ym != 0.f) y -= s.ym * x[c - W];
  if (s.yp != 0.f) y -= s.yp * x[c + W];
  if (s.zm != 0.f) y -= s.zm * x[c - HW];
  if (s.zp != 0.f) y -= s.zp * x[c + HW];
  return y;
}

__device__ __forceinline__ void decode(const LevelDev& L, int c, int& i, int& j, int& k) {
  i = c % L.W; j = (c / L.W) % L.H; k = c / (L.W * L.H);
}

// ---- V-cycle phases, one cell each -----------------------------------------------------------------------

// one damped-Jacobi sweep xin -> xout (xin null: from zero)
__device__ __forceinline__ void smooth_cell(const LevelDev& L, int b, int c, const float* xin, float* xout) {
  const size_t base = (size_t)b * L.N;
  int i, j, k; decode(L, c, i, j, k);
  const St s = stencil_at(L, base, c, i, j, k);
  float v = 0.f;
  if (s.dof) {
    if (xin) {
      const float* xs = xin + base;
      v = xs[c];
      if (s.d > 0.f) v = v + kOmega * (L.b[base + c] - apply_st(s, xs, c, L.W, L.H * L.W)) / s.d;
    } else if (s.d > 0.f) {
      v = kOmega * L.b[base + c] / s.d;
    }
  }
  xout[base + c] = v;
}

// coarse right-hand side = P^T (b - A x) of the finer level: the residuals of the aggregate's children, summed in a fixed order
__device__ __forceinline__ void restrict_cell(const LevelDev& F, const LevelDev& C, bool is3d, int b, int c) {
  const size_t fb = (size_t)b * F.N, cb = (size_t)b * C.N;
  int I, J, K; decode(C, c, I, J, K);
  float sum = 0.f;
  const int nk = is3d ? 2 : 1;
  for (int dk = 0; dk < nk; ++dk)
    for (int dj = 0; dj < 2; ++dj)
      for (int di = 0; di < 2; ++di) {
        const int i = 2 * I + di, j = 2 * J + dj, k = is3d ? 2 * K + dk : K;
        if (i >= F.W || j >= F.H || k >= F.D) continue;
        const int fc = (k * F.H + j) * F.W + i;
        const St s = stencil_at(F, fb, fc, i, j, k);
        if (s.dof) sum += F.b[fb + fc] - apply_st(s, F.x + fb, fc, F.W, F.H * F.W);
      }
  C.b[cb + c] = sum;
}

// x += c P x_coarse on the degrees of freedom
__device__ __forceinline__ void prolong_cell(const LevelDev& F, const LevelDev& C, bool is3d, int b, int c) {
  const size_t fb = (size_t)b * F.N, cb = (size_t)b * C.N;
  if (!dof_at(F, fb, c)) return;
  int i, j, k; decode(F, c, i, j, k);
  const int cc = ((is3d ? k / 2 : k) * C.H + j / 2) * C.W + i / 2;
  F.x[fb + c] = F.x[fb + c] + kCorr * C.x[cb + cc];
}

// Galerkin coarse operator of one aggregate: diag = sum of the children's diagonals - 2 x the couplings inside the aggregate,
// face weight = sum of the children's couplings across the aggregate's lower face
__device__ __forceinline__ float4 coarsen_cell(const LevelDev& F, const LevelDev& C, bool is3d, int b, int c) {
  const size_t fb = (size_t)b * F.N;
  int I, J, K; decode(C, c, I, J, K);
  float d = 0.f, wx = 0.f, wy = 0.f, wz = 0.f;
  bool any = false;
  const int nk = is3d ? 2 : 1;
  for (int dk = 0; dk < nk; ++dk)
    for (int dj = 0; dj < 2; ++dj)
      for (int di = 0; di < 2; ++di) {
        const int i = 2 * I + di, j = 2 * J + dj, k = is3d ? 2 * K + dk : K;
        if (i >= F.W || j >= F.H || k >= F.D) continue;
        const St s = stencil_at(F, fb, (k * F.H + j) * F.W + i, i, j, k);
        if (!s.dof) continue;
        any = true;
        d += s.d;
        if (di == 1) d -= 2.f * s.xm; else wx += s.xm;
        if (dj == 1) d -= 2.f * s.ym; else wy += s.ym;
        if (is3d) { if (dk == 1) d -= 2.f * s.zm; else wz += s.zm; }
      }
  return any ? make_float4(d, wx, wy, wz) : make_float4(-1.f, 0.f, 0.f, 0.f);
}

// ---- kernels -------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void pcg_code_kernel(GridDims g, int is3d, int quirks, const float* __restrict__ flags,
                                                       unsigned short* __restrict__ code) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)g.B * g.DHW) return;
  const int b = (int)(idx / g.DHW), c = (int)(idx % g.DHW);
  const int i = c % g.W, j = (c / g.W) % g.H, k = c / g.HW;
  code[idx] = (unsigned short)cell_code(g, is3d != 0, quirks != 0, flags + (size_t)b * g.DHW, i, j, k);
}

__global__ __launch_bounds__(256) void pcg_coarsen_kernel(LevelDev F, LevelDev C, int is3d, int B, float4* __restrict__ op) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)B * C.N) return;
  op[idx] = coarsen_cell(F, C, is3d != 0, (int)(idx / C.N), (int)(idx % C.N));
}

// y = A x straight from flags (fnx_poisson_apply: no workspace)
__global__ __launch_bounds__(256) void pcg_apply_flags_kernel(GridDims g, int is3d, int quirks, const float* __restrict__ flags,
                                                              const float* __restrict__ x, float* __restrict__ y) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)g.B * g.DHW) return;
  const int b = (int)(idx / g.DHW), c = (int)(idx % g.DHW);
  const int i = c % g.W, j = (c / g.W) % g.H, k = c / g.HW;
  const size_t base = (size_t)b * g.DHW;
  const St s = code_stencil(cell_code(g, is3d != 0, quirks != 0, flags + base, i, j, k), is3d ? 6.f : 4.f);
  y[idx] = apply_st(s, x + base, c, g.W, g.HW);
}

__device__ __forceinline__ bool sample_done(const PcgScalars* sc, int b) { return sc && sc[b].done; }

__global__ __launch_bounds__(256) void pcg_smooth_kernel(LevelDev L, int B, const float* xin, float* xout, const PcgScalars* sc) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)B * L.N) return;
  const int b = (int)(idx / L.N);
  if (sample_done(sc, b)) return;
  smooth_cell(L, b, (int)(idx % L.N), xin, xout);
}

__global__ __launch_bounds__(256) void pcg_restrict_kernel(LevelDev F, LevelDev C, int is3d, int B, const PcgScalars* sc) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)B * C.N) return;
  const int b = (int)(idx / C.N);
  if (sample_done(sc, b)) return;
  restrict_cell(F, C, is3d != 0, b, (int)(idx % C.N));
}

__global__ __launch_bounds__(256) void pcg_prolong_kernel(LevelDev F, LevelDev C, int is3d, int B, const PcgScalars* sc) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)B * F.N) return;
  const int b = (int)(idx / F.N);
  if (sample_done(sc, b)) return;
  prolong_cell(F, C, is3d != 0, b, (int)(idx % F.N));
}

// the V-cycle from level l0 down to the coarsest and back, one workgroup per sample
__global__ __launch_bounds__(kSmallThreads) void pcg_vcycle_small_kernel(LevelSet S, int l0, int is3d, const PcgScalars* sc) {
  const int b = blockIdx.x;
  if (sample_done(sc, b)) return;
  const int tid = threadIdx.x;
  const bool z3 = is3d != 0;
  for (int l = l0; l < S.L - 1; ++l) {
    const LevelDev& L = S.lv[l];
    for (int c = tid; c < L.N; c += kSmallThreads) smooth_cell(L, b, c, nullptr, L.t);
    __syncthreads();
    for (int c = tid; c < L.N; c += kSmallThreads) smooth_cell(L, b, c, L.t, L.x);
    __syncthreads();
    const LevelDev& C = S.lv[l + 1];
    for (int c = tid; c < C.N; c += kSmallThreads) restrict_cell(L, C, z3, b, c);
    __syncthreads();
  }
  {
    const LevelDev& L = S.lv[S.L - 1];
    for (int sw = 0; sw < kCoarsestSweeps; sw += 2) {
      for (int c = tid; c < L.N; c += kSmallThreads) smooth_cell(L, b, c, sw == 0 ? nullptr : L.x, L.t);
      __syncthreads();
      for (int c = tid; c < L.N; c += kSmallThreads) smooth_cell(L, b, c, L.t, L.x);
      __syncthreads();
    }
  }
  for (int l = S.L - 2; l >= l0; --l) {
    const LevelDev& L = S.lv[l];
    for (int c = tid; c < L.N; c += kSmallThreads) prolong_cell(L, S.lv[l + 1], z3, b, c);
    __syncthreads();
    for (int c = tid; c < L.N; c += kSmallThreads) smooth_cell(L, b, c, L.x, L.t);
    __syncthreads();
    for (int c = tid; c < L.N; c += kSmallThreads) smooth_cell(L, b, c, L.t, L.x);
    __syncthreads();
  }
}

// ---- CG vector kernels: grid (nblk, B), a fixed cell -> workgroup map, fp64 partials per workgroup --------------------

template <int NQ>
__device__ __forceinline__ void store_partials(double (&v)[NQ], double* part, int b, int nblk) {
  __shared__ double sh[NQ][kRed / 64];
#pragma unroll
  for (int q = 0; q < NQ; ++q)
    for (int off = 32; off > 0; off >>= 1) v[q] += __shfl_xor(v[q], off);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0)
    for (int q = 0; q < NQ; ++q) sh[q][w] = v[q];
  __syncthreads();
  if (threadIdx.x == 0)
    for (int q = 0; q < NQ; ++q) part[((size_t)b * kNQ + q) * nblk + blockIdx.x] = ((sh[q][0] + sh[q][1]) + sh[q][2]) + sh[q][3];
}

#define PCG_CELL_LOOP(c, N) for (int c = blockIdx.x * kRed + threadIdx.x; c < (N); c += gridDim.x * kRed)

// sum of div, number of degrees of freedom, number of them with a Dirichlet neighbour
__global__ __launch_bounds__(kRed) void pcg_init_kernel(LevelDev L, const float* __restrict__ div, double* part) {
  const int b = blockIdx.y;
  const size_t base = (size_t)b * L.N;
  double v[3] = {0.0, 0.0, 0.0};
  PCG_CELL_LOOP(c, L.N) {
    const unsigned m = L.code[base + c];
    if (m & C_DOF) { v[0] += (double)div[base + c]; v[1] += 1.0; if (m & C_DIR) v[2] += 1.0; }
  }
  store_partials<3>(v, part, b, gridDim.x);
}

// r = div - mean (singular samples) on the degrees of freedom, 0 elsewhere; x = 0; sum r^2
__global__ __launch_bounds__(kRed) void pcg_rhs_kernel(LevelDev L, const float* __restrict__ div, const PcgScalars* sc,
                                                       float* __restrict__ r, float* __restrict__ x, double* part) {
  const int b = blockIdx.y;
  const size_t base = (size_t)b * L.N;
  const double mean = sc[b].mean;
  double v[1] = {0.0};
  PCG_CELL_LOOP(c, L.N) {
    const float rv = (L.code[base + c] & C_DOF) ? (float)((double)div[base + c] - mean) : 0.f;
    r[base + c] = rv; x[base + c] = 0.f;
    v[0] += (double)rv * rv;
  }
  store_partials<1>(v, part, b, gridDim.x);
}

// sum x over the degrees of freedom
__global__ __launch_bounds__(kRed) void pcg_sum_kernel(LevelDev L, const float* __restrict__ x, double* part) {
  const int b = blockIdx.y;
  const size_t base = (size_t)b * L.N;
  double v[1] = {0.0};
  PCG_CELL_LOOP(c, L.N) {
    if (L.code[base + c] & C_DOF) v[0] += (double)x[base + c];
  }
  store_partials<1>(v, part, b, gridDim.x);
}

// r.z, sum z and sum r over the degrees of freedom: on singular samples z is used with its mean removed (below)
__global__ __launch_bounds__(kRed) void pcg_rz_kernel(LevelDev L, const float* __restrict__ r, const float* __restrict__ z,
                                                      const PcgScalars* sc, double* part) {
  const int b = blockIdx.y;
  const size_t base = (size_t)b * L.N;
  double v[3] = {0.0, 0.0, 0.0};
  if (!sc[b].done) {
    PCG_CELL_LOOP(c, L.N) {
      if (!(L.code[base + c] & C_DOF)) continue;
      const double rv = r[base + c], zv = z[base + c];
      v[0] += rv * zv; v[1] += zv; v[2] += rv;
    }
  }
  store_partials<3>(v, part, b, gridDim.x);
}

// p_new = (z - mean z) + beta p_old (first: z - mean z), Ap = A p_new; sums p.Ap and Ap (the latter keeps r mean-zero on singular
// samples).  mean z is 0 on regular samples.  On singular ones the V-cycle's coarse levels integrate rounding into a constant
// component of z that grows against z's variation as r shrinks; left in p, A p then cancels catastrophically in fp32 and CG breaks
// down (measured: the 1024^2 plume stalled at 3.8e-3).  Removing it is Q M^-1 Q on mean-zero r: still symmetric.
__global__ __launch_bounds__(kRed) void pcg_dir_apply_kernel(LevelDev L, const float* __restrict__ z, const float* __restrict__ p_old,
                                                             float* __restrict__ p_new, float* __restrict__ Ap, const PcgScalars* sc,
                                                             int first, double* part) {
  const int b = blockIdx.y;
  const size_t base = (size_t)b * L.N;
  double v[2] = {0.0, 0.0};
  if (!sc[b].done) {
    const float beta = first ? 0.f : sc[b].beta, zm = sc[b].zmean;
    const float* zs = z + base;
    const float* ps = p_old + base;
    auto P = [&](int q) { return first ? zs[q] - zm : (zs[q] - zm) + beta * ps[q]; };
    const int W = L.W, HW = L.H * L.W;
    PCG_CELL_LOOP(c, L.N) {
      const St s = code_stencil(L.code[base + c], L.denom);
      if (!s.dof) { p_new[base + c] = 0.f; Ap[base + c] = 0.f; continue; }
      const float pc = P(c);
      float y = s.d * pc;
      if (s.xm != 0.f) y -= P(c - 1);
      if (s.xp != 0.f) y -= P(c + 1);
      if (s.ym != 0.f) y -= P(c - W);
      if (s.yp != 0.f) y -= P(c + W);
      if (s.zm != 0.f) y -= P(c - HW);
      if (s.zp != 0.f) y -= P(c + HW);
      p_new[base + c] = pc; Ap[base + c] = y;
      v[0] += (double)pc * y; v[1] += (double)y;
    }
  }
  store_partials<2>(v, part, b, gridDim.x);
}

// the warm start's direction: d = x0 on the degrees of freedom, 0 elsewhere, and Ap = A d; sums d.b, d.Ap and Ap, b the projected
// right-hand side pcg_rhs_kernel forms (div - mean).  Runs BEFORE pcg_rhs_kernel, which zeroes x: x0 may be x.
__global__ __launch_bounds__(kRed) void pcg_guess_kernel(LevelDev L, const float* __restrict__ x0, const float* __restrict__ div,
                                                         float* __restrict__ d, float* __restrict__ Ap, const PcgScalars* sc, double* part) {
  const int b = blockIdx.y;
  const size_t base = (size_t)b * L.N;
  const double mean = sc[b].mean;
  const float* xs = x0 + base;
  const int W = L.W, HW = L.H * L.W;
  double v[3] = {0.0, 0.0, 0.0};
  PCG_CELL_LOOP(c, L.N) {
    const St s = code_stencil(L.code[base + c], L.denom);
    if (!s.dof) { d[base + c] = 0.f; Ap[base + c] = 0.f; continue; }
    const float dc = xs[c];
    float y = s.d * dc;                               // (a weight is only non-zero towards a degree of freedom)
    if (s.xm != 0.f) y -= xs[c - 1];
    if (s.xp != 0.f) y -= xs[c + 1];
    if (s.ym != 0.f) y -= xs[c - W];
    if (s.yp != 0.f) y -= xs[c + W];
    if (s.zm != 0.f) y -= xs[c - HW];
    if (s.zp != 0.f) y -= xs[c + HW];
    d[base + c] = dc; Ap[base + c] = y;
    const float bv = (float)((double)div[base + c] - mean);
    v[0] += (double)dc * bv; v[1] += (double)dc * y; v[2] += (double)y;
  }
  store_partials<3>(v, part, b, gridDim.x);
}

// x += alpha p, r -= alpha (Ap - mean(Ap)); sum r^2
__global__ __launch_bounds__(kRed) void pcg_update_kernel(LevelDev L, const float* __restrict__ p, const float* __restrict__ Ap,
                                                          float* __restrict__ x, float* __restrict__ r, const PcgScalars* sc, double* part) {
  const int b = blockIdx.y;
  const size_t base = (size_t)b * L.N;
  double v[1] = {0.0};
  if (!sc[b].done) {
    const float alpha = sc[b].alpha, mAp = sc[b].mAp;
    PCG_CELL_LOOP(c, L.N) {
      if (!(L.code[base + c] & C_DOF)) continue;
      x[base + c] = x[base + c] + alpha * p[base + c];
      const float rv = r[base + c] - alpha * (Ap[base + c] - mAp);
      r[base + c] = rv;
      v[0] += (double)rv * rv;
    }
  }
  store_partials<1>(v, part, b, gridDim.x);
}

// singular samples: x -= its mean over the degrees of freedom
__global__ __launch_bounds__(256) void pcg_shift_kernel(LevelDev L, int B, float* __restrict__ x, const PcgScalars* sc) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)B * L.N) return;
  const int b = (int)(idx / L.N);
  if (!sc[b].singular || !(L.code[idx] & C_DOF)) return;
  x[idx] = x[idx] - (float)sc[b].xmean;
}

__device__ double sum_partials(const double* p, int n, double* sh) {
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < n; i += kRed) s += p[i];
  sh[tid] = s;
  __syncthreads();
  for (int w = kRed / 2; w > 0; w >>= 1) {
    if (tid < w) sh[tid] = sh[tid] + sh[tid + w];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// the scalar part of a CG step, all samples in one workgroup
__global__ __launch_bounds__(kRed) void pcg_finalize_kernel(int mode, int B, int nblk, const double* part, PcgScalars* sc, PcgGlobal* gl,
                                                            float tol, float* residual) {
  __shared__ double sh[kRed];
  __shared__ double q[kNQ];
  const int nq = (mode == FIN_INIT || mode == FIN_RZ0 || mode == FIN_BETA) ? 3 : (mode == FIN_ALPHA ? 2 : 1);
  for (int b = 0; b < B; ++b) {
    for (int k = 0; k < nq; ++k) {
      const double s = sum_partials(part + ((size_t)b * kNQ + k) * nblk, nblk, sh);
      if (threadIdx.x == 0) q[k] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      PcgScalars& S = sc[b];
      switch (mode) {
        case FIN_INIT:
          S.n = q[1];
          S.singular = q[1] > 0.0 && q[2] == 0.0;            // no degree of freedom touches a Dirichlet cell: constants are null vectors
          S.mean = S.singular ? q[0] / q[1] : 0.0;
          S.done = 0; S.iters = 0; S.converged = 0; S.relres = 0.f;
          S.alpha = S.beta = S.mAp = S.zmean = 0.f; S.rz = 0.0; S.xmean = 0.0; S.best = 1.f;
          break;
        case FIN_BNORM:
          S.bnorm = sqrt(q[0]);
          if (!(S.bnorm > 0.0) || !isfinite(S.bnorm)) {     // b = 0: x = 0 is the answer
            S.done = 1; S.converged = S.bnorm == 0.0; S.relres = S.bnorm == 0.0 ? 0.f : NAN;
          } else {
            S.relres = 1.f;
          }
          break;
        case FIN_RZ0:
        case FIN_BETA: {
          if (S.done) break;
          // r.(z - mean z) = r.z - mean z * sum r
          const double zm = S.singular ? q[1] / S.n : 0.0;
          const double rz = q[0] - zm * q[2];
          if (!(rz > 0.0) || !isfinite(rz)) { S.done = 1; break; }
          S.zmean = (float)zm;
          if (mode == FIN_BETA) S.beta = (float)(rz / S.rz);
          S.rz = rz;
          break;
        }
        case FIN_ALPHA:
          if (S.done) break;
          if (!(q[0] > 0.0) || !isfinite(q[0])) { S.done = 1; break; }
          S.alpha = (float)(S.rz / q[0]);
          S.mAp = S.singular ? (float)(q[1] / S.n) : 0.f;
          break;
        case FIN_CHECK:
          if (S.done) break;
          ++S.iters;
          S.relres = (float)(sqrt(q[0]) / S.bnorm);
          if (tol > 0.f && S.relres <= tol) { S.done = 1; S.converged = 1; }
          else if (!isfinite(S.relres) || S.relres > 100.f * S.best) S.done = 1;   // diverging: an inconsistent system (sealed pocket)
          if (S.relres < S.best) S.best = S.relres;
          break;
        case FIN_XMEAN:
          S.xmean = S.singular ? q[0] / S.n : 0.0;
          break;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && mode != FIN_INIT && mode != FIN_XMEAN) {
    int all = 1; float mx = 0.f;
    for (int b = 0; b < B; ++b) {
      all &= sc[b].done;
      const float r = sc[b].relres;
      if (!(r <= mx)) mx = r;                                 // NaN propagates
    }
    gl->all_done = all; gl->res = mx;
    if (residual) *residual = mx;
  }
}

// the scalar part of the warm start (pcg_finalize_kernel is the cold solve's and stays as it is).  FIN_GUESS, behind FIN_INIT: alpha =
// a0 = d.b / d.Ad and mAp, or the guess is rejected.  FIN_START, behind the line-search step's pcg_update_kernel: FIN_CHECK without the
// iteration count; like FIN_CHECK it publishes the batch's stop flag and residual.
__global__ __launch_bounds__(kRed) void pcg_finalize_guess_kernel(int mode, int B, int nblk, const double* part, PcgScalars* sc, PcgGlobal* gl,
                                                                  float tol, float* residual) {
  __shared__ double sh[kRed];
  __shared__ double q[kNQ];
  const int nq = mode == FIN_GUESS ? 3 : 1;
  for (int b = 0; b < B; ++b) {
    for (int k = 0; k < nq; ++k) {
      const double s = sum_partials(part + ((size_t)b * kNQ + k) * nblk, nblk, sh);
      if (threadIdx.x == 0) q[k] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      PcgScalars& S = sc[b];
      if (mode == FIN_GUESS) {
        const float a0 = (float)(q[0] / q[1]);
        const float m = S.singular ? (float)(q[2] / S.n) : 0.f;
        if (!(q[1] > 0.0) || !isfinite(q[0]) || !isfinite(q[1]) || !isfinite(a0) || !isfinite(m)) S.done = kHeld;
        else { S.alpha = a0; S.mAp = m; }
      } else if (S.done == kHeld) {
        S.done = 0;                                           // rejected: x = 0, r = b, relres 1 as FIN_BNORM left them
      } else if (!S.done) {
        S.relres = (float)(sqrt(q[0]) / S.bnorm);
        if (tol > 0.f && S.relres <= tol) { S.done = 1; S.converged = 1; }
        else if (!isfinite(S.relres)) S.done = 1;
        if (S.relres < S.best) S.best = S.relres;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && mode == FIN_START) {
    int all = 1; float mx = 0.f;
    for (int b = 0; b < B; ++b) {
      all &= sc[b].done;
      const float r = sc[b].relres;
      if (!(r <= mx)) mx = r;                                 // NaN propagates
    }
    gl->all_done = all; gl->res = mx;
    if (residual) *residual = mx;
  }
}

// ---- host side --------------------------------------------------------------------------------------------

struct Hier { int L, ls; int D[kMaxLevels], H[kMaxLevels], W[kMaxLevels], N[kMaxLevels]; };

Hier make_hier(const GridDims& g, bool is3d) {
  Hier h{};
  int D = g.D, H = g.H, W = g.W;
  h.D[0] = D; h.H[0] = H; h.W[0] = W; h.N[0] = D * H * W; h.L = 1;
  while (h.L < kMaxLevels && (W > 4 || H > 4 || (is3d && D > 4))) {
    W = (W + 1) / 2; H = (H + 1) / 2;
    if (is3d) D = (D + 1) / 2;
    h.D[h.L] = D; h.H[h.L] = H; h.W[h.L] = W; h.N[h.L] = D * H * W; ++h.L;
  }
  h.ls = h.L - 1;
  for (int l = 0; l < h.L; ++l)
    if (h.N[l] <= kSmallCells) { h.ls = l; break; }
  return h;
}

inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }
inline int nblk_of(int N) { const int n = (N + kRed - 1) / kRed; return n < kMaxBlk ? n : kMaxBlk; }
inline unsigned grid1(size_t n) { return (unsigned)((n + 255) / 256); }

struct Carve {
  char* p; size_t off;
  void* take(size_t bytes) { void* r = p ? p + off : nullptr; off += al(bytes); return r; }
};

struct Kept { unsigned short* code; float4* op[kMaxLevels]; };
Kept carve_kept(const Hier& h, int B, void* base, size_t* bytes) {
  Carve c{(char*)base, 0};
  Kept k{};
  k.code = (unsigned short*)c.take((size_t)B * h.N[0] * 2);
  for (int l = 1; l < h.L; ++l) k.op[l] = (float4*)c.take((size_t)B * h.N[l] * 16);
  *bytes = c.off;
  return k;
}

struct Scratch {
  float* x[kMaxLevels]; float* b[kMaxLevels]; float* t[kMaxLevels];
  float *r, *z, *pA, *pB, *Ap;
  double* part; PcgScalars* sc; PcgGlobal* gl;
};
Scratch carve_scratch(const Hier& h, int B, void* base, size_t* bytes) {
  Carve c{(char*)base, 0};
  Scratch s{};
  const size_t n0 = (size_t)B * h.N[0] * 4;
  s.t[0] = (float*)c.take(n0);
  for (int l = 1; l < h.L; ++l) {
    const size_t n = (size_t)B * h.N[l] * 4;
    s.x[l] = (float*)c.take(n); s.b[l] = (float*)c.take(n); s.t[l] = (float*)c.take(n);
  }
  s.r = (float*)c.take(n0); s.z = (float*)c.take(n0); s.pA = (float*)c.take(n0); s.pB = (float*)c.take(n0);
  s.Ap = (float*)c.take(n0);
  s.part = (double*)c.take((size_t)B * kNQ * kMaxBlk * 8);
  s.sc = (PcgScalars*)c.take((size_t)B * sizeof(PcgScalars));
  s.gl = (PcgGlobal*)c.take(sizeof(PcgGlobal));
  *bytes = c.off;
  return s;
}

LevelSet level_set(const Hier& h, bool is3d, const Kept& k, const Scratch& s, const float* r, float* z) {
  LevelSet S{};
  S.L = h.L;
  for (int l = 0; l < h.L; ++l) {
    LevelDev& L = S.lv[l];
    L.D = h.D[l]; L.H = h.H[l]; L.W = h.W[l]; L.N = h.N[l];
    L.denom = is3d ? 6.f : 4.f;
    if (l == 0) { L.code = k.code; L.x = z; L.b = const_cast<float*>(r); L.t = s.t[0]; }
    else { L.op = k.op[l]; L.x = s.x[l]; L.b = s.b[l]; L.t = s.t[l]; }
  }
  return S;
}

void vcycle(const LevelSet& S, int ls, bool is3d, int B, const PcgScalars* sc, hipStream_t st) {
  for (int l = 0; l < ls; ++l) {
    const LevelDev& L = S.lv[l];
    const unsigned gl = grid1((size_t)B * L.N);
    pcg_smooth_kernel<<<gl, 256, 0, st>>>(L, B, nullptr, L.t, sc);
    pcg_smooth_kernel<<<gl, 256, 0, st>>>(L, B, L.t, L.x, sc);
    pcg_restrict_kernel<<<grid1((size_t)B * S.lv[l + 1].N), 256, 0, st>>>(L, S.lv[l + 1], is3d ? 1 : 0, B, sc);
  }
  pcg_vcycle_small_kernel<<<B, kSmallThreads, 0, st>>>(S, ls, is3d ? 1 : 0, sc);
  for (int l = ls - 1; l >= 0; --l) {
    const LevelDev& L = S.lv[l];
    const unsigned gl = grid1((size_t)B * L.N);
    pcg_prolong_kernel<<<gl, 256, 0, st>>>(L, S.lv[l + 1], is3d ? 1 : 0, B, sc);
    pcg_smooth_kernel<<<gl, 256, 0, st>>>(L, B, L.x, L.t, sc);
    pcg_smooth_kernel<<<gl, 256, 0, st>>>(L, B, L.t, L.x, sc);
  }
}

#define PCG_HIP(expr)                                                                                      \
  do {                                                                                                     \
    hipError_t e_ = (expr);                                                                                \
    if (e_ != hipSuccess) return set_error(FNX_EHIP, "HIP error: %s (%s)", hipGetErrorString(e_), #expr); \
  } while (0)

}  // namespace

size_t pcg_kept_bytes(const GridDims& g, bool is3d) {
  size_t n = 0;
  carve_kept(make_hier(g, is3d), g.B, nullptr, &n);
  return n;
}

size_t pcg_scratch_bytes(const GridDims& g, bool is3d) {
  size_t n = 0;
  carve_scratch(make_hier(g, is3d), g.B, nullptr, &n);
  return n;
}

void launch_pcg_build(const GridDims& g, bool is3d, bool quirks, const float* flags, void* kept, hipStream_t s) {
  const Hier h = make_hier(g, is3d);
  size_t nb;
  const Kept k = carve_kept(h, g.B, kept, &nb);
  pcg_code_kernel<<<grid1((size_t)g.B * g.DHW), 256, 0, s>>>(g, is3d ? 1 : 0, quirks ? 1 : 0, flags, k.code);
  const Scratch none{};
  const LevelSet S = level_set(h, is3d, k, none, nullptr, nullptr);
  for (int l = 1; l < h.L; ++l)
    pcg_coarsen_kernel<<<grid1((size_t)g.B * h.N[l]), 256, 0, s>>>(S.lv[l - 1], S.lv[l], is3d ? 1 : 0, g.B, k.op[l]);
}

void launch_poisson_apply(const GridDims& g, bool is3d, bool quirks, const float* flags, const float* x, float* y, hipStream_t s) {
  pcg_apply_flags_kernel<<<grid1((size_t)g.B * g.DHW), 256, 0, s>>>(g, is3d ? 1 : 0, quirks ? 1 : 0, flags, x, y);
}

void launch_pcg_precondition(const GridDims& g, bool is3d, const void* kept, void* scratch, const float* r, float* z, hipStream_t s) {
  const Hier h = make_hier(g, is3d);
  size_t nb;
  const Kept k = carve_kept(h, g.B, const_cast<void*>(kept), &nb);
  const Scratch sc = carve_scratch(h, g.B, scratch, &nb);
  vcycle(level_set(h, is3d, k, sc, r, z), h.ls, is3d, g.B, nullptr, s);
}

int pcg_solve(const GridDims& g, bool is3d, const void* kept, void* scratch, const float* div, const float* p0, float* p, float* residual,
              float tol, int max_iter, int* iters_done, bool verbose, hipStream_t st) {
  const Hier h = make_hier(g, is3d);
  const int B = g.B, N = h.N[0], nblk = nblk_of(N);
  size_t nb;
  const Kept k = carve_kept(h, B, const_cast<void*>(kept), &nb);
  const Scratch s = carve_scratch(h, B, scratch, &nb);
  const LevelSet S = level_set(h, is3d, k, s, s.r, s.z);
  const LevelDev& L0 = S.lv[0];
  const dim3 rg(nblk, B);
  auto fin = [&](int mode) { pcg_finalize_kernel<<<1, kRed, 0, st>>>(mode, B, nblk, s.part, s.sc, s.gl, tol, residual); };
  auto fin_guess = [&](int mode) { pcg_finalize_guess_kernel<<<1, kRed, 0, st>>>(mode, B, nblk, s.part, s.sc, s.gl, tol, residual); };
  // b = div projected onto the range of A where constants are null vectors; x (= p) = 0
  pcg_init_kernel<<<rg, kRed, 0, st>>>(L0, div, s.part);
  fin(FIN_INIT);
  // the guess is read before anything writes p (p0 may be p): d -> pA (free until the first direction lands in pB), A d -> Ap
  if (p0) {
    pcg_guess_kernel<<<rg, kRed, 0, st>>>(L0, p0, div, s.pA, s.Ap, s.sc, s.part);
    fin_guess(FIN_GUESS);
  }
  pcg_rhs_kernel<<<rg, kRed, 0, st>>>(L0, div, s.sc, s.r, p, s.part);
  fin(FIN_BNORM);
  float* P[2] = {s.pA, s.pB};
  int it = 0;
  PcgGlobal hg{0.f, 0};
  bool run = max_iter > 0;
  if (p0) {
    // x = a0 d, r = b - a0 (A d - mean(A d)): the update of a CG step, skipped by the samples FIN_GUESS holds
    pcg_update_kernel<<<rg, kRed, 0, st>>>(L0, s.pA, s.Ap, p, s.r, s.sc, s.part);
    fin_guess(FIN_START);
    PCG_HIP(hipGetLastError());
    if (verbose || tol > 0.f) {
      std::vector<PcgScalars> hs(B);
      PCG_HIP(hipMemcpyAsync(hs.data(), s.sc, (size_t)B * sizeof(PcgScalars), hipMemcpyDeviceToHost, st));
      PCG_HIP(hipMemcpyAsync(&hg, s.gl, sizeof(hg), hipMemcpyDeviceToHost, st));
      PCG_HIP(hipStreamSynchronize(st));
      if (verbose) {
        printf("PCG warm start: a0");
        for (int b = 0; b < B; ++b) printf(" %g", (double)hs[b].alpha);
        printf(", residual %g\n", (double)hg.res);
      }
      if (hg.all_done) run = false;             // every sample starts within p_tol (or with b = 0)
    }
  }
  if (run) {
    // z = M^-1 r; the first direction is z
    vcycle(S, h.ls, is3d, B, s.sc, st);
    pcg_rz_kernel<<<rg, kRed, 0, st>>>(L0, s.r, s.z, s.sc, s.part);
    fin(FIN_RZ0);
  }
  while (run && it < max_iter) {
    pcg_dir_apply_kernel<<<rg, kRed, 0, st>>>(L0, s.z, P[it & 1], P[(it + 1) & 1], s.Ap, s.sc, it == 0 ? 1 : 0, s.part);
    fin(FIN_ALPHA);
    pcg_update_kernel<<<rg, kRed, 0, st>>>(L0, P[(it + 1) & 1], s.Ap, p, s.r, s.sc, s.part);
    fin(FIN_CHECK);
    PCG_HIP(hipGetLastError());
    ++it;
    if (verbose || (tol > 0.f && (it % kCheckEvery == 0 || it == max_iter))) {
      PCG_HIP(hipMemcpyAsync(&hg, s.gl, sizeof(hg), hipMemcpyDeviceToHost, st));
      PCG_HIP(hipStreamSynchronize(st));
      if (verbose) printf("PCG iteration %d: residual %g\n", it, (double)hg.res);
      if (hg.all_done) break;
    }
    if (it == max_iter) break;
    vcycle(S, h.ls, is3d, B, s.sc, st);
    pcg_rz_kernel<<<rg, kRed, 0, st>>>(L0, s.r, s.z, s.sc, s.part);
    fin(FIN_BETA);
  }
  // singular samples: the solution with mean zero over the degrees of freedom
  pcg_sum_kernel<<<rg, kRed, 0, st>>>(L0, p, s.part);
  fin(FIN_XMEAN);
  pcg_shift_kernel<<<grid1((size_t)B * N), 256, 0, st>>>(L0, B, p, s.sc);
  PCG_HIP(hipGetLastError());
  if (iters_done || verbose) {
    std::vector<PcgScalars> hs(B);
    PCG_HIP(hipMemcpyAsync(hs.data(), s.sc, (size_t)B * sizeof(PcgScalars), hipMemcpyDeviceToHost, st));
    PCG_HIP(hipStreamSynchronize(st));
    if (iters_done)
      for (int b = 0; b < B; ++b) iters_done[b] = hs[b].iters;
    if (verbose) {
      int conv = 0;
      for (int b = 0; b < B; ++b) conv += hs[b].converged;
      if (conv == B) printf("PCG max residual fell below p_tol (%g) (terminating)\n", (double)tol);
      else if (tol <= 0.f) printf("PCG ran its %d iterations (p_tol <= 0) (terminating)\n", max_iter);
      else printf("PCG stopped after %d iterations with %d of %d samples not converged (max iteration count or breakdown)\n", it, B - conv, B);
      fflush(stdout);
    }
  }
  return FNX_OK;
}

}  // namespace fnx
