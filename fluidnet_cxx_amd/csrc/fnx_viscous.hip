// The two viscous-flow operators in 3D for gfx950: addViscosity and setWallBcsStick.  The reference has neither in 3D (viscosity.py
// never defines mask_fluid_k; set_wall_bcs_stick.py:85-87 has misspelt names): what they compute is stated by the numpy model
// tests/viscous_model_nd.py with the axis as a loop variable, and these kernels give its float32 bits.  Every +, -, * and / is one
// rounding: the unit is compiled with -ffp-contract=off.  The 2D operators stay in fnx_stencils.hip.
#include "fnx_device.h"
#include "fnx_kernels.h"

namespace {

#define FNX_STICK 128.0f

// ---- addViscosity (3D) ------------------------------------------------------------------------------------------------------------------
// out = m (u + coef s), s = u(x+) + u(y+) + u(z+) + u(x-) + u(y-) + u(z-) - 6u summed in that order, m = cell and its low neighbour along
// the component are fluid; border cells copied.  28 algorithmic bytes a cell (three components and flags in, three components out) and a
// dozen flops: bandwidth-bound.  A block takes a tile of VX columns by VY rows and marches VZ planes along z, one thread per column:
// a thread keeps the k-1, k and k+1 values of its own column in registers (each plane is read once for the z direction, the k+1 loads
// are issued a whole iteration ahead of their first use), and the x +- 1 / y +- 1 neighbours of plane k come from an LDS tile of the
// plane with a one-cell halo, double-buffered so that one barrier a plane is enough.  The halo of plane k+1 is fetched with the plane
// itself: row VY-tile - 1 by the first wave, row + VY by the last, the two halo columns by 2 * VY lanes of the second wave.
constexpr int VX = 64, VY = 8, VZ = 8;
constexpr int VLX = VX + 2, VLY = VY + 2;      // the tile with its halo; 66 floats a row: rows start on different banks

__global__ __launch_bounds__(VX* VY) void add_viscosity3d_kernel(GridDims g, int nchunk, const float* __restrict__ Uin,
                                                                 float* __restrict__ Uout, const float* __restrict__ flags,
                                                                 float coef) {
  __shared__ float tile[2][4][VLY][VLX];       // [buffer][u, v, w, flags]
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int i = blockIdx.x * VX + tx, j = blockIdx.y * VY + ty;
  const int b = blockIdx.z / nchunk;
  const int kb = (blockIdx.z - b * nchunk) * VZ;
  const int ke = kb + VZ < g.D ? kb + VZ : g.D;
  const bool own = (i < g.W) & (j < g.H);
  // the halo cell this thread fetches besides its own column, if any: (hj, hi), stored at tile[..][hy][hx]
  int hi = -1, hj = -1, hx = 0, hy = 0;
  if (ty == 0) { hi = i; hj = j - 1; hx = tx + 1; hy = 0; }
  if (ty == VY - 1) { hi = i; hj = j + 1; hx = tx + 1; hy = VY + 1; }
  if (VY > 2 && ty == 1 && (tx & 31) < VY) {
    const bool right = tx >= 32;
    hy = (tx & 31) + 1;
    hj = blockIdx.y * VY + (tx & 31);
    hi = blockIdx.x * VX + (right ? VX : -1);
    hx = right ? VX + 1 : 0;
  }
  const bool halo = (hi >= 0) & (hi < g.W) & (hj >= 0) & (hj < g.H);
  const bool has_slot = (ty == 0) | (ty == VY - 1) | (VY > 2 && ty == 1 && (tx & 31) < VY);
  const size_t col = (size_t)j * g.W + i, hcol = (size_t)(halo ? hj : 0) * g.W + (halo ? hi : 0);
  const float* ub = Uin + (size_t)b * 3 * g.DHW;
  const float* fb = flags + (size_t)b * g.DHW;
  float* wb = Uout + (size_t)b * 3 * g.DHW;

  // c = 0..2: the components, 3: flags
  auto load = [&](int c, int k, size_t o, bool ok) -> float {
    if (!ok || k < 0 || k >= g.D) return 0.f;
    const float* p = c < 3 ? ub + (size_t)c * g.DHW : fb;
    return p[(size_t)k * g.HW + o];
  };
  float um[4], uc[4], up[4], hc[4], hn[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    um[c] = load(c, kb - 1, col, own);
    uc[c] = load(c, kb, col, own);
    hc[c] = load(c, kb, hcol, halo);
  }
  for (int k = kb; k < ke; ++k) {
    const int buf = k & 1;
#pragma unroll
    for (int c = 0; c < 4; ++c) {                // plane k + 1: used from the next iteration on (and as the z neighbour below)
      up[c] = load(c, k + 1, col, own);
      hn[c] = load(c, k + 1, hcol, halo);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      tile[buf][c][ty + 1][tx + 1] = uc[c];
      if (has_slot) tile[buf][c][hy][hx] = hc[c];
    }
    __syncthreads();
    if (own) {
      const size_t o = (size_t)k * g.HW + col;
      if (is_border<true>(g, i, j, k)) {
#pragma unroll
        for (int c = 0; c < 3; ++c) wb[(size_t)c * g.DHW + o] = uc[c];
      } else {
        const bool fluid = uc[3] == FNX_FLUID;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float (*t)[VLX] = tile[buf][c];
          const float flo = c == 0 ? tile[buf][3][ty + 1][tx] : (c == 1 ? tile[buf][3][ty][tx + 1] : um[3]);
          const float m = (fluid && flo == FNX_FLUID) ? 1.f : 0.f;
          float s = t[ty + 1][tx + 2] + t[ty + 2][tx + 1];
          s = s + up[c];
          s = s + t[ty + 1][tx];
          s = s + t[ty][tx + 1];
          s = s + um[c];
          s = s - (6.f * uc[c]);
          wb[(size_t)c * g.DHW + o] = m * (uc[c] + coef * s);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) { um[c] = uc[c]; uc[c] = up[c]; hc[c] = hn[c]; }
  }
}

// ---- setWallBcsStick (3D) ---------------------------------------------------------------------------------------------------------------
// One thread per cell and one pass: every value is a function of the INPUT field and of flags within distance 2.  The z-slab
// convention is setWallBcs's: "index along z > 0" is tested on the global plane (k + zoff) and on the local one.
constexpr int BX = 64, BY = 4;

template <int COMP>
__device__ __forceinline__ float slip3(const GridDims& g, const float* __restrict__ u, const float* __restrict__ fl,
                                       const float* __restrict__ st, int k, int j, int i) {
  const size_t o = (size_t)k * g.HW + (size_t)j * g.W + i;
  const float fc = fl[o];
  if (fc == FNX_OBST) return 0.f;
  const bool cont = fc == FNX_FLUID || st[o] == FNX_STICK;
  const bool above0 = COMP == 0 ? i > 0 : (COMP == 1 ? j > 0 : (k + g.zoff > 0 && k > 0));
  if (cont && above0 && fl[o - (COMP == 0 ? 1 : (COMP == 1 ? g.W : g.HW))] == FNX_OBST) return 0.f;
  return u[(size_t)COMP * g.DHW + o];
}

// the ghost value of component COMP on a stick cell; v: the cell's own slip value, flo: the flag of its low neighbour along COMP (0
// where there is none)
template <int COMP>
__device__ __forceinline__ float ghost3(const GridDims& g, const float* __restrict__ u, const float* __restrict__ fl,
                                        const float* __restrict__ st, float v, float flo, int k, int j, int i) {
  float t = 0.f;
  int n = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (a == COMP) continue;
#pragma unroll
    for (int d = -1; d <= 1; d += 2) {
      const int ni = i + (a == 0 ? d : 0), nj = j + (a == 1 ? d : 0), nk = k + (a == 2 ? d : 0);
      if (ni < 0 || ni >= g.W || nj < 0 || nj >= g.H || nk < 0 || nk >= g.D) continue;
      if (fl[(size_t)nk * g.HW + (size_t)nj * g.W + ni] != FNX_FLUID) continue;
      const float sv = slip3<COMP>(g, u, fl, st, nk, nj, ni);
      t = n == 0 ? -sv : t - sv;
      ++n;
    }
  }
  // the wall-face rule: across a fluid/obstacle face the normal component keeps its slip value
  if (n >= 1 && flo != FNX_FLUID) v = __fdiv_rn(t, (float)n);
  return v;
}

__global__ __launch_bounds__(BX* BY) void set_wall_bcs_stick3d_kernel(GridDims g, const float* __restrict__ Uin,
                                                                      float* __restrict__ Uout, const float* __restrict__ flags,
                                                                      const float* __restrict__ stick) {
  const int i = blockIdx.x * BX + threadIdx.x, j = blockIdx.y * BY + threadIdx.y;
  const int bk = blockIdx.z;
  const int b = bk / g.KN, k = g.K0 + (bk - b * g.KN);
  if (i >= g.W || j >= g.H) return;
  const float* u = Uin + (size_t)b * 3 * g.DHW;
  const float* fl = flags + (size_t)b * g.DHW;
  const float* st = stick + (size_t)b * g.DHW;
  const size_t o = (size_t)k * g.HW + (size_t)j * g.W + i;
  // the cell's own nine values first, none of them behind a test of another: nearly every cell is done with these (slip3 of the cell
  // itself, with its loads side by side instead of one after the other)
  const float fc = fl[o];
  const bool S = st[o] == FNX_STICK;
  const bool above0[3] = {i > 0, j > 0, k + g.zoff > 0 && k > 0};
  const int off[3] = {1, g.W, g.HW};
  float flo[3], v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    flo[c] = above0[c] ? fl[o - off[c]] : 0.f;
    v[c] = u[(size_t)c * g.DHW + o];
  }
  const bool cont = fc == FNX_FLUID || S;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    if (fc == FNX_OBST || (cont && flo[c] == FNX_OBST)) v[c] = 0.f;
  if (S) {
    v[0] = ghost3<0>(g, u, fl, st, v[0], flo[0], k, j, i);
    v[1] = ghost3<1>(g, u, fl, st, v[1], flo[1], k, j, i);
    v[2] = ghost3<2>(g, u, fl, st, v[2], flo[2], k, j, i);
  }
  float* w = Uout + (size_t)b * 3 * g.DHW + o;
#pragma unroll
  for (int c = 0; c < 3; ++c) w[(size_t)c * g.DHW] = v[c];
}

}  // namespace

namespace fnx {

void launch_add_viscosity3d(const GridDims& g, const float* Uin, float* Uout, const float* flags, float coef, hipStream_t s) {
  const int nchunk = (g.D + VZ - 1) / VZ;
  const dim3 grid((g.W + VX - 1) / VX, (g.H + VY - 1) / VY, g.B * nchunk);
  add_viscosity3d_kernel<<<grid, dim3(VX, VY), 0, s>>>(g, nchunk, Uin, Uout, flags, coef);
}

void launch_set_wall_bcs_stick3d(const GridDims& g, const float* Uin, float* Uout, const float* flags, const float* stick,
                                 hipStream_t s) {
  const dim3 grid((g.W + BX - 1) / BX, (g.H + BY - 1) / BY, g.B * g.KN);
  set_wall_bcs_stick3d_kernel<<<grid, dim3(BX, BY), 0, s>>>(g, Uin, Uout, flags, stick);
}

}  // namespace fnx
