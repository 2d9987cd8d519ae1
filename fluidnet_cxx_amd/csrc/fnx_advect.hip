// MacCormack / semi-Lagrangian advection kernels for gfx950.
//
// Replaces advectScalar (cpp/fluids_init.cpp:265-382) and advectVel (:656-807): the reference issues
// ~3300 / ~1400 ATen ops per call; here each advection is two launches (forward pass; backward pass fused
// with the MacCormack correction and clamp), one thread per cell, x fastest so every field read that is
// not a gather is a coalesced 256-B wave access.  Gathers (trace end points, clamp neighbourhoods) stay
// within a few cells of the thread's own cell and are served by L1/L2.
//
// Bit-parity: see fnx_device.h.  Compiled with -ffp-contract=off.
#include "../../include/fluidnet_hip.h"
#include "fnx_cells.h"
#include "fnx_device.h"
#include "fnx_kernels.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// Scalar: one semi-Lagrangian pass (SemiLagrangeEulerFluidNet[SavePos], fluids_init.cpp:12-133).
// Writes dst (border -> 0) and, if cell_out != nullptr, the clamped cell of the traced position
// (what getClampBounds :175-178 derives from fwd_pos).
// ---------------------------------------------------------------------------------------------------
template <bool IS3D, bool QUIRKS, bool SAMPLE_OUTSIDE>
__device__ __forceinline__ void sl_scalar_cell(const GridDims& g, const CellId& c, float dt, const float* __restrict__ src,
                                                           const float* __restrict__ U,
                                                           const float* __restrict__ flags, float* __restrict__ dst,
                                                           int* __restrict__ cell_out) {
  constexpr int NC = IS3D ? 3 : 2;
  const Field fs{src + (size_t)c.b * g.DHW}, ff{flags + (size_t)c.b * g.DHW}, fu{U + (size_t)c.b * NC * g.DHW};
  const size_t o = (size_t)c.k * g.HW + c.j * g.W + c.i;
  const float ctr[3] = { (float)c.i + 0.5f, (float)c.j + 0.5f, (float)(c.k + g.zoff) + 0.5f };   // global z
  float val = 0.f;
  float p[3] = { ctr[0], ctr[1], ctr[2] };
  if (!is_border<IS3D>(g, c.i, c.j, c.k)) {
    if (ff.p[o] != FNX_FLUID) {
      val = fs.p[o];                                   // "don't advect solid geometry"
    } else {
      float cen[3], disp[3];
      get_centered<IS3D>(g, fu, c.i, c.j, c.k, cen);
#pragma unroll
      for (int a = 0; a < 3; ++a) disp[a] = (-dt) * cen[a];
      line_trace(g, ff, ctr, disp, p);
      val = SAMPLE_OUTSIDE ? interpol<IS3D>(g, fs, 0, p[0], p[1], p[2])
                           : interpol_with_fluid<IS3D, QUIRKS>(g, fs, ff, p[0], p[1], p[2]);
    }
  }
  dst[(size_t)c.b * g.DHW + o] = val;
  if (cell_out) {
    const int i0 = clampi((int)p[0], 0, g.W - 1), j0 = clampi((int)p[1], 0, g.H - 1);
    // Q10: k0 = 0 in the reference.  Stored with a +1 plane bias so that global plane -1.. maps to a valid int
    const int k0 = (IS3D && !QUIRKS) ? clampi((int)p[2], 0, g.Dglob - 1) - g.zoff : -g.zoff;
    cell_out[(size_t)c.b * g.DHW + o] = IS3D ? (k0 + 1) * g.HW + j0 * g.W + i0 : ((j0 << 16) | i0);   // 2D: W, H < 65536 (host check)
  }
}

template <bool IS3D, bool QUIRKS, bool SAMPLE_OUTSIDE>
__global__ __launch_bounds__(BX* BY) void sl_scalar_kernel(GridDims g, float dt, const float* __restrict__ src,
                                                           const float* __restrict__ U,
                                                           const float* __restrict__ flags, float* __restrict__ dst,
                                                           int* __restrict__ cell_out) {
  const CellId c = cell_id<IS3D>(g);
  if (!c.valid) return;
  sl_scalar_cell<IS3D, QUIRKS, SAMPLE_OUTSIDE>(g, c, dt, src, U, flags, dst, cell_out);
}

// ---------------------------------------------------------------------------------------------------
// 3D clamp bounds of MacCormackClampFluidNet (:154-263) as a field: for every cell c of the compute window the min / max
// of src over the 3x3x3 box around c, taken over the cells that are inside the (local) domain and -- unless
// sample_outside_fluid -- fluid.  The backward kernel then fetches ONE 8-byte pair at the traced cell instead of walking
// 27 cells x 2 fields per thread.  min/max are exact, commutative and NaN-ignoring (v_min_f32 / v_max_f32 order -0 < +0),
// so the separable evaluation gives the same bits as the reference's 27-step fold; "no cell qualified" (the reference
// then keeps the forward value) is encoded as mn = NaN.
// src and box are B * C plane stacks (bc = b * C + c) over B samples of flags: the density is C = 1, the passive scalars
// (fnx_scalars.hip) bring their channels.
// A wave covers 62 columns (lanes 0 / 63 are halo columns) x BOX_R rows and marches along z: per plane it reduces
// rows j0-1..j0+BOX_R in x (DPP) and y, and keeps the reduced planes k-1, k, k+1 in registers.  (2D: the 9 cells are
// walked in the backward kernels, cheaper than a separate pass.)
// ---------------------------------------------------------------------------------------------------
constexpr int BOX_R = 8, BOX_ZC = 16;

__device__ __forceinline__ float dppf_left(float v) {     // lane-1 (0.0 into lane 0: a halo lane, never stored)
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, true));
}
__device__ __forceinline__ float dppf_right(float v) {    // lane+1
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, true));
}
__device__ __forceinline__ unsigned dppu_left(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, true); }
__device__ __forceinline__ unsigned dppu_right(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xf, 0xf, true); }

template <bool SAMPLE_OUTSIDE>
__global__ __launch_bounds__(256) void box_minmax_kernel(GridDims g, int C, const float* __restrict__ src,
                                                         const float* __restrict__ flags, float2* __restrict__ box,
                                                         int nzc) {
  const int lane = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.y);
  const int x = blockIdx.x * 62 - 1 + lane;
  const int j0 = (blockIdx.y * 4 + w) * BOX_R;
  const int bz = blockIdx.z;
  const int zc = bz % nzc, bc = bz / nzc;                 // bc: plane stack b * C + c of src and box
  const int k_lo = g.K0 + zc * BOX_ZC, k_hi = min(k_lo + BOX_ZC, g.K0 + g.KN);      // planes of the compute window
  if (j0 >= g.H) return;
  const bool xin = (x >= 0) & (x < g.W);
  const int xc = clampi(x, 0, g.W - 1);
  const size_t base = (size_t)bc * g.DHW, fbase = (size_t)(bc / C) * g.DHW;
  // all loads of a plane are unconditional (clamped rows / planes) so they issue back to back; validity only gates `ok`
  auto plane = [&](int k, float* omn, float* omx, unsigned* oan) {
    float sv[BOX_R + 2], fv[BOX_R + 2];
    const bool kin = (k >= 0) & (k < g.D);                           // the reference's box is clipped to the grid
    const size_t ok_ = (size_t)clampi(k, 0, g.D - 1) * g.HW + xc;
#pragma unroll
    for (int rr = 0; rr < BOX_R + 2; ++rr) {
      const size_t o = ok_ + (size_t)clampi(j0 - 1 + rr, 0, g.H - 1) * g.W;
      sv[rr] = src[base + o];
      fv[rr] = SAMPLE_OUTSIDE ? FNX_FLUID : flags[fbase + o];
    }
    float rmn[BOX_R + 2], rmx[BOX_R + 2]; unsigned ran[BOX_R + 2];
#pragma unroll
    for (int rr = 0; rr < BOX_R + 2; ++rr) {
      const int j = j0 - 1 + rr;
      const bool ok = xin & kin & (j >= 0) & (j < g.H) & (fv[rr] == FNX_FLUID);
      const float vmn = ok ? sv[rr] : INFINITY, vmx = ok ? sv[rr] : -INFINITY;
      const unsigned va = ok ? 1u : 0u;
      rmn[rr] = fminf(fminf(dppf_left(vmn), vmn), dppf_right(vmn));
      rmx[rr] = fmaxf(fmaxf(dppf_left(vmx), vmx), dppf_right(vmx));
      ran[rr] = dppu_left(va) | va | dppu_right(va);
    }
#pragma unroll
    for (int r = 0; r < BOX_R; ++r) {
      omn[r] = fminf(fminf(rmn[r], rmn[r + 1]), rmn[r + 2]);
      omx[r] = fmaxf(fmaxf(rmx[r], rmx[r + 1]), rmx[r + 2]);
      oan[r] = ran[r] | ran[r + 1] | ran[r + 2];
    }
  };
  const bool lane_out = (lane >= 1) & (lane <= 62) & xin;
  float mn[3][BOX_R], mx[3][BOX_R]; unsigned an[3][BOX_R];           // xy-reduced planes k-1, k, k+1
  plane(k_lo - 1, mn[0], mx[0], an[0]);
  plane(k_lo, mn[1], mx[1], an[1]);
  for (int k = k_lo; k < k_hi; ++k) {
    plane(k + 1, mn[2], mx[2], an[2]);
#pragma unroll
    for (int r = 0; r < BOX_R; ++r) {
      const bool any = (an[0][r] | an[1][r] | an[2][r]) != 0;
      const float lo = fminf(fminf(mn[0][r], mn[1][r]), mn[2][r]), hi = fmaxf(fmaxf(mx[0][r], mx[1][r]), mx[2][r]);
      if (lane_out && j0 + r < g.H)
        box[base + (size_t)k * g.HW + (size_t)(j0 + r) * g.W + x] = make_float2(any ? lo : __builtin_nanf(""), hi);
    }
#pragma unroll
    for (int r = 0; r < BOX_R; ++r) {
      mn[0][r] = mn[1][r]; mx[0][r] = mx[1][r]; an[0][r] = an[1][r];
      mn[1][r] = mn[2][r]; mx[1][r] = mx[2][r]; an[1][r] = an[2][r];
    }
  }
}

// Backward pass on fwd + MacCormackCorrect (:135-148) + MacCormackClampFluidNet (:154-263)
template <bool IS3D, bool QUIRKS, bool SAMPLE_OUTSIDE>
__device__ __forceinline__ void sl_scalar_bwd_clamp_cell(const GridDims& g, const CellId& c, float dt, float half_s,
                                                                     const float* __restrict__ src,
                                                                     const float* __restrict__ fwd,
                                                                     const int* __restrict__ cell_in,
                                                                     const float* __restrict__ U,
                                                                     const float* __restrict__ flags,
                                                                     const float2* __restrict__ box,
                                                                     float* __restrict__ dst) {
  constexpr int NC = IS3D ? 3 : 2;
  const Field fs{src + (size_t)c.b * g.DHW}, fw{fwd + (size_t)c.b * g.DHW}, ff{flags + (size_t)c.b * g.DHW},
      fu{U + (size_t)c.b * NC * g.DHW};
  const size_t o = (size_t)c.k * g.HW + c.j * g.W + c.i;
  const bool border = is_border<IS3D>(g, c.i, c.j, c.k);
  const bool fluid = ff.p[o] == FNX_FLUID;
  const float f = fw.p[o];
  float bwd = 0.f;
  if (!border) {
    if (!fluid) {
      bwd = f;
    } else {
      const float ctr[3] = { (float)c.i + 0.5f, (float)c.j + 0.5f, (float)(c.k + g.zoff) + 0.5f };
      float cen[3], disp[3], p[3];
      get_centered<IS3D>(g, fu, c.i, c.j, c.k, cen);
      const float ndt = -dt;
#pragma unroll
      for (int a = 0; a < 3; ++a) disp[a] = (-ndt) * cen[a];
      line_trace(g, ff, ctr, disp, p);
      bwd = SAMPLE_OUTSIDE ? interpol<IS3D>(g, fw, 0, p[0], p[1], p[2])
                           : interpol_with_fluid<IS3D, QUIRKS>(g, fw, ff, p[0], p[1], p[2]);
    }
  }
  float d = f;
  if (fluid) d = f + half_s * (fs.p[o] - bwd);          // applied on border cells too (reference :371)
  if (!border) {
    // traced cell: 3D (k0+1)*HW + j0*W + i0 (no integer division on the common path), 2D (j0 << 16) | i0
    const int cell = cell_in[(size_t)c.b * g.DHW + o];
    float mn, mx;
    bool any;
    int k0 = 0, j0 = 0, i0 = 0;
    if (IS3D && box != nullptr && cell >= g.HW && cell < g.HW + g.DHW) {
      // the traced cell lies in this slab: its clamp bounds were reduced once by box_minmax_kernel
      const float2 bb = box[(size_t)c.b * g.DHW + (size_t)(cell - g.HW)];
      mn = bb.x; mx = bb.y;
      any = !(mn != mn);
    } else {
      if (IS3D) {
        const int kb = cell / g.HW;                         // local plane + 1
        k0 = kb - 1;
        const int r = cell - kb * g.HW;
        j0 = r / g.W; i0 = r - j0 * g.W;
      } else {
        j0 = (int)((unsigned)cell >> 16); i0 = cell & 0xffff;   // (unsigned: rows >= 32768 set the sign bit)
      }
      // 2D (9 cells: cheaper than a separate pass), or traced into a plane this slab does not hold: walk the clipped
      // box directly, as the reference does
      mn = INFINITY; mx = -INFINITY; any = false;
      // 3x3(x3) neighbourhood of the traced cell: every load is unconditional (clamped address) and the
      // in-domain / is-fluid tests only gate the min/max, so the 18-54 loads are independent and issue back to back.
#pragma unroll
      for (int dk = (IS3D ? -1 : 0); dk <= (IS3D ? 1 : 0); ++dk) {
        const int kk = k0 + dk;
        const bool vk = (kk + g.zoff >= 0) & (kk + g.zoff < g.Dglob) & (kk >= 0) & (kk < g.D);   // in the domain and in this slab
        const int kc = clampi(kk, 0, g.D - 1);
#pragma unroll
        for (int dj = -1; dj <= 1; ++dj) {
          const int jj = j0 + dj;
          const bool vj = vk & (jj >= 0) & (jj < g.H);
          const int jc = clampi(jj, 0, g.H - 1);
#pragma unroll
          for (int di = -1; di <= 1; ++di) {
            const int ii = i0 + di;
            const bool vi = vj & (ii >= 0) & (ii < g.W);
            const size_t q = (size_t)kc * g.HW + jc * g.W + clampi(ii, 0, g.W - 1);
            const float s = fs.p[q];
            const bool ok = vi & (SAMPLE_OUTSIDE || ff.p[q] == FNX_FLUID);
            mn = ok ? fminf(mn, s) : mn;
            mx = ok ? fmaxf(mx, s) : mx;
            any = any | ok;
          }
        }
      }
    }
    d = any ? fmaxf(mn, fminf(mx, d)) : f;
  }
  dst[(size_t)c.b * g.DHW + o] = d;
}

template <bool IS3D, bool QUIRKS, bool SAMPLE_OUTSIDE>
__global__ __launch_bounds__(BX* BY) void sl_scalar_bwd_clamp_kernel(GridDims g, float dt, float half_s,
                                                                     const float* __restrict__ src,
                                                                     const float* __restrict__ fwd,
                                                                     const int* __restrict__ cell_in,
                                                                     const float* __restrict__ U,
                                                                     const float* __restrict__ flags,
                                                                     const float2* __restrict__ box,
                                                                     float* __restrict__ dst) {
  const CellId c = cell_id<IS3D>(g);
  if (!c.valid) return;
  sl_scalar_bwd_clamp_cell<IS3D, QUIRKS, SAMPLE_OUTSIDE>(g, c, dt, half_s, src, fwd, cell_in, U, flags, box, dst);
}

// ---------------------------------------------------------------------------------------------------
// Velocity: SemiLagrangeEulerFluidNetMAC (:388-451), no line trace.
// ---------------------------------------------------------------------------------------------------
template <bool IS3D, bool QUIRKS, int COMP>
__device__ __forceinline__ float sl_mac_component(const GridDims& g, const Field& src, const Field& fu, int i, int j,
                                                  int k, float dt) {
  float v[3];
  get_at_mac<IS3D, QUIRKS, COMP>(g, fu, i, j, k, v);
  const float px = ((float)i + 0.5f) + v[0] * (-dt);
  const float py = ((float)j + 0.5f) + v[1] * (-dt);
  const float pz = ((float)(k + g.zoff) + 0.5f) + v[2] * (-dt);
  return interpol<IS3D>(g, src, COMP, px, py, pz);
}

template <bool IS3D, bool QUIRKS>
__device__ __forceinline__ void sl_mac_cell(const GridDims& g, const CellId& c, float dt, const float* __restrict__ src,
                                                        const float* __restrict__ U, const float* __restrict__ flags,
                                                        float* __restrict__ dst) {
  constexpr int NC = IS3D ? 3 : 2;
  const Field fs{src + (size_t)c.b * NC * g.DHW}, fu{U + (size_t)c.b * NC * g.DHW};
  const size_t o = (size_t)c.k * g.HW + c.j * g.W + c.i;
  float r[3] = { 0.f, 0.f, 0.f };
  if (!is_border<IS3D>(g, c.i, c.j, c.k)) {
    if (flags[(size_t)c.b * g.DHW + o] != FNX_FLUID) {
      r[0] = fs.p[(size_t)g.DHW + o];                    // reference writes src channel 1 into channel 0 (:413-416)
      if (IS3D) r[2] = fs.p[(size_t)2 * g.DHW + o];
    } else {
      r[0] = sl_mac_component<IS3D, QUIRKS, 0>(g, fs, fu, c.i, c.j, c.k, dt);
      r[1] = sl_mac_component<IS3D, QUIRKS, 1>(g, fs, fu, c.i, c.j, c.k, dt);
      if (IS3D && !QUIRKS) r[2] = sl_mac_component<IS3D, QUIRKS, 2>(g, fs, fu, c.i, c.j, c.k, dt);   // Q12: 0 in ref
    }
  }
  float* d = dst + (size_t)c.b * NC * g.DHW + o;
#pragma unroll
  for (int a = 0; a < NC; ++a) d[(size_t)a * g.DHW] = r[a];
}

template <bool IS3D, bool QUIRKS>
__global__ __launch_bounds__(BX* BY) void sl_mac_kernel(GridDims g, float dt, const float* __restrict__ src,
                                                        const float* __restrict__ U, const float* __restrict__ flags,
                                                        float* __restrict__ dst) {
  const CellId c = cell_id<IS3D>(g);
  if (!c.valid) return;
  sl_mac_cell<IS3D, QUIRKS>(g, c, dt, src, U, flags, dst);
}

// min/max of channel `comp` of orig over the 4(8) corners at trunc(pos -/+ v)  (doClampComponentMAC :500-614)
template <bool IS3D>
__device__ __forceinline__ void clamp_bounds_mac(const GridDims& g, const float* __restrict__ oc, const float pos[3],
                                                 const float v[3], float& mn, float& mx) {
#pragma unroll
  for (int l = 0; l < 2; ++l) {
    const int qx = (int)(l == 0 ? pos[0] - v[0] : pos[0] + v[0]);
    const int qy = (int)(l == 0 ? pos[1] - v[1] : pos[1] + v[1]);
    const int qz = (int)(l == 0 ? pos[2] - v[2] : pos[2] + v[2]);
    const int i0 = clampi(qx, 0, g.W - 2), j0 = clampi(qy, 0, g.H - 2);
    const int k0 = IS3D ? clampi(clampi(qz, 0, g.Dglob - 2) - g.zoff, 0, g.D - 2) : 0;
    const float* q = oc + (size_t)k0 * g.HW + j0 * g.W + i0;
    // reference visiting order: 000, 100, 010, 110 [, 001, 101, 011, 111] (x is the first digit)
    float o;
    o = q[0]; mn = fminf(mn, o); mx = fmaxf(mx, o);
    o = q[1]; mn = fminf(mn, o); mx = fmaxf(mx, o);
    o = q[g.W]; mn = fminf(mn, o); mx = fmaxf(mx, o);
    o = q[g.W + 1]; mn = fminf(mn, o); mx = fmaxf(mx, o);
    if (IS3D) {
      const float* r = q + g.HW;
      o = r[0]; mn = fminf(mn, o); mx = fmaxf(mx, o);
      o = r[1]; mn = fminf(mn, o); mx = fmaxf(mx, o);
      o = r[g.W]; mn = fminf(mn, o); mx = fmaxf(mx, o);
      o = r[g.W + 1]; mn = fminf(mn, o); mx = fmaxf(mx, o);
    }
  }
}

template <bool IS3D, bool QUIRKS, int COMP>
__device__ __forceinline__ float mac_bwd_correct_clamp(const GridDims& g, const Field& forig, const Field& ffwd,
                                                       const Field& fu, const Field& ff, int i, int j, int k, float dt,
                                                       float half_s, bool fluid) {
  const size_t o = (size_t)k * g.HW + j * g.W + i;
  const float f = ffwd.p[(size_t)COMP * g.DHW + o];
  float v[3];
  get_at_mac<IS3D, QUIRKS, COMP>(g, fu, i, j, k, v);
  // backward pass: SL(fwd, -dt): displacement v * (-(-dt)) == v * dt, also the clamp velocity (:640-648)
  const float vd[3] = { v[0] * dt, v[1] * dt, v[2] * dt };
  float bwd;
  if (!fluid) {
    bwd = COMP == 0 ? ffwd.p[(size_t)g.DHW + o] : (COMP == 1 ? 0.f : f);   // Q1 pass-through of SL(fwd)
  } else if (COMP == 2 && QUIRKS) {
    bwd = 0.f;
  } else {
    bwd = interpol<IS3D>(g, ffwd, COMP, ((float)i + 0.5f) + vd[0], ((float)j + 0.5f) + vd[1], ((float)(k + g.zoff) + 0.5f) + vd[2]);
  }
  // MacCormackCorrectMAC :453-498
  bool skip = !fluid;
  const int idx = COMP == 0 ? i : (COMP == 1 ? j : k + g.zoff);
  if (idx > 0 && !(COMP == 2 && k == 0)) {
    const size_t om = o - (COMP == 0 ? 1 : (COMP == 1 ? g.W : g.HW));
    if (ff.p[om] != FNX_FLUID) skip = true;
  }
  const float corr = skip ? f : f + half_s * (forig.p[(size_t)COMP * g.DHW + o] - bwd);
  float mn = INFINITY, mx = -INFINITY;
  const float pos[3] = { (float)i, (float)j, (float)(k + g.zoff) };
  clamp_bounds_mac<IS3D>(g, forig.p + (size_t)COMP * g.DHW, pos, vd, mn, mx);
  return fmaxf(fminf(corr, mx), mn);
}

template <bool IS3D, bool QUIRKS>
__device__ __forceinline__ void sl_mac_bwd_clamp_cell(const GridDims& g, const CellId& c, float dt, float half_s,
                                                                  const float* __restrict__ orig,
                                                                  const float* __restrict__ fwd,
                                                                  const float* __restrict__ U,
                                                                  const float* __restrict__ flags,
                                                                  float* __restrict__ dst) {
  constexpr int NC = IS3D ? 3 : 2;
  const Field fo{orig + (size_t)c.b * NC * g.DHW}, fw{fwd + (size_t)c.b * NC * g.DHW},
      fu{U + (size_t)c.b * NC * g.DHW}, ff{flags + (size_t)c.b * g.DHW};
  const size_t o = (size_t)c.k * g.HW + c.j * g.W + c.i;
  float r[3] = { 0.f, 0.f, 0.f };
  if (!is_border<IS3D>(g, c.i, c.j, c.k)) {
    const bool fluid = ff.p[o] == FNX_FLUID;
    r[0] = mac_bwd_correct_clamp<IS3D, QUIRKS, 0>(g, fo, fw, fu, ff, c.i, c.j, c.k, dt, half_s, fluid);
    r[1] = mac_bwd_correct_clamp<IS3D, QUIRKS, 1>(g, fo, fw, fu, ff, c.i, c.j, c.k, dt, half_s, fluid);
    if (IS3D) r[2] = mac_bwd_correct_clamp<IS3D, QUIRKS, 2>(g, fo, fw, fu, ff, c.i, c.j, c.k, dt, half_s, fluid);
  }
  float* d = dst + (size_t)c.b * NC * g.DHW + o;
#pragma unroll
  for (int a = 0; a < NC; ++a) d[(size_t)a * g.DHW] = r[a];
}

template <bool IS3D, bool QUIRKS>
__global__ __launch_bounds__(BX* BY) void sl_mac_bwd_clamp_kernel(GridDims g, float dt, float half_s,
                                                                  const float* __restrict__ orig,
                                                                  const float* __restrict__ fwd,
                                                                  const float* __restrict__ U,
                                                                  const float* __restrict__ flags,
                                                                  float* __restrict__ dst) {
  const CellId c = cell_id<IS3D>(g);
  if (!c.valid) return;
  sl_mac_bwd_clamp_cell<IS3D, QUIRKS>(g, c, dt, half_s, orig, fwd, U, flags, dst);
}

// ---------------------------------------------------------------------------------------------------
// Phase-ordered ("flat") velocity passes.  The per-component functions above interleave loads and their use: compiled,
// the backward pass is ~60 dependent load -> wait round trips per thread (clusters of 1-13 loads).  Here all components
// go through the same expressions phase by phase: (A) every load that depends on the cell only (own values, -1 flags,
// the 9 face-velocity operands per component), (B) every gather that depends on the face velocities (8 trilinear
// corners and 2 x 8 clamp corners per component) in one batch, (C) the arithmetic.  A non-fluid cell computes its
// (unused) sample anyway -- addresses are clamped, so that is safe -- and takes the reference's pass-through by select.
// Same operations in the same order per value: same bits.  Measured: 2D 1024^2 advection 39 -> 36 us; 3D unchanged
// (1.06 ms at 512x512x64): there the scalar half with its line trace sets the pace.
// ---------------------------------------------------------------------------------------------------
template <bool IS3D>
__device__ __forceinline__ void sl_mac_bwd_clamp_cell_flat(const GridDims& g, const CellId& c, float dt, float half_s,
                                                           const float* __restrict__ orig,
                                                           const float* __restrict__ fwd,
                                                           const float* __restrict__ U,
                                                           const float* __restrict__ flags,
                                                           float* __restrict__ dst) {
  constexpr int NC = IS3D ? 3 : 2, NK = IS3D ? 8 : 4;
  const Field fo{orig + (size_t)c.b * NC * g.DHW}, fw{fwd + (size_t)c.b * NC * g.DHW},
      fu{U + (size_t)c.b * NC * g.DHW}, ff{flags + (size_t)c.b * g.DHW};
  const size_t o = (size_t)c.k * g.HW + c.j * g.W + c.i;
  float* d = dst + (size_t)c.b * NC * g.DHW + o;
  if (is_border<IS3D>(g, c.i, c.j, c.k)) {
#pragma unroll
    for (int a = 0; a < NC; ++a) d[(size_t)a * g.DHW] = 0.f;
    return;
  }
  const int i = c.i, j = c.j, k = c.k;
  // ---- (A) loads that depend on the cell only
  const float fcell = ff.p[o];
  float f[NC], og[NC], fmn[NC], v[NC][3];
  bool chk[NC];
#pragma unroll
  for (int a = 0; a < NC; ++a) {
    f[a] = fw.p[(size_t)a * g.DHW + o];
    og[a] = fo.p[(size_t)a * g.DHW + o];
    const int idx = a == 0 ? i : (a == 1 ? j : k + g.zoff);
    chk[a] = idx > 0 && !(a == 2 && k == 0);
    fmn[a] = ff.p[o - (chk[a] ? (a == 0 ? 1 : (a == 1 ? g.W : g.HW)) : 0)];
  }
  get_at_mac<IS3D, false, 0>(g, fu, i, j, k, v[0]);
  get_at_mac<IS3D, false, 1>(g, fu, i, j, k, v[1]);
  if (IS3D) get_at_mac<IS3D, false, 2>(g, fu, i, j, k, v[2]);
  // ---- (B) gathers that depend on the face velocities
  float vd[NC][3];
  Lerp L[NC];
  float Iv[NC][NK], Cv[NC][2][NK];
  const float pos[3] = { (float)i, (float)j, (float)(k + g.zoff) };
#pragma unroll
  for (int a = 0; a < NC; ++a) {
#pragma unroll
    for (int q = 0; q < 3; ++q) vd[a][q] = v[a][q] * dt;
    L[a] = lerp_setup<IS3D>(g, ((float)i + 0.5f) + vd[a][0], ((float)j + 0.5f) + vd[a][1], ((float)(k + g.zoff) + 0.5f) + vd[a][2]);
    const float* q = fw.p + (size_t)a * g.DHW + (size_t)L[a].z0 * g.HW + L[a].y0 * g.W + L[a].x0;
    Iv[a][0] = q[0]; Iv[a][1] = q[g.W]; Iv[a][2] = q[1]; Iv[a][3] = q[g.W + 1];
    if (IS3D) { const float* r = q + g.HW; Iv[a][4] = r[0]; Iv[a][5] = r[g.W]; Iv[a][6] = r[1]; Iv[a][7] = r[g.W + 1]; }
#pragma unroll
    for (int l = 0; l < 2; ++l) {
      const int qx = (int)(l == 0 ? pos[0] - vd[a][0] : pos[0] + vd[a][0]);
      const int qy = (int)(l == 0 ? pos[1] - vd[a][1] : pos[1] + vd[a][1]);
      const int qz = (int)(l == 0 ? pos[2] - vd[a][2] : pos[2] + vd[a][2]);
      const int i0 = clampi(qx, 0, g.W - 2), j0 = clampi(qy, 0, g.H - 2);
      const int k0 = IS3D ? clampi(clampi(qz, 0, g.Dglob - 2) - g.zoff, 0, g.D - 2) : 0;
      const float* p = fo.p + (size_t)a * g.DHW + (size_t)k0 * g.HW + j0 * g.W + i0;
      Cv[a][l][0] = p[0]; Cv[a][l][1] = p[1]; Cv[a][l][2] = p[g.W]; Cv[a][l][3] = p[g.W + 1];
      if (IS3D) { const float* r = p + g.HW; Cv[a][l][4] = r[0]; Cv[a][l][5] = r[1]; Cv[a][l][6] = r[g.W]; Cv[a][l][7] = r[g.W + 1]; }
    }
  }
  // ---- (C) arithmetic (mac_bwd_correct_clamp)
  const bool fluid = fcell == FNX_FLUID;
#pragma unroll
  for (int a = 0; a < NC; ++a) {
    const float lo = (Iv[a][0] * L[a].t0 + Iv[a][1] * L[a].t1) * L[a].s0 + (Iv[a][2] * L[a].t0 + Iv[a][3] * L[a].t1) * L[a].s1;
    float smp = lo;
    if (IS3D) {
      const float hi = (Iv[a][4] * L[a].t0 + Iv[a][5] * L[a].t1) * L[a].s0 + (Iv[a][6] * L[a].t0 + Iv[a][7] * L[a].t1) * L[a].s1;
      smp = lo * L[a].f0 + hi * L[a].f1;
    }
    const float bwd = fluid ? smp : (a == 0 ? f[1] : (a == 1 ? 0.f : f[a]));      // Q1 pass-through of SL(fwd)
    const bool skip = !fluid | (chk[a] & (fmn[a] != FNX_FLUID));
    const float corr = skip ? f[a] : f[a] + half_s * (og[a] - bwd);
    float mn = INFINITY, mx = -INFINITY;
#pragma unroll
    for (int l = 0; l < 2; ++l)
#pragma unroll
      for (int q = 0; q < NK; ++q) { mn = fminf(mn, Cv[a][l][q]); mx = fmaxf(mx, Cv[a][l][q]); }
    d[(size_t)a * g.DHW] = fmaxf(fminf(corr, mx), mn);
  }
}

// forward pass (sl_mac_cell), the same way
template <bool IS3D>
__device__ __forceinline__ void sl_mac_cell_flat(const GridDims& g, const CellId& c, float dt, const float* __restrict__ src,
                                                 const float* __restrict__ U, const float* __restrict__ flags,
                                                 float* __restrict__ dst) {
  constexpr int NC = IS3D ? 3 : 2, NK = IS3D ? 8 : 4;
  const Field fs{src + (size_t)c.b * NC * g.DHW}, fu{U + (size_t)c.b * NC * g.DHW};
  const size_t o = (size_t)c.k * g.HW + c.j * g.W + c.i;
  float* d = dst + (size_t)c.b * NC * g.DHW + o;
  if (is_border<IS3D>(g, c.i, c.j, c.k)) {
#pragma unroll
    for (int a = 0; a < NC; ++a) d[(size_t)a * g.DHW] = 0.f;
    return;
  }
  const int i = c.i, j = c.j, k = c.k;
  const float fcell = flags[(size_t)c.b * g.DHW + o];
  float own[NC], v[NC][3];
#pragma unroll
  for (int a = 0; a < NC; ++a) own[a] = fs.p[(size_t)a * g.DHW + o];
  get_at_mac<IS3D, false, 0>(g, fu, i, j, k, v[0]);
  get_at_mac<IS3D, false, 1>(g, fu, i, j, k, v[1]);
  if (IS3D) get_at_mac<IS3D, false, 2>(g, fu, i, j, k, v[2]);
  Lerp L[NC];
  float Iv[NC][NK];
#pragma unroll
  for (int a = 0; a < NC; ++a) {
    const float px = ((float)i + 0.5f) + v[a][0] * (-dt);
    const float py = ((float)j + 0.5f) + v[a][1] * (-dt);
    const float pz = ((float)(k + g.zoff) + 0.5f) + v[a][2] * (-dt);
    L[a] = lerp_setup<IS3D>(g, px, py, pz);
    const float* q = fs.p + (size_t)a * g.DHW + (size_t)L[a].z0 * g.HW + L[a].y0 * g.W + L[a].x0;
    Iv[a][0] = q[0]; Iv[a][1] = q[g.W]; Iv[a][2] = q[1]; Iv[a][3] = q[g.W + 1];
    if (IS3D) { const float* r = q + g.HW; Iv[a][4] = r[0]; Iv[a][5] = r[g.W]; Iv[a][6] = r[1]; Iv[a][7] = r[g.W + 1]; }
  }
  const bool fluid = fcell == FNX_FLUID;
#pragma unroll
  for (int a = 0; a < NC; ++a) {
    const float lo = (Iv[a][0] * L[a].t0 + Iv[a][1] * L[a].t1) * L[a].s0 + (Iv[a][2] * L[a].t0 + Iv[a][3] * L[a].t1) * L[a].s1;
    float smp = lo;
    if (IS3D) {
      const float hi = (Iv[a][4] * L[a].t0 + Iv[a][5] * L[a].t1) * L[a].s0 + (Iv[a][6] * L[a].t0 + Iv[a][7] * L[a].t1) * L[a].s1;
      smp = lo * L[a].f0 + hi * L[a].f1;
    }
    // non-fluid cell: the reference writes src channel 1 into channel 0, 0 into channel 1, src channel 2 into channel 2 (:413-416)
    d[(size_t)a * g.DHW] = fluid ? smp : (a == 0 ? own[1] : (a == 1 ? 0.f : own[2]));
  }
}

// ---------------------------------------------------------------------------------------------------
// The density and the velocity MacCormack advections of one time step in two launches instead of four (forward passes
// together, backward/clamp passes together; 3D: the clamp-bounds pass in between).  In 2D at 128^2 .. 1024^2 each pass
// is a 7-14 us launch that is mostly ramp-up; in 3D the two chains share their velocity loads (1.13 -> 1.06 ms at
// 256^3).  The cell functions are the ones above, so the results are the same bits.
// ---------------------------------------------------------------------------------------------------
template <bool IS3D, bool QUIRKS, bool SAMPLE_OUTSIDE>
__global__ __launch_bounds__(BX* BY) void advect_fwd_kernel(GridDims g, float dt, const float* __restrict__ rho,
                                                              const float* __restrict__ U,
                                                              const float* __restrict__ flags,
                                                              float* __restrict__ rho_fwd, int* __restrict__ cell_out,
                                                              float* __restrict__ U_fwd) {
  const CellId c = cell_id<IS3D>(g);
  if (!c.valid) return;
  sl_scalar_cell<IS3D, QUIRKS, SAMPLE_OUTSIDE>(g, c, dt, rho, U, flags, rho_fwd, cell_out);
  if (QUIRKS) sl_mac_cell<IS3D, QUIRKS>(g, c, dt, U, U, flags, U_fwd);
  else sl_mac_cell_flat<IS3D>(g, c, dt, U, U, flags, U_fwd);
}

template <bool IS3D, bool QUIRKS, bool SAMPLE_OUTSIDE>
__global__ __launch_bounds__(BX* BY) void advect_bwd_kernel(GridDims g, float dt, float half_s,
                                                              const float* __restrict__ rho,
                                                              const float* __restrict__ rho_fwd,
                                                              const int* __restrict__ cell_in,
                                                              const float* __restrict__ U,
                                                              const float* __restrict__ U_fwd,
                                                              const float* __restrict__ flags,
                                                              const float2* __restrict__ box,
                                                              float* __restrict__ rho_dst, float* __restrict__ U_dst) {
  const CellId c = cell_id<IS3D>(g);
  if (!c.valid) return;
  sl_scalar_bwd_clamp_cell<IS3D, QUIRKS, SAMPLE_OUTSIDE>(g, c, dt, half_s, rho, rho_fwd, cell_in, U, flags, box, rho_dst);
  if (QUIRKS) sl_mac_bwd_clamp_cell<IS3D, QUIRKS>(g, c, dt, half_s, U, U_fwd, U, flags, U_dst);
  else sl_mac_bwd_clamp_cell_flat<IS3D>(g, c, dt, half_s, U, U_fwd, U, flags, U_dst);
}

#include "fnx_advect_march.h"
#include "fnx_advect_tile2d.h"

// the grid with the compute window widened by `by` planes (clipped to the array)
inline GridDims widened(GridDims d, int by) {
  const int a = d.K0 - by < 0 ? 0 : d.K0 - by, b = d.K0 + d.KN + by > d.D ? d.D : d.K0 + d.KN + by;
  d.K0 = a; d.KN = b - a;
  return d;
}

inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

// fix-up bitmaps of the tile kernels (fnx_advect_march.h, fnx_advect_tile2d.h): one 64-bit word per 64-cell row segment of the array,
// four of them: forward density, forward velocity, backward density, backward velocity
inline size_t fix_words(const GridDims& g) { return (size_t)g.B * g.D * g.H * ((g.W + 63) / 64); }

// z-marching tile kernels (fnx_advect_march.h): the planes of the compute window are cut into chunks so that the
// launch is a whole number of rounds of resident workgroups (3 per CU); a chunk re-reads 2 lead-in planes.
void tile_launch_geometry(const GridDims& g, int& ntx, int& nty, int& zchunk, unsigned& G) {
  const int slots = 3 * cu_count();
  ntx = (g.W + 63) / 64; nty = (g.H + ATR - 1) / ATR;
  const long ntiles = (long)ntx * nty * g.B;
  long nzc = (2l * slots + ntiles - 1) / ntiles;          // two rounds of workgroups
  if (nzc < 1) nzc = 1;
  zchunk = (int)((g.KN + nzc - 1) / nzc);
  if (zchunk < 8) zchunk = g.KN < 8 ? g.KN : 8;
  nzc = (g.KN + zchunk - 1) / zchunk;
  long n = ntiles * nzc;
  G = (unsigned)(((n + 7) / 8) * 8);
}

// The one dispatch of run-time choices to template arguments: `k` is a generic lambda that receives IS3D, QUIRKS, SAMPLE_OUTSIDE
// and WHAT as IC<> constants (fnx_cells.h)
template <class K> void with_what(int what, K k) {
  if (what == fnx::ADVECT_BOTH) k(IC<fnx::ADVECT_BOTH>{}); else if (what == fnx::ADVECT_RHO) k(IC<fnx::ADVECT_RHO>{}); else k(IC<fnx::ADVECT_VEL>{});
}
template <class K> void dispatch(const fnx::AdvectPlan& p, bool sample_outside, K k) {
  with_semantics(p.is3d, p.quirks, sample_outside, [&](auto is3d, auto quirks, auto outside) {
    with_what(p.what, [&](auto what) { k(is3d, quirks, outside, what); });
  });
}

}  // namespace

namespace fnx {

// Which kernels an advection call runs.
// 3D default semantics: the z-marching LDS tile kernels (fnx_advect_march.h); quirks mode and plane ranges beyond the
// tile kernels' 32-bit offsets: one thread per cell
// 2D: LDS tile kernels (fnx_advect_tile2d.h) on grids large enough to pay for the two fix-up launches (measured, advection per
// step, tiles vs one thread per cell: 2048^2 105 vs 129 us, 1024^2 38.6 vs 37.2, 128^2 17.6 vs 12.6), wherever a row offset
// fits the tiles' 32-bit buffer offsets
AdvectPlan advect_plan(const GridDims& g, bool is3d, bool quirks, int what, bool orig_is_U, int method, int request) {
  AdvectPlan p;
  p.g = p.gfwd = g;
  p.is3d = is3d; p.quirks = is3d && quirks; p.what = what;
  p.maccormack = method == FNX_ADVECT_MACCORMACK;
  p.fwd = p.bwd = AdvectPath::CELLS;
  p.bwd_fused = false;
  // one thread per cell: the pair runs advect_fwd_kernel / advect_bwd_kernel (phase-ordered velocity passes outside quirks mode), a
  // stand-alone advection sl_scalar_kernel / sl_scalar_bwd_clamp_kernel or sl_mac_kernel / sl_mac_bwd_clamp_kernel
  p.cells_pair = what == ADVECT_BOTH;
  if (!p.maccormack) return p;                           // Euler: the forward pass alone, on the compute window, straight into dst
  p.gfwd = widened(g, 2);                                // what the backward pass / clamp read at |U dt| <= 1
  const bool want_tiles = request == FNX_ADVECT_PLAN_TILES || request == FNX_ADVECT_PLAN_TILES_SPLIT ||
                          (request == FNX_ADVECT_PLAN_AUTO && (is3d || (size_t)g.HW * g.B >= ((size_t)3 << 19)));
  // the tile kernels advect U by itself (every call of simulate.py:93 without viscosity); advect_vel of another field stays per cell
  if (!want_tiles || (what == ADVECT_VEL && !orig_is_U)) return p;
  if (!is3d) {
    if ((size_t)g.HW < 0x3fffffffu) p.fwd = p.bwd = AdvectPath::TILES_2D;
    return p;
  }
  if (p.quirks) return p;
  const bool fwd_fits = (size_t)(p.gfwd.KN + 2) * p.gfwd.HW < 0x3fffffffu, bwd_fits = (size_t)(g.KN + 2) * g.HW < 0x3fffffffu;
  // the pair takes the tiles for whichever pass fits (its per-cell kernels and the tile kernels exchange the same fields); a
  // stand-alone advection takes them only when both passes fit
  if (what != ADVECT_BOTH && !(fwd_fits && bwd_fits)) return p;
  if (fwd_fits) p.fwd = AdvectPath::TILES_3D;
  if (bwd_fits) p.bwd = AdvectPath::TILES_3D;
  // The 3D backward pass of the pair is ONE march for density and velocity (advect3d_bwd_tile_kernel, round 6): 761-769 against 772-775 us
  // per pair of a developed 512 x 512 x 64 plume in alternating rounds on one box (profiles/r06/b_advect_ab_alternating.txt) -- 1 %: the
  // marches are VALU-issue bound and the fused one issues 96 % of their instructions; the traffic it saves was not the bound.
  // FNX_ADVECT_PLAN_TILES_SPLIT keeps the two separate marches (what the stand-alone advections run) for A/B timing.
  p.bwd_fused = bwd_fits && what == ADVECT_BOTH && request != FNX_ADVECT_PLAN_TILES_SPLIT;
  return p;
}

AdvectWs advect_workspace(const GridDims& g, bool is3d, int what, void* base) {
  AdvectWs w{};
  const size_t n = (size_t)g.B * g.DHW;
  auto take = [&](size_t bytes) { void* r = base ? (char*)base + w.bytes : nullptr; w.bytes += al(bytes); return r; };
  if (what & ADVECT_RHO) {
    w.rho_fwd = (float*)take(n * 4);
    w.cell = (int*)take(n * 4);
    if (is3d) w.box = (float2*)take(n * 8);              // 2D: the 3x3 clamp box is walked in the backward kernel
  }
  if (what & ADVECT_VEL) w.U_fwd = (float*)take(n * 4 * (is3d ? 3 : 2));
  w.fix = (unsigned long long*)take(4 * 8 * fix_words(g));
  return w;
}

void launch_box_minmax(const GridDims& g, int channels, bool sample_outside, const float* src, const float* flags, float2* box,
                       hipStream_t s) {
  const int nzc = (g.KN + BOX_ZC - 1) / BOX_ZC;
  const dim3 grid((g.W + 61) / 62, (g.H + 4 * BOX_R - 1) / (4 * BOX_R), g.B * channels * nzc);
  with_flag(sample_outside, [&](auto outside) {
    box_minmax_kernel<decltype(outside)::value><<<grid, dim3(64, 4), 0, s>>>(g, channels, src, flags, box, nzc);
  });
}

// MacCormack: forward pass(es) on p.gfwd into the workspace, backward pass fused with the correction and the clamp on p.g into dst;
// the density and the velocity of a pair both by the OLD U (simulate.py:75-93).  Euler: the forward pass into dst.
void launch_advect(const AdvectPlan& p, const AdvectArgs& a, const AdvectWs& w, hipStream_t s) {
  const GridDims &g = p.g, &gf = p.gfwd;
  const float dt = a.dt, half_s = a.half_s;
  const dim3 block(BX, BY);
  const bool do_s = p.what & ADVECT_RHO, do_v = p.what & ADVECT_VEL, mac = p.maccormack;
  float* const rho_fwd = mac ? w.rho_fwd : a.rho_dst;
  float* const U_fwd = mac ? w.U_fwd : a.U_dst;
  const size_t nwords = fix_words(g);
  unsigned long long *ff_s = do_s ? w.fix : nullptr, *ff_v = do_v ? w.fix + nwords : nullptr;
  unsigned long long *fb_s = do_s ? w.fix + 2 * nwords : nullptr, *fb_v = do_v ? w.fix + 3 * nwords : nullptr;
  dispatch(p, a.sample_outside, [&](auto is3d_, auto quirks_, auto outside_, auto what_) {
    constexpr bool IS3D = decltype(is3d_)::value, Q = decltype(quirks_)::value, SO = decltype(outside_)::value;
    constexpr int WH = decltype(what_)::value;
    // ---- forward
    if (p.fwd == AdvectPath::TILES_2D) {
      const int ntx = (g.W + 63) / 64, nty = (g.H + T2R - 1) / T2R;
      const unsigned nfix = (unsigned)(((size_t)g.B * g.H * ntx + 255) / 256);
      advect2d_fwd_tile_kernel<SO, WH><<<dim3((unsigned)(ntx * nty * g.B)), 64 * T2NW, 0, s>>>(g, dt, a.rho, a.U, a.flags, rho_fwd, w.cell, U_fwd, ff_s, ff_v, ntx, nty);
      advect2d_fwd_fix_kernel<SO><<<nfix, 256, 0, s>>>(g, dt, a.rho, a.U, a.flags, rho_fwd, w.cell, U_fwd, ff_s, ff_v, ntx);
    } else if (p.fwd == AdvectPath::TILES_3D) {
      // (the tile kernel also reduces the clamp bounds of the density step from the rho planes it streams)
      int ntx, nty, zchunk; unsigned G;
      tile_launch_geometry(gf, ntx, nty, zchunk, G);
      const unsigned nfix = (unsigned)(((size_t)gf.B * gf.KN * gf.H * ntx + 255) / 256);
      advect3d_fwd_tile_kernel<SO, WH><<<dim3(G), 64 * ATNW, 0, s>>>(gf, dt, a.rho, a.U, a.flags, rho_fwd, w.cell, U_fwd, w.box, ff_s, ff_v, ntx, nty, zchunk);
      advect3d_fwd_fix_kernel<SO><<<dim3(nfix), 256, 0, s>>>(gf, dt, a.rho, a.U, a.flags, rho_fwd, w.cell, U_fwd, ff_s, ff_v, ntx);
    } else {
      if (p.cells_pair) advect_fwd_kernel<IS3D, Q, SO><<<cell_grid(gf), block, 0, s>>>(gf, dt, a.rho, a.U, a.flags, rho_fwd, w.cell, U_fwd);
      if (!p.cells_pair && do_s) sl_scalar_kernel<IS3D, Q, SO><<<cell_grid(gf), block, 0, s>>>(gf, dt, a.rho, a.U, a.flags, rho_fwd, w.cell);
      if (!p.cells_pair && do_v) sl_mac_kernel<IS3D, Q><<<cell_grid(gf), block, 0, s>>>(gf, dt, a.orig, a.U, a.flags, U_fwd);
      if constexpr (IS3D)                                // the clamp bounds of the density step as a field
        if (mac && do_s) launch_box_minmax(gf, 1, SO, a.rho, a.flags, w.box, s);
    }
    if (!mac) return;
    // ---- backward, correction and clamp
    if (p.bwd == AdvectPath::TILES_2D) {
      const int ntx = (g.W + 63) / 64, nty = (g.H + T2R - 1) / T2R;
      const unsigned nfix = (unsigned)(((size_t)g.B * g.H * ntx + 255) / 256);
      advect2d_bwd_tile_kernel<SO, WH><<<dim3((unsigned)(ntx * nty * g.B)), 64 * T2NW, 0, s>>>(g, dt, half_s, a.rho, rho_fwd, w.cell, a.U, U_fwd, a.flags, a.rho_dst, a.U_dst, fb_s, fb_v, ntx, nty);
      advect2d_bwd_fix_kernel<SO><<<nfix, 256, 0, s>>>(g, dt, half_s, a.rho, rho_fwd, w.cell, a.U, U_fwd, a.flags, a.rho_dst, a.U_dst, fb_s, fb_v, ntx);
    } else if (p.bwd == AdvectPath::TILES_3D) {
      int ntx, nty, zchunk; unsigned G;
      tile_launch_geometry(g, ntx, nty, zchunk, G);
      const unsigned nfix = (unsigned)(((size_t)g.B * g.KN * g.H * ntx + 255) / 256);
      if (p.bwd_fused) advect3d_bwd_tile_kernel<SO><<<dim3(G), 64 * ATNW, 0, s>>>(g, dt, half_s, a.rho, rho_fwd, w.cell, a.U, U_fwd, a.flags, w.box, a.rho_dst, a.U_dst, fb_s, fb_v, ntx, nty, zchunk);
      if (!p.bwd_fused && do_s) advect3d_bwd_scalar_tile_kernel<SO><<<dim3(G), 64 * ATNW, 0, s>>>(g, dt, half_s, a.rho, rho_fwd, w.cell, a.U, a.flags, w.box, a.rho_dst, fb_s, ntx, nty, zchunk);
      if (!p.bwd_fused && do_v) advect3d_bwd_vel_tile_kernel<<<dim3(G), 64 * ATNW, 0, s>>>(g, dt, half_s, a.U, U_fwd, a.flags, a.U_dst, fb_v, ntx, nty, zchunk);
      advect3d_bwd_fix_kernel<SO><<<dim3(nfix), 256, 0, s>>>(g, dt, half_s, a.rho, rho_fwd, w.cell, a.U, U_fwd, a.flags, w.box, a.rho_dst, a.U_dst, fb_s, fb_v, ntx);
    } else {
      if (p.cells_pair) advect_bwd_kernel<IS3D, Q, SO><<<cell_grid(g), block, 0, s>>>(g, dt, half_s, a.rho, rho_fwd, w.cell, a.U, U_fwd, a.flags, w.box, a.rho_dst, a.U_dst);
      if (!p.cells_pair && do_s) sl_scalar_bwd_clamp_kernel<IS3D, Q, SO><<<cell_grid(g), block, 0, s>>>(g, dt, half_s, a.rho, rho_fwd, w.cell, a.U, a.flags, w.box, a.rho_dst);
      if (!p.cells_pair && do_v) sl_mac_bwd_clamp_kernel<IS3D, Q><<<cell_grid(g), block, 0, s>>>(g, dt, half_s, a.orig, U_fwd, a.U, a.flags, a.U_dst);
    }
  });
}

}  // namespace fnx
