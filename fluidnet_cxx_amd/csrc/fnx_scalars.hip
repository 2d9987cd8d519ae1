// Passive scalar transport for gfx950: C fields through ONE pair of obstacle-aware line traces.
//
// fnx_advect.hip advects one scalar per call, and what a call spends most of its instructions on -- the centred velocity, the line
// trace, the Lerp weights, the fluid bits of the interpolation corners, the validity of the clamp neighbourhood -- depends on U, flags
// and dt alone.  Here a thread does that once per pass and pushes every channel through the same sample points.  The per-channel
// arithmetic is, operand for operand and parenthesis for parenthesis, that of interpol / interpol_with_fluid (fnx_device.h) and of
// sl_scalar_cell / sl_scalar_bwd_clamp_cell (fnx_advect.hip): every channel comes out with the bits fnx_advect_scalar gives for it
// alone.  One thread per cell, x fastest; whole single domains only (the C ABI refuses compute windows and z-slab views).
//
// Channels go in compile-time chunks of CHUNK (a remainder chunk of 1..CHUNK-1 behind it): per-channel values live in arrays indexed by
// unrolled loops only, and a chunk's corner loads are all written ahead of the first use.
//
// MacCormack is a forward launch, in 3D a launch that reduces every channel's clamp bounds to a field, and a backward launch.
//
// Bit-parity: see fnx_device.h.  Compiled with -ffp-contract=off.  No atomics.
#include "../../include/fluidnet_hip.h"
#include "fnx_device.h"
#include "fnx_kernels.h"

namespace {

constexpr int BX = 64, BY = 4;
// Channels per chunk.  Measured on a developed plume with 1, 2 and 4: a chunk of 4 holds 32 corner values and costs the
// 3D kernels half of their waves (106-133 VGPRs, 3-4 waves per SIMD, against 42-58 and 8), and the line trace -- a chain of
// dependent flag loads -- lives on occupancy: one channel at a time was the fastest at every size but one (128^3, C = 8: 2 was 4 %
// ahead).  The chunk code below is written for any CHUNK <= 4.
constexpr int CHUNK = 1;

struct CellId { int b, k, j, i; bool valid; };

template <bool IS3D>
__device__ __forceinline__ CellId cell_id(const GridDims& g) {
  CellId c;
  c.i = blockIdx.x * BX + threadIdx.x;
  c.j = blockIdx.y * BY + threadIdx.y;
  const int bk = blockIdx.z;
  c.b = IS3D ? bk / g.D : bk;
  c.k = IS3D ? bk - c.b * g.D : 0;
  c.valid = (c.i < g.W) & (c.j < g.H);
  return c;
}

// What a sample at one traced position needs besides the field: weights, the offset of corner a and the corners' fluid bits
// (bit 0..7 = a b c d e f g h of interpol_with_fluid: a = (x0,y0), b = (x0,y0+1), c = (x0+1,y0), d = (x0+1,y0+1), e..h one plane up)
struct Recipe { Lerp L; int o; unsigned fl; };

template <bool IS3D, bool QUIRKS, bool SAMPLE_OUTSIDE>
__device__ __forceinline__ Recipe make_recipe(const GridDims& g, const Field& ff, const float p[3]) {
  Recipe r;
  r.L = lerp_setup<IS3D>(g, p[0], p[1], p[2]);
  r.o = r.L.z0 * g.HW + r.L.y0 * g.W + r.L.x0;          // < DHW < 2^31
  r.fl = 0xffu;
  if (!SAMPLE_OUTSIDE) {
    const float* m = ff.p + r.o;
    unsigned fl = (m[0] == FNX_FLUID ? 1u : 0u) | (m[g.W] == FNX_FLUID ? 2u : 0u) | (m[1] == FNX_FLUID ? 4u : 0u) |
                  (m[g.W + 1] == FNX_FLUID ? 8u : 0u);
    if (IS3D) {
      const float* n = m + g.HW;
      const bool fe = n[0] == FNX_FLUID, f_ = n[g.W] == FNX_FLUID;
      // Q15: grid.cpp:204-205 reads the g/h flags at x0 instead of x0+1
      const bool fg = QUIRKS ? fe : (n[1] == FNX_FLUID), fh = QUIRKS ? f_ : (n[g.W + 1] == FNX_FLUID);
      fl |= (fe ? 16u : 0u) | (f_ ? 32u : 0u) | (fg ? 64u : 0u) | (fh ? 128u : 0u);
    }
    r.fl = fl;
  }
  return r;
}

template <bool IS3D>
__device__ __forceinline__ void load_corners(const GridDims& g, const float* __restrict__ q, float I[8]) {
  I[0] = q[0]; I[1] = q[g.W]; I[2] = q[1]; I[3] = q[g.W + 1];
  if (IS3D) { const float* r = q + g.HW; I[4] = r[0]; I[5] = r[g.W]; I[6] = r[1]; I[7] = r[g.W + 1]; }
}

// interpol (SAMPLE_OUTSIDE) / interpol_with_fluid of fnx_device.h on loaded corners
template <bool IS3D, bool SAMPLE_OUTSIDE>
__device__ __forceinline__ float sample(const Lerp& L, unsigned fl, const float I[8]) {
  const float Ia = I[0], Ib = I[1], Ic = I[2], Id = I[3];
  float plain = (Ia * L.t0 + Ib * L.t1) * L.s0 + (Ic * L.t0 + Id * L.t1) * L.s1;
  if (SAMPLE_OUTSIDE) {
    if (!IS3D) return plain;
    const float hi = (I[4] * L.t0 + I[5] * L.t1) * L.s0 + (I[6] * L.t0 + I[7] * L.t1) * L.s1;
    return plain * L.f0 + hi * L.f1;
  }
  float vab, vcd, v; bool fab, fcd, flu;
  lerp1d_fluid(Ia, (fl & 1u) != 0, Ib, (fl & 2u) != 0, L.t0, L.t1, vab, fab);
  lerp1d_fluid(Ic, (fl & 4u) != 0, Id, (fl & 8u) != 0, L.t0, L.t1, vcd, fcd);
  lerp1d_fluid(vab, fab, vcd, fcd, L.s0, L.s1, v, flu);
  if (IS3D) {
    const float Ie = I[4], If = I[5], Ig = I[6], Ih = I[7];
    float vef, vgh, vhi; bool fef, fgh, fhi;
    lerp1d_fluid(Ie, (fl & 16u) != 0, If, (fl & 32u) != 0, L.t0, L.t1, vef, fef);
    lerp1d_fluid(Ig, (fl & 64u) != 0, Ih, (fl & 128u) != 0, L.t0, L.t1, vgh, fgh);
    lerp1d_fluid(vef, fef, vgh, fgh, L.s0, L.s1, vhi, fhi);
    const float vlo = v; const bool flo = flu;
    lerp1d_fluid(vlo, flo, vhi, fhi, L.f0, L.f1, v, flu);
    const float hi = (Ie * L.t0 + If * L.t1) * L.s0 + (Ig * L.t0 + Ih * L.t1) * L.s1;
    plain = plain * L.f0 + hi * L.f1;
  }
  return flu ? v : plain;
}

// the traced position of an interior fluid cell (sl_scalar_cell: disp = (-dt) * centred velocity), `p` = the cell centre elsewhere
template <bool IS3D>
__device__ __forceinline__ void trace(const GridDims& g, const Field& fu, const Field& ff, const CellId& c, float mdt, float p[3]) {
  const float ctr[3] = { (float)c.i + 0.5f, (float)c.j + 0.5f, (float)(c.k + g.zoff) + 0.5f };
  float cen[3], disp[3];
  get_centered<IS3D>(g, fu, c.i, c.j, c.k, cen);
#pragma unroll
  for (int a = 0; a < 3; ++a) disp[a] = mdt * cen[a];
  line_trace(g, ff, ctr, disp, p);
}

// ---------------------------------------------------------------------------------------------------
// Forward pass: border -> 0, non-fluid -> copy, fluid -> the sample at the traced position
// ---------------------------------------------------------------------------------------------------
template <bool IS3D, bool SAMPLE_OUTSIDE, int N>
__device__ __forceinline__ void fwd_chunk(const GridDims& g, const float* __restrict__ s, float* __restrict__ d, int o, const Recipe& r,
                                          bool border, bool fluid) {
  float I[N][8], own[N];
#pragma unroll
  for (int n = 0; n < N; ++n) {
    const float* sn = s + (size_t)n * g.DHW;
    load_corners<IS3D>(g, sn + r.o, I[n]);
    own[n] = sn[o];
  }
#pragma unroll
  for (int n = 0; n < N; ++n) {
    const float smp = sample<IS3D, SAMPLE_OUTSIDE>(r.L, r.fl, I[n]);
    d[(size_t)n * g.DHW + o] = border ? 0.f : (fluid ? smp : own[n]);      // "don't advect solid geometry"
  }
}

template <bool IS3D, bool QUIRKS, bool SAMPLE_OUTSIDE>
__global__ __launch_bounds__(BX* BY) void advect_scalars_fwd_kernel(GridDims g, float dt, int C, const float* __restrict__ src,
                                                                    const float* __restrict__ U, const float* __restrict__ flags,
                                                                    float* __restrict__ dst, int* __restrict__ cell_out) {
  const CellId c = cell_id<IS3D>(g);
  if (!c.valid) return;
  constexpr int NC = IS3D ? 3 : 2;
  const Field ff{flags + (size_t)c.b * g.DHW}, fu{U + (size_t)c.b * NC * g.DHW};
  const int o = c.k * g.HW + c.j * g.W + c.i;
  float p[3] = { (float)c.i + 0.5f, (float)c.j + 0.5f, (float)(c.k + g.zoff) + 0.5f };
  const bool border = is_border<IS3D>(g, c.i, c.j, c.k);
  const bool fluid = !border && ff.p[o] == FNX_FLUID;
  if (fluid) trace<IS3D>(g, fu, ff, c, -dt, p);
  if (cell_out) {                                       // packed exactly as sl_scalar_cell packs it
    const int i0 = clampi((int)p[0], 0, g.W - 1), j0 = clampi((int)p[1], 0, g.H - 1);
    const int k0 = (IS3D && !QUIRKS) ? clampi((int)p[2], 0, g.Dglob - 1) - g.zoff : -g.zoff;      // Q10
    cell_out[(size_t)c.b * g.DHW + o] = IS3D ? (k0 + 1) * g.HW + j0 * g.W + i0 : ((j0 << 16) | i0);
  }
  // (a border or non-fluid cell samples at its own centre -- clamped addresses, the value is dropped by the select)
  const Recipe r = make_recipe<IS3D, QUIRKS, SAMPLE_OUTSIDE>(g, ff, p);
  const float* s = src + (size_t)c.b * C * g.DHW;
  float* d = dst + (size_t)c.b * C * g.DHW;
  int ch = 0;
  for (; ch + CHUNK <= C; ch += CHUNK)
    fwd_chunk<IS3D, SAMPLE_OUTSIDE, CHUNK>(g, s + (size_t)ch * g.DHW, d + (size_t)ch * g.DHW, o, r, border, fluid);
  s += (size_t)ch * g.DHW; d += (size_t)ch * g.DHW;
  const int rem = C - ch;                               // < CHUNK
  if constexpr (CHUNK > 3) if (rem == 3) fwd_chunk<IS3D, SAMPLE_OUTSIDE, 3>(g, s, d, o, r, border, fluid);
  if constexpr (CHUNK > 2) if (rem == 2) fwd_chunk<IS3D, SAMPLE_OUTSIDE, 2>(g, s, d, o, r, border, fluid);
  if constexpr (CHUNK > 1) if (rem == 1) fwd_chunk<IS3D, SAMPLE_OUTSIDE, 1>(g, s, d, o, r, border, fluid);
}

// ---------------------------------------------------------------------------------------------------
// 3D clamp bounds as a field per channel, the reduction of box_minmax_kernel (fnx_advect.hip) over the B * C planes stacks: for every
// cell the min / max of its channel over the 3x3x3 box clipped to the grid, taken over the cells that are fluid (unless
// sample_outside_fluid); "no cell qualified" is mn = NaN.  min / max are exact, commutative and NaN-ignoring, so the separable
// evaluation gives the bits of the reference's 27-step fold.  A wave covers 62 columns (lanes 0 / 63 are halo columns) x BOX_R rows and
// marches along z with the xy-reduced planes k-1, k, k+1 in registers.  The backward kernel then fetches ONE 8-byte pair per channel
// at the traced cell: walking the 27 cells per channel there instead took 2152 against 1238 us for four channels at 256^3.
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
__global__ __launch_bounds__(256) void advect_scalars_box_kernel(GridDims g, int C, const float* __restrict__ src,
                                                                 const float* __restrict__ flags, float2* __restrict__ box, int nzc) {
  const int lane = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.y);
  const int x = blockIdx.x * 62 - 1 + lane;
  const int j0 = (blockIdx.y * 4 + w) * BOX_R;
  const int bz = blockIdx.z;
  const int zc = bz % nzc, bc = bz / nzc;                 // bc: plane stack b * C + c of src and box
  const int k_lo = zc * BOX_ZC, k_hi = min(k_lo + BOX_ZC, g.D);
  if (j0 >= g.H) return;
  const bool xin = (x >= 0) & (x < g.W);
  const int xc = clampi(x, 0, g.W - 1);
  const size_t base = (size_t)bc * g.DHW, fbase = (size_t)(bc / C) * g.DHW;
  // all loads of a plane are unconditional (clamped rows / planes) so they issue back to back; validity only gates `ok`
  auto plane = [&](int k, float* omn, float* omx, unsigned* oan) {
    float sv[BOX_R + 2], fv[BOX_R + 2];
    const bool kin = (k >= 0) & (k < g.D);
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

// ---------------------------------------------------------------------------------------------------
// Backward pass on fwd + MacCormackCorrect + MacCormackClampFluidNet (sl_scalar_bwd_clamp_cell).  The clamp neighbourhood is the
// 3x3(x3) box around the traced cell of the forward pass.  3D: the channel's bounds are in `box` (above).  2D: which of the 9 cells
// count (in the domain and, unless sample_outside_fluid, fluid) is one bit mask per thread, `m` (bit (dj+1)*3 + (di+1)); the channels
// walk the box with clamped addresses in the reference's order.
// ---------------------------------------------------------------------------------------------------
struct Box { int j0, i0; unsigned m; int cell; };        // 2D: j0, i0, m;  3D: cell = the offset of the traced cell in its plane stack

template <bool IS3D, bool SAMPLE_OUTSIDE, int N>
__device__ __forceinline__ void bwd_chunk(const GridDims& g, float half_s, const float* __restrict__ s, const float* __restrict__ fw,
                                          const float2* __restrict__ box, float* __restrict__ d, int o, const Recipe& r, bool border,
                                          bool fluid, const Box& bx) {
  float I[N][8], own[N], f[N];
  float2 bb[N];
#pragma unroll
  for (int n = 0; n < N; ++n) {
    load_corners<IS3D>(g, fw + (size_t)n * g.DHW + r.o, I[n]);
    own[n] = s[(size_t)n * g.DHW + o];
    f[n] = fw[(size_t)n * g.DHW + o];
    if (IS3D) bb[n] = box[(size_t)n * g.DHW + bx.cell];
  }
  float dd[N];
#pragma unroll
  for (int n = 0; n < N; ++n) {
    const float bwd = border ? 0.f : sample<IS3D, SAMPLE_OUTSIDE>(r.L, r.fl, I[n]);
    dd[n] = fluid ? f[n] + half_s * (own[n] - bwd) : f[n];          // applied on border cells too (reference :371)
  }
  if (!border) {
    float mn[N], mx[N];
    bool any[N];
    if (IS3D) {
#pragma unroll
      for (int n = 0; n < N; ++n) { mn[n] = bb[n].x; mx[n] = bb[n].y; any[n] = !(mn[n] != mn[n]); }
    } else {
#pragma unroll
      for (int n = 0; n < N; ++n) { mn[n] = INFINITY; mx[n] = -INFINITY; any[n] = bx.m != 0; }
#pragma unroll
      for (int dj = -1; dj <= 1; ++dj) {
        const int jc = clampi(bx.j0 + dj, 0, g.H - 1);
#pragma unroll
        for (int di = -1; di <= 1; ++di) {
          const int q = jc * g.W + clampi(bx.i0 + di, 0, g.W - 1);
          const bool ok = ((bx.m >> ((dj + 1) * 3 + (di + 1))) & 1u) != 0;
#pragma unroll
          for (int n = 0; n < N; ++n) {
            const float v = s[(size_t)n * g.DHW + q];
            mn[n] = ok ? fminf(mn[n], v) : mn[n];
            mx[n] = ok ? fmaxf(mx[n], v) : mx[n];
          }
        }
      }
    }
#pragma unroll
    for (int n = 0; n < N; ++n) dd[n] = any[n] ? fmaxf(mn[n], fminf(mx[n], dd[n])) : f[n];        // no cell qualified: the forward value
  }
#pragma unroll
  for (int n = 0; n < N; ++n) d[(size_t)n * g.DHW + o] = dd[n];
}

template <bool IS3D, bool QUIRKS, bool SAMPLE_OUTSIDE>
__global__ __launch_bounds__(BX* BY) void advect_scalars_bwd_kernel(GridDims g, float dt, float half_s, int C,
                                                                    const float* __restrict__ src, const float* __restrict__ fwd,
                                                                    const int* __restrict__ cell_in, const float* __restrict__ U,
                                                                    const float* __restrict__ flags, const float2* __restrict__ box,
                                                                    float* __restrict__ dst) {
  const CellId c = cell_id<IS3D>(g);
  if (!c.valid) return;
  constexpr int NC = IS3D ? 3 : 2;
  const Field ff{flags + (size_t)c.b * g.DHW}, fu{U + (size_t)c.b * NC * g.DHW};
  const int o = c.k * g.HW + c.j * g.W + c.i;
  float p[3] = { (float)c.i + 0.5f, (float)c.j + 0.5f, (float)(c.k + g.zoff) + 0.5f };
  const bool border = is_border<IS3D>(g, c.i, c.j, c.k);
  const bool fluid = ff.p[o] == FNX_FLUID;
  const float ndt = -dt;
  if (!border && fluid) trace<IS3D>(g, fu, ff, c, -ndt, p);
  const Recipe r = make_recipe<IS3D, QUIRKS, SAMPLE_OUTSIDE>(g, ff, p);
  Box bx{0, 0, 0u, 0};
  if (!border) {
    // traced cell: 3D (k0+1)*HW + j0*W + i0 with k0 a plane of this (whole) domain, 2D (j0 << 16) | i0
    const int cell = cell_in[(size_t)c.b * g.DHW + o];
    if (IS3D) {
      bx.cell = clampi(cell - g.HW, 0, g.DHW - 1);
    } else {
      bx.j0 = (int)((unsigned)cell >> 16); bx.i0 = cell & 0xffff;
#pragma unroll
      for (int dj = -1; dj <= 1; ++dj) {
        const int jj = bx.j0 + dj;
        const bool vj = (jj >= 0) & (jj < g.H);
        const int jc = clampi(jj, 0, g.H - 1);
#pragma unroll
        for (int di = -1; di <= 1; ++di) {
          const int ii = bx.i0 + di;
          const bool vi = vj & (ii >= 0) & (ii < g.W);
          const int q = jc * g.W + clampi(ii, 0, g.W - 1);
          const bool ok = vi & (SAMPLE_OUTSIDE || ff.p[q] == FNX_FLUID);
          bx.m |= ok ? (1u << ((dj + 1) * 3 + (di + 1))) : 0u;
        }
      }
    }
  }
  const float* s = src + (size_t)c.b * C * g.DHW;
  const float* fw = fwd + (size_t)c.b * C * g.DHW;
  const float2* bp = IS3D ? box + (size_t)c.b * C * g.DHW : nullptr;
  float* d = dst + (size_t)c.b * C * g.DHW;
  int ch = 0;
  for (; ch + CHUNK <= C; ch += CHUNK)
    bwd_chunk<IS3D, SAMPLE_OUTSIDE, CHUNK>(g, half_s, s + (size_t)ch * g.DHW, fw + (size_t)ch * g.DHW, bp + (size_t)ch * g.DHW,
                                           d + (size_t)ch * g.DHW, o, r, border, fluid, bx);
  s += (size_t)ch * g.DHW; fw += (size_t)ch * g.DHW; bp += (size_t)ch * g.DHW; d += (size_t)ch * g.DHW;
  const int rem = C - ch;                               // < CHUNK
  if constexpr (CHUNK > 3) if (rem == 3) bwd_chunk<IS3D, SAMPLE_OUTSIDE, 3>(g, half_s, s, fw, bp, d, o, r, border, fluid, bx);
  if constexpr (CHUNK > 2) if (rem == 2) bwd_chunk<IS3D, SAMPLE_OUTSIDE, 2>(g, half_s, s, fw, bp, d, o, r, border, fluid, bx);
  if constexpr (CHUNK > 1) if (rem == 1) bwd_chunk<IS3D, SAMPLE_OUTSIDE, 1>(g, half_s, s, fw, bp, d, o, r, border, fluid, bx);
}

inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

// run-time choices -> template arguments (quirks mode exists in 3D only, the rule of fnx_advect.hip)
template <int V> struct IC { static constexpr int value = V; };
template <class K> void with_flag(bool b, K k) { if (b) k(IC<1>{}); else k(IC<0>{}); }

}  // namespace

namespace fnx {

AdvectScalarsWs advect_scalars_workspace(const GridDims& g, bool is3d, int channels, void* base) {
  AdvectScalarsWs w{};
  const size_t n = (size_t)g.B * g.DHW;
  auto take = [&](size_t bytes) { void* r = base ? (char*)base + w.bytes : nullptr; w.bytes += al(bytes); return r; };
  w.fwd = (float*)take(n * 4 * (size_t)channels);
  w.cell = (int*)take(n * 4);
  if (is3d) w.box = (float2*)take(n * 8 * (size_t)channels);     // 2D: the 3x3 clamp box is walked in the backward kernel
  return w;
}

void launch_advect_scalars(const GridDims& g, bool is3d, bool quirks, bool maccormack, bool sample_outside, float dt, float half_s,
                           int channels, const float* src, const float* U, const float* flags, float* dst, const AdvectScalarsWs& w,
                           hipStream_t s) {
  const dim3 block(BX, BY), grid((g.W + BX - 1) / BX, (g.H + BY - 1) / BY, g.B * g.D);
  with_flag(is3d, [&](auto is3d_) {
    with_flag(is3d && quirks, [&](auto quirks_) {
      if constexpr (decltype(is3d_)::value || !decltype(quirks_)::value)
        with_flag(sample_outside, [&](auto outside_) {
          constexpr bool IS3D = decltype(is3d_)::value, Q = decltype(quirks_)::value, SO = decltype(outside_)::value;
          if (!maccormack) {                             // Euler: the forward pass straight into dst
            advect_scalars_fwd_kernel<IS3D, Q, SO><<<grid, block, 0, s>>>(g, dt, channels, src, U, flags, dst, nullptr);
            return;
          }
          advect_scalars_fwd_kernel<IS3D, Q, SO><<<grid, block, 0, s>>>(g, dt, channels, src, U, flags, w.fwd, w.cell);
          if constexpr (IS3D) {                          // the clamp bounds of every channel as a field
            const int nzc = (g.D + BOX_ZC - 1) / BOX_ZC;
            const dim3 bgrid((g.W + 61) / 62, (g.H + 4 * BOX_R - 1) / (4 * BOX_R), g.B * channels * nzc);
            advect_scalars_box_kernel<SO><<<bgrid, dim3(64, 4), 0, s>>>(g, channels, src, flags, w.box, nzc);
          }
          advect_scalars_bwd_kernel<IS3D, Q, SO><<<grid, block, 0, s>>>(g, dt, half_s, channels, src, w.fwd, w.cell, U, flags, w.box, dst);
        });
    });
  });
}

}  // namespace fnx
