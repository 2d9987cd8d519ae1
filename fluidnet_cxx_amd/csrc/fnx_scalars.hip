// Passive scalar transport for gfx950: C fields through ONE pair of obstacle-aware line traces.
//
// fnx_advect.hip advects one scalar per call, and what a call spends most of its instructions on -- the centred velocity, the line
// trace, the Lerp weights, the fluid bits of the interpolation corners, the validity of the clamp neighbourhood -- depends on U, flags
// and dt alone.  Here a thread does that once per pass and pushes every channel through the same sample points.  The per-channel
// arithmetic is, operand for operand and parenthesis for parenthesis, that of interpol / interpol_with_fluid (fnx_device.h) and of
// sl_scalar_cell / sl_scalar_bwd_clamp_cell (fnx_advect.hip): every channel comes out with the bits fnx_advect_scalar gives for it
// alone.  One thread per cell, x fastest (fnx_cells.h); whole single domains only (the C ABI refuses compute windows and z-slab views).
//
// Channels go one at a time.  Measured on a developed plume against compile-time chunks of 2 and 4 channels: a chunk of 4
// holds 32 corner values and costs the 3D kernels half of their waves (106-133 VGPRs, 3-4 waves per SIMD, against 42-58 and 8), and the
// line trace -- a chain of dependent flag loads -- lives on occupancy: one channel at a time was the fastest at every size but one
// (128^3, C = 8: 2 was 4 % ahead).
//
// MacCormack is a forward launch, in 3D a launch that reduces every channel's clamp bounds to a field (box_minmax_kernel of
// fnx_advect.hip over the B * C plane stacks), and a backward launch.
//
// Bit-parity: see fnx_device.h.  Compiled with -ffp-contract=off.  No atomics.
#include "../../include/fluidnet_hip.h"
#include "fnx_cells.h"
#include "fnx_device.h"
#include "fnx_kernels.h"

namespace {

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
  for (int ch = 0; ch < C; ++ch) {
    const float* sc = s + (size_t)ch * g.DHW;
    float I[8];
    load_corners<IS3D>(g, sc + r.o, I);
    const float own = sc[o];
    const float smp = sample<IS3D, SAMPLE_OUTSIDE>(r.L, r.fl, I);
    d[(size_t)ch * g.DHW + o] = border ? 0.f : (fluid ? smp : own);      // "don't advect solid geometry"
  }
}

// ---------------------------------------------------------------------------------------------------
// Backward pass on fwd + MacCormackCorrect + MacCormackClampFluidNet (sl_scalar_bwd_clamp_cell).  The clamp neighbourhood is the
// 3x3(x3) box around the traced cell of the forward pass.  3D: the channel's bounds are in `box`, ONE 8-byte pair per channel at the
// traced cell (walking the 27 cells per channel here instead took 2152 against 1238 us for four channels at 256^3).
// 2D: which of the 9 cells count (in the domain and, unless sample_outside_fluid, fluid) is one bit mask per thread, `m` (bit
// (dj+1)*3 + (di+1)); the channels walk the box with clamped addresses in the reference's order.
// ---------------------------------------------------------------------------------------------------
struct Box { int j0, i0; unsigned m; int cell; };        // 2D: j0, i0, m;  3D: cell = the offset of the traced cell in its plane stack

// one channel: s, fw, box, d are its plane stacks
template <bool IS3D, bool SAMPLE_OUTSIDE>
__device__ __forceinline__ void bwd_channel(const GridDims& g, float half_s, const float* __restrict__ s, const float* __restrict__ fw,
                                            const float2* __restrict__ box, float* __restrict__ d, int o, const Recipe& r, bool border,
                                            bool fluid, const Box& bx) {
  float I[8];
  load_corners<IS3D>(g, fw + r.o, I);
  const float own = s[o], f = fw[o];
  float2 bb;
  // The bounds load goes out with the corner loads.  Left to itself hipcc sinks it under `!border` below, behind the sample's arithmetic:
  // measured 5 to 7 % slower for C >= 2 at 128^3 and 256^3 (docs/history/r35_one_cell_idiom.md).  The empty asm pins it here.
  if (IS3D) { bb = box[bx.cell]; asm volatile("" : "+v"(bb.x), "+v"(bb.y)); }
  const float smp = sample<IS3D, SAMPLE_OUTSIDE>(r.L, r.fl, I);      // not under the select: the corner loads stay unconditional
  const float bwd = border ? 0.f : smp;
  float dd = fluid ? f + half_s * (own - bwd) : f;       // applied on border cells too (reference :371)
  if (!border) {
    float mn, mx;
    bool any;
    if (IS3D) {
      mn = bb.x; mx = bb.y; any = !(mn != mn);
    } else {
      mn = INFINITY; mx = -INFINITY; any = bx.m != 0;
#pragma unroll
      for (int dj = -1; dj <= 1; ++dj) {
        const int jc = clampi(bx.j0 + dj, 0, g.H - 1);
#pragma unroll
        for (int di = -1; di <= 1; ++di) {
          const int q = jc * g.W + clampi(bx.i0 + di, 0, g.W - 1);
          const bool ok = ((bx.m >> ((dj + 1) * 3 + (di + 1))) & 1u) != 0;
          const float v = s[q];
          mn = ok ? fminf(mn, v) : mn;
          mx = ok ? fmaxf(mx, v) : mx;
        }
      }
    }
    dd = any ? fmaxf(mn, fminf(mx, dd)) : f;             // no cell qualified: the forward value
  }
  d[o] = dd;
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
  for (int ch = 0; ch < C; ++ch) {
    const size_t co = (size_t)ch * g.DHW;                // the channel's plane stack
    bwd_channel<IS3D, SAMPLE_OUTSIDE>(g, half_s, s + co, fw + co, bp + co, d + co, o, r, border, fluid, bx);
  }
}

inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

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
  const dim3 block(BX, BY), grid = cell_grid(g);
  with_semantics(is3d, quirks, sample_outside, [&](auto is3d_, auto quirks_, auto outside_) {
    constexpr bool IS3D = decltype(is3d_)::value, Q = decltype(quirks_)::value, SO = decltype(outside_)::value;
    if (!maccormack) {                                   // Euler: the forward pass straight into dst
      advect_scalars_fwd_kernel<IS3D, Q, SO><<<grid, block, 0, s>>>(g, dt, channels, src, U, flags, dst, nullptr);
      return;
    }
    advect_scalars_fwd_kernel<IS3D, Q, SO><<<grid, block, 0, s>>>(g, dt, channels, src, U, flags, w.fwd, w.cell);
    if constexpr (IS3D) launch_box_minmax(g, channels, SO, src, flags, w.box, s);      // the clamp bounds of every channel as a field
    advect_scalars_bwd_kernel<IS3D, Q, SO><<<grid, block, 0, s>>>(g, dt, half_s, channels, src, w.fwd, w.cell, U, flags, w.box, dst);
  });
}

}  // namespace fnx
