// Training of the Conv3d bank net (fnx_banknet3d.hip; mconf['model'] = 'FluidNet3D'), exact fp32: a forward that also writes every ReLU
// output ("tape") and the backward with respect to the twelve parameter tensors.
//
//   forward   the inference forward's six launches aimed at the tape: conv1 and the five ReLU convolutions are fnx_banknet3d.hip's own
//             kernels with tape pointers where they took the workspace (bank3d_forward_front); the last launch is the convolution body
//             of fnx_banknet3d_tile.h under its `tail + tape` epilogue, which also stores b1, t, c2a, c2b and c3 from the accumulator
//             registers.  The same arithmetic in the same order, so p has the inference forward's bits.  No workspace.
//   backward  fifteen launches, then one reduction:
//     bank_tail_backward         convOut, conv3 and conv2 twice over the flattened D H W cells of a sample, 16 cells a wave: the 2D
//                                unit's bank_tail_bwd_kernel itself (see there for the operand maps), launched on the 1x1x1 block of
//                                this unit's packed_t through fnx_banknet_train.h.  g_t (B,16,D,H,W) goes to the workspace.
//     bank3d_pool_bwd_kernel     one streaming pass over g_t: g_b2 = (b2 > 0) x the sum of the 2x2x2 children, g_b4 = (b4 > 0) x the sum of
//                                the 4x4x4 children (in the order z, y, x), and g_t becomes g_b1 = g_t (b1 > 0) in place.
//     bank3d_conv_bwd_kernel     the forward's z-marching convolution body on the transposed, tap-flipped weights of packed_t with a zero
//                                bias: `mask` epilogue for g_h = convT(block.2)(g_b) (h > 0), `plain` for g_a = convT(block.0)(g_h), at each
//                                of the three levels with bank3d_conv_plan of that level.  Zero padding at the level's own border.
//     bank3d_wgrad_kernel        the weight gradient of one bank layer at one level, dW[tap][cout][cin] = sum over the level's cells of
//                                g_out[cout][cell] in[cin][cell + tap - 1]: per tap one v_mfma_f32_16x16x4_f32 per four cells of a row, the
//                                cells being K.  See WG_* below.  Six launches.
//     bank3d_conv1_bwd_kernel    g_a = (a > 0) (g_a1 + up2(g_a2) / 8 + up4(g_a4) / 64) into conv1's 864 weight and 16 bias gradients: VALU.
//     bank3d_reduce_kernel       adds the per-workgroup partial sums in index order in fp64 (a bank tensor's levels in the order quarter,
//                                half, full) and writes grad_blob.
// A launch with partial sums has min(work items, cap) workgroups and workgroup s takes the items s, s + n, ...: the split is a function of
// (B, D, H, W) alone (fnx_banknet3d_backward_plan).  No atomics, no host synchronisation; grad_p, x and the tape are only read.  Every
// index into an activation or gradient tensor is 64-bit.
#include "fnx_banknet_train.h"

namespace fnx {
// fnx_banknet3d.hip: conv1 (x -> a, a2, a4) and the five ReLU convolutions of the forward, into the eight tensors given
void bank3d_forward_front(int B, int D, int H, int W, const float* pk, const float* x, float* a, float* h, float* a2, float* h2, float* b2,
                          float* a4, float* h4, float* b4, hipStream_t s);

namespace {

// packed_t of the 3D net: fnx_banknet_train.h with 27 taps
__global__ void bank3d_pack_t_kernel(const float* __restrict__ blob, float* __restrict__ pt) {
  bank_pack_t(blob, pt, 27, B3_WB0, B3_WB2, B3_W2);
}

// ---- forward ----
__global__ __launch_bounds__(256, 2) void bank3d_tail_tape_kernel(const float* __restrict__ wpk, const float* __restrict__ bias,
                                                               const float* __restrict__ tail, const float* __restrict__ in, int d, int h,
                                                               int w, int tiles_y, int chunk, const float* __restrict__ l2,
                                                               const float* __restrict__ l4, float* __restrict__ p, Bank3dTapeOut tape) {
  bank3d_conv_body<EPI3_TAIL_TAPE>(wpk, bias, tail, in, d, h, w, tiles_y, chunk, nullptr, l2, l4, p, nullptr, tape);
}

void bank3d_forward_train(const FnxGrid* g, const void* packed, const float* x, float* p, float* tape, int /*mode*/, hipStream_t s) {
  const int B = g->B, D = g->D, H = g->H, W = g->W;
  const float* pk = (const float*)packed;
  const BankTapeLayout T = bank_tape_layout(3, B, D, H, W);
  auto at = [&](int n) { return tape + T.e[n].off; };
  ProfScope ps(FNX_PROF_CONV_MFMA16, s);
  bank3d_forward_front(B, D, H, W, pk, x, at(TP_A), at(TP_H1), at(TP_A2), at(TP_H2), at(TP_B2), at(TP_A4), at(TP_H4), at(TP_B4), s);
  const Bank3dConvPlan pl = bank3d_conv_plan(B, D, H, W);
  bank3d_tail_tape_kernel<<<dim3((unsigned)pl.tiles_x, (unsigned)(pl.tiles_y * pl.chunks), (unsigned)B), 256, 0, s>>>(
      pk + P3_WB2, pk + P3_BB2, pk + P3_W2, at(TP_H1), D, H, W, pl.tiles_y, pl.chunk, at(TP_B2), at(TP_B4), p,
      Bank3dTapeOut{at(TP_B1), at(TP_T), at(TP_C2A), at(TP_C2B), at(TP_C3)});
}

// ---- backward ----
constexpr int WG_SPLIT = 256;              // workgroups of a weight-gradient launch: one per CU (the tail's and conv1's: MAX_SPLIT)
// floats of a workgroup's partial sums (the tail's: TAIL_P of fnx_banknet_train.h)
constexpr int WG_P = 27 * 256 + 16;        // [tap 27][cout 16][cin 16], then the bias
constexpr int C1_P3 = 880;                 // conv1 in the blob's own order: [16][2][27], then the bias

// One thread per (sample, channel, quarter-level cell): its 4 x 4 x 4 children of g_t, four consecutive x at a time.
// gt (B,16,D,H,W) becomes g_b1 in place; gb2 (B,16,D/2,H/2,W/2), gb4 (B,16,D/4,H/4,W/4).
__global__ __launch_bounds__(256) void bank3d_pool_bwd_kernel(float* __restrict__ gt, const float* __restrict__ b1, const float* __restrict__ b2,
                                                              const float* __restrict__ b4, float* __restrict__ gb2, float* __restrict__ gb4,
                                                              int D, int H, int W, size_t total) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int D4 = D / 4, H4 = H / 4, W4 = W / 4, H2 = H / 2, W2 = W / 2;
  const int qx = (int)(i % W4), qy = (int)((i / W4) % H4), qz = (int)((i / ((size_t)W4 * H4)) % D4);
  const size_t bc = i / ((size_t)W4 * H4 * D4);                  // b * 16 + channel
  const size_t HW = (size_t)H * W;
  float* const g1 = gt + bc * D * HW;
  const float* const m1 = b1 + bc * D * HW;
  float s2[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) s2[k] = 0.f;
#pragma unroll
  for (int dz = 0; dz < 4; ++dz)
#pragma unroll
    for (int dy = 0; dy < 4; ++dy) {
      const size_t at = (size_t)(4 * qz + dz) * HW + (size_t)(4 * qy + dy) * W + 4 * qx;      // W is a multiple of 4: 16-byte aligned
      const float4 v = *reinterpret_cast<const float4*>(g1 + at);
      const float4 m = *reinterpret_cast<const float4*>(m1 + at);
      const int k = (dz >> 1) * 4 + (dy >> 1) * 2;
      s2[k] += v.x;                                               // a half-level cell's children in the order z, y, x
      s2[k] += v.y;
      s2[k + 1] += v.z;
      s2[k + 1] += v.w;
      *reinterpret_cast<float4*>(g1 + at) = make_float4(m.x > 0.f ? v.x : 0.f, m.y > 0.f ? v.y : 0.f, m.z > 0.f ? v.z : 0.f, m.w > 0.f ? v.w : 0.f);
    }
  float s4 = 0.f;
  const size_t lev2 = (size_t)(D / 2) * H2 * W2;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    s4 += s2[k];                                                  // the quarter-level cell: its eight half-level cells in the order z, y, x
    const size_t at = bc * lev2 + ((size_t)(2 * qz + (k >> 2)) * H2 + 2 * qy + ((k >> 1) & 1)) * W2 + 2 * qx + (k & 1);
    gb2[at] = b2[at] > 0.f ? s2[k] : 0.f;
  }
  gb4[i] = b4[i] > 0.f ? s4 : 0.f;
}

// the input gradients: in (B,16,d,h,w) -> out; MASK: masked by mask > 0
template <int EPI>
__global__ __launch_bounds__(256) void bank3d_conv_bwd_kernel(const float* __restrict__ wpk, const float* __restrict__ bias,
                                                              const float* __restrict__ in, int d, int h, int w, int tiles_y, int chunk,
                                                              float* __restrict__ out, const float* __restrict__ mask) {
  static_assert(EPI == EPI3_MASK || EPI == EPI3_PLAIN, "the backward's epilogues");
  bank3d_conv_body<EPI>(wpk, bias, nullptr, in, d, h, w, tiles_y, chunk, out, nullptr, nullptr, nullptr, mask, Bank3dTapeOut{});
}

// ---- the weight gradient of a bank layer at one level, marching along z ----
// A workgroup of four waves takes work items (sample, y tile, x tile, z chunk) of WG_TH x WG_TW cells and WG_CHUNK planes.  LDS holds a
// ring of three `in` planes (the tile + one halo cell, zero outside the level's domain, z included) and the g_out plane of the tile's own
// cells (zero outside the domain), both as [channel][cell]: both MFMA operands have the channel on the 16-lane axis and the cell on
// lane >> 4.  A step is four consecutive cells of a tile row: A = g_out at (channel lane & 15, cell x4 + (lane >> 4)), read once, and per
// tap B = `in` at the same lane map shifted by the tap: 27 MFMAs into 27 accumulators (108 registers), which live across all the items
// of the workgroup.  Only the tile's own cells are steps, so no halo cell, wrap column or out-of-domain position reaches A.
// While plane z is computed, plane z + 2 of `in` and plane z + 1 of g_out are on their way from HBM in registers.
constexpr int WG_TH = 4, WG_TW = 36, WG_CHUNK = 4;
constexpr int WG_PI = WG_TW + 2, WG_NI = (WG_TH + 2) * WG_PI;    // the `in` plane: pitch 38, 228 cells
constexpr int WG_PG = WG_TW, WG_NG = WG_TH * WG_PG;              // the g_out plane: pitch 36, 144 cells
constexpr int WG_SI = (WG_NI + 29) / 32 * 32 + 2;                // channel strides = 2 (mod 32): a half-wave reads channels c = 0 .. 15 at
constexpr int WG_SG = (WG_NG + 29) / 32 * 32 + 2;                //   cells n, n + 1, banks (2 c + n + {0, 1}) mod 32: 32 distinct banks
constexpr int WG_LI = (WG_NI + 15) / 16, WG_LG = WG_NG / 16;     // values of a plane per thread: 16 threads a channel
constexpr int WG_STEPS = WG_TH * (WG_TW / 4);                    // 36 steps a plane, nine a wave
constexpr int WG_LDS = 3 * 16 * WG_SI + 16 * WG_SG;
static_assert(WG_SI >= WG_NI && WG_SI % 32 == 2 && WG_SG >= WG_NG && WG_SG % 32 == 2, "channel strides");
static_assert(WG_TW % 4 == 0 && WG_NG % 16 == 0 && WG_STEPS % 4 == 0, "four cells a step, whole steps a wave");
static_assert(WG_LDS * 4 <= 64 * 1024 && WG_LDS >= 4 * 256 + 256, "static LDS; the waves' sums go through it");

struct Bank3dWgPlan { int tiles_x, tiles_y, chunks, items, groups; };
inline Bank3dWgPlan bank3d_wg_plan(int B, int d, int h, int w) {
  Bank3dWgPlan pl{};
  pl.tiles_x = (w + WG_TW - 1) / WG_TW;
  pl.tiles_y = (h + WG_TH - 1) / WG_TH;
  pl.chunks = (d + WG_CHUNK - 1) / WG_CHUNK;
  const long long items = (long long)B * pl.tiles_x * pl.tiles_y * pl.chunks;      // < 2^31: the entry points bound B and D H W
  pl.items = (int)items;
  pl.groups = items < WG_SPLIT ? (int)items : WG_SPLIT;
  return pl;
}

// gout, in (B,16,d,h,w) -> partial [gridDim.x][WG_P]
__global__ __launch_bounds__(256, 2) void bank3d_wgrad_kernel(const float* __restrict__ gout, const float* __restrict__ in, int d, int h, int w,
                                                              Bank3dWgPlan pl, float* __restrict__ partial) {
  __shared__ float lds[WG_LDS];
  float* const lg = lds + 3 * 16 * WG_SI;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lch = tid >> 4, lcell = tid & 15;                     // what this thread loads: channel lch, cells lcell + 16 j
  const size_t hw = (size_t)h * w, dhw = (size_t)d * hw;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[27];
#pragma unroll
  for (int t = 0; t < 27; ++t) acc[t] = zero4;
  float bs = 0.f;

  for (int item = blockIdx.x; item < pl.items; item += gridDim.x) {
    const int tx = item % pl.tiles_x, ty = (item / pl.tiles_x) % pl.tiles_y;
    const int zc = (item / (pl.tiles_x * pl.tiles_y)) % pl.chunks, b = item / (pl.tiles_x * pl.tiles_y * pl.chunks);
    const int x0 = tx * WG_TW, y0 = ty * WG_TH, z0 = zc * WG_CHUNK, z1 = min(d, z0 + WG_CHUNK);
    const float* inb = in + ((size_t)b * 16 + lch) * dhw;
    const float* gob = gout + ((size_t)b * 16 + lch) * dhw;
    // offsets inside a plane, relative to the tile's first cell (they fit an int: a plane has fewer than 2^31 cells)
    int ioff[WG_LI], goff[WG_LG];
    unsigned iok = 0, gok = 0;
#pragma unroll
    for (int j = 0; j < WG_LI; ++j) {
      const int n = lcell + 16 * j, gy = y0 - 1 + n / WG_PI, gx = x0 - 1 + n % WG_PI;
      const bool ok = n < WG_NI && gy >= 0 && gy < h && gx >= 0 && gx < w;
      ioff[j] = ok ? gy * w + gx : 0;
      if (ok) iok |= 1u << j;
    }
#pragma unroll
    for (int j = 0; j < WG_LG; ++j) {
      const int n = lcell + 16 * j, gy = y0 + n / WG_PG, gx = x0 + n % WG_PG;
      const bool ok = gy < h && gx < w;
      goff[j] = ok ? gy * w + gx : 0;
      if (ok) gok |= 1u << j;
    }
    float pi[WG_LI], pg[WG_LG];
    auto fetch_in = [&](int z) {                                  // plane z of `in`, zero outside the domain
      const bool zin = z >= 0 && z < d;
      const float* src = inb + (size_t)(zin ? z : 0) * hw;
#pragma unroll
      for (int j = 0; j < WG_LI; ++j) pi[j] = (zin && ((iok >> j) & 1)) ? src[ioff[j]] : 0.f;
    };
    auto stash_in = [&](int z) {                                  // into the slot of plane z: (z + 1) % 3  (z >= -1)
      float* dst = lds + ((z + 1) % 3) * 16 * WG_SI + lch * WG_SI + lcell;
#pragma unroll
      for (int j = 0; j < WG_LI; ++j)
        if (lcell + 16 * j < WG_NI) dst[16 * j] = pi[j];
    };
    auto fetch_g = [&](int z) {                                   // plane z of g_out (z0 <= z < z1)
      const float* src = gob + (size_t)z * hw;
#pragma unroll
      for (int j = 0; j < WG_LG; ++j) pg[j] = ((gok >> j) & 1) ? src[goff[j]] : 0.f;
    };
    auto stash_g = [&]() {
      float* dst = lg + lch * WG_SG + lcell;
#pragma unroll
      for (int j = 0; j < WG_LG; ++j) dst[16 * j] = pg[j];
    };

    __syncthreads();                                              // the previous item's reads are done
    for (int z = z0 - 1; z <= z0 + 1; ++z) {
      fetch_in(z);
      stash_in(z);
    }
    fetch_g(z0);
    stash_g();
    __syncthreads();
    for (int z = z0; z < z1; ++z) {
      const bool more = z + 1 < z1;
      if (more) {                                                 // in flight during the MFMAs
        fetch_in(z + 2);
        fetch_g(z + 1);
      }
#pragma unroll 1
      for (int step = wave; step < WG_STEPS; step += 4) {
        const int y = step / (WG_TW / 4), x4 = (step - y * (WG_TW / 4)) * 4 + g;
        const float av = lg[c * WG_SG + y * WG_PG + x4];
        bs += av;
#pragma unroll
        for (int dz = 0; dz < 3; ++dz) {
          const float* bp = lds + ((z + dz) % 3) * 16 * WG_SI + c * WG_SI + y * WG_PI + x4;      // the slot of plane z - 1 + dz
#pragma unroll
          for (int t = 0; t < 9; ++t)
            acc[dz * 9 + t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bp[(t / 3) * WG_PI + (t % 3)], acc[dz * 9 + t], 0, 0, 0);
        }
      }
      __syncthreads();                                            // every wave is done with plane z - 1 and with g_out of plane z
      if (more) {
        stash_in(z + 2);                                          // the slot of plane z - 1
        stash_g();
      }
      __syncthreads();
    }
  }
  // the four waves in order, one tap at a time: D register r is row cout = 4g + r, column cin = c
  float* const po = partial + (size_t)blockIdx.x * WG_P;
#pragma unroll
  for (int t = 0; t < 27; ++t) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) lds[wave * 256 + (4 * g + r) * 16 + c] = acc[t][r];
    __syncthreads();
    po[t * 256 + tid] = (lds[tid] + lds[256 + tid]) + (lds[512 + tid] + lds[768 + tid]);
  }
  __syncthreads();
  lds[wave * 64 + lane] = bs;                                     // per (channel c, cell slot g)
  __syncthreads();
  if (tid < 16) {
    float v = 0.f;
    for (int wv = 0; wv < 4; ++wv)
      for (int k = 0; k < 4; ++k) v += lds[wv * 64 + k * 16 + tid];
    po[27 * 256 + tid] = v;
  }
}

// wave w: output channels 4w .. 4w+3; a lane: one cell of a unit of 64; blockIdx.y: conv1's input channel
__global__ __launch_bounds__(256) void bank3d_conv1_bwd_kernel(const float* __restrict__ x, const float* __restrict__ a,
                                                               const float* __restrict__ ga1, const float* __restrict__ ga2,
                                                               const float* __restrict__ ga4, float* __restrict__ partial, int D, int H, int W,
                                                               int ups, int nunits) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ci = blockIdx.y;
  const int N = D * H * W, HW = H * W, D2 = D / 2, H2 = H / 2, W2 = W / 2, D4 = D / 4, H4 = H / 4, W4 = W / 4;
  float acc[4][27], bs[4];
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) {
    bs[ch] = 0.f;
#pragma unroll
    for (int k = 0; k < 27; ++k) acc[ch][k] = 0.f;
  }
  for (int u = blockIdx.x; u < nunits; u += gridDim.x) {
    const int b = u / ups, n = (u - b * ups) * 64 + lane;
    if (n >= N) continue;
    const int z = n / HW, rem = n - z * HW, y = rem / W, xx = rem - y * W;
    const float* xb = x + ((size_t)b * 2 + ci) * N;
    float in[27];
#pragma unroll
    for (int dz = 0; dz < 3; ++dz)
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const int zz = z + dz - 1, yy = y + dy - 1, xc = xx + dx - 1;
          const bool inside = zz >= 0 && zz < D && yy >= 0 && yy < H && xc >= 0 && xc < W;
          in[dz * 9 + dy * 3 + dx] = inside ? xb[(size_t)zz * HW + (size_t)yy * W + xc] : 0.f;
        }
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      const size_t bc = (size_t)b * 16 + 4 * wave + ch;
      float gv = (ga1[bc * N + n] + 0.125f * ga2[((bc * D2 + z / 2) * H2 + y / 2) * W2 + xx / 2]) +
                 0.015625f * ga4[((bc * D4 + z / 4) * H4 + y / 4) * W4 + xx / 4];
      gv = a[bc * N + n] > 0.f ? gv : 0.f;
      bs[ch] += gv;
#pragma unroll
      for (int k = 0; k < 27; ++k) acc[ch][k] = fmaf(gv, in[k], acc[ch][k]);
    }
  }
  float* const po = partial + (size_t)blockIdx.x * C1_P3;
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) {
#pragma unroll
    for (int k = 0; k < 28; ++k) {
      float v = k < 27 ? acc[ch][k] : bs[ch];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
      if (lane == 0) {
        if (k < 27) po[(4 * wave + ch) * 54 + ci * 27 + k] = v;
        else if (ci == 0) po[864 + 4 * wave + ch] = v;
      }
    }
  }
}

struct Bank3dSplits { int tail, wg[3], c1; };      // wg: quarter, half, full resolution
struct Bank3dPartials { const float *tail, *w2[3], *w0[3], *c1; };      // w2: block.2, w0: block.0
__global__ __launch_bounds__(256) void bank3d_reduce_kernel(Bank3dPartials P, float* __restrict__ out, Bank3dSplits ns) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= B3_FLOATS) return;
  double v = 0.0;
  if (q < B3_WB0) {
    for (int s = 0; s < ns.c1; ++s) v += (double)P.c1[(size_t)s * C1_P3 + q];
  } else if (q < B3_W2) {
    const bool first = q < B3_WB2;                                // block.0
    const int j = q - (first ? B3_WB0 : B3_WB2);
    int at;
    if (j < 6912) {
      const int co = j / 432, ci = (j / 27) % 16, tap = j % 27;
      at = tap * 256 + co * 16 + ci;
    } else {
      at = j;                                                     // 6912 + channel
    }
    for (int l = 0; l < 3; ++l) {
      const float* src = first ? P.w0[l] : P.w2[l];
      for (int s = 0; s < ns.wg[l]; ++s) v += (double)src[(size_t)s * WG_P + at];
    }
  } else {
    const int at = bank_tail_partial_at(q - B3_W2 + BLOB_W2);      // the tail at the 2D blob's distances
    for (int s = 0; s < ns.tail; ++s) v += (double)P.tail[(size_t)s * TAIL_P + at];
  }
  out[q] = (float)v;
}

// the backward's launch plan and workspace: a function of (B, D, H, W) alone
struct Bank3dBwdPlan {
  BankUnits u;                     // the tail's and conv1's units of 64 cells
  Bank3dWgPlan wg[3];              // quarter, half, full
  Bank3dSplits ns;
  float *g1, *h1, *g2, *h2, *g4, *h4;        // per level: g_b, over which g_a is written, and g_h
  float *ptail, *pw2[3], *pw0[3], *pc1;
  size_t bytes;
};
Bank3dBwdPlan bank3d_bwd_plan(int B, int D, int H, int W, void* base) {
  Bank3dBwdPlan p{};
  const size_t N = (size_t)D * H * W;
  p.u = bank_units(B, N);                                         // < 2^31: B <= 65535 and N < 2^31 would not do; see bank3d_bwd_range_ok
  for (int l = 0; l < 3; ++l) {
    const int R = 4 >> l;
    p.wg[l] = bank3d_wg_plan(B, D / R, H / R, W / R);
    p.ns.wg[l] = p.wg[l].groups;
  }
  p.ns.tail = p.ns.c1 = p.u.split;
  size_t off = 0;
  auto take = [&](size_t floats) { float* r = base ? (float*)((char*)base + off) : nullptr; off += al256(floats * 4); return r; };
  p.g1 = take(B * 16 * N); p.h1 = take(B * 16 * N);               // 2 x (64 + 8 + 1) = 146 bytes a full-resolution cell
  p.g2 = take(B * 16 * (N / 8)); p.h2 = take(B * 16 * (N / 8));
  p.g4 = take(B * 16 * (N / 64)); p.h4 = take(B * 16 * (N / 64));
  p.ptail = take((size_t)p.ns.tail * TAIL_P);
  for (int l = 0; l < 3; ++l) {
    p.pw2[l] = take((size_t)p.ns.wg[l] * WG_P);
    p.pw0[l] = take((size_t)p.ns.wg[l] * WG_P);
  }
  p.pc1 = take((size_t)p.ns.c1 * C1_P3);
  p.bytes = off;
  return p;
}
// the backward counts a batch's units of 64 cells and its weight-gradient items in an int
inline bool bank3d_bwd_range_ok(const FnxGrid* g) {
  return ((size_t)g->D * g->H * g->W + 63) / 64 * (size_t)g->B < ((size_t)1 << 31);
}

bool bank3d_backward(const FnxGrid* g, const void* packed_t, const float* x, const float* grad_p, const float* tape, float* grad_blob,
                     int /*mode*/, void* ws, hipStream_t s) {
  const int B = g->B, D = g->D, H = g->H, W = g->W;
  const float* pt = (const float*)packed_t;
  const BankTapeLayout T = bank_tape_layout(3, B, D, H, W);
  const Bank3dBwdPlan p = bank3d_bwd_plan(B, D, H, W, ws);
  auto at = [&](int n) { return tape + T.e[n].off; };
  ProfScope ps(FNX_PROF_CONV_MFMA16, s);
  const int N = D * H * W;
  bank_tail_backward(pt + PT3_W2T, grad_p, at(TP_T), at(TP_C2A), at(TP_C2B), at(TP_C3), p.g1, p.ptail, N, p.u.ups, p.u.nunits, p.ns.tail, s);
  {
    const size_t total = (size_t)B * 16 * (N / 64);
    bank3d_pool_bwd_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(p.g1, at(TP_B1), at(TP_B2), at(TP_B4), p.g2, p.g4, D, H, W, total);
  }
  // a level: g_h = convT(block.2)(g_b) (h > 0); block.2's weight gradient; g_a = convT(block.0)(g_h) over g_b; block.0's weight gradient
  auto level = [&](int l, int R, float* gb, float* gh, const float* th, const float* ta) {
    const int d = D / R, h = H / R, w = W / R;
    const Bank3dConvPlan pl = bank3d_conv_plan(B, d, h, w);
    const dim3 grid((unsigned)pl.tiles_x, (unsigned)(pl.tiles_y * pl.chunks), (unsigned)B);
    bank3d_conv_bwd_kernel<EPI3_MASK><<<grid, 256, 0, s>>>(pt + PT3_WB2T, pt + PT3_ZERO, gb, d, h, w, pl.tiles_y, pl.chunk, gh, th);
    bank3d_wgrad_kernel<<<p.wg[l].groups, 256, 0, s>>>(gb, th, d, h, w, p.wg[l], p.pw2[l]);
    bank3d_conv_bwd_kernel<EPI3_PLAIN><<<grid, 256, 0, s>>>(pt + PT3_WB0T, pt + PT3_ZERO, gh, d, h, w, pl.tiles_y, pl.chunk, gb, nullptr);
    bank3d_wgrad_kernel<<<p.wg[l].groups, 256, 0, s>>>(gh, ta, d, h, w, p.wg[l], p.pw0[l]);
  };
  level(0, 4, p.g4, p.h4, at(TP_H4), at(TP_A4));
  level(1, 2, p.g2, p.h2, at(TP_H2), at(TP_A2));
  level(2, 1, p.g1, p.h1, at(TP_H1), at(TP_A));
  bank3d_conv1_bwd_kernel<<<dim3((unsigned)p.ns.c1, 2), 256, 0, s>>>(x, at(TP_A), p.g1, p.g2, p.g4, p.pc1, D, H, W, p.u.ups, p.u.nunits);
  Bank3dPartials P{};
  P.tail = p.ptail; P.c1 = p.pc1;
  for (int l = 0; l < 3; ++l) { P.w2[l] = p.pw2[l]; P.w0[l] = p.pw0[l]; }
  bank3d_reduce_kernel<<<(B3_FLOATS + 255) / 256, 256, 0, s>>>(P, grad_blob, p.ns);
  return true;
}

size_t bank3d_bwd_plan_bytes(const FnxGrid* g) { return bank3d_bwd_plan(g->B, g->D, g->H, g->W, nullptr).bytes; }

bool bank3d_sized(const FnxGrid* g) { return g && g->is3D && g->B >= 1 && g->D >= 4 && g->H >= 4 && g->W >= 4; }
// the net's record (fnx_fluidnet.h): its input is kept in the tape, the backward's conv1 reads it again
size_t bank3d_tape_x(const FnxGrid* g) { return bank_tape_layout(3, g->B, g->D, g->H, g->W).e[TP_X].off; }
constexpr NetTrain NET3 = {3, bank_status, bank3d_forward_train, bank3d_backward, bank3d_bwd_plan_bytes, bank3d_tape_x};
constexpr BankTrainDim DIM3 = {NET3, bank3d_sized, bank3d_bwd_range_ok};

}  // namespace
}  // namespace fnx

extern "C" {

int fnx_banknet3d_tape_entries(void) { return fnx::N_BANK_TAPE; }

size_t fnx_banknet3d_tape_layout(const FnxGrid* g, FnxTapeEntry3D* entries) {
  if (!fnx::bank3d_sized(g) || g->D % 4 || g->H % 4 || g->W % 4) {
    fnx::set_error(FNX_EINVAL, "%s: a 3D grid with D, H and W positive multiples of 4 is needed", __func__);
    return 0;
  }
  return fnx::bank_fill_tape(fnx::bank_tape_layout(3, g->B, g->D, g->H, g->W), nullptr, entries);
}

size_t fnx_banknet3d_packed_t_bytes(void) { return (size_t)fnx::PT3_FLOATS * sizeof(float); }

int fnx_banknet3d_pack_t(const float* weights_blob, void* packed_t, void* stream) {
  if (!weights_blob || !packed_t) return fnx::set_error(FNX_EINVAL, "%s: null argument", __func__);
  fnx::bank3d_pack_t_kernel<<<(fnx::PT3_FLOATS + 255) / 256, 256, 0, (hipStream_t)stream>>>(weights_blob, (float*)packed_t);
  return fnx::bank_status();
}

size_t fnx_banknet3d_backward_ws_bytes(const FnxGrid* g) { return fnx::bank_size_query<fnx::DIM3>(g, fnx::bank_bwd_ws<fnx::DIM3>); }

int fnx_banknet3d_backward_launches(void) { return 8; }

int fnx_banknet3d_backward_plan(const FnxGrid* g, FnxBankBwdLaunch* launches) {
  if (!launches || !fnx::bank3d_sized(g) || g->D % 4 || g->H % 4 || g->W % 4 || !fnx::bank3d_bwd_range_ok(g))
    return fnx::set_error(FNX_EINVAL, "%s: a 3D grid with D, H and W positive multiples of 4 within the backward's range is needed", __func__);
  const fnx::Bank3dBwdPlan p = fnx::bank3d_bwd_plan(g->B, g->D, g->H, g->W, (void*)256);      // (a base that is not null: offsets + 256)
  auto off = [](const float* q) { return (size_t)((const char*)q - (const char*)256); };
  int n = 0;
  auto put = [&](const char* name, int level, long long items, int groups, int cap, int pf, const float* at, int d0, int d1, int d2, int d3) {
    FnxBankBwdLaunch& L = launches[n++];
    snprintf(L.name, sizeof(L.name), "%s", name);
    L.level = level; L.items = items; L.workgroups = groups; L.cap = cap; L.partial_floats = pf; L.partial_offset = off(at);
    L.dims[0] = d0; L.dims[1] = d1; L.dims[2] = d2; L.dims[3] = d3;
  };
  put("tail", 1, p.u.nunits, p.ns.tail, fnx::MAX_SPLIT, fnx::TAIL_P, p.ptail, p.u.ups, 64, 0, 0);
  for (int l = 0; l < 3; ++l) {
    put("wgrad.2", 4 >> l, p.wg[l].items, p.wg[l].groups, fnx::WG_SPLIT, fnx::WG_P, p.pw2[l], p.wg[l].tiles_x, p.wg[l].tiles_y, p.wg[l].chunks,
        fnx::WG_CHUNK);
    put("wgrad.0", 4 >> l, p.wg[l].items, p.wg[l].groups, fnx::WG_SPLIT, fnx::WG_P, p.pw0[l], p.wg[l].tiles_x, p.wg[l].tiles_y, p.wg[l].chunks,
        fnx::WG_CHUNK);
  }
  put("conv1", 1, p.u.nunits, p.ns.c1, fnx::MAX_SPLIT, fnx::C1_P3, p.pc1, p.u.ups, 64, 0, 0);
  return FNX_OK;
}

int fnx_banknet3d_forward_train(const FnxGrid* g, const void* packed, const float* x, float* p, float* tape, int precision_mode, void* stream) {
  return fnx::bank_forward_train<fnx::DIM3>(__func__, g, packed, x, p, tape, precision_mode, stream);
}

int fnx_banknet3d_backward(const FnxGrid* g, const void* packed_t, const float* x, const float* grad_p, const float* tape, float* grad_blob,
                           int precision_mode, void* ws, size_t ws_bytes, void* stream) {
  return fnx::bank_backward<fnx::DIM3>(__func__, g, packed_t, x, grad_p, tape, grad_blob, precision_mode, ws, ws_bytes, stream);
}

size_t fnx_fluidnet_bank3d_train_ws_bytes(const FnxGrid* g) { return fnx::bank_size_query<fnx::DIM3>(g, fnx::bank_train_ws<fnx::DIM3>); }

int fnx_fluidnet_bank3d_forward_train(const FnxGrid* g, const void* packed, const float* input, float normalize_threshold, float* p_out,
                                      float* U_out, float* flags_out, float* scale_out, float* tape, int precision_mode, void* ws,
                                      size_t ws_bytes, void* stream) {
  return fnx::bank_whole_forward_train<fnx::DIM3>(__func__, g, packed, input, normalize_threshold, p_out, U_out, flags_out, scale_out, tape,
                                                  precision_mode, ws, ws_bytes, stream);
}

int fnx_fluidnet_bank3d_backward(const FnxGrid* g, const void* packed_t, const float* flags, const float* scale, const float* grad_p,
                                 const float* grad_U, const float* tape, float* grad_blob, int precision_mode, void* ws, size_t ws_bytes,
                                 void* stream) {
  return fnx::bank_whole_backward<fnx::DIM3>(__func__, g, packed_t, flags, scale, grad_p, grad_U, tape, grad_blob, precision_mode, ws, ws_bytes,
                                             stream);
}

}  // extern "C"
