// What the units of the Conv3d bank net share (fnx_banknet3d.hip: inference; fnx_banknet3d_train.hip: tape forward and backward): the
// blob's and the packed image's offsets, the tile geometry, the launch plan and the workspace of the inference forward, and the body of
// the z-marching 16 -> 16 convolution with its epilogue as a template parameter.  fnx_banknet3d_tile.h is to these units what
// fnx_banknet_tile.h is to the 2D ones.  The layout of the kernel and of the MFMA operands is described at the top of fnx_banknet3d.hip.
#pragma once
#include "fnx_banknet_tile.h"

namespace fnx {
namespace {

// the blob: conv1, convBank.block.0, convBank.block.2, conv2, conv3, convOut; each weight (Cout, Cin, 3|1, 3|1, 3|1) then bias
// (the 1x1x1 layers behind conv2's weight as in the 2D blob: fnx_banknet_tile.h, bank_pack_tail)
constexpr int B3_W1 = 0, B3_B1 = 864, B3_WB0 = 880, B3_WB2 = 7808, B3_W2 = 14736, B3_FLOATS = B3_W2 + BLOB_FLOATS - BLOB_W2;
static_assert(B3_FLOATS == 15153, "the 3D blob");
// the packed image (floats)
constexpr int P3_W1 = 0;             // [cin 2][tap 27][cout 16]: the 16 weights of one input value are 64 consecutive bytes
constexpr int P3_B1 = 864;           // 16
constexpr int P3_WB0 = 880;          // [tap 27][kc 4][lane 64] = W[cout = lane & 15][cin = 4 kc + (lane >> 4)][tap = 9 dz + 3 dy + dx]
constexpr int P3_BB0 = 7792;         // 16
constexpr int P3_WB2 = 7808;
constexpr int P3_BB2 = 14720;
constexpr int P3_W2 = 14736;         // the 1x1x1 tail in the 2D image's layout (fnx_banknet_tile.h: PK_W2), 3 x 272
constexpr int P3_FLOATS = 15552;     // 62 208 bytes, a multiple of 256

// ---- the 16 -> 16 convolution, marching along z -----------------------------------------------------------------------------------------
constexpr int CV_TH = 4, CV_TW = 30;
constexpr int CV_P = CV_TW + 2, CV_ROWS = CV_TH + 2;            // pitch 32
constexpr int CV_NA = CV_ROWS * CV_P;                           // 192 cells of an input plane
constexpr int CV_Q = CV_TH * CV_P, CV_G = CV_Q / 16;            // 128 flattened positions, 8 groups: two a wave
constexpr int CV_SMIN = 16 * CV_G + 2 * CV_P + 2;               // a position reads up to 2 P + 2 beyond itself
constexpr int CV_S = (CV_SMIN + 15) / 32 * 32 + 16;             // 208
constexpr int CV_SLOT = 16 * CV_S;                              // floats of a ring slot
constexpr int CV_LOADS = 16 * CV_NA / 256;                      // 12 values of a plane per thread
static_assert(CV_G == 8 && CV_Q % 16 == 0 && CV_S >= CV_SMIN && CV_S % 32 == 16 && 4 * CV_SLOT * 4 <= 64 * 1024, "tile geometry");
static_assert(16 * CV_NA % 256 == 0, "plane load");

// What follows the accumulators of a plane:
//   RELU       out = relu(acc)                                                          (the inference forward's five first convolutions)
//   TAIL       relu, the two coarser results added, the four 1x1x1 layers on the accumulator registers; only p is written
//   TAIL_TAPE  TAIL, and b1 (after the ReLU, before the levels are added), t, c2a, c2b and c3 go to the tape from the same registers
//   MASK       out = acc where the tape entry `mask` is > 0 at the cell, else 0; no ReLU   (the backward: g_h)
//   PLAIN      out = acc                                                                    (the backward: g_a of a level)
enum Bank3dEpi { EPI3_RELU, EPI3_TAIL, EPI3_TAIL_TAPE, EPI3_MASK, EPI3_PLAIN };
// where EPI3_TAIL_TAPE writes: contiguous (B,16,d,h,w) tensors, c3 (B,8,d,h,w)
struct Bank3dTapeOut { float *b, *t, *c2a, *c2b, *c3; };

// in (B, 16, d, h, w) -> out (B, 16, d, h, w); the tails: l2, l4 the coarser banks' results, p (B, 1, d, h, w) instead.
// grid: (x tiles, y tiles * z chunks, B); the workgroup computes planes [zc * chunk, min(d, (zc + 1) * chunk)).  256 threads.
template <int EPI>
__device__ __forceinline__ void bank3d_conv_body(const float* __restrict__ wpk, const float* __restrict__ bias, const float* __restrict__ tail,
                                                 const float* __restrict__ in, int d, int h, int w, int tiles_y, int chunk,
                                                 float* __restrict__ out, const float* __restrict__ l2, const float* __restrict__ l4,
                                                 float* __restrict__ p, const float* __restrict__ mask, const Bank3dTapeOut& tape) {
  constexpr bool TAIL = EPI == EPI3_TAIL || EPI == EPI3_TAIL_TAPE;
  constexpr int HALVES_UNROLLED = EPI == EPI3_TAIL_TAPE ? 1 : 2;
  __shared__ float lds[4 * CV_SLOT];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.z;
  const int x0 = blockIdx.x * CV_TW, y0 = (blockIdx.y % tiles_y) * CV_TH;
  const int z0 = (blockIdx.y / tiles_y) * chunk, z1 = min(d, z0 + chunk);
  const size_t hw = (size_t)h * w, dhw = (size_t)d * hw;
  const float* inb = in + (size_t)b * 16 * dhw;

  for (int i = tid; i < 4 * CV_SLOT; i += 256) lds[i] = 0.f;      // the pad of every plane, read by positions that are dropped

  // what this thread loads of every plane: value j is channel ch, cell (y0 - 1 + row, x0 - 1 + col)
  size_t goff[CV_LOADS];
  int loff[CV_LOADS];
  unsigned okmask = 0;
#pragma unroll
  for (int j = 0; j < CV_LOADS; ++j) {
    const int i = tid + 256 * j;
    const int ch = i / CV_NA, rem = i % CV_NA;
    const int gy = y0 - 1 + rem / CV_P, gx = x0 - 1 + rem % CV_P;
    const bool ok = gy >= 0 && gy < h && gx >= 0 && gx < w;
    goff[j] = ok ? (size_t)ch * dhw + (size_t)gy * w + gx : 0;
    loff[j] = ch * CV_S + rem;
    if (ok) okmask |= 1u << j;
  }
  float pre[CV_LOADS];
  auto fetch = [&](int z) {                                       // plane z of the level, zero outside its domain
    const bool zin = z >= 0 && z < d;
    const float* src = inb + (size_t)(zin ? z : 0) * hw;
#pragma unroll
    for (int j = 0; j < CV_LOADS; ++j) pre[j] = (zin && ((okmask >> j) & 1)) ? src[goff[j]] : 0.f;
  };
  auto stash = [&](int z) {                                       // into the slot of plane z: (z + 1) & 3  (z >= -1)
    float* dst = lds + ((z + 1) & 3) * CV_SLOT;
#pragma unroll
    for (int j = 0; j < CV_LOADS; ++j) dst[loff[j]] = pre[j];
  };

  float wa[108];
#pragma unroll
  for (int i = 0; i < 108; ++i) wa[i] = wpk[i * 64 + lane];
  f32x4 b4;
#pragma unroll
  for (int r = 0; r < 4; ++r) b4[r] = bias[4 * (lane >> 4) + r];
  float wt[3][4];
  f32x4 bt[3];
  if constexpr (TAIL) {
#pragma unroll
    for (int l = 0; l < 3; ++l)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        wt[l][r] = tail[l * 272 + r * 64 + lane];
        bt[l][r] = tail[l * 272 + 256 + 4 * (lane >> 4) + r];
      }
  }

  __syncthreads();                                                // the zeros are in place
  for (int z = z0 - 1; z <= z0 + 1; ++z) {
    fetch(z);
    stash(z);
  }
  __syncthreads();

  // this wave's two groups of positions; its lanes' cells
  const int q0 = 32 * wave + (lane & 15), q1 = q0 + 16;
  const int ry = q0 / CV_P;                                       // both groups lie in row `wave` (P = 32)
  const int gy = y0 + ry, gx0 = x0 + q0 % CV_P, gx1 = x0 + q1 % CV_P;
  const bool ok0 = gy < h && q0 % CV_P < CV_TW && gx0 < w, ok1 = gy < h && q1 % CV_P < CV_TW && gx1 < w;
  const int lbase = (lane >> 4) * CV_S + q0;
  const int g4 = 4 * (lane >> 4);

  for (int z = z0; z < z1; ++z) {
    if (z + 2 <= z1) fetch(z + 2);                                // in flight during the MFMAs (plane z1 + 1 is never read)
    f32x4 acc0 = b4, acc1 = b4;
#pragma unroll
    for (int dz = 0; dz < 3; ++dz) {
      const float* sp = lds + ((z + dz) & 3) * CV_SLOT + lbase;   // the slot of plane z - 1 + dz
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) {
          const int off = kc * 4 * CV_S + (t / 3) * CV_P + (t % 3);
          acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[(dz * 9 + t) * 4 + kc], sp[off], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[(dz * 9 + t) * 4 + kc], sp[off + 16], acc1, 0, 0, 0);
        }
    }
    if constexpr (!TAIL) {
      const size_t cell = (size_t)b * 16 * dhw + (size_t)z * hw + (size_t)gy * w;
      float* ob = out + cell;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if constexpr (EPI == EPI3_RELU) {
          if (ok0) ob[(size_t)(g4 + r) * dhw + gx0] = fmaxf(acc0[r], 0.f);
          if (ok1) ob[(size_t)(g4 + r) * dhw + gx1] = fmaxf(acc1[r], 0.f);
        } else if constexpr (EPI == EPI3_MASK) {
          const float* mb = mask + cell;
          if (ok0) ob[(size_t)(g4 + r) * dhw + gx0] = mb[(size_t)(g4 + r) * dhw + gx0] > 0.f ? acc0[r] : 0.f;
          if (ok1) ob[(size_t)(g4 + r) * dhw + gx1] = mb[(size_t)(g4 + r) * dhw + gx1] > 0.f ? acc1[r] : 0.f;
        } else {
          if (ok0) ob[(size_t)(g4 + r) * dhw + gx0] = acc0[r];
          if (ok1) ob[(size_t)(g4 + r) * dhw + gx1] = acc1[r];
        }
      }
    } else {
      const int d2 = d / 2, h2 = h / 2, w2 = w / 2, d4 = d / 4, h4 = h / 4, w4 = w / 4;
      const float* l2b = l2 + (size_t)b * 16 * d2 * h2 * w2;
      const float* l4b = l4 + (size_t)b * 16 * d4 * h4 * w4;
      const int cy = gy < h ? gy : h - 1;                         // every lane runs the MFMAs; a lane without a cell reads a clamped one
      // (the taping tail runs the two groups one after the other through one copy of the epilogue: its stores' addresses, twice over,
      // do not fit next to the 108 weight operands at two waves a SIMD)
#pragma unroll HALVES_UNROLLED
      for (int half = 0; half < 2; ++half) {
        const int gx = half ? gx1 : gx0;
        const int cx = gx < w ? gx : w - 1;
        const f32x4 v = half ? acc1 : acc0;
        const bool okh = half ? ok1 : ok0;
        // the tape: (B,16,d,h,w) offset of channel 0 at the row of this wave (uniform: a wave's positions lie in tile row `wave`), and of
        // this lane's channel g4 at its cell inside that row
        const size_t trow = (size_t)b * 16 * dhw + (size_t)z * hw + (size_t)(y0 + wave) * w;
        const size_t tlane = (size_t)g4 * dhw + gx;
        f32x4 t;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const size_t ch = g4 + r;
          t[r] = (fmaxf(v[r], 0.f) + l2b[((ch * d2 + z / 2) * h2 + cy / 2) * w2 + cx / 2]) + l4b[((ch * d4 + z / 4) * h4 + cy / 4) * w4 + cx / 4];
        }
        if constexpr (EPI == EPI3_TAIL_TAPE) {
          if (okh) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              (tape.b + trow + (size_t)r * dhw)[tlane] = fmaxf(v[r], 0.f);
              (tape.t + trow + (size_t)r * dhw)[tlane] = t[r];
            }
          }
        }
        // conv2, conv2 again, conv3, convOut: register r of a result is the B operand of input channels 4g + r
#pragma unroll
        for (int l = 0; l < 4; ++l) {
          const int m = l == 0 ? 0 : l - 1;
          f32x4 hh = bt[m];
#pragma unroll
          for (int r = 0; r < 4; ++r) hh = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[m][r], t[r], hh, 0, 0, 0);
          if (l < 3) {
#pragma unroll
            for (int r = 0; r < 4; ++r) t[r] = fmaxf(hh[r], 0.f);
            if constexpr (EPI == EPI3_TAIL_TAPE) {
              if (okh && l < 2) {
                float* dst = l == 0 ? tape.c2a : tape.c2b;
#pragma unroll
                for (int r = 0; r < 4; ++r) (dst + trow + (size_t)r * dhw)[tlane] = t[r];
              } else if (okh && lane < 32) {                      // conv3 has the 8 channels of lane groups 0 and 1: (B,8,d,h,w)
                const size_t row8 = trow - (size_t)b * 8 * dhw;
#pragma unroll
                for (int r = 0; r < 4; ++r) (tape.c3 + row8 + (size_t)r * dhw)[tlane] = t[r];
              }
            }
          } else {
            t = hh;
          }
        }
        if (okh && lane < 16) p[(size_t)b * dhw + (size_t)z * hw + (size_t)gy * w + gx] = t[0];
      }
    }
    if (z + 2 <= z1) stash(z + 2);                                // the slot of plane z - 2, which no wave reads since the last barrier
    __syncthreads();
  }
}

// ---- the launch plan: a host function of (B, D, H, W) alone -----------------------------------------------------------------------------
constexpr long long BANK3D_TARGET_GROUPS = 4096;
struct Bank3dConvPlan { int tiles_x, tiles_y, chunk, chunks; };
inline Bank3dConvPlan bank3d_conv_plan(int B, int d, int h, int w) {
  Bank3dConvPlan pl{};
  pl.tiles_x = (w + CV_TW - 1) / CV_TW;
  pl.tiles_y = (h + CV_TH - 1) / CV_TH;
  // split z until about 4096 workgroups are in flight (16 a CU), but keep at least four planes a chunk: a chunk loads two planes more
  const long long tiles = (long long)B * pl.tiles_x * pl.tiles_y;
  long long want = (BANK3D_TARGET_GROUPS + tiles - 1) / tiles;
  const int most = d / 4 > 1 ? d / 4 : 1;
  if (want > most) want = most;
  if (want < 1) want = 1;
  pl.chunk = (int)((d + want - 1) / want);
  pl.chunks = (d + pl.chunk - 1) / pl.chunk;
  return pl;
}

struct Bank3dWs { float *a, *h, *a2, *h2, *b2, *a4, *h4, *b4; size_t bytes; };
inline Bank3dWs bank3d_ws_layout(int B, int D, int H, int W, void* base) {
  const size_t n1 = (size_t)B * 16 * D * H * W * 4, n2 = n1 / 8, n4 = n1 / 64;      // bytes: 64 + 64 + 3 * 8 + 3 * 1 = 155 a cell
  size_t off = 0;
  auto take = [&](size_t bytes) { float* r = base ? (float*)((char*)base + off) : nullptr; off += al256(bytes); return r; };
  Bank3dWs ws{};
  ws.a = take(n1); ws.h = take(n1);
  ws.a2 = take(n2); ws.h2 = take(n2); ws.b2 = take(n2);
  ws.a4 = take(n4); ws.h4 = take(n4); ws.b4 = take(n4);
  ws.bytes = off;
  return ws;
}

}  // namespace
}  // namespace fnx
