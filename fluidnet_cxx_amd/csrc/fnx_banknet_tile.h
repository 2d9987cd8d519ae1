// What the units of the 16-channel bank net share (fnx_banknet.hip: 2D inference; fnx_banknet_train.hip: 2D tape forward and backward;
// fnx_banknet3d.hip: 3D inference; fnx_banknet3d_train.hip: 3D tape forward and backward, through fnx_banknet3d_tile.h).  All of them: the pieces of the weight packing and the checks every entry point makes before the
// device.  The 2D units: the blob's and the packed image's offsets, the geometry of a level tile, the 3x3 bank convolution on
// v_mfma_f32_16x16x4_f32 and the body of a level kernel (with a compile-time switch that also writes the tape).
// The layout of the kernels and of the MFMA operands is described at the top of fnx_banknet.hip.
#pragma once
#include <hip/hip_runtime.h>
#include "fnx_fluidnet.h"
#include "fnx_kernels.h"
#include "../../include/fluidnet_hip.h"

namespace fnx {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

// the blob: conv1, convBank.block.0, convBank.block.2, conv2, conv3, convOut; each weight (Cout, Cin, k, k) then bias
// (float offsets: conv1 0 / 288, block.0 304 / 2608, block.2 2624 / 4928, conv2 4944 / 5200, conv3 5216 / 5344, convOut 5352 / 5360)
constexpr int BLOB_W1 = 0, BLOB_B1 = 288, BLOB_WB0 = 304, BLOB_BB0 = 2608, BLOB_WB2 = 2624, BLOB_BB2 = 4928, BLOB_W2 = 4944, BLOB_B2 = 5200,
              BLOB_W3 = 5216, BLOB_B3 = 5344, BLOB_WO = 5352, BLOB_BO = 5360, BLOB_FLOATS = 5361;
// the packed image (floats)
constexpr int PK_W1 = 0;            // [cout 16][cin 2][3][3], the blob's own order
constexpr int PK_B1 = 288;          // 16
constexpr int PK_WB0 = 304;         // [tap 9][kc 4][lane 64] = W[cout = lane & 15][cin = 4 kc + (lane >> 4)][tap]
constexpr int PK_BB0 = 2608;        // 16
constexpr int PK_WB2 = 2624;
constexpr int PK_BB2 = 4928;
// the 1x1 tail, 272 floats per layer: [r 4][lane 64] = W[cout = lane & 15][cin = 4 (lane >> 4) + r], then 16 biases; rows and input
// channels a layer does not have are zero (conv3: 8 rows; convOut: row 0, input channels 0..7)
constexpr int PK_W2 = 4944;         // conv2 4944, conv3 5216, convOut 5488
constexpr int PK_FLOATS = 5760;

// The geometry of a level-R tile (floats).
template <int R, int TH, int TW>
struct BankTile {
  static constexpr int P = TW + 4;                       // pitch of the planes: the tile and two halo cells on either side
  static constexpr int ROWS = TH + 4;
  static constexpr int NA = ROWS * P;                    // pooled cells
  static constexpr int Q0 = (TH + 2) * P;                // flattened positions of cB0 (the tile + 1), of cB2 (the tile)
  static constexpr int Q2 = TH * P;
  static constexpr int G0 = (Q0 + 15) / 16, G2 = (Q2 + 15) / 16;
  // a wave takes two groups at a time, so positions up to 16 (G0 + 1) are computed, and a position reads up to 2 P + 2 beyond itself
  static constexpr int SMIN = 16 * (G0 + 1) + 2 * P + 2;
  static constexpr int S = (SMIN + 15) / 32 * 32 + 16;   // >= SMIN, = 16 (mod 32)
  static constexpr int XH = ROWS * R + 2, XW = P * R + 2;
  static constexpr int XFLOATS = 2 * XH * XW;
  static constexpr int BUF2 = 16 * S > XFLOATS ? 16 * S : XFLOATS;     // the x tile, then b0
  static constexpr int LDS_FLOATS = 16 * S + BUF2;
  static_assert(S >= SMIN && S % 32 == 16 && NA <= S, "plane stride");
  static_assert(LDS_FLOATS * 4 <= 64 * 1024, "static LDS");
};

constexpr int TILE_H = 8, TILE_W1 = 32, TILE_WC = 16;   // level 1: 8 x 32 cells; levels 2 and 4: 8 x 16

// One 3x3 bank convolution over `ngroups` groups of 16 flattened positions of the LDS planes at `src` (stride S, pitch P), two groups per
// wave and step (two independent accumulators).  epi(q of this lane, the four channels 4 (lane >> 4) + r after bias, before ReLU).
template <int P, int S, typename Epi>
__device__ __forceinline__ void bank_conv(const float* __restrict__ wpk, const float* __restrict__ bias, const float* src, int ngroups,
                                          int wave, int lane, Epi epi) {
  float wa[36];
#pragma unroll
  for (int i = 0; i < 36; ++i) wa[i] = wpk[i * 64 + lane];
  f32x4 b4;
#pragma unroll
  for (int r = 0; r < 4; ++r) b4[r] = bias[4 * (lane >> 4) + r];
  const float* sp = src + (lane >> 4) * S + (lane & 15);
  for (int grp = 2 * wave; grp < ngroups; grp += 8) {
    const float* s0 = sp + grp * 16;
    f32x4 acc0 = b4, acc1 = b4;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) {
        const int off = kc * 4 * S + (t / 3) * P + (t % 3);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[t * 4 + kc], s0[off], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[t * 4 + kc], s0[off + 16], acc1, 0, 0, 0);
      }
    epi(grp * 16 + (lane & 15), acc0);
    epi(grp * 16 + 16 + (lane & 15), acc1);
  }
}

// What the 2D and the 3D pack kernel share.  Float j of a 16 -> 16 convolution's image, [tap][kc 4][lane 64] =
// W[cout = lane & 15][cin = 4 kc + (lane >> 4)][tap] then the 16 biases, from the blob's (16, 16, taps) weight at w, whose bias follows it.
__device__ __forceinline__ float bank_pack_conv16(const float* __restrict__ blob, int w, int taps, int j) {
  float v;
  if (j < 256 * taps) {
    const int lane = j & 63, kc = (j >> 6) & 3, tap = j >> 8;
    v = blob[w + ((lane & 15) * 16 + 4 * kc + (lane >> 4)) * taps + tap];
  } else {
    v = blob[w + j];
  }
  return v;
}
// Float j of the tail's image (3 x 272, see PK_W2) from the blob with conv2's weight at w2: the 1x1 layers have one tap in either
// dimension, so conv2, conv3 and convOut follow it at the same distances in both blobs.
__device__ __forceinline__ float bank_pack_tail(const float* __restrict__ blob, int w2, int j) {
  const int layer = j / 272;                              // conv2, conv3, convOut
  j %= 272;
  const int cout_n = layer == 0 ? 16 : (layer == 1 ? 8 : 1), cin_n = layer == 2 ? 8 : 16;
  const int wsrc = w2 + (layer == 0 ? 0 : (layer == 1 ? 272 : 408)), bsrc = w2 + (layer == 0 ? 256 : (layer == 1 ? 400 : 416));
  float v = 0.f;
  if (j < 256) {
    const int lane = j & 63, r = j >> 6;
    const int cout = lane & 15, cin = 4 * (lane >> 4) + r;
    if (cout < cout_n && cin < cin_n) v = blob[wsrc + cout * cin_n + cin];
  } else if (j - 256 < cout_n) {
    v = blob[bsrc + j - 256];
  }
  return v;
}
static_assert(BLOB_B2 - BLOB_W2 == 256 && BLOB_W3 - BLOB_W2 == 272 && BLOB_B3 - BLOB_W2 == 400 && BLOB_WO - BLOB_W2 == 408 &&
              BLOB_BO - BLOB_W2 == 416, "bank_pack_tail's table");

// Where a taping level launch writes (contiguous (B,C,h,w) tensors of the level it runs at; see fnx_banknet_tape_layout): the pooled
// relu(conv1) it recomputes, the output of block.0 and of block.2 after their ReLUs and, at full resolution, the sum of the three levels
// and the outputs of the 1x1 layers after their ReLUs.
struct BankTapeOut { float *a, *h, *b, *t, *c2a, *c2b, *c3; };

// The body of a level kernel.  x (B, 2, H, W).  R = 4, 2: out (B, 16, H/R, W/R).  R = 1: l2, l4 the coarser results, p (B, 1, H, W).
// 256 threads.  TAPE: the same arithmetic, and every ReLU output of the tile's own cells goes to `tape` as well.
template <int R, int TH, int TW, bool TAPE>
__device__ __forceinline__ void bank_level_tile(const float* __restrict__ pk, const float* __restrict__ x, int H, int W,
                                                float* __restrict__ out, const float* __restrict__ l2, const float* __restrict__ l4,
                                                float* __restrict__ p, const BankTapeOut& tape) {
  using T = BankTile<R, TH, TW>;
  constexpr int P = T::P, S = T::S;
  __shared__ float lds[T::LDS_FLOATS];
  float* const la = lds;                 // pooled relu(conv1): [16][S]
  float* const lx = lds + 16 * S;        // x tile [2][XH][XW], then b0 [16][S]
  float* const lb = lx;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.z;
  const int HR = H / R, WR = W / R;
  const int ty0 = blockIdx.y * TH, tx0 = blockIdx.x * TW;

  // 1. the x tile
  {
    const int oy = (ty0 - 2) * R - 1, ox = (tx0 - 2) * R - 1;
    const float* xb = x + (size_t)b * 2 * H * W;
    for (int i = tid; i < T::XFLOATS; i += 256) {
      const int c = i / (T::XH * T::XW), rem = i % (T::XH * T::XW);
      const int gy = oy + rem / T::XW, gx = ox + rem % T::XW;
      float v = 0.f;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = xb[((size_t)c * H + gy) * W + gx];
      lx[i] = v;
    }
  }
  __syncthreads();

  // 2. relu(conv1) pooled over R x R: wave w computes channels 4w .. 4w+3 of every pooled cell
  {
    float w1[4][18], b1[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      b1[c] = pk[PK_B1 + 4 * wave + c];
#pragma unroll
      for (int k = 0; k < 18; ++k) w1[c][k] = pk[PK_W1 + (4 * wave + c) * 18 + k];
    }
    for (int n = lane; n < T::NA; n += 64) {
      const int y = n / P, xx = n % P;
      const int ly = ty0 - 2 + y, lxx = tx0 - 2 + xx;
      float pool[4] = {0.f, 0.f, 0.f, 0.f};
      if (ly >= 0 && ly < HR && lxx >= 0 && lxx < WR) {
        float in[2][R + 2][R + 2];
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int dy = 0; dy < R + 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < R + 2; ++dx) in[c][dy][dx] = lx[(c * T::XH + y * R + dy) * T::XW + xx * R + dx];
#pragma unroll
        for (int py = 0; py < R; ++py)
#pragma unroll
          for (int px = 0; px < R; ++px) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              float acc = b1[c];
#pragma unroll
              for (int ci = 0; ci < 2; ++ci)
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                  for (int dx = 0; dx < 3; ++dx) acc = fmaf(w1[c][ci * 9 + dy * 3 + dx], in[ci][py + dy][px + dx], acc);
              pool[c] += fmaxf(acc, 0.f);
            }
          }
#pragma unroll
        for (int c = 0; c < 4; ++c) pool[c] *= 1.f / (float)(R * R);
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) la[(4 * wave + c) * S + n] = pool[c];
    }
  }
  __syncthreads();

  if constexpr (TAPE) {
    // the tile's own pooled cells (step 3 only reads `la`, so no barrier is needed behind this)
    float* ab = tape.a + (size_t)b * 16 * HR * WR;
    for (int i = tid; i < 16 * TH * TW; i += 256) {
      const int ch = i / (TH * TW), rem = i % (TH * TW);
      const int y = rem / TW, xx = rem % TW;
      const int ly = ty0 + y, lxx = tx0 + xx;
      if (ly < HR && lxx < WR) ab[((size_t)ch * HR + ly) * WR + lxx] = la[ch * S + (y + 2) * P + xx + 2];
    }
  }

  // 3. cB0 on the tile + 1: position q = (y, x) of b0 is level cell (ty0 - 1 + y, tx0 - 1 + x)
  bank_conv<P, S>(pk + PK_WB0, pk + PK_BB0, la, T::G0, wave, lane, [&](int q, f32x4 v) {
    const int y = q / P, xx = q % P;
    const int ly = ty0 - 1 + y, lxx = tx0 - 1 + xx;
    const bool in = ly >= 0 && ly < HR && lxx >= 0 && lxx < WR;
#pragma unroll
    for (int r = 0; r < 4; ++r) lb[(4 * (lane >> 4) + r) * S + q] = in ? fmaxf(v[r], 0.f) : 0.f;
    if constexpr (TAPE) {
      if (in && y >= 1 && y <= TH && xx >= 1 && xx <= TW) {
        float* hb = tape.h + (size_t)b * 16 * HR * WR;
#pragma unroll
        for (int r = 0; r < 4; ++r) hb[((size_t)(4 * (lane >> 4) + r) * HR + ly) * WR + lxx] = fmaxf(v[r], 0.f);
      }
    }
  });
  __syncthreads();

  // 4. cB2 on the tile: position q = (y, x) is level cell (ty0 + y, tx0 + x)
  if constexpr (R != 1) {
    float* ob = out + (size_t)b * 16 * HR * WR;
    bank_conv<P, S>(pk + PK_WB2, pk + PK_BB2, lb, T::G2, wave, lane, [&](int q, f32x4 v) {
      const int y = q / P, xx = q % P;
      const int ly = ty0 + y, lxx = tx0 + xx;
      if (y < TH && xx < TW && ly < HR && lxx < WR) {
#pragma unroll
        for (int r = 0; r < 4; ++r) ob[((size_t)(4 * (lane >> 4) + r) * HR + ly) * WR + lxx] = fmaxf(v[r], 0.f);
      }
    });
  } else {
    float wt[3][4];
    f32x4 bt[3];
#pragma unroll
    for (int l = 0; l < 3; ++l) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        wt[l][r] = pk[PK_W2 + l * 272 + r * 64 + lane];
        bt[l][r] = pk[PK_W2 + l * 272 + 256 + 4 * (lane >> 4) + r];
      }
    }
    const int H2 = H / 2, W2 = W / 2, H4 = H / 4, W4 = W / 4;
    const float* l2b = l2 + (size_t)b * 16 * H2 * W2;
    const float* l4b = l4 + (size_t)b * 16 * H4 * W4;
    float* pb = p + (size_t)b * H * W;
    bank_conv<P, S>(pk + PK_WB2, pk + PK_BB2, lb, T::G2, wave, lane, [&](int q, f32x4 v) {
      const int y = q / P, xx = q % P;
      const int ly = ty0 + y, lxx = tx0 + xx;
      const bool valid = y < TH && xx < TW && ly < H && lxx < W;
      const int cy = ly < H ? ly : H - 1, cx = lxx < W ? lxx : W - 1;     // (every lane runs the MFMAs; a lane without a cell reads a clamped one)
      // (B,16,H,W) offset of this lane's channel r at its cell, for the tape
      const size_t cell = (size_t)b * 16 * H * W + (size_t)(4 * (lane >> 4)) * H * W + (size_t)cy * W + cx;
      f32x4 t;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ch = 4 * (lane >> 4) + r;
        t[r] = (fmaxf(v[r], 0.f) + l2b[((size_t)ch * H2 + cy / 2) * W2 + cx / 2]) + l4b[((size_t)ch * H4 + cy / 4) * W4 + cx / 4];
      }
      if constexpr (TAPE) {
        if (valid) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            tape.b[cell + (size_t)r * H * W] = fmaxf(v[r], 0.f);
            tape.t[cell + (size_t)r * H * W] = t[r];
          }
        }
      }
      // conv2, conv2 again, conv3, convOut: register r of a result is the B operand of input channels 4g + r
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        const int m = l == 0 ? 0 : l - 1;
        f32x4 h = bt[m];
#pragma unroll
        for (int r = 0; r < 4; ++r) h = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[m][r], t[r], h, 0, 0, 0);
        if (l < 3) {
#pragma unroll
          for (int r = 0; r < 4; ++r) t[r] = fmaxf(h[r], 0.f);
          if constexpr (TAPE) {
            if (valid && l < 2) {
              float* dst = l == 0 ? tape.c2a : tape.c2b;
#pragma unroll
              for (int r = 0; r < 4; ++r) dst[cell + (size_t)r * H * W] = t[r];
            } else if (valid && lane < 32) {             // conv3 has the 8 channels of lane groups 0 and 1: (B,8,H,W)
              const size_t c8 = (size_t)b * 8 * H * W + (size_t)(4 * (lane >> 4)) * H * W + (size_t)cy * W + cx;
#pragma unroll
              for (int r = 0; r < 4; ++r) tape.c3[c8 + (size_t)r * H * W] = t[r];
            }
          }
        } else {
          t = h;
        }
      }
      if (valid && lane < 16) pb[(size_t)ly * W + lxx] = t[0];
    });
  }
}

struct BankWs { float* l2; float* l4; size_t bytes; };
inline BankWs banknet_ws_layout(int B, int H, int W, void* base) {
  BankWs w{};
  const size_t n2 = al256((size_t)B * 16 * (H / 2) * (W / 2) * 4), n4 = al256((size_t)B * 16 * (H / 4) * (W / 4) * 4);
  w.l2 = (float*)base;
  w.l4 = base ? (float*)((char*)base + n2) : nullptr;
  w.bytes = n2 + n4;
  return w;
}

inline int bank_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? FNX_OK : set_error(FNX_EHIP, "HIP error in a bank-net launch: %s", hipGetErrorString(e));
}

// The checks the entry points of the bank nets share, before any device call, each refusal with its own text.  ndim: 2 (the 'FluidNet'
// model) or 3 ('FluidNet3D').  want_of(g): the workspace the entry point needs for a grid that passed the checks in front of it
// (nullptr: none).
inline int check_bank_call(const char* fn, int ndim, const FnxGrid* g, bool args, int precision_mode, size_t (*want_of)(const FnxGrid*),
                           size_t ws_bytes) {
  if (!g || !args) return set_error(FNX_EINVAL, "%s: null argument", fn);
  // what depends on the dimension: the kind of grid, D, and the range the kernels launch on (3D: grid y is (y tiles) x (z tiles or chunks))
  const bool is3 = ndim == 3;
  const size_t cells = (size_t)g->D * g->H * g->W;
  const bool kind_ok = is3 ? g->is3D && g->D >= 4 : !g->is3D && g->D == 1;
  const bool d_ok = !is3 || g->D % 4 == 0;
  const bool range_ok = is3 ? cells < ((size_t)1 << 31) && (size_t)(g->D / 4) * (g->H / 4) <= 65535 : cells < ((size_t)1 << 27);
  if (!kind_ok)
    return is3 ? set_error(FNX_EINVAL, "%s: the Conv3d bank net ('FluidNet3D' model) is 3D only (is3D = %d, D = %d)", fn, g->is3D, g->D)
               : set_error(FNX_EINVAL, "%s: the bank net ('FluidNet' model) is 2D only (is3D = %d, D = %d)", fn, g->is3D, g->D);
  const int mode = net_mode(precision_mode);
  if (mode < 0)
    return set_error(FNX_EINVAL, "%s: unknown precision_mode %d (FNX_PRECISION_FP32, _FP32_DIRECT, _BF16X6, _BF16X3, _FP32_F4 or _FP32_F2)", fn,
                     precision_mode);
  if (mode == FNX_PRECISION_BF16X6 || mode == FNX_PRECISION_BF16X3)
    return set_error(FNX_EINVAL, "%s: the bank net runs in fp32 arithmetic only (FNX_PRECISION_FP32, _FP32_F4, _FP32_F2 or _FP32_DIRECT), "
                     "not in the bf16 modes (precision_mode %d)", fn, precision_mode);
  if (g->B < 1 || g->B > 65535) return set_error(FNX_EINVAL, "%s: batch size %d is outside 1 .. 65535", fn, g->B);
  if (!d_ok) return set_error(FNX_EINVAL, "%s: D = %d must be a positive multiple of 4 (the three levels are added)", fn, g->D);
  if (g->H < 4 || g->H % 4) return set_error(FNX_EINVAL, "%s: H = %d must be a positive multiple of 4 (the three levels are added)", fn, g->H);
  if (g->W < 4 || g->W % 4) return set_error(FNX_EINVAL, "%s: W = %d must be a positive multiple of 4 (the three levels are added)", fn, g->W);
  if (!range_ok)
    return is3 ? set_error(FNX_EINVAL, "%s: D * H * W = %zu cells per sample (D = %d, H = %d) is beyond the bank kernels' launch range", fn,
                           cells, g->D, g->H)
               : set_error(FNX_EINVAL, "%s: H * W = %zu cells per sample is beyond the bank kernels' range", fn, cells);
  const size_t want = want_of ? want_of(g) : 0;
  if (ws_bytes < want) return set_error(FNX_EWORKSPACE, "%s: workspace of %zu bytes is too small (%zu needed)", fn, ws_bytes, want);
  return FNX_OK;
}

}  // namespace
}  // namespace fnx
