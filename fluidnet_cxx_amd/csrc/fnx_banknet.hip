// The reference's 16-channel "bank" pressure net (lib/model.py:177-209, mconf['model'] = 'FluidNet'), 2D inference forward, exact fp32.
//
//   a  = relu(conv1(x))                               2 -> 16, 3x3, zero padding at the full-resolution border
//   a1 = avgpool2(a), a2 = avgpool4(a)
//   bank(t) = relu(cB2(relu(cB0(t))))                 16 -> 16 -> 16, 3x3, zero padding at THAT level's border, one set of weights
//   t  = (bank(a) + up2(bank(a1))) + up4(bank(a2))    nearest: source index i / 2, i / 4
//   t  = relu(conv2(t)); t = relu(conv2(t)); t = relu(conv3(t)); p = convOut(t)      1x1: 16 -> 16 (twice), 16 -> 8, 8 -> 1
//
// Three launches of one kernel template, banknet_level_kernel<R>: R = 4, then 2, then 1.  A workgroup of four waves owns a TH x TW tile
// of level-R cells and
//   1. loads the 2-channel x of the tile, its two-cell halo at level R and one more full-resolution pixel into LDS (zero outside the domain),
//   2. recomputes relu(conv1(x)) for every pooled cell of the tile + 2 and pools it in registers: plane `a` (16 channels, pitch P = TW + 4).
//      conv1 is 288 MAC per pixel; recomputing it per level is cheaper than storing 16 channels at full resolution.  Wave w owns the
//      output channels 4w .. 4w+3, so its 76 weights are wave-uniform.  A pooled cell outside the level's domain is a zero ACTIVATION
//      (what the bank convolutions' zero padding sees), not the pooled conv1 of zero input,
//   3. cB0 on the tile + 1 into plane `b0` (same pitch; a cell outside the level's domain is again a zero activation),
//   4. cB2 on the tile.  R = 4, 2: the result goes to the workspace, (B, 16, H/R, W/R).  R = 1: the two coarser results are added at
//      (i / 2, j / 2) and (i / 4, j / 4) and the four 1x1 layers run on the accumulator registers; only p is written.
//
// The bank convolutions are implicit GEMMs on v_mfma_f32_16x16x4_f32:  D[cout 16][cell 16] += A[cout][k] * B[k][cell],  k = four
// consecutive input channels of one tap: 36 MFMAs per 16 cells.  The 16 cells are 16 consecutive positions q of the FLATTENED plane
// (q = y * P + x), so that the B operand of tap (dy, dx) is the plane at q + dy * P + dx for every lane; the two positions per row that
// wrap into the next row are computed and never used.  Operand maps (lane l):  A[l & 15][k = l >> 4],  B[k = l >> 4][l & 15],
// D: column l & 15, rows 4 * (l >> 4) + r in register r.  A: the 36 weights of a convolution sit in 36 registers of each lane for the
// whole tile (packed in that lane order).  B: one ds_read_b32 per MFMA; the plane stride S = 16 (mod 32) floats puts the two channel
// planes of a 32-lane group on disjoint banks.  D holds channels 4g .. 4g+3 of one cell in lane group g: register r of the result IS the
// B operand of a following 1x1 layer whose A operand carries the weights of input channels 4g + r, which is how the tail is packed.
// No atomics; a cell's value is a fixed-order sum that does not depend on the batch or on the tile it falls into.
#include <hip/hip_runtime.h>
#include "fnx_cnn.h"
#include "fnx_kernels.h"
#include "../../include/fluidnet_hip.h"

namespace fnx {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

// the blob: conv1, convBank.block.0, convBank.block.2, conv2, conv3, convOut; each weight (Cout, Cin, k, k) then bias
// (float offsets: conv1 0 / 288, block.0 304 / 2608, block.2 2624 / 4928, conv2 4944 / 5200, conv3 5216 / 5344, convOut 5352 / 5360)
constexpr int BLOB_WB0 = 304, BLOB_WB2 = 2624, BLOB_W2 = 4944, BLOB_B2 = 5200, BLOB_W3 = 5216, BLOB_B3 = 5344, BLOB_WO = 5352, BLOB_BO = 5360,
              BLOB_FLOATS = 5361;
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

__global__ void banknet_pack_kernel(const float* __restrict__ blob, float* __restrict__ pk) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= PK_FLOATS) return;
  float v = 0.f;
  if (i < PK_WB0) {
    v = blob[i];                                              // conv1 and its bias
  } else if (i < PK_W2) {
    const bool second = i >= PK_WB2;
    const int j = i - (second ? PK_WB2 : PK_WB0);
    const int src = second ? BLOB_WB2 : BLOB_WB0;
    if (j < 2304) {
      const int lane = j & 63, kc = (j >> 6) & 3, tap = j >> 8;
      v = blob[src + ((lane & 15) * 16 + 4 * kc + (lane >> 4)) * 9 + tap];
    } else {
      v = blob[src + j];                                      // the bias follows the weight in both
    }
  } else {
    const int layer = (i - PK_W2) / 272, j = (i - PK_W2) % 272;
    const int cout_n = layer == 0 ? 16 : (layer == 1 ? 8 : 1), cin_n = layer == 2 ? 8 : 16;
    const int wsrc = layer == 0 ? BLOB_W2 : (layer == 1 ? BLOB_W3 : BLOB_WO), bsrc = layer == 0 ? BLOB_B2 : (layer == 1 ? BLOB_B3 : BLOB_BO);
    if (j < 256) {
      const int lane = j & 63, r = j >> 6;
      const int cout = lane & 15, cin = 4 * (lane >> 4) + r;
      if (cout < cout_n && cin < cin_n) v = blob[wsrc + cout * cin_n + cin];
    } else if (j - 256 < cout_n) {
      v = blob[bsrc + j - 256];
    }
  }
  pk[i] = v;
}

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

// x (B, 2, H, W).  R = 4, 2: out (B, 16, H/R, W/R).  R = 1: l2, l4 the coarser results, p (B, 1, H, W).  256 threads.
template <int R, int TH, int TW>
__global__ __launch_bounds__(256) void banknet_level_kernel(const float* __restrict__ pk, const float* __restrict__ x, int H, int W,
                                                            float* __restrict__ out, const float* __restrict__ l2,
                                                            const float* __restrict__ l4, float* __restrict__ p) {
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

  // 3. cB0 on the tile + 1: position q = (y, x) of b0 is level cell (ty0 - 1 + y, tx0 - 1 + x)
  bank_conv<P, S>(pk + PK_WB0, pk + PK_BB0, la, T::G0, wave, lane, [&](int q, f32x4 v) {
    const int ly = ty0 - 1 + q / P, lxx = tx0 - 1 + q % P;
    const bool in = ly >= 0 && ly < HR && lxx >= 0 && lxx < WR;
#pragma unroll
    for (int r = 0; r < 4; ++r) lb[(4 * (lane >> 4) + r) * S + q] = in ? fmaxf(v[r], 0.f) : 0.f;
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
      f32x4 t;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ch = 4 * (lane >> 4) + r;
        t[r] = (fmaxf(v[r], 0.f) + l2b[((size_t)ch * H2 + cy / 2) * W2 + cx / 2]) + l4b[((size_t)ch * H4 + cy / 4) * W4 + cx / 4];
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
        } else {
          t = h;
        }
      }
      if (valid && lane < 16) pb[(size_t)ly * W + lxx] = t[0];
    });
  }
}

constexpr int TILE_H = 8, TILE_W1 = 32, TILE_WC = 16;   // level 1: 8 x 32 cells; levels 2 and 4: 8 x 16

inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }
struct BankWs { float* l2; float* l4; size_t bytes; };
BankWs banknet_ws_layout(int B, int H, int W, void* base) {
  BankWs w{};
  const size_t n2 = al256((size_t)B * 16 * (H / 2) * (W / 2) * 4), n4 = al256((size_t)B * 16 * (H / 4) * (W / 4) * 4);
  w.l2 = (float*)base;
  w.l4 = base ? (float*)((char*)base + n2) : nullptr;
  w.bytes = n2 + n4;
  return w;
}

void banknet_forward(int B, int H, int W, const float* pk, const float* x, float* p, void* ws, hipStream_t s) {
  const BankWs w = banknet_ws_layout(B, H, W, ws);
  ProfScope ps(FNX_PROF_CONV_MFMA16, s);
  auto grid = [&](int R, int tw) { return dim3((unsigned)((W / R + tw - 1) / tw), (unsigned)((H / R + TILE_H - 1) / TILE_H), (unsigned)B); };
  banknet_level_kernel<4, TILE_H, TILE_WC><<<grid(4, TILE_WC), 256, 0, s>>>(pk, x, H, W, w.l4, nullptr, nullptr, nullptr);
  banknet_level_kernel<2, TILE_H, TILE_WC><<<grid(2, TILE_WC), 256, 0, s>>>(pk, x, H, W, w.l2, nullptr, nullptr, nullptr);
  banknet_level_kernel<1, TILE_H, TILE_W1><<<grid(1, TILE_W1), 256, 0, s>>>(pk, x, H, W, nullptr, w.l2, w.l4, p);
}

// The scratch of the whole forward: the flags copy, the divergence, the net's input, scale_std's partial sums, the per-sample scales, the
// net's own workspace; each rounded up to 256 bytes.
struct BankFluidnetWs { float* flags; float* div; float* x; double* partial; float* scale; void* net; size_t bytes; };
BankFluidnetWs bank_fluidnet_ws_layout(int B, int H, int W, void* base) {
  const size_t full = (size_t)B * H * W;
  size_t off = 0;
  auto take = [&](size_t bytes) { void* r = base ? (char*)base + off : nullptr; off += al256(bytes); return r; };
  BankFluidnetWs w{};
  w.flags = (float*)take(full * 4);
  w.div = (float*)take(full * 4);
  w.x = (float*)take(full * 2 * 4);
  w.partial = (double*)take(scale_std_scratch_bytes(B));
  w.scale = (float*)take(sizeof(float) * B);
  w.net = take(banknet_ws_layout(B, H, W, nullptr).bytes);
  w.bytes = off;
  return w;
}

int bank_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? FNX_OK : set_error(FNX_EHIP, "HIP error in a bank-net launch: %s", hipGetErrorString(e));
}

// The checks the bank net's entry points share, before any device call, each refusal with its own text.
int check_bank_call(const char* fn, const FnxGrid* g, bool args, int precision_mode, bool whole, size_t ws_bytes) {
  if (!g || !args) return set_error(FNX_EINVAL, "%s: null argument", fn);
  if (g->is3D || g->D != 1)
    return set_error(FNX_EINVAL, "%s: the bank net ('FluidNet' model) is 2D only (is3D = %d, D = %d)", fn, g->is3D, g->D);
  const int mode = net_mode(precision_mode);
  if (mode < 0)
    return set_error(FNX_EINVAL, "%s: unknown precision_mode %d (FNX_PRECISION_FP32, _FP32_DIRECT, _BF16X6, _BF16X3, _FP32_F4 or _FP32_F2)", fn,
                     precision_mode);
  if (mode == FNX_PRECISION_BF16X6 || mode == FNX_PRECISION_BF16X3)
    return set_error(FNX_EINVAL, "%s: the bank net runs in fp32 arithmetic only (FNX_PRECISION_FP32, _FP32_F4, _FP32_F2 or _FP32_DIRECT), "
                     "not in the bf16 modes (precision_mode %d)", fn, precision_mode);
  if (g->B < 1 || g->B > 65535) return set_error(FNX_EINVAL, "%s: batch size %d is outside 1 .. 65535", fn, g->B);
  if (g->H < 4 || g->H % 4) return set_error(FNX_EINVAL, "%s: H = %d must be a positive multiple of 4 (the three levels are added)", fn, g->H);
  if (g->W < 4 || g->W % 4) return set_error(FNX_EINVAL, "%s: W = %d must be a positive multiple of 4 (the three levels are added)", fn, g->W);
  if ((size_t)g->H * g->W >= ((size_t)1 << 27))
    return set_error(FNX_EINVAL, "%s: H * W = %zu cells per sample is beyond the bank kernels' range", fn, (size_t)g->H * g->W);
  const size_t want = whole ? bank_fluidnet_ws_layout(g->B, g->H, g->W, nullptr).bytes : banknet_ws_layout(g->B, g->H, g->W, nullptr).bytes;
  if (ws_bytes < want) return set_error(FNX_EWORKSPACE, "%s: workspace of %zu bytes is too small (%zu needed)", fn, ws_bytes, want);
  return FNX_OK;
}

}  // namespace
}  // namespace fnx

extern "C" {

size_t fnx_banknet_weight_floats(void) { return fnx::BLOB_FLOATS; }
size_t fnx_banknet_packed_bytes(void) { return (size_t)fnx::PK_FLOATS * sizeof(float); }

int fnx_banknet_pack(const float* weights_blob, void* packed, void* stream) {
  if (!weights_blob || !packed) return fnx::set_error(FNX_EINVAL, "%s: null argument", __func__);
  fnx::banknet_pack_kernel<<<(fnx::PK_FLOATS + 255) / 256, 256, 0, (hipStream_t)stream>>>(weights_blob, (float*)packed);
  return fnx::bank_status();
}

size_t fnx_banknet_ws_bytes(const FnxGrid* g, int whole_forward) {
  if (!g || g->B < 1 || g->H < 4 || g->W < 4) return 0;
  return whole_forward ? fnx::bank_fluidnet_ws_layout(g->B, g->H, g->W, nullptr).bytes : fnx::banknet_ws_layout(g->B, g->H, g->W, nullptr).bytes;
}

int fnx_banknet_forward(const FnxGrid* g, const void* packed, const float* x, float* p, int precision_mode, void* ws, size_t ws_bytes,
                        void* stream) {
  if (int rc = fnx::check_bank_call(__func__, g, packed && x && p && ws, precision_mode, false, ws_bytes)) return rc;
  fnx::banknet_forward(g->B, g->H, g->W, (const float*)packed, x, p, ws, (hipStream_t)stream);
  return fnx::bank_status();
}

int fnx_fluidnet_bank_forward(const FnxGrid* g, const void* packed, const float* input, float thr, float* p_out, float* U_out,
                              int precision_mode, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = fnx::check_bank_call(__func__, g, packed && input && p_out && U_out && ws, precision_mode, true, ws_bytes)) return rc;
  const GridDims d = make_dims(g->B, 1, g->H, g->W, g->z_offset, g->D_global);
  hipStream_t s = (hipStream_t)stream;
  const fnx::BankFluidnetWs w = fnx::bank_fluidnet_ws_layout(g->B, g->H, g->W, ws);
  // FluidNet.forward around the net, with the launches of fnx_fluidnet_forward (lib/model.py:104-226)
  fnx::launch_gather_input(d, 2, input, U_out, w.flags, s);                               // :104-119
  if (int rc = fnx_velocity_divergence(g, U_out, w.flags, w.div, stream)) return rc;      // :125-126
  fnx::launch_scale_std(d, 2, U_out, thr, w.partial, w.scale, s);                         // :129-144
  fnx::launch_pack_input(d, 2, w.div, w.flags, w.scale, U_out, w.x, s);                   // :146-168
  fnx::banknet_forward(g->B, g->H, g->W, (const float*)packed, w.x, p_out, w.net, s);     // :179-209
  if (int rc = fnx_velocity_update(g, p_out, U_out, w.flags, stream)) return rc;          // :213-218
  fnx::launch_unscale(d, 2, w.scale, p_out, U_out, s);                                    // :221-223
  if (int rc = fnx_set_wall_bcs(g, U_out, w.flags, stream)) return rc;                    // :226
  return fnx::bank_status();
}

}  // extern "C"
