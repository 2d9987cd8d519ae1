// Training of the 16-channel bank net (fnx_banknet.hip) in 2D, exact fp32: a forward that also writes every ReLU output ("tape") and the
// backward with respect to the twelve parameter tensors.
//
//   forward   the three level launches of the inference forward with the tape switch of bank_level_tile on (fnx_banknet_tile.h): the
//             same arithmetic, so p has the inference forward's bits; the two coarser banks' results are read back from the tape.
//   backward  four kinds of launch, then one reduction:
//     bank_tail_bwd_kernel       convOut, conv3 and conv2 twice, per group of 16 cells on v_mfma_f32_16x16x4_f32.  The gradient of a 1x1
//                                layer's input is  D[cin][cell] += A[cin][k] B[k][cell]  with k = four output channels: the masked gradient
//                                sits on the accumulator registers (lane group g holds channels 4g .. 4g+3 of a cell) and register r IS the
//                                B operand of output channels 4g + r, the mirror of the forward's tail.  The weight gradients are
//                                D[cout][cin] += A[cout][k] B[k][cin] with k = four cells; the operands go through a 16 x 16 transpose in
//                                LDS.  conv2's accumulator takes both applications.  g_t (B,16,H,W) goes to the workspace.  It indexes
//                                flattened cells, so it is the 3D unit's tail backward as well: bank_tail_backward, at the end of
//                                this file, launches it on the 1x1 block of either unit's packed_t (fnx_banknet_train.h).
//     bank_level_bwd_kernel<R>   R = 1, 2, 4: the mirror of the forward's level kernel on a TH x TW tile of level-R cells.  g_b = g_t (R = 1)
//                                or the sum of its R x R children (the adjoint of nearest upsampling), masked by b > 0, on the tile + 2;
//                                g_h = convT(block.2) of it masked by h > 0 on the tile + 1; g_a = convT(block.0) of that on the tile,
//                                written to the workspace at the level's resolution.  convT is bank_conv on the transposed, tap-flipped
//                                weights of packed_t, with zero padding at the level's own border.  Both weight gradients run while the
//                                planes are in LDS: per tap  D[cout][cin] += A[cout][k] B[k][cin],  k = four cells of a tile row, A the
//                                masked gradient at the tile's own cells (nothing of the halo, the wrap columns or beyond the domain: the
//                                march only visits the tile's rows, and cells beyond the domain hold zero), B the layer's input shifted by
//                                the tap; 2 x 9 accumulators (72 registers) live across the workgroup's tiles.
//     bank_conv1_bwd_kernel      g_a = g_a1 + up2(g_a2) / 4 + up4(g_a4) / 16 (the adjoint of the average pooling), masked by a > 0,
//                                into conv1's 288 weight and 16 bias gradients: plain VALU sums.
//     bank_reduce_kernel         adds the per-workgroup partial sums in index order in fp64 (the three levels of a bank tensor in the
//                                order quarter, half, full) and writes grad_blob.
// A launch has min(work items, 512) workgroups and workgroup s takes the items s, s + n, ...: the split is a function of (B, H, W) alone.
// No atomics, no host synchronisation; grad_p, x and the tape are only read.
#include "fnx_banknet_train.h"

namespace fnx {
namespace {

// packed_t of the 2D net: fnx_banknet_train.h with nine taps
__global__ void banknet_pack_t_kernel(const float* __restrict__ blob, float* __restrict__ pt) {
  bank_pack_t(blob, pt, 9, BLOB_WB0, BLOB_WB2, BLOB_W2);
}

// ---- forward ----
template <int R, int TH, int TW>
__global__ __launch_bounds__(256) void banknet_level_tape_kernel(const float* __restrict__ pk, const float* __restrict__ x, int H, int W,
                                                                 float* __restrict__ out, const float* __restrict__ l2,
                                                                 const float* __restrict__ l4, float* __restrict__ p, BankTapeOut tape) {
  bank_level_tile<R, TH, TW, true>(pk, x, H, W, out, l2, l4, p, tape);
}

void banknet_forward_train(const FnxGrid* g, const void* packed, const float* x, float* p, float* tape, int /*mode*/, hipStream_t s) {
  const int B = g->B, H = g->H, W = g->W;
  const float* pk = (const float*)packed;
  const BankTapeLayout T = bank_tape_layout(2, B, 1, H, W);
  auto at = [&](int n) { return tape + T.e[n].off; };
  ProfScope ps(FNX_PROF_CONV_MFMA16, s);
  auto grid = [&](int R, int tw) { return dim3((unsigned)((W / R + tw - 1) / tw), (unsigned)((H / R + TILE_H - 1) / TILE_H), (unsigned)B); };
  banknet_level_tape_kernel<4, TILE_H, TILE_WC><<<grid(4, TILE_WC), 256, 0, s>>>(pk, x, H, W, at(TP_B4), nullptr, nullptr, nullptr,
                                                                                 BankTapeOut{at(TP_A4), at(TP_H4)});
  banknet_level_tape_kernel<2, TILE_H, TILE_WC><<<grid(2, TILE_WC), 256, 0, s>>>(pk, x, H, W, at(TP_B2), nullptr, nullptr, nullptr,
                                                                                 BankTapeOut{at(TP_A2), at(TP_H2)});
  banknet_level_tape_kernel<1, TILE_H, TILE_W1><<<grid(1, TILE_W1), 256, 0, s>>>(
      pk, x, H, W, nullptr, at(TP_B2), at(TP_B4), p, BankTapeOut{at(TP_A), at(TP_H1), at(TP_B1), at(TP_T), at(TP_C2A), at(TP_C2B), at(TP_C3)});
}

// ---- backward ----
// floats of a workgroup's partial sums (the tail's: TAIL_P of fnx_banknet_train.h)
constexpr int LEV_P = 4640;               // block.2 [tap 9][cout 16][cin 16], block.0 the same; then their biases, 16 each
constexpr int C1_P = 304;                 // conv1 in the blob's own order: [16][18], then the bias

__global__ __launch_bounds__(256) void bank_tail_bwd_kernel(const float* __restrict__ pt, const float* __restrict__ grad_p,
                                                            const float* __restrict__ tt, const float* __restrict__ c2a,
                                                            const float* __restrict__ c2b, const float* __restrict__ c3,
                                                            float* __restrict__ g_t, float* __restrict__ partial, int HW, int ups, int nunits) {
  constexpr int TS = 16 * 17;                 // a 16 x 16 transpose tile, pitch 17
  __shared__ float st[4 * 8 * TS];
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* const sw = st + wave * 8 * TS;
  float a2t[4], a3t[4], wo[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    a2t[r] = pt[PT_W2T + r * 64 + lane];
    a3t[r] = pt[PT_W3T + r * 64 + lane];
    wo[r] = pt[PT_WO + 4 * g + r];
  }
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 dO = zero4, d3 = zero4, d2 = zero4;
  float bO = 0.f, b3 = 0.f, b2 = 0.f;
  for (int u = blockIdx.x; u < nunits; u += gridDim.x) {
    const int b = u / ups, n = (u - b * ups) * 64 + wave * 16 + c;
    const bool valid = n < HW;
    const int nn = valid ? n : HW - 1;
    const float gp = valid ? grad_p[(size_t)b * HW + nn] : 0.f;
    const size_t o16 = ((size_t)b * 16 + 4 * g) * HW + nn, o8 = ((size_t)b * 8 + 4 * (g & 1)) * HW + nn;
    f32x4 vc3, vc2b, vc2a, vt;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      vc3[r] = valid && g < 2 ? c3[o8 + (size_t)r * HW] : 0.f;
      vc2b[r] = valid ? c2b[o16 + (size_t)r * HW] : 0.f;
      vc2a[r] = valid ? c2a[o16 + (size_t)r * HW] : 0.f;
      vt[r] = valid ? tt[o16 + (size_t)r * HW] : 0.f;
    }
    // the gradients of the pre-activations: register r of a lane is channel 4g + r of its cell
    f32x4 gc3, gc2b = zero4, gc2a = zero4, gt = zero4;
#pragma unroll
    for (int r = 0; r < 4; ++r) gc3[r] = vc3[r] > 0.f ? gp * wo[r] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) gc2b = __builtin_amdgcn_mfma_f32_16x16x4f32(a3t[r], gc3[r], gc2b, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) gc2b[r] = vc2b[r] > 0.f ? gc2b[r] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) gc2a = __builtin_amdgcn_mfma_f32_16x16x4f32(a2t[r], gc2b[r], gc2a, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) gc2a[r] = vc2a[r] > 0.f ? gc2a[r] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) gt = __builtin_amdgcn_mfma_f32_16x16x4f32(a2t[r], gc2a[r], gt, 0, 0, 0);
    if (valid) {
#pragma unroll
      for (int r = 0; r < 4; ++r) g_t[o16 + (size_t)r * HW] = gt[r];
    }
    // [channel][cell] tiles for the weight gradients: grad_p (row 0), g_c3, g_c2b, g_c2a; c3, c2b, c2a, t
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int at = (4 * g + r) * 17 + c;
      sw[0 * TS + at] = (g == 0 && r == 0) ? gp : 0.f;
      sw[1 * TS + at] = gc3[r];
      sw[2 * TS + at] = gc2b[r];
      sw[3 * TS + at] = gc2a[r];
      sw[4 * TS + at] = vc3[r];
      sw[5 * TS + at] = vc2b[r];
      sw[6 * TS + at] = vc2a[r];
      sw[7 * TS + at] = vt[r];
    }
    __syncthreads();
    // lane: channel c of both operands, cell 4 step + g
#pragma unroll
    for (int step = 0; step < 4; ++step) {
      const int at = c * 17 + 4 * step + g;
      const float aO = sw[0 * TS + at], a3 = sw[1 * TS + at], a2b = sw[2 * TS + at], a2a = sw[3 * TS + at];
      dO = __builtin_amdgcn_mfma_f32_16x16x4f32(aO, sw[4 * TS + at], dO, 0, 0, 0);
      d3 = __builtin_amdgcn_mfma_f32_16x16x4f32(a3, sw[5 * TS + at], d3, 0, 0, 0);
      d2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2b, sw[6 * TS + at], d2, 0, 0, 0);     // the second application: (g at c2b, c2a)
      d2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2a, sw[7 * TS + at], d2, 0, 0, 0);     // the first: (g at c2a, t)
      bO += aO;
      b3 += a3;
      b2 += a2b + a2a;
    }
  }
  // the four waves in order: D register r is row 4g + r, column c; a bias sum is per (channel c, cell slot g)
  __syncthreads();
  float* const red = st;                      // [wave][768 + 192]
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    red[wave * 960 + 0 + (4 * g + r) * 16 + c] = dO[r];
    red[wave * 960 + 256 + (4 * g + r) * 16 + c] = d3[r];
    red[wave * 960 + 512 + (4 * g + r) * 16 + c] = d2[r];
  }
  red[wave * 960 + 768 + lane] = bO;
  red[wave * 960 + 832 + lane] = b3;
  red[wave * 960 + 896 + lane] = b2;
  __syncthreads();
  float* const po = partial + (size_t)blockIdx.x * TAIL_P;
  for (int q = tid; q < TAIL_P; q += 256) {
    float v = 0.f;
    if (q < 768) {
      v = (red[q] + red[960 + q]) + (red[1920 + q] + red[2880 + q]);
    } else {
      const int which = (q - 768) >> 4, ch = (q - 768) & 15;
      for (int w = 0; w < 4; ++w)
        for (int k = 0; k < 4; ++k) v += red[w * 960 + 768 + which * 64 + k * 16 + ch];
    }
    po[q] = v;
  }
}

// the planes of a backward level tile: bank_conv's geometry with a stride = 17 (mod 32), on which the weight gradients' operand reads
// (lane: channel lane & 15, cell lane >> 4) fall into 32 distinct banks per half-wave.  Every level runs on 8 x 32 tiles: the 72
// accumulators and a convolution's 36 operands admit two workgroups per CU, which is what the planes of that tile admit too.
template <int R, int TH, int TW>
struct BankBwdTile {
  using F = BankTile<1, TH, TW>;        // (the planes' geometry does not depend on the level)
  static constexpr int P = F::P, NA = F::NA, Q0 = F::Q0, G0 = F::G0, G2 = F::G2;
  static constexpr int S = (F::SMIN + 14) / 32 * 32 + 17;
  static constexpr int LDS_FLOATS = 32 * S;
  static_assert(S >= F::SMIN && S % 32 == 17 && NA <= S && 16 * (G0 + 1) <= S, "plane stride");
  static_assert(LDS_FLOATS * 4 <= 64 * 1024 && LDS_FLOATS >= 4 * 256, "static LDS");
  static_assert(TW % 4 == 0, "the weight gradients take four cells of a row a step");
};

// gt (B,16,H,W); b, h, a: the tape's entries of level R; ga (B,16,H/R,W/R); partial [gridDim.x][LEV_P]
template <int R, int TH, int TW>
__global__ __launch_bounds__(256, 2) void bank_level_bwd_kernel(const float* __restrict__ pt, const float* __restrict__ gt,
                                                                const float* __restrict__ tb, const float* __restrict__ th,
                                                                const float* __restrict__ ta, float* __restrict__ ga,
                                                                float* __restrict__ partial, int H, int W, int ntx, int nty, int ntiles) {
  using T = BankBwdTile<R, TH, TW>;
  constexpr int P = T::P, S = T::S;
  __shared__ float lds[T::LDS_FLOATS];
  float* const pa = lds;                  // g_b on the tile + 2, then a on the tile + 1
  float* const pb = lds + 16 * S;         // h on the tile + 1, then g_h in its place
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int HR = H / R, WR = W / R;
  const size_t lev = (size_t)HR * WR;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc2[9], acc0[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc2[t] = acc0[t] = zero4;
  float bs2 = 0.f, bs0 = 0.f;

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int tx = tile % ntx, ty = (tile / ntx) % nty, b = tile / (ntx * nty);
    const int ty0 = ty * TH, tx0 = tx * TW;
    const float* gtb = gt + (size_t)b * 16 * H * W;
    const float* tbb = tb + (size_t)b * 16 * lev;
    const float* thb = th + (size_t)b * 16 * lev;
    const float* tab = ta + (size_t)b * 16 * lev;
    float* gab = ga + (size_t)b * 16 * lev;
    __syncthreads();                       // the previous tile's reads of both planes are done
    // g_b on the tile + 2: position (y, x) is level cell (ty0 - 2 + y, tx0 - 2 + x); zero beyond the domain
    for (int i = tid; i < 16 * T::NA; i += 256) {
      const int ch = i / T::NA, n = i - ch * T::NA;
      const int y = n / P, xx = n - y * P;
      const int ly = ty0 - 2 + y, lx = tx0 - 2 + xx;
      float v = 0.f;
      if (ly >= 0 && ly < HR && lx >= 0 && lx < WR && tbb[(size_t)ch * lev + (size_t)ly * WR + lx] > 0.f) {
        const float* src = gtb + ((size_t)ch * H + (size_t)ly * R) * W + (size_t)lx * R;
#pragma unroll
        for (int py = 0; py < R; ++py)
#pragma unroll
          for (int px = 0; px < R; ++px) v += src[(size_t)py * W + px];
      }
      pa[ch * S + n] = v;
    }
    // h on the tile + 1: position (y, x) is level cell (ty0 - 1 + y, tx0 - 1 + x)
    for (int i = tid; i < 16 * T::Q0; i += 256) {
      const int ch = i / T::Q0, n = i - ch * T::Q0;
      const int y = n / P, xx = n - y * P;
      const int ly = ty0 - 1 + y, lx = tx0 - 1 + xx;
      float v = 0.f;
      if (xx < TW + 2 && ly >= 0 && ly < HR && lx >= 0 && lx < WR) v = thb[(size_t)ch * lev + (size_t)ly * WR + lx];
      pb[ch * S + n] = v;
    }
    __syncthreads();
    // block.2's weight gradient over the tile's own cells: A = g_b at (y + 2, x + 2), B = h at (y + dy, x + dx)
    for (int step = wave; step < TH * (TW / 4); step += 4) {
      const int y = step / (TW / 4), x4 = (step - y * (TW / 4)) * 4 + g;
      const float av = pa[c * S + (y + 2) * P + x4 + 2];
      const float* bp = pb + c * S + y * P + x4;
      bs2 += av;
#pragma unroll
      for (int t = 0; t < 9; ++t) acc2[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bp[(t / 3) * P + (t % 3)], acc2[t], 0, 0, 0);
    }
    __syncthreads();                       // h is overwritten next
    // g_h on the tile + 1, masked by h > 0 and the domain, in h's place (a lane reads and writes only its own positions)
    bank_conv<P, S>(pt + PT_WB2T, pt + PT_ZERO, pa, T::G0, wave, lane, [&](int q, f32x4 v) {
      const int y = q / P, xx = q - y * P;
      const int ly = ty0 - 1 + y, lx = tx0 - 1 + xx;
      const bool in = q < T::Q0 && xx < TW + 2 && ly >= 0 && ly < HR && lx >= 0 && lx < WR;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float* at = pb + (4 * g + r) * S + q;
        *at = (in && *at > 0.f) ? v[r] : 0.f;
      }
    });
    __syncthreads();
    // a on the tile + 1 over g_b, which is done with
    for (int i = tid; i < 16 * T::Q0; i += 256) {
      const int ch = i / T::Q0, n = i - ch * T::Q0;
      const int y = n / P, xx = n - y * P;
      const int ly = ty0 - 1 + y, lx = tx0 - 1 + xx;
      float v = 0.f;
      if (xx < TW + 2 && ly >= 0 && ly < HR && lx >= 0 && lx < WR) v = tab[(size_t)ch * lev + (size_t)ly * WR + lx];
      pa[ch * S + n] = v;
    }
    // g_a on the tile
    bank_conv<P, S>(pt + PT_WB0T, pt + PT_ZERO, pb, T::G2, wave, lane, [&](int q, f32x4 v) {
      const int y = q / P, xx = q - y * P;
      const int ly = ty0 + y, lx = tx0 + xx;
      if (y < TH && xx < TW && ly < HR && lx < WR) {
#pragma unroll
        for (int r = 0; r < 4; ++r) gab[(size_t)(4 * g + r) * lev + (size_t)ly * WR + lx] = v[r];
      }
    });
    __syncthreads();
    // block.0's weight gradient: A = g_h at (y + 1, x + 1), B = a at (y + dy, x + dx)
    for (int step = wave; step < TH * (TW / 4); step += 4) {
      const int y = step / (TW / 4), x4 = (step - y * (TW / 4)) * 4 + g;
      const float av = pb[c * S + (y + 1) * P + x4 + 1];
      const float* bp = pa + c * S + y * P + x4;
      bs0 += av;
#pragma unroll
      for (int t = 0; t < 9; ++t) acc0[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bp[(t / 3) * P + (t % 3)], acc0[t], 0, 0, 0);
    }
  }
  // the four waves in order, one tap at a time: D register r is row cout = 4g + r, column cin = c
  float* const po = partial + (size_t)blockIdx.x * LEV_P;
#pragma unroll
  for (int t = 0; t < 18; ++t) {
    const f32x4 d = t < 9 ? acc2[t % 9] : acc0[t % 9];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) lds[wave * 256 + (4 * g + r) * 16 + c] = d[r];
    __syncthreads();
    po[t * 256 + tid] = (lds[tid] + lds[256 + tid]) + (lds[512 + tid] + lds[768 + tid]);
  }
  __syncthreads();
  lds[wave * 64 + lane] = bs2;
  lds[256 + wave * 64 + lane] = bs0;
  __syncthreads();
  if (tid < 32) {
    const int which = tid >> 4, ch = tid & 15;
    float v = 0.f;
    for (int w = 0; w < 4; ++w)
      for (int k = 0; k < 4; ++k) v += lds[which * 256 + w * 64 + k * 16 + ch];
    po[4608 + tid] = v;
  }
}

// wave w: output channels 4w .. 4w+3; a lane: one cell of a unit of 64
__global__ __launch_bounds__(256) void bank_conv1_bwd_kernel(const float* __restrict__ x, const float* __restrict__ a,
                                                             const float* __restrict__ ga1, const float* __restrict__ ga2,
                                                             const float* __restrict__ ga4, float* __restrict__ partial, int H, int W, int ups,
                                                             int nunits) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int HW = H * W, H2 = H / 2, W2 = W / 2, H4 = H / 4, W4 = W / 4;
  float acc[4][18], bs[4];
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) {
    bs[ch] = 0.f;
#pragma unroll
    for (int k = 0; k < 18; ++k) acc[ch][k] = 0.f;
  }
  for (int u = blockIdx.x; u < nunits; u += gridDim.x) {
    const int b = u / ups, n = (u - b * ups) * 64 + lane;
    if (n >= HW) continue;
    const int y = n / W, xx = n - y * W;
    float in[18];
#pragma unroll
    for (int ci = 0; ci < 2; ++ci)
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const int yy = y + dy - 1, xc = xx + dx - 1;
          const bool inside = yy >= 0 && yy < H && xc >= 0 && xc < W;
          in[ci * 9 + dy * 3 + dx] = inside ? x[((size_t)b * 2 + ci) * HW + (size_t)yy * W + xc] : 0.f;
        }
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      const size_t bc = (size_t)b * 16 + 4 * wave + ch;
      float gv = ga1[bc * HW + n] + 0.25f * ga2[(bc * H2 + y / 2) * W2 + xx / 2] + 0.0625f * ga4[(bc * H4 + y / 4) * W4 + xx / 4];
      gv = a[bc * HW + n] > 0.f ? gv : 0.f;
      bs[ch] += gv;
#pragma unroll
      for (int k = 0; k < 18; ++k) acc[ch][k] = fmaf(gv, in[k], acc[ch][k]);
    }
  }
  float* const po = partial + (size_t)blockIdx.x * C1_P;
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) {
#pragma unroll
    for (int k = 0; k < 19; ++k) {
      float v = k < 18 ? acc[ch][k] : bs[ch];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
      if (lane == 0) po[k < 18 ? (4 * wave + ch) * 18 + k : 288 + 4 * wave + ch] = v;
    }
  }
}

struct BankSplits { int tail, lev[3], c1; };      // lev: quarter, half, full resolution
__global__ __launch_bounds__(256) void bank_reduce_kernel(const float* __restrict__ ptail, const float* __restrict__ plev4,
                                                          const float* __restrict__ plev2, const float* __restrict__ plev1,
                                                          const float* __restrict__ pc1, float* __restrict__ out, BankSplits ns) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= BLOB_FLOATS) return;
  double v = 0.0;
  if (q < BLOB_WB0) {
    for (int s = 0; s < ns.c1; ++s) v += (double)pc1[(size_t)s * C1_P + q];
  } else if (q < BLOB_W2) {
    const int slot = q < BLOB_WB2 ? 1 : 0, j = q - (slot ? BLOB_WB0 : BLOB_WB2);
    int at;
    if (j < 2304) {
      const int co = j / 144, ci = (j / 9) % 16, tap = j % 9;
      at = slot * 2304 + tap * 256 + co * 16 + ci;
    } else {
      at = 4608 + slot * 16 + (j - 2304);
    }
    for (int s = 0; s < ns.lev[0]; ++s) v += (double)plev4[(size_t)s * LEV_P + at];
    for (int s = 0; s < ns.lev[1]; ++s) v += (double)plev2[(size_t)s * LEV_P + at];
    for (int s = 0; s < ns.lev[2]; ++s) v += (double)plev1[(size_t)s * LEV_P + at];
  } else {
    const int at = bank_tail_partial_at(q);
    for (int s = 0; s < ns.tail; ++s) v += (double)ptail[(size_t)s * TAIL_P + at];
  }
  out[q] = (float)v;
}

// the backward's launch plan and workspace: a function of (B, H, W) alone
struct BankBwdPlan {
  BankUnits u;                     // the tail's and conv1's units of 64 cells
  int ntx[3], nty[3], ntiles[3];   // level tiles: quarter, half, full
  BankSplits ns;
  float *gt, *ga1, *ga2, *ga4, *ptail, *plev[3], *pc1;
  size_t bytes;
};
BankBwdPlan bank_bwd_plan(int B, int H, int W, void* base) {
  BankBwdPlan p{};
  const size_t HW = (size_t)H * W;
  p.u = bank_units(B, HW);
  for (int l = 0; l < 3; ++l) {
    const int R = 4 >> l, tw = TILE_W1;
    p.ntx[l] = (W / R + tw - 1) / tw;
    p.nty[l] = (H / R + TILE_H - 1) / TILE_H;
    p.ntiles[l] = B * p.ntx[l] * p.nty[l];
    p.ns.lev[l] = split_of(p.ntiles[l]);
  }
  p.ns.tail = p.ns.c1 = p.u.split;
  size_t off = 0;
  auto take = [&](size_t floats) { float* r = base ? (float*)((char*)base + off) : nullptr; off += al256(floats * 4); return r; };
  p.gt = take(B * 16 * HW);
  p.ga1 = take(B * 16 * HW);
  p.ga2 = take(B * 16 * (HW / 4));
  p.ga4 = take(B * 16 * (HW / 16));
  p.ptail = take((size_t)p.ns.tail * TAIL_P);
  for (int l = 0; l < 3; ++l) p.plev[l] = take((size_t)p.ns.lev[l] * LEV_P);
  p.pc1 = take((size_t)p.ns.c1 * C1_P);
  p.bytes = off;
  return p;
}
size_t bank_bwd_plan_bytes(const FnxGrid* g) { return bank_bwd_plan(g->B, g->H, g->W, nullptr).bytes; }

bool banknet_backward(const FnxGrid* g, const void* packed_t, const float* x, const float* grad_p, const float* tape, float* grad_blob,
                      int /*mode*/, void* ws, hipStream_t s) {
  const int B = g->B, H = g->H, W = g->W;
  const float* pt = (const float*)packed_t;
  const BankTapeLayout T = bank_tape_layout(2, B, 1, H, W);
  const BankBwdPlan p = bank_bwd_plan(B, H, W, ws);
  auto at = [&](int n) { return tape + T.e[n].off; };
  ProfScope ps(FNX_PROF_CONV_MFMA16, s);
  bank_tail_backward(pt + PT_W2T, grad_p, at(TP_T), at(TP_C2A), at(TP_C2B), at(TP_C3), p.gt, p.ptail, H * W, p.u.ups, p.u.nunits, p.ns.tail, s);
  bank_level_bwd_kernel<4, TILE_H, TILE_W1><<<p.ns.lev[0], 256, 0, s>>>(pt, p.gt, at(TP_B4), at(TP_H4), at(TP_A4), p.ga4, p.plev[0], H, W,
                                                                        p.ntx[0], p.nty[0], p.ntiles[0]);
  bank_level_bwd_kernel<2, TILE_H, TILE_W1><<<p.ns.lev[1], 256, 0, s>>>(pt, p.gt, at(TP_B2), at(TP_H2), at(TP_A2), p.ga2, p.plev[1], H, W,
                                                                        p.ntx[1], p.nty[1], p.ntiles[1]);
  bank_level_bwd_kernel<1, TILE_H, TILE_W1><<<p.ns.lev[2], 256, 0, s>>>(pt, p.gt, at(TP_B1), at(TP_H1), at(TP_A), p.ga1, p.plev[2], H, W,
                                                                        p.ntx[2], p.nty[2], p.ntiles[2]);
  bank_conv1_bwd_kernel<<<p.ns.c1, 256, 0, s>>>(x, at(TP_A), p.ga1, p.ga2, p.ga4, p.pc1, H, W, p.u.ups, p.u.nunits);
  bank_reduce_kernel<<<(BLOB_FLOATS + 255) / 256, 256, 0, s>>>(p.ptail, p.plev[0], p.plev[1], p.plev[2], p.pc1, grad_blob, p.ns);
  return true;
}

bool bank2d_sized(const FnxGrid* g) { return g && !g->is3D && g->D == 1 && g->B >= 1 && g->H >= 4 && g->W >= 4; }
// the net's record (fnx_fluidnet.h): its input is kept in the tape, the backward's conv1 reads it again
size_t bank_tape_x(const FnxGrid* g) { return bank_tape_layout(2, g->B, 1, g->H, g->W).e[TP_X].off; }
constexpr NetTrain NET2 = {2, bank_status, banknet_forward_train, banknet_backward, bank_bwd_plan_bytes, bank_tape_x};
constexpr BankTrainDim DIM2 = {NET2, bank2d_sized, nullptr};

}  // namespace

// The kernel reads its three blocks at pt[PT_W2T + ...], pt[PT_W3T + ...] and pt[PT_WO + ...], so it is given tail_t - PT_W2T: the 2D
// image's own start, or 9216 floats into the 3D image (never a pointer before the allocation).
static_assert(PT3_W3T - PT3_W2T == PT_W3T - PT_W2T && PT3_WO - PT3_W2T == PT_WO - PT_W2T && PT3_W2T >= PT_W2T,
              "the 1x1 block sits alike in both images of packed_t");
void bank_tail_backward(const float* tail_t, const float* grad_p, const float* tt, const float* c2a, const float* c2b, const float* c3,
                        float* g_t, float* partial, int N, int ups, int nunits, int split, hipStream_t s) {
  bank_tail_bwd_kernel<<<split, 256, 0, s>>>(tail_t - PT_W2T, grad_p, tt, c2a, c2b, c3, g_t, partial, N, ups, nunits);
}

}  // namespace fnx

extern "C" {

int fnx_banknet_tape_entries(void) { return fnx::N_BANK_TAPE; }

size_t fnx_banknet_tape_layout(const FnxGrid* g, FnxTapeEntry* entries) {
  if (!g || g->is3D || g->D != 1 || g->B < 1 || g->H < 4 || g->H % 4 || g->W < 4 || g->W % 4) {
    fnx::set_error(FNX_EINVAL, "%s: a 2D grid with H and W positive multiples of 4 is needed", __func__);
    return 0;
  }
  return fnx::bank_fill_tape(fnx::bank_tape_layout(2, g->B, 1, g->H, g->W), entries, nullptr);
}

size_t fnx_banknet_packed_t_bytes(void) { return (size_t)fnx::PT_FLOATS * sizeof(float); }

int fnx_banknet_pack_t(const float* weights_blob, void* packed_t, void* stream) {
  if (!weights_blob || !packed_t) return fnx::set_error(FNX_EINVAL, "%s: null argument", __func__);
  fnx::banknet_pack_t_kernel<<<(fnx::PT_FLOATS + 255) / 256, 256, 0, (hipStream_t)stream>>>(weights_blob, (float*)packed_t);
  return fnx::bank_status();
}

size_t fnx_banknet_backward_ws_bytes(const FnxGrid* g) { return fnx::bank_size_query<fnx::DIM2>(g, fnx::bank_bwd_ws<fnx::DIM2>); }

int fnx_banknet_forward_train(const FnxGrid* g, const void* packed, const float* x, float* p, float* tape, int precision_mode, void* stream) {
  return fnx::bank_forward_train<fnx::DIM2>(__func__, g, packed, x, p, tape, precision_mode, stream);
}

int fnx_banknet_backward(const FnxGrid* g, const void* packed_t, const float* x, const float* grad_p, const float* tape, float* grad_blob,
                         int precision_mode, void* ws, size_t ws_bytes, void* stream) {
  return fnx::bank_backward<fnx::DIM2>(__func__, g, packed_t, x, grad_p, tape, grad_blob, precision_mode, ws, ws_bytes, stream);
}

size_t fnx_fluidnet_bank_train_ws_bytes(const FnxGrid* g) { return fnx::bank_size_query<fnx::DIM2>(g, fnx::bank_train_ws<fnx::DIM2>); }

int fnx_fluidnet_bank_forward_train(const FnxGrid* g, const void* packed, const float* input, float normalize_threshold, float* p_out,
                                    float* U_out, float* flags_out, float* scale_out, float* tape, int precision_mode, void* ws,
                                    size_t ws_bytes, void* stream) {
  return fnx::bank_whole_forward_train<fnx::DIM2>(__func__, g, packed, input, normalize_threshold, p_out, U_out, flags_out, scale_out, tape,
                                                  precision_mode, ws, ws_bytes, stream);
}

int fnx_fluidnet_bank_backward(const FnxGrid* g, const void* packed_t, const float* flags, const float* scale,
                               const float* grad_p, const float* grad_U, const float* tape, float* grad_blob, int precision_mode, void* ws,
                               size_t ws_bytes, void* stream) {
  return fnx::bank_whole_backward<fnx::DIM2>(__func__, g, packed_t, flags, scale, grad_p, grad_U, tape, grad_blob, precision_mode, ws, ws_bytes,
                                             stream);
}

}  // extern "C"
