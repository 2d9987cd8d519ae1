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
#include "fnx_banknet_tile.h"

namespace fnx {
namespace {

__global__ void banknet_pack_kernel(const float* __restrict__ blob, float* __restrict__ pk) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= PK_FLOATS) return;
  float v = 0.f;
  if (i < PK_WB0) {
    v = blob[i];                                              // conv1 and its bias
  } else if (i < PK_W2) {
    const bool second = i >= PK_WB2;
    v = bank_pack_conv16(blob, second ? BLOB_WB2 : BLOB_WB0, 9, i - (second ? PK_WB2 : PK_WB0));
  } else {
    v = bank_pack_tail(blob, BLOB_W2, i - PK_W2);
  }
  pk[i] = v;
}

// x (B, 2, H, W).  R = 4, 2: out (B, 16, H/R, W/R).  R = 1: l2, l4 the coarser results, p (B, 1, H, W).  256 threads.
template <int R, int TH, int TW>
__global__ __launch_bounds__(256) void banknet_level_kernel(const float* __restrict__ pk, const float* __restrict__ x, int H, int W,
                                                            float* __restrict__ out, const float* __restrict__ l2,
                                                            const float* __restrict__ l4, float* __restrict__ p) {
  bank_level_tile<R, TH, TW, false>(pk, x, H, W, out, l2, l4, p, BankTapeOut{});
}

void banknet_forward(int B, int H, int W, const float* pk, const float* x, float* p, void* ws, hipStream_t s) {
  const BankWs w = banknet_ws_layout(B, H, W, ws);
  ProfScope ps(FNX_PROF_CONV_MFMA16, s);
  auto grid = [&](int R, int tw) { return dim3((unsigned)((W / R + tw - 1) / tw), (unsigned)((H / R + TILE_H - 1) / TILE_H), (unsigned)B); };
  banknet_level_kernel<4, TILE_H, TILE_WC><<<grid(4, TILE_WC), 256, 0, s>>>(pk, x, H, W, w.l4, nullptr, nullptr, nullptr);
  banknet_level_kernel<2, TILE_H, TILE_WC><<<grid(2, TILE_WC), 256, 0, s>>>(pk, x, H, W, w.l2, nullptr, nullptr, nullptr);
  banknet_level_kernel<1, TILE_H, TILE_W1><<<grid(1, TILE_W1), 256, 0, s>>>(pk, x, H, W, nullptr, w.l2, w.l4, p);
}

// the workspace of the net alone and of the whole forward (the flags copy, fnx_fluidnet.h's FluidnetWs with the net's at its end)
size_t bank_net_ws(const FnxGrid* g) { return banknet_ws_layout(g->B, g->H, g->W, nullptr).bytes; }
size_t bank_whole_ws(const FnxGrid* g) { return fluidnet_whole_ws_bytes(g->B, (size_t)g->H * g->W, bank_net_ws(g)); }

}  // namespace

// the net as FluidNet.forward's wrapper runs it (fnx_fluidnet.h)
const Net& banknet_net() {
  static const Net net = {2, FNX_NET_BANK, bank_status, bank_net_ws,
                          [](const FnxGrid* g, const void* packed, const float* x, float* p, int, void* ws, hipStream_t s) {
                            banknet_forward(g->B, g->H, g->W, (const float*)packed, x, p, ws, s);               // model.py:179-209
                          }};
  return net;
}
int check_bank_grid(const char* fn, const FnxGrid* g, int precision_mode) {
  return check_bank_call(fn, 2, g, true, precision_mode, nullptr, 0);
}
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
  return whole_forward ? fnx::bank_whole_ws(g) : fnx::bank_net_ws(g);
}

int fnx_banknet_forward(const FnxGrid* g, const void* packed, const float* x, float* p, int precision_mode, void* ws, size_t ws_bytes,
                        void* stream) {
  if (int rc = fnx::check_bank_call(__func__, 2, g, packed && x && p && ws, precision_mode, fnx::bank_net_ws, ws_bytes)) return rc;
  fnx::banknet_forward(g->B, g->H, g->W, (const float*)packed, x, p, ws, (hipStream_t)stream);
  return fnx::bank_status();
}

// FluidNet.forward (lib/model.py:104-226) around the net, as fnx_fluidnet_forward runs it around the ScaleNet
int fnx_fluidnet_bank_forward(const FnxGrid* g, const void* packed, const float* input, float thr, float* p_out, float* U_out,
                              int precision_mode, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = fnx::check_bank_call(__func__, 2, g, packed && input && p_out && U_out && ws, precision_mode, fnx::bank_whole_ws, ws_bytes))
    return rc;
  return fnx::fluidnet_whole_forward(fnx::banknet_net(), g, packed, input, thr, p_out, U_out, precision_mode, ws, stream);
}

}  // extern "C"
