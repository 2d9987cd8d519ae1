// The Conv3d counterpart of the 16-channel bank net (mconf['model'] = 'FluidNet3D'; the reference's net of lib/model.py:177-209 with every
// module replaced by its 3D sibling), inference forward, exact fp32.
//
//   a  = relu(conv1(x))                               2 -> 16, 3x3x3, zero padding at the full-resolution border
//   a2 = avgpool3d(a, 2), a4 = avgpool3d(a, 4)
//   bank(t) = relu(cB2(relu(cB0(t))))                 16 -> 16 -> 16, 3x3x3, zero padding at THAT level's border (z included), one set of weights
//   t  = (bank(a) + up2(bank(a2))) + up4(bank(a4))    nearest: source index k / 2, i / 2, j / 2 and k / 4, i / 4, j / 4
//   t  = relu(conv2(t)); t = relu(conv2(t)); t = relu(conv3(t)); p = convOut(t)      1x1x1: 16 -> 16 (twice), 16 -> 8, 8 -> 1
//
// Unlike the 2D net this one is bound by the matrix pipe (34 560 FLOP a voxel), so the layers stay separate and the activations go
// through HBM (155 bytes of workspace a full-resolution cell).  Six launches:
//   bank3d_conv1_kernel          x -> a, a2, a4.  VALU.  A workgroup owns 4 x 8 x 64 cells (z, y, x); a thread owns one 2x2x2 pooling window:
//                                it computes the 16 channels of its eight cells (weights broadcast from LDS), writes them and their mean; the
//                                eight window means of a 4x4x4 window are added through LDS in one fixed order.
//   bank3d_conv_kernel<false>    Conv3d 16 -> 16 + bias + ReLU at one level: block.0 on a4, a2 and a, block.2 on the two coarser levels.
//   bank3d_conv_kernel<true>     block.2 at full resolution with the epilogue of the 2D net's R = 1 kernel: ReLU, the two coarser results
//                                added in the order above, the four 1x1x1 layers on the accumulator registers; only p is written.
// The convolution is an implicit GEMM on v_mfma_f32_16x16x4_f32 that marches along z.  A workgroup of four waves owns a TH x TW tile of
// (y, x) and a range of z.  LDS holds a ring of four input planes, 16 channels x (TH + 2) rows of pitch P = TW + 2, zero where the level's
// domain ends (a zero ACTIVATION): while plane k is computed from the slots of k - 1, k and k + 1, plane k + 2 is on its way from HBM in
// registers; it is written to the fourth slot after the MFMAs, and one barrier a plane separates the steps.  M = 16 output channels,
// N = 16 consecutive positions q = y * P + x of the flattened plane (the two positions a row that wrap are computed and dropped), K = 4
// input channels of one tap: 108 MFMAs per 16 cells, their 108 A operands in registers for the whole march, B one ds_read_b32 each from
// planes whose stride S = 16 (mod 32) floats keeps the two channels of a 32-lane group on disjoint banks.  A wave owns two groups of 16
// positions (two independent accumulator chains).  Operand maps as in fnx_banknet.hip.
// No atomics.  A cell's value is one fixed-order sum (bias, then dz, dy, dx, the input channels four at a time) that depends neither on
// the batch, nor on the tile, nor on how z was split.  The sample is grid z.  Every index into an activation tensor is 64-bit.
#include "fnx_banknet3d_tile.h"

namespace fnx {
namespace {

__global__ void bank3d_pack_kernel(const float* __restrict__ blob, float* __restrict__ pk) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P3_FLOATS) return;
  float v = 0.f;
  if (i < P3_B1) {
    const int cout = i & 15, k = i >> 4;                      // k = cin * 27 + tap, the blob's own order inside an output channel
    v = blob[B3_W1 + cout * 54 + k];
  } else if (i < P3_WB0) {
    v = blob[B3_B1 + i - P3_B1];
  } else if (i < P3_W2) {
    const bool second = i >= P3_WB2;
    v = bank_pack_conv16(blob, second ? B3_WB2 : B3_WB0, 27, i - (second ? P3_WB2 : P3_WB0));
  } else {
    v = bank_pack_tail(blob, B3_W2, i - P3_W2);
  }
  pk[i] = v;
}

// ---- conv1 and the two poolings ---------------------------------------------------------------------------------------------------------
constexpr int C1_TD = 4, C1_TH = 8, C1_TW = 64;                              // cells of a workgroup: multiples of 4, so no pooling window crosses
constexpr int C1_XD = C1_TD + 2, C1_XH = C1_TH + 2, C1_XW = C1_TW + 2;       // the x tile with its halo
constexpr int C1_XFLOATS = 2 * C1_XD * C1_XH * C1_XW;                        // 7 920
constexpr int C1_WIN = (C1_TD / 2) * (C1_TH / 2) * (C1_TW / 2);              // 256 windows of 2x2x2 = 256 threads
static_assert(C1_WIN == 256 && C1_XFLOATS >= 16 * C1_WIN, "the window means reuse the x tile's LDS");

// x (B, 2, D, H, W) -> a (B, 16, D, H, W), a2 (B, 16, D/2, H/2, W/2), a4 (B, 16, D/4, H/4, W/4).  256 threads.
// grid: (x tiles, y tiles * z tiles, B)
__global__ __launch_bounds__(256) void bank3d_conv1_kernel(const float* __restrict__ pk, const float* __restrict__ x, int D, int H, int W,
                                                           int tiles_y, float* __restrict__ a, float* __restrict__ a2,
                                                           float* __restrict__ a4) {
  __shared__ float lds[C1_XFLOATS];
  __shared__ float lw[P3_WB0];                                  // conv1's weights and bias: every lane reads the same address (a broadcast)
  const int tid = threadIdx.x;
  const int b = blockIdx.z;
  for (int i = tid; i < P3_WB0; i += 256) lw[i] = pk[i];
  const int x0 = blockIdx.x * C1_TW, y0 = (blockIdx.y % tiles_y) * C1_TH, z0 = (blockIdx.y / tiles_y) * C1_TD;
  const size_t HW = (size_t)H * W, DHW = (size_t)D * HW;
  {
    const float* xb = x + (size_t)b * 2 * DHW;
    for (int i = tid; i < C1_XFLOATS; i += 256) {
      const int xx = i % C1_XW, r = i / C1_XW;
      const int yy = r % C1_XH, zz = (r / C1_XH) % C1_XD, c = r / (C1_XH * C1_XD);
      const int gz = z0 - 1 + zz, gy = y0 - 1 + yy, gx = x0 - 1 + xx;
      float v = 0.f;
      if (gz >= 0 && gz < D && gy >= 0 && gy < H && gx >= 0 && gx < W) v = xb[(size_t)c * DHW + (size_t)gz * HW + (size_t)gy * W + gx];
      lds[i] = v;
    }
  }
  __syncthreads();
  // this thread's window: cells (z0 + 2 wz + pz, y0 + 2 wy + py, x0 + 2 wx + px)
  const int wx = tid & 31, wy = (tid >> 5) & 3, wz = tid >> 7;
  const int cz = z0 + 2 * wz, cy = y0 + 2 * wy, cx = x0 + 2 * wx;
  const bool inside = cz < D && cy < H && cx < W;              // D, H, W are even: a window is inside or outside as a whole
  float pool[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) pool[c] = 0.f;
  if (inside) {
    float* ab = a + (size_t)b * 16 * DHW;
    for (int pz = 0; pz < 2; ++pz)
      for (int py = 0; py < 2; ++py) {
        __asm__ volatile("" ::: "memory");                        // the 880 weights are read again per pair of cells, not hoisted into registers
        float acc[2][16];
#pragma unroll
        for (int c = 0; c < 16; ++c) acc[0][c] = acc[1][c] = lw[P3_B1 + c];
        const float* lp = lds + ((2 * wz + pz) * C1_XH + 2 * wy + py) * C1_XW + 2 * wx;
#pragma unroll
        for (int ci = 0; ci < 2; ++ci)
#pragma unroll
          for (int dz = 0; dz < 3; ++dz)
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
              float in[4];
#pragma unroll
              for (int k = 0; k < 4; ++k) in[k] = lp[((ci * C1_XD + dz) * C1_XH + dy) * C1_XW + k];
#pragma unroll
              for (int dx = 0; dx < 3; ++dx) {
                const float* wrow = lw + P3_W1 + (ci * 27 + dz * 9 + dy * 3 + dx) * 16;
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                  acc[0][c] = fmaf(wrow[c], in[dx], acc[0][c]);
                  acc[1][c] = fmaf(wrow[c], in[dx + 1], acc[1][c]);
                }
              }
            }
        const size_t cell = (size_t)(cz + pz) * HW + (size_t)(cy + py) * W + cx;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
          const float v0 = fmaxf(acc[0][c], 0.f), v1 = fmaxf(acc[1][c], 0.f);
          *reinterpret_cast<float2*>(ab + (size_t)c * DHW + cell) = make_float2(v0, v1);        // cx and W are even: 8-byte aligned
          pool[c] += v0;                                                                        // the window's order: z, y, x
          pool[c] += v1;
        }
      }
    const int D2 = D / 2, H2 = H / 2, W2 = W / 2;
    float* a2b = a2 + (size_t)b * 16 * D2 * H2 * W2;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      pool[c] *= 0.125f;
      a2b[(((size_t)c * D2 + cz / 2) * H2 + cy / 2) * W2 + cx / 2] = pool[c];
    }
  }
  __syncthreads();                                             // every thread is done with the x tile
#pragma unroll
  for (int c = 0; c < 16; ++c) lds[c * C1_WIN + tid] = pool[c];
  __syncthreads();
  // the 4x4x4 windows: 1 x 2 x 16 of them and 16 channels = 512 values, two a thread; eight window means in the order z, y, x
  const int D4 = D / 4, H4 = H / 4, W4 = W / 4;
  float* a4b = a4 + (size_t)b * 16 * D4 * H4 * W4;
  for (int i = tid; i < 16 * 32; i += 256) {
    const int qx = i & 15, qy = (i >> 4) & 1, c = i >> 5;
    if (z0 < D && y0 + 4 * qy < H && x0 + 4 * qx < W) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) s += lds[c * C1_WIN + (k >> 2) * 128 + (2 * qy + ((k >> 1) & 1)) * 32 + 2 * qx + (k & 1)];
      a4b[(((size_t)c * D4 + z0 / 4) * H4 + y0 / 4 + qy) * W4 + x0 / 4 + qx] = s * 0.125f;
    }
  }
}

// ---- the 16 -> 16 convolution, marching along z: fnx_banknet3d_tile.h's body under the forward's two epilogues ----------------------------
// in (B, 16, d, h, w) -> out = relu(conv(in) + bias) (B, 16, d, h, w); TAIL: l2, l4 the coarser banks' results, p (B, 1, d, h, w) instead.
template <bool TAIL>
__global__ __launch_bounds__(256) void bank3d_conv_kernel(const float* __restrict__ wpk, const float* __restrict__ bias,
                                                          const float* __restrict__ tail, const float* __restrict__ in, int d, int h, int w,
                                                          int tiles_y, int chunk, float* __restrict__ out, const float* __restrict__ l2,
                                                          const float* __restrict__ l4, float* __restrict__ p) {
  bank3d_conv_body<TAIL ? EPI3_TAIL : EPI3_RELU>(wpk, bias, tail, in, d, h, w, tiles_y, chunk, out, l2, l4, p, nullptr, Bank3dTapeOut{});
}

// conv1 and the five ReLU convolutions of the forward, into the eight tensors they write (the inference workspace, or the tape)
void bank3d_front(int B, int D, int H, int W, const float* pk, const float* x, const Bank3dWs& ws, hipStream_t s) {
  {
    const int ty = (H + C1_TH - 1) / C1_TH, tz = (D + C1_TD - 1) / C1_TD;
    bank3d_conv1_kernel<<<dim3((unsigned)((W + C1_TW - 1) / C1_TW), (unsigned)(ty * tz), (unsigned)B), 256, 0, s>>>(pk, x, D, H, W, ty, ws.a,
                                                                                                                  ws.a2, ws.a4);
  }
  auto conv = [&](int R, bool second, const float* in, float* out) {
    const int d = D / R, h = H / R, w = W / R;
    const Bank3dConvPlan pl = bank3d_conv_plan(B, d, h, w);
    bank3d_conv_kernel<false><<<dim3((unsigned)pl.tiles_x, (unsigned)(pl.tiles_y * pl.chunks), (unsigned)B), 256, 0, s>>>(
        pk + (second ? P3_WB2 : P3_WB0), pk + (second ? P3_BB2 : P3_BB0), nullptr, in, d, h, w, pl.tiles_y, pl.chunk, out, nullptr, nullptr,
        nullptr);
  };
  conv(4, false, ws.a4, ws.h4);
  conv(4, true, ws.h4, ws.b4);
  conv(2, false, ws.a2, ws.h2);
  conv(2, true, ws.h2, ws.b2);
  conv(1, false, ws.a, ws.h);
}

void bank3d_forward(int B, int D, int H, int W, const float* pk, const float* x, float* p, void* wsp, hipStream_t s) {
  const Bank3dWs ws = bank3d_ws_layout(B, D, H, W, wsp);
  ProfScope ps(FNX_PROF_CONV_MFMA16, s);
  bank3d_front(B, D, H, W, pk, x, ws, s);
  const Bank3dConvPlan pl = bank3d_conv_plan(B, D, H, W);
  bank3d_conv_kernel<true><<<dim3((unsigned)pl.tiles_x, (unsigned)(pl.tiles_y * pl.chunks), (unsigned)B), 256, 0, s>>>(
      pk + P3_WB2, pk + P3_BB2, pk + P3_W2, ws.h, D, H, W, pl.tiles_y, pl.chunk, nullptr, ws.b2, ws.b4, p);
}

// the workspace of the net alone and of the whole forward (the flags copy, fnx_fluidnet.h's FluidnetWs with the net's at its end)
size_t bank3d_net_ws(const FnxGrid* g) { return bank3d_ws_layout(g->B, g->D, g->H, g->W, nullptr).bytes; }
size_t bank3d_whole_ws(const FnxGrid* g) { return fluidnet_whole_ws_bytes(g->B, (size_t)g->D * g->H * g->W, bank3d_net_ws(g)); }

}  // namespace

// the net as FluidNet.forward's wrapper runs it (fnx_fluidnet.h)
const Net& banknet3d_net() {
  static const Net net = {3, FNX_NET_BANK3D, bank_status, bank3d_net_ws,
                          [](const FnxGrid* g, const void* packed, const float* x, float* p, int, void* ws, hipStream_t s) {
                            bank3d_forward(g->B, g->D, g->H, g->W, (const float*)packed, x, p, ws, s);
                          }};
  return net;
}

void bank3d_forward_front(int B, int D, int H, int W, const float* pk, const float* x, float* a, float* h, float* a2, float* h2, float* b2,
                          float* a4, float* h4, float* b4, hipStream_t s) {
  bank3d_front(B, D, H, W, pk, x, Bank3dWs{a, h, a2, h2, b2, a4, h4, b4, 0}, s);
}

}  // namespace fnx

extern "C" {

size_t fnx_banknet3d_weight_floats(void) { return fnx::B3_FLOATS; }
size_t fnx_banknet3d_packed_bytes(void) { return (size_t)fnx::P3_FLOATS * sizeof(float); }

int fnx_banknet3d_pack(const float* weights_blob, void* packed, void* stream) {
  if (!weights_blob || !packed) return fnx::set_error(FNX_EINVAL, "%s: null argument", __func__);
  fnx::bank3d_pack_kernel<<<(fnx::P3_FLOATS + 255) / 256, 256, 0, (hipStream_t)stream>>>(weights_blob, (float*)packed);
  return fnx::bank_status();
}

size_t fnx_banknet3d_ws_bytes(const FnxGrid* g, int whole_forward) {
  if (!g || g->B < 1 || g->D < 4 || g->H < 4 || g->W < 4) return 0;
  return whole_forward ? fnx::bank3d_whole_ws(g) : fnx::bank3d_net_ws(g);
}

int fnx_banknet3d_launch_plan(const FnxGrid* g, int level, int plan[6]) {
  if (!g || !plan || (level != 1 && level != 2 && level != 4) || g->B < 1 || g->D < 4 || g->H < 4 || g->W < 4 || g->D % 4 || g->H % 4 || g->W % 4)
    return fnx::set_error(FNX_EINVAL, "%s: a grid with D, H and W positive multiples of 4 and a level of 1, 2 or 4", __func__);
  const fnx::Bank3dConvPlan pl = fnx::bank3d_conv_plan(g->B, g->D / level, g->H / level, g->W / level);
  plan[0] = pl.tiles_x; plan[1] = pl.tiles_y; plan[2] = pl.chunks; plan[3] = pl.chunk; plan[4] = fnx::CV_TH; plan[5] = fnx::CV_TW;
  return FNX_OK;
}

int fnx_banknet3d_forward(const FnxGrid* g, const void* packed, const float* x, float* p, int precision_mode, void* ws, size_t ws_bytes,
                          void* stream) {
  if (int rc = fnx::check_bank_call(__func__, 3, g, packed && x && p && ws, precision_mode, fnx::bank3d_net_ws, ws_bytes)) return rc;
  fnx::bank3d_forward(g->B, g->D, g->H, g->W, (const float*)packed, x, p, ws, (hipStream_t)stream);
  return fnx::bank_status();
}

// FluidNet.forward around the net, as fnx_fluidnet_bank_forward, on three velocity components
int fnx_fluidnet_bank3d_forward(const FnxGrid* g, const void* packed, const float* input, float thr, float* p_out, float* U_out,
                                int precision_mode, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = fnx::check_bank_call(__func__, 3, g, packed && input && p_out && U_out && ws, precision_mode, fnx::bank3d_whole_ws, ws_bytes))
    return rc;
  return fnx::fluidnet_whole_forward(fnx::banknet3d_net(), g, packed, input, thr, p_out, U_out, precision_mode, ws, stream);
}

}  // extern "C"
