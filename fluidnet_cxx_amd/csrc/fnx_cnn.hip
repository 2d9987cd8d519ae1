// MultiScale pressure-net forward (lib/multi_scale_net.py:118-127) for gfx950; FluidNet.forward around it: fnx_fluidnet.hip.
//
// The 32/64/128-channel 3x3(x3) layers (95 % of the FLOPs) run as implicit GEMM on the matrix cores in exact fp32
// (conv3_mfma_kernel, 32x32x2 MFMA); the 5x5(x5) layers 3->32 and 32->8 on the 16x16x4 MFMA (conv5_mfma16_kernel, the 32->8
// layer with the final 1x1 in its epilogue); the remaining thin layers (2->32 and 32->1 3x3) are bandwidth-shaped and use direct
// kernels (conv_direct_kernel, conv3_to1_kernel).  Which kernel family runs a layer and where its weights sit: PLAN.
#include "fnx_cnn.h"
#include <assert.h>
#include <stdlib.h>
#include <type_traits>
#include "fnx_fluidnet.h"
#include "fnx_kernels.h"
#include "../../include/fluidnet_hip.h"

namespace fnx {
int launch_status(bool is3d) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? FNX_OK : set_error(FNX_EHIP, "HIP error in a CNN launch: %s%s", hipGetErrorString(e),
                                              is3d ? " (a grid the net cannot take -- D a multiple of 4?)" : "");
}


namespace {

constexpr int co_tile(int cout) { return cout >= 16 ? 16 : cout; }
constexpr int pad_to(int v, int m) { return (v + m - 1) / m * m; }

// ---------------------------------------------------------------------------------------------------
// The plan of a layer: the kernel family that runs it and where each of its images sits in the packed buffer.  scalenet_pack,
// launch_conv and the towers' tail fusion take both from PLAN and derive neither.
// ---------------------------------------------------------------------------------------------------
enum class Family {
  DIRECT,   // conv_direct_kernel, packed [Cout/CO_T][Cin][taps][CO_T]: the 2->32 3x3(x3) layer; the final 1x1 only runs fused (PAIR)
  TO1,      // conv3_to1_kernel: 3x3(x3) to one channel, the half- and quarter-resolution towers' last layers
  PAIR,     // conv5_mfma16_kernel PAIR: 5x5(x5) 32->8 with the next layer (1x1, 8->1) in its epilogue
  KPACK,    // conv5_mfma16_kernel with K packed over (tap, channel): 5x5(x5) 3->32
  MFMA,     // 3x3(x3), Cin % 16 == 0, Cout % 32 == 0: bf16 pieces, F(4x4), F(2x2) or implicit GEMM (launch_conv)
};
struct LayerPlan { Family fam; MfmaImages im; };   // im: the float offsets into the packed buffer (fnx_cnn.h)
struct NetPlan { LayerPlan layer[N_LAYERS]; };

constexpr Family family_of(const ConvLayer& L) {
  if (is_mfma_layer(L.cin, L.cout, L.k)) return Family::MFMA;
  if (L.k == 3 && L.cout == 1 && L.cin % 4 == 0) return Family::TO1;
  if (L.k == 5 && L.cout == 8 && L.cin % 8 == 0) return Family::PAIR;
  if (L.k == 5 && L.cin == 3 && L.cout > 16 && L.cout <= 32) return Family::KPACK;
  return Family::DIRECT;
}
// what the launchers assume of the table: a PAIR layer is followed by the 1x1 8->1 (no ReLU) it fuses, and a DIRECT layer that
// launches on its own is 3x3(x3) with whole 16-channel output groups
constexpr bool plan_ok() {
  for (int l = 0; l < N_LAYERS; ++l) {
    const ConvLayer& L = LAYERS[l];
    if (family_of(L) == Family::PAIR &&
        !(l + 1 < N_LAYERS && LAYERS[l + 1].k == 1 && LAYERS[l + 1].cin == 8 && LAYERS[l + 1].cout == 1 && !LAYERS[l + 1].relu))
      return false;
    if (family_of(L) == Family::DIRECT && !(L.k == 3 && L.cout % 16 == 0) && !(l > 0 && family_of(LAYERS[l - 1]) == Family::PAIR))
      return false;
  }
  return true;
}
static_assert(plan_ok(), "LAYERS holds a layer no launcher takes");

constexpr NetPlan make_plan(bool is3d) {
  NetPlan P{};
  size_t off = 0;
  for (int l = 0; l < N_LAYERS; ++l) {
    const ConvLayer& L = LAYERS[l];
    LayerPlan& p = P.layer[l];
    p.fam = family_of(L);
    if (p.fam == Family::MFMA) {
      p.im = mfma_images(is3d, L.cin, L.cout, off);
    } else {
      const size_t kd = is3d ? L.k : 1;
      p.im.taps = off;
      switch (p.fam) {
        case Family::PAIR: off += kd * 30 * pad_to(L.cin, 4) * 16; break;    // [dz][r][wx 0..5][Cin padded to 4][16]
        // [taps][Cin padded to 4][Cout padded to 16], of which the packed-K image [dz][(25 Cin) padded to 4][Cout padded to 32] uses the front
        case Family::KPACK: off += (size_t)layer_taps(L, is3d) * pad_to(L.cin, 4) * pad_to(L.cout, 16); break;
        default: off += layer_weight_floats(L, is3d);
      }
      p.im.bias = off;
      p.im.end = al64(off + L.cout);
    }
    off = p.im.end;
  }
  return P;
}
constexpr NetPlan PLAN[2] = {make_plan(false), make_plan(true)};
inline const LayerPlan* plan(bool is3d) { return PLAN[is3d].layer; }
// packed images outlive a build (callers size and keep them): the offsets are pinned to what they have been since the plan exists
constexpr bool plan_is(const NetPlan& P, const size_t (&taps)[N_LAYERS], const size_t (&bias)[N_LAYERS]) {
  for (int l = 0; l < N_LAYERS; ++l)
    if (P.layer[l].im.taps != taps[l] || P.layer[l].im.bias != bias[l]) return false;
  return true;
}
constexpr bool images_are(const MfmaImages& im, size_t wino2, size_t wino3, size_t wbf, size_t wino4) {
  return im.wide && im.wino2 == wino2 && im.wino3 == wino3 && im.wbf == wbf && im.wino4 == wino4;
}
static_assert(plan_is(PLAN[0], {0, 640, 152256, 236288, 236608, 239872, 391488, 997824, 1604096, 1688128, 1688448, 1691712, 1843328, 2449664,
                                3055936, 3139968, 3155392},
                      {576, 152192, 236224, 236576, 239808, 391424, 997696, 1604032, 1688064, 1688416, 1691648, 1843264, 2449536, 3055872,
                       3139904, 3155328, 3155400}), "the 2D packed image moved");
static_assert(plan_is(PLAN[1], {0, 1792, 456512, 708480, 709376, 725440, 1180160, 2998912, 4817600, 5069568, 5070464, 5086528, 5541248, 7360000,
                                9178688, 9430656, 9507520},
                      {1728, 456448, 708416, 709344, 725376, 1180096, 2998784, 4817536, 5069504, 5070432, 5086464, 5541184, 7359872, 9178624,
                       9430592, 9507456, 9507528}), "the 3D packed image moved");
static_assert(images_are(PLAN[0].layer[6].im, 465216, 596288, 727360, 923968) && images_are(PLAN[1].layer[6].im, 1401344, 1794560, 2187776, 2777600) &&
              !PLAN[0].layer[8].im.wide && PLAN[0].layer[8].im.wino3 == 1655296 && PLAN[1].layer[8].im.wino3 == 4971200,
              "an MFMA layer's images moved within it");

// blob: (Cout,Cin,taps) -> packed [taps][Cin][Cout]   (implicit-GEMM layers: the A operand of the MFMA reads 32
// consecutive output channels per lane half)
__global__ void pack_layer_mfma_kernel(const float* __restrict__ w, const float* __restrict__ bias,
                                       float* __restrict__ pw, float* __restrict__ pb, int cin, int cout, int taps) {
  const int n = cin * cout * taps;
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) {
    const int co = q / (cin * taps);
    const int r = q - co * cin * taps;
    const int ci = r / taps, t = r - ci * taps;
    pw[((size_t)t * cin + ci) * cout + co] = w[q];
  }
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < cout; q += gridDim.x * blockDim.x) pb[q] = bias[q];
}

// Cin of 2 or 3 (the first layer of a scale): the MFMA K runs over (tap, channel) pairs of a z plane, k = tap * Cin + channel,
// padded to a multiple of 4 -- 13 / 19 K-groups of four per plane instead of 25 with one or two empty channels each
// (Family::KPACK: conv5_mfma16_kernel<4, 2, ., false, KPC = Cin>, Cout padded to 32).
// blob: (Cout,Cin 2|3,taps 5x5[x5]) -> packed [dz][k = (r*5+s)*Cin + ci, padded to 4][Cout padded to 32], zeros in the padding
__global__ void pack_layer_kpack_kernel(const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ pw,
                                        float* __restrict__ pb, int cin, int cout, int kd, int cout_pad) {
  const int krows = (25 * cin + 3) / 4 * 4;
  const int n = kd * krows * cout_pad;
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) {
    const int co = q % cout_pad, r1 = q / cout_pad;
    const int k = r1 % krows, dz = r1 / krows;
    const int tap = k / cin, ci = k - tap * cin;
    pw[q] = (co < cout && tap < 25) ? w[((size_t)co * cin + ci) * (kd * 25) + dz * 25 + tap] : 0.f;
  }
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < cout; q += gridDim.x * blockDim.x) pb[q] = bias[q];
}

// blob: (Cout<=8,Cin,taps 5x5[x5]) -> packed [dz][r][wx 0..5][Cin padded to 4][dx*8 + cout]: the weight of tap (r, wx-dx)
// for output pixel dx of a pair, zero where wx-dx is not one of the 5 taps
__global__ void pack_layer_pair_kernel(const float* __restrict__ w, const float* __restrict__ bias,
                                       float* __restrict__ pw, float* __restrict__ pb, int cin, int cout, int kd,
                                       int cin_pad) {
  const int n = kd * 30 * cin_pad * 16;
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) {
    const int m = q % 16, r1 = q / 16;
    const int ci = r1 % cin_pad, r2 = r1 / cin_pad;
    const int wx = r2 % 6, r3 = r2 / 6;
    const int r = r3 % 5, dz = r3 / 5;
    const int dx = m >> 3, co = m & 7, sx = wx - dx;
    const int taps = kd * 25;
    pw[q] = (co < cout && ci < cin && sx >= 0 && sx < 5) ? w[((size_t)co * cin + ci) * taps + (dz * 5 + r) * 5 + sx] : 0.f;
  }
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < cout; q += gridDim.x * blockDim.x) pb[q] = bias[q];
}

// blob: (Cout,Cin,taps) -> packed [Cout/CO_T][Cin][taps][CO_T]
__global__ void pack_layer_kernel(const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ pw,
                                  float* __restrict__ pb, int cin, int cout, int taps, int cot) {
  const int n = cin * cout * taps;
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) {
    const int co = q / (cin * taps);
    const int r = q - co * cin * taps;
    const int ci = r / taps, t = r - ci * taps;
    const int grp = co / cot, tt = co - grp * cot;
    pw[(((size_t)grp * cin + ci) * taps + t) * cot + tt] = w[q];
  }
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < cout; q += gridDim.x * blockDim.x) pb[q] = bias[q];
}

struct ConvArgs {
  const float* x; float* y; const float* w; const float* bias;
  int B, cin, cout, D, H, W, relu, groups;
  // Optional fused tail (conv5_mfma16_kernel PAIR only): a 1x1(x1) convolution cout -> 1 applied in the epilogue -- y then has ONE
  // channel: y = tail_b[0] + sum_c tail_w[c] * act(conv)[c].  multi_scale_net.py:116: the net's last 5x5 layer (32 -> 8) and its
  // final 1x1 (8 -> 1); the 8-channel tensor between them is never written.
  const float* tail_w; const float* tail_b;
};

// Thin layers (the 2->32 3x3(x3) layer: KS 3, CO_T 16): direct convolution.  A thread owns a vertical strip of RY output pixels x CO_T
// output channels, so each input row it loads (coalesced along x across the wave) feeds up to KS output rows:
// (RY+KS-1)*KS loads per RY*KS*KS taps instead of one load per tap.
template <int KS, int CO_T, bool IS3D, int RY>
__global__ __launch_bounds__(256) void conv_direct_kernel(ConvArgs a) {
  constexpr int KD = IS3D ? KS : 1, PAD = KS / 2, PD = IS3D ? PAD : 0, TAPS = KD * KS * KS;
  const int i = blockIdx.x * 64 + threadIdx.x, j0 = (blockIdx.y * 4 + threadIdx.y) * RY;
  int z = blockIdx.z;
  const int k = z % a.D; z /= a.D;
  const int grp = z % a.groups; const int b = z / a.groups;
  if (i >= a.W || j0 >= a.H) return;
  const size_t plane = (size_t)a.H * a.W, vol = plane * a.D;
  float acc[RY][CO_T];
#pragma unroll
  for (int t = 0; t < CO_T; ++t) {
    const float bv = a.bias[grp * CO_T + t];
#pragma unroll
    for (int ry = 0; ry < RY; ++ry) acc[ry][t] = bv;
  }
  const float* wg = a.w + (size_t)grp * a.cin * TAPS * CO_T;
  const float* xb = a.x + (size_t)b * a.cin * vol;
  for (int ci = 0; ci < a.cin; ++ci) {
    const float* xc = xb + (size_t)ci * vol;
    const float* wc = wg + (size_t)ci * TAPS * CO_T;
#pragma unroll
    for (int dz = 0; dz < KD; ++dz) {
      const int zz = k + dz - PD;
      const bool zin = (zz >= 0) & (zz < a.D);
#pragma unroll
      for (int row = 0; row < RY + KS - 1; ++row) {        // input row j0 - PAD + row
        const int yy = j0 + row - PAD;
        const bool yin = zin & (yy >= 0) & (yy < a.H);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const int xx = i + s - PAD;
          const bool in = yin & (xx >= 0) & (xx < a.W);
          const float v = in ? xc[(size_t)(zin ? zz : 0) * plane + (size_t)(yin ? yy : 0) * a.W + (in ? xx : 0)] : 0.f;
#pragma unroll
          for (int ry = 0; ry < RY; ++ry) {
            const int r = row - ry;                        // tap row for output row ry
            if (r >= 0 && r < KS) {
              const float* wt = wc + ((dz * KS + r) * KS + s) * CO_T;
#pragma unroll
              for (int t = 0; t < CO_T; ++t) acc[ry][t] = fmaf(v, wt[t], acc[ry][t]);
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int ry = 0; ry < RY; ++ry) {
    if (j0 + ry >= a.H) break;
    float* yb = a.y + ((size_t)b * a.cout + grp * CO_T) * vol + (size_t)k * plane + (size_t)(j0 + ry) * a.W + i;
#pragma unroll
    for (int t = 0; t < CO_T; ++t) {
      float v = acc[ry][t];
      if (a.relu) v = fmaxf(v, 0.f);
      yb[(size_t)t * vol] = v;
    }
  }
}

// Family::DIRECT (3x3(x3), Cout a multiple of 16: plan_ok), and the MFMA layers beyond what the MFMA kernels can address
void launch_conv_direct(const ConvArgs& a, bool is3d, hipStream_t s) {
  constexpr int RY = 4;
  const dim3 grid((a.W + 63) / 64, (a.H + 4 * RY - 1) / (4 * RY), a.B * a.groups * a.D), block(64, 4);
  if (is3d) conv_direct_kernel<3, 16, true, RY><<<grid, block, 0, s>>>(a);
  else conv_direct_kernel<3, 16, false, RY><<<grid, block, 0, s>>>(a);
}

// 3x3(x3) convolution to ONE output channel (the towers' last layers, 32 -> 1, at half and quarter resolution).  In the strip
// kernel above a thread walks all Cin channels of its 4 output rows alone: 4 chains of 9 Cin dependent FMAs on launches of a few
// dozen workgroups (256^2: 25.6 us for 37 MFLOP).  Here the block's four waves split the INPUT CHANNELS: wave q accumulates
// channels q, q + 4, ... of the block's 4 output rows (each input row it loads feeds up to 3 output rows), the partial sums meet in
// LDS and wave r finishes output row r: sums of the four partials in wave order + bias.  4x the workgroups, chains a quarter as long.
template <bool IS3D>
__global__ __launch_bounds__(256) void conv3_to1_kernel(ConvArgs a) {
  constexpr int KS = 3, KD = IS3D ? KS : 1, PAD = 1, PD = IS3D ? 1 : 0, TAPS = KD * KS * KS, RY = 4;
  __shared__ float part[4][RY][64];
  const int lane = threadIdx.x, q = threadIdx.y;
  const int i = blockIdx.x * 64 + lane, j0 = blockIdx.y * RY;
  int z = blockIdx.z;
  const int k = z % a.D; const int b = z / a.D;
  const size_t plane = (size_t)a.H * a.W, vol = plane * a.D;
  float acc[RY] = {0.f, 0.f, 0.f, 0.f};
  const float* xb = a.x + (size_t)b * a.cin * vol;
  for (int ci = q; ci < a.cin; ci += 4) {
    const float* xc = xb + (size_t)ci * vol;
    const float* wc = a.w + (size_t)ci * TAPS;              // packed [1][Cin][taps][1]
#pragma unroll
    for (int dz = 0; dz < KD; ++dz) {
      const int zz = k + dz - PD;
      const bool zin = (zz >= 0) & (zz < a.D);
#pragma unroll
      for (int row = 0; row < RY + KS - 1; ++row) {
        const int yy = j0 + row - PAD;
        const bool yin = zin & (yy >= 0) & (yy < a.H);
#pragma unroll
        for (int t = 0; t < KS; ++t) {
          const int xx = i + t - PAD;
          const bool in = yin & (xx >= 0) & (xx < a.W);
          const float v = in ? xc[(size_t)(zin ? zz : 0) * plane + (size_t)(yin ? yy : 0) * a.W + (in ? xx : 0)] : 0.f;
#pragma unroll
          for (int ry = 0; ry < RY; ++ry) {
            const int r = row - ry;
            if (r >= 0 && r < KS) acc[ry] = fmaf(v, wc[(dz * KS + r) * KS + t], acc[ry]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int ry = 0; ry < RY; ++ry) part[q][ry][lane] = acc[ry];
  __syncthreads();
  const int j = j0 + q;                                     // wave q finishes output row q
  if (i < a.W && j < a.H) {
    float v = ((part[0][q][lane] + part[1][q][lane]) + part[2][q][lane]) + part[3][q][lane];
    v += a.bias[0];
    if (a.relu) v = fmaxf(v, 0.f);
    a.y[(size_t)b * vol + (size_t)k * plane + (size_t)j * a.W + i] = v;
  }
}

// ---------------------------------------------------------------------------------------------------
// Implicit-GEMM 3x3(x3) convolution on the matrix cores, exact fp32 (v_mfma_f32_32x32x2_f32).
//   D[cout 32][pixel 32] += A[cout][k] * B[k][pixel],  k = two consecutive input channels of one tap
//   A: lane -> W[tap][c + (lane>>5)][cout0 + (lane&31)]      (one coalesced 256-B global/L1 read per wave)
//   B: lane -> X[c + (lane>>5)][y + r - 1][x0 + (lane&31) + s - 1]  from the LDS halo tile (conflict-free rows)
//   D: lane holds pixel (lane&31) and 16 output channels -> every store is a 128-B row segment
// Workgroup = 4 waves stacked in y; wave tile = 32 px x PR rows x (CB*32) output channels (PR*CB accumulators of
// 16 VGPRs).  Input channels are staged through LDS 8 at a time ((4PR+2) x 34 halo rows).  3D: the z taps are an
// outer loop over the three input planes.
// ---------------------------------------------------------------------------------------------------
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr int MF_CHUNK = 8;       // input channels per LDS stage
constexpr int MF_COLS = 34;       // 32 + halo

// CH = input channels per LDS stage; WPS = waves per SIMD the register budget is sized for (2: 256 VGPRs, 3: 168)
typedef __amdgpu_buffer_rsrc_t BufRsrcC;
__device__ __forceinline__ BufRsrcC make_rsrc_c(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}
// 16 bytes per lane global -> LDS (buffer_load_dwordx4 ... lds: the wave's 1 KiB lands at `dst`, wave-uniform).  In a __device__
// function of its own: called from a __global__ template directly, the 16-byte form fails the builtin's size check in the HOST
// pass (no gfx950 there), silently, and the kernel's host stub is then never emitted (undefined symbol at load time).
typedef __attribute__((address_space(3))) float* LdsF;
__device__ __forceinline__ void dma4_to_lds(const BufRsrcC r, LdsF dst, unsigned voff) {      // 4 bytes per lane: 64 consecutive floats at `dst`
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)dst, 4, voff, 0, 0, 0);
}
__device__ __forceinline__ void dma16_to_lds(const BufRsrcC r, LdsF dst, unsigned voff, unsigned soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)dst, 16, voff, soff, 0, 0);
}

template <int CB, int PR, bool IS3D, int CH = MF_CHUNK, int WPS = 2>
__global__ __launch_bounds__(256, WPS) void conv3_mfma_kernel(ConvArgs a) {
  constexpr int ROWS = 4 * PR + 2;
  constexpr int KD = IS3D ? 3 : 1;
  constexpr int RW = CB * 32;                    // output channels (floats) per weight row
  constexpr int WROWS = 9 * CH;            // (tap, cin) rows per stage
  constexpr int LPR = RW / 4;                    // lanes per row at 16 B per lane
  constexpr int RPI = 64 / LPR;                  // rows per wave-wide LDS DMA instruction
  constexpr int NWI = (WROWS + RPI - 1) / RPI;   // wave-instructions per stage
  __shared__ __attribute__((aligned(16))) float tile2[2][CH * ROWS * MF_COLS];     // halo tile, double-buffered
  // weights of the stage, [tap][cin][cout], double-buffered in two SEPARATE arrays: the compiler then knows that the DMA
  // into one cannot alias the reads of the other and does not drain vmcnt (the next stage's loads, just issued) in
  // front of the MFMAs
  __shared__ __attribute__((aligned(16))) float wbuf0[NWI * 256];
  __shared__ __attribute__((aligned(16))) float wbuf1[NWI * 256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const int x0 = blockIdx.x * 32, y0 = blockIdx.y * (4 * PR);
  int zb = blockIdx.z;
  const int ngrp = a.cout / (CB * 32);
  const int grp = zb % ngrp; zb /= ngrp;
  const int z = zb % a.D; const int b = zb / a.D;
  const int cout0 = grp * CB * 32;
  const size_t plane = (size_t)a.H * a.W, vol = plane * a.D;

  f32x16 acc[PR][CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float bv = a.bias[cout0 + cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * half];
#pragma unroll
      for (int pr = 0; pr < PR; ++pr) acc[pr][cb][r] = bv;
    }
  }

  const float* xb = a.x + (size_t)b * a.cin * vol;
  // Per-thread staging slots: element idx = threadIdx.x + 256*t of the [CH][ROWS][34] halo tile.  The global
  // offset (relative to the chunk's first channel and the z plane) and the in-image predicate never change, so they
  // are computed once; each stage is then NLD independent loads issued back to back (clamped address + select).
  constexpr int NEL = CH * ROWS * MF_COLS;
  constexpr int NLD = (NEL + 255) / 256;
  // Loads go through a buffer resource spanning the stage's CH channel volumes: an out-of-image element gets an
  // out-of-range offset and the hardware returns 0 -- no select between the load and the LDS store (the compiler hoists
  // such a select to the load and drains vmcnt there, in front of the MFMAs the load is supposed to hide under).
  unsigned uoff[NLD];
#pragma unroll
  for (int t = 0; t < NLD; ++t) {
    const int idx = threadIdx.x + 256 * t;
    const int cc = idx / (ROWS * MF_COLS);
    const int rem = idx - cc * ROWS * MF_COLS;
    const int row = rem / MF_COLS, col = rem - row * MF_COLS;
    const int gx = x0 - 1 + col, gy = y0 - 1 + row;
    const bool ok = (idx < NEL) & (gx >= 0) & (gx < a.W) & (gy >= 0) & (gy < a.H);
    uoff[t] = ok ? (unsigned)(((size_t)cc * vol + (size_t)gy * a.W + gx) * 4) : 0xfffffff0u;   // vol*CH*4 < 2^32 is checked by the host
  }
  const unsigned stage_bytes = (unsigned)((size_t)CH * vol * 4 - 1) + 1u;
  float stage[NLD];
  auto prefetch = [&](int dz, int c0) {
    const int zz = IS3D ? z + dz - 1 : 0;
    // (the plane offset is folded into the base; the range then ends zz planes late, inside the next channel or the
    // allocation's tail, never beyond what an in-image offset of this stage can reach)
    const BufRsrcC r = make_rsrc_c(xb + (size_t)c0 * vol + (size_t)zz * plane, stage_bytes - (unsigned)((size_t)zz * plane * 4));
#pragma unroll
    for (int t = 0; t < NLD; ++t) stage[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, uoff[t], 0, 0));
  };
  // Weights of one stage go global -> LDS directly (buffer_load_dwordx4 ... lds: 1 KiB per wave-instruction, no VGPRs),
  // one stage ahead of their use; the A operand is then a conflict-free ds_read_b32.  (A buffer load, not global_load_lds:
  // behind the FLAT-encoded DMA the compiler turns every later wait into a wait for everything -- the operand reads of the
  // next MFMA group, just issued, included; docs/history/r05_wino3_pipeline.md.)  The lane's part of the offset is fixed,
  // the stage's part is scalar: no address arithmetic on the vector ALU per stage.
  const BufRsrcC wrs = make_rsrc_c(a.w, 0x7ffffff0u);
  constexpr int NWQ = (NWI + 3) / 4;
  unsigned wvoff[NWQ];
#pragma unroll
  for (int q = 0; q < NWQ; ++q) {
    int row = (wave + 4 * q) * RPI + lane / LPR;
    if (row > WROWS - 1) row = WROWS - 1;               // tail lanes re-read the last row (their LDS slots are never used)
    const int tap = row / CH, ci = row - tap * CH;
    wvoff[q] = (unsigned)(((size_t)tap * a.cin + ci) * a.cout + cout0 + (lane % LPR) * 4) * 4u;
  }
  auto stage_weights = [&](int dz, int c0, float* wdst) {
    const unsigned soff = (unsigned)(((size_t)dz * 9 * a.cin + c0) * a.cout) * 4u;
#pragma unroll
    for (int q = 0; q < NWQ; ++q) {
      const int wi = wave + 4 * q;                      // wave-uniform
      if (wi < NWI) dma16_to_lds(wrs, (LdsF)&wdst[0] + wi * 256, wvoff[q], soff);
    }
  };
  // iteration space: (dz, c0) pairs with an in-range z plane
  const int nchunk = a.cin / CH;
  int dz_lo = 0, dz_hi = KD;
  if (IS3D) { if (z == 0) dz_lo = 1; if (z == a.D - 1) dz_hi = KD - 1; }
  const int niter = (dz_hi - dz_lo) * nchunk;
  if (niter > 0) { prefetch(dz_lo, 0); stage_weights(dz_lo, 0, wbuf0); }
  auto stage_body = [&](int it, float* wcur, float* wnext) __attribute__((always_inline)) {
    // Both LDS images are double-buffered: buffer (it&1) was last read in iteration it-2 and every wave has passed
    // the barrier of iteration it-1 since, so it can be overwritten without a barrier in front -> one barrier per stage.
    float* tile = tile2[it & 1];
#pragma unroll
    for (int t = 0; t < NLD; ++t)
      if (threadIdx.x + 256 * t < NEL) tile[threadIdx.x + 256 * t] = stage[t];
    __syncthreads();                                   // tile stores + the stage's weight DMA (vmcnt(0)) visible to all
    if (it + 1 < niter) {                              // both in flight during the MFMAs
      prefetch(dz_lo + (it + 1) / nchunk, ((it + 1) % nchunk) * CH);
      stage_weights(dz_lo + (it + 1) / nchunk, ((it + 1) % nchunk) * CH, wnext);
    }
    {
      // Operand pipeline: the A/B values of group g+1 (one tap x 2 channels: CB + PR LDS values) are read while the
      // PR*CB MFMAs of group g issue, so no MFMA waits on an LDS round trip (left to itself the scheduler parks each
      // ds_read right in front of its first use).
      const float* wl = &wcur[l31 + half * RW];
      const float* tl = &tile[half * ROWS * MF_COLS + (wave * PR) * MF_COLS + l31];
      constexpr int NCP = CH / 2, NG = 9 * NCP;
      float av[2][CB], bv[2][PR];
      auto load_group = [&](int g, float (&A)[CB], float (&B)[PR]) __attribute__((always_inline)) {
        const int tap = g / NCP, cp = (g % NCP) * 2;
        const int r = tap / 3, sx = tap - 3 * r;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) A[cb] = wl[(tap * CH + cp) * RW + cb * 32];
#pragma unroll
        for (int pr = 0; pr < PR; ++pr) B[pr] = tl[cp * ROWS * MF_COLS + (pr + r) * MF_COLS + sx];
      };
      load_group(0, av[0], bv[0]);
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        if (g + 1 < NG) load_group(g + 1, av[(g + 1) & 1], bv[(g + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int pr = 0; pr < PR; ++pr)
#pragma unroll
          for (int cb = 0; cb < CB; ++cb)
            acc[pr][cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[g & 1][cb], bv[g & 1][pr], acc[pr][cb], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };
  for (int it = 0; it < niter; it += 2) {                // niter is even: Cin is a multiple of 2*CH
    stage_body(it, wbuf0, wbuf1);
    stage_body(it + 1, wbuf1, wbuf0);
  }
  const int x = x0 + l31;
  if (x < a.W) {
#pragma unroll
    for (int pr = 0; pr < PR; ++pr) {
      const int y = y0 + wave * PR + pr;
      if (y >= a.H) continue;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int co = cout0 + cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          float v = acc[pr][cb][r];
          if (a.relu) v = fmaxf(v, 0.f);
          a.y[((size_t)b * a.cout + co) * vol + (size_t)z * plane + (size_t)y * a.W + x] = v;
        }
      }
    }
  }
}

#include "fnx_cnn_wino3.h"
#include "fnx_cnn_bf16x6.h"
#include "fnx_cnn_wino4.h"
#include "fnx_cnn_mfma16.h"

// Family::PAIR (Cout 8, the 1x1 tail in the epilogue) or Family::KPACK (Cin 3)
void launch_conv_mfma16(const ConvArgs& a, bool is3d, bool pair, hipStream_t s) {
  const dim3 grid((a.W + 63) / 64, (a.H + 7) / 8, a.B * a.D);
  const int cin_pad = pad_to(a.cin, 4);
  if (pair) {
    if (is3d) conv5_mfma16_kernel<4, 1, true, true><<<grid, 256, 0, s>>>(a, cin_pad);
    else conv5_mfma16_kernel<4, 1, false, true><<<grid, 256, 0, s>>>(a, cin_pad);
  } else if (is3d) conv5_mfma16_kernel<4, 2, true, false, 3><<<grid, 256, 0, s>>>(a, cin_pad);
  else conv5_mfma16_kernel<4, 2, false, false, 3><<<grid, 256, 0, s>>>(a, cin_pad);
}

template <int CB, int PR, int CH = MF_CHUNK, int WPS = 2>
void launch_conv_mfma_t(const ConvArgs& a, bool is3d, hipStream_t s) {
  const dim3 grid((a.W + 31) / 32, (a.H + 4 * PR - 1) / (4 * PR), a.B * a.D * (a.cout / (CB * 32)));
  if (is3d) conv3_mfma_kernel<CB, PR, true, CH, WPS><<<grid, 256, 0, s>>>(a);
  else conv3_mfma_kernel<CB, PR, false, CH, WPS><<<grid, 256, 0, s>>>(a);
}

void launch_conv_mfma(const ConvArgs& a, bool is3d, hipStream_t s) {
  // small images (the quarter-resolution tower): shorter tiles (16 -> 8 -> 4 rows per block) until the launch has a
  // block for every CU slot.  (Measured and not kept: 128 output channels per wave; 8-row tiles with 4-channel stages at
  // 3 waves/SIMD, 2.5 % slower.)
  const int ngrp = a.cout / (a.cout % 64 == 0 ? 64 : 32);
  auto blocks = [&](int rows) { return (long)((a.W + 31) / 32) * ((a.H + rows - 1) / rows) * a.B * a.D * ngrp; };
  const int pr = blocks(16) >= 512 ? 4 : (blocks(8) >= 512 ? 2 : 1);
  if (a.cout % 64 == 0) {
    if (pr == 4) launch_conv_mfma_t<2, 4>(a, is3d, s); else if (pr == 2) launch_conv_mfma_t<2, 2>(a, is3d, s); else launch_conv_mfma_t<2, 1>(a, is3d, s);
  } else {
    if (pr == 4) launch_conv_mfma_t<1, 4>(a, is3d, s); else if (pr == 2) launch_conv_mfma_t<1, 2>(a, is3d, s); else launch_conv_mfma_t<1, 1>(a, is3d, s);
  }
}

// Winograd F(2x2,3x3) for the 3x3(x3) MFMA layers, when the launch fills the chip (one persistent workgroup per CU slot);
// false: nothing launched (small grid), the caller uses the direct kernel
bool launch_conv_wino(const ConvArgs& a, bool is3d, const float* w3, hipStream_t s) {
  if (a.cin % (4 * W3C) != 0 || a.cout % 32 != 0) return false;
  if (a.D != 1 && !is3d) return false;
  if ((size_t)16 * a.D * a.H * a.W * 4 >= 0xfffffff0u) return false;   // the epilogue's 32-bit offsets span a wave's 16 output channels
  // 64 output channels per workgroup where Cout allows it; 8-wave workgroups (two pixel groups share a stage's weights)
  // when the launch is large enough (measured at 1024^2: 64->32 297 -> 274 us against 4-wave workgroups)
  const int ncg = a.cout % 64 == 0 ? 2 : 1;
  int npg = 2 / ncg;
  if (ncg == 2 && (long)((a.W + 31) / 32) * ((a.H + 7) / 8) * a.B * a.D * (a.cout / 64) >= 512) npg = 2;   // 8 waves
  if (ncg == 1) npg = 2;
  assert(wino3_rw(a.cout) == 32 * ncg);
  const int ntx = (a.W + 31) / 32, nty = (a.H + 4 * npg - 1) / (4 * npg);
  const long nt = (long)ntx * nty * a.B * a.D * (a.cout / (32 * ncg));
  const int slots = cu_count() * (ncg * npg == 4 ? 1 : 2);      // 8-wave workgroups fill a CU's registers; two 4-wave ones fit
  if (nt < (npg * ncg == 4 ? 512 : 1024) || nt > 0x7fffffffl) return false;
  const int nwg = (int)(nt < slots ? nt : slots);
  if (is3d) {
    if (ncg == 2 && npg == 2) conv3_wino3_kernel<2, 2, true><<<nwg, 512, 0, s>>>(a, w3, ntx, nty, (int)nt);
    else if (ncg == 2) conv3_wino3_kernel<2, 1, true><<<nwg, 256, 0, s>>>(a, w3, ntx, nty, (int)nt);
    else conv3_wino3_kernel<1, 2, true><<<nwg, 256, 0, s>>>(a, w3, ntx, nty, (int)nt);
  } else if (ncg == 2 && npg == 2) conv3_wino3_kernel<2, 2><<<nwg, 512, 0, s>>>(a, w3, ntx, nty, (int)nt);
  else if (ncg == 2) conv3_wino3_kernel<2, 1><<<nwg, 256, 0, s>>>(a, w3, ntx, nty, (int)nt);
  else conv3_wino3_kernel<1, 2><<<nwg, 256, 0, s>>>(a, w3, ntx, nty, (int)nt);
  return true;
}

// A Family::MFMA layer (3x3(x3), Cin % 16 == 0, Cout % 32 == 0) by the mode rule: the bf16 pieces, F(4x4), F(2x2) or the implicit GEMM.
// a.w / a.bias: the tap image [taps][Cin][Cout] and the bias; wbf, wino4 (wide layers) and wino3: the other images of the same weights.
// false: nothing launched (an activation beyond the MFMA kernels' 32-bit ranges).  Also runs the input-gradient convolutions of the
// training backward on transposed images (conv_mfma_images).
bool launch_conv_mfma_family(const ConvArgs& a, bool is3d, int mode, bool wide, const float* wbf, const float* wino4, const float* wino3,
                             hipStream_t s) {
  const int B = a.B, D = a.D, H = a.H, W = a.W;
  const int taps = is3d ? 27 : 9;
  if ((mode == FNX_PRECISION_BF16X6 || mode == FNX_PRECISION_BF16X3) && wide) {
    ProfScope ps(FNX_PROF_CONV_BF16, s);
    const int nprod = mode == FNX_PRECISION_BF16X3 ? 3 : 6;
    if (launch_conv_wbf(a, is3d, (const unsigned*)wbf, s, nprod)) {
      // six (three) bf16 MFMA products per Winograd-domain multiply (16 per 2x2 outputs and z tap)
      prof_add_work(FNX_PROF_CONV_BF16, (double)B * D * H * W * 2.0 * a.cin * a.cout * 4.0 * (is3d ? 3 : 1) * (double)nprod);
      return true;
    }
  }
  // (the MFMA kernels address a stage of 8 channel volumes through one 32-bit buffer range: 2^27 cells per sample at
  // most; beyond that -- 137 GB per 128-channel activation -- the direct kernel still works)
  if ((size_t)MF_CHUNK * D * H * W * 4 >= 0xf0000000ull) return false;
  ProfScope ps(FNX_PROF_CONV_MFMA, s);
  const double px = (double)B * D * H * W, mac = 2.0 * a.cin * a.cout;
  // F(4x4): the default (256^3 CNN step 92.2 -> 81.0 ms; 1024^2 2.29 -> 2.14 ms: replayed graphs, alternating runs on one box)
  if (mode == FNX_PRECISION_FP32 && wide && launch_conv_wino4(a, wino4, is3d, s)) {
    prof_add_work(FNX_PROF_CONV_MFMA, px * mac * 2.25 * (is3d ? 3 : 1));  // 36 multiplies per 4x4 outputs (per z tap)
    return true;
  }
  if (mode != FNX_PRECISION_FP32_DIRECT && launch_conv_wino(a, is3d, wino3, s)) {
    prof_add_work(FNX_PROF_CONV_MFMA, px * mac * 4.0 * (is3d ? 3 : 1));   // 16 multiplies per 2x2 outputs (per z tap)
    return true;
  }
  launch_conv_mfma(a, is3d, s);
  prof_add_work(FNX_PROF_CONV_MFMA, px * mac * taps);
  return true;
}

// Layer l of the net from x into y.  mode: FNX_PRECISION_* as net_mode leaves it (FP32_DIRECT: no Winograd, every layer a direct sum over
// its taps; BF16X6 / BF16X3: conv3_wbf_kernel where it applies).  A PAIR layer also applies layer l + 1 (y then has one channel).
void launch_conv(int l, bool is3d, int mode, const float* packed, const float* x, float* y, int B, int D, int H, int W, hipStream_t s) {
  const ConvLayer& L = LAYERS[l];
  const LayerPlan& P = plan(is3d)[l];
  const MfmaImages* tail = P.fam == Family::PAIR ? &plan(is3d)[l + 1].im : nullptr;
  ConvArgs a{x, y, packed + P.im.taps, packed + P.im.bias, B, L.cin, L.cout, D, H, W, L.relu, L.cout / co_tile(L.cout),
             tail ? packed + tail->taps : nullptr, tail ? packed + tail->bias : nullptr};
  switch (P.fam) {
    case Family::MFMA:
      if (launch_conv_mfma_family(a, is3d, mode, P.im.wide, packed + P.im.wbf, packed + P.im.wino4, packed + P.im.wino3, s)) return;
      break;
    case Family::PAIR:
    case Family::KPACK: {
      ProfScope ps(FNX_PROF_CONV_MFMA16, s);
      launch_conv_mfma16(a, is3d, P.fam == Family::PAIR, s);
      prof_add_work(FNX_PROF_CONV_MFMA16, (double)B * D * H * W * 2.0 * L.cin * L.cout * layer_taps(L, is3d));
      return;
    }
    case Family::TO1: {
      ProfScope ps(FNX_PROF_CONV_DIRECT, s);
      const dim3 grid((W + 63) / 64, (H + 3) / 4, B * D), block(64, 4);
      if (is3d) conv3_to1_kernel<true><<<grid, block, 0, s>>>(a); else conv3_to1_kernel<false><<<grid, block, 0, s>>>(a);
      return;
    }
    case Family::DIRECT: break;
  }
  ProfScope ps(FNX_PROF_CONV_DIRECT, s);
  launch_conv_direct(a, is3d, s);
}

// x (B,C,Di,Hi,Wi) -> channels [c_off, c_off+C) of y (B,Ctot,Do,Ho,Wo)
// ZWin: either tensor may hold a window of planes of a deeper notional tensor (the nested crops of multiscale_forward_crop):
// the interpolation runs in the notional depths (full_in -> full_out), x holds notional planes [in_off, in_off + Di) and y the
// notional planes [out_off, out_off + Do); a source plane outside x's window is clamped into it (only planes nobody uses read
// such values).  {Di, 0, Do, 0} = whole tensors.
struct ZWin { int full_in, in_off, full_out, out_off; };
// One launch resamples up to TWO sources into consecutive channel ranges of y (the concatenations of multi_scale_net.py:121-125:
// [x resampled (2 channels), the coarser tower's output resampled (1 channel)]): source 0 fills channels [c_off, c_off + s0.C), source 1
// the next s1.C (s1.C = 0: one source).
struct RSrc { const float* x; int C, Di, Hi, Wi; ZWin zw; };
// One thread per output pixel (lanes along x, blockIdx.y = row, blockIdx.z = (sample, plane)): the interpolation indices and weights
// of a source are computed once and applied to all of its channels (the flat-index version paid an integer division chain and the
// weights per channel value: 22 us for the 3 M values of the full-resolution concat at 1024^2).
__device__ __forceinline__ void resize_source(const RSrc& S, float* __restrict__ y, int b, int k, int j, int i, int Do, int Ho, int Wo,
                                              int Ctot, int c0) {
  const int Di = S.Di, Hi = S.Hi, Wi = S.Wi;
  int x0, x1, y0, y1, z0, z1; float sx0, sx1, t0, t1, f0, f1;
  src_index(i, Wi, Wo, x0, x1, sx0, sx1);
  src_index(j, Hi, Ho, y0, y1, t0, t1);
  src_index(k + S.zw.out_off, S.zw.full_in, S.zw.full_out, z0, z1, f0, f1);
  z0 -= S.zw.in_off; z1 -= S.zw.in_off;
  z0 = z0 < 0 ? 0 : (z0 > Di - 1 ? Di - 1 : z0);
  z1 = z1 < 0 ? 0 : (z1 > Di - 1 ? Di - 1 : z1);
  const bool in_z = S.zw.full_in > 1 || S.zw.full_out > 1;
  const size_t vin = (size_t)Di * Hi * Wi, vout = (size_t)Do * Ho * Wo;
  const float* xi = S.x + (size_t)b * S.C * vin;
  float* yo = y + ((size_t)b * Ctot + c0) * vout + ((size_t)k * Ho + j) * Wo + i;
  const size_t o00 = ((size_t)z0 * Hi + y0) * Wi, o01 = ((size_t)z0 * Hi + y1) * Wi, o10 = ((size_t)z1 * Hi + y0) * Wi, o11 = ((size_t)z1 * Hi + y1) * Wi;
  for (int c = 0; c < S.C; ++c, xi += vin, yo += vout) {
    const float lo = t0 * (sx0 * xi[o00 + x0] + sx1 * xi[o00 + x1]) + t1 * (sx0 * xi[o01 + x0] + sx1 * xi[o01 + x1]);
    float v = lo;
    if (in_z) {
      const float hi = t0 * (sx0 * xi[o10 + x0] + sx1 * xi[o10 + x1]) + t1 * (sx0 * xi[o11 + x0] + sx1 * xi[o11 + x1]);
      v = f0 * lo + f1 * hi;
    }
    *yo = v;
  }
}
__global__ __launch_bounds__(256) void resize_kernel(RSrc s0, RSrc s1, float* __restrict__ y, int B, int Do, int Ho, int Wo, int Ctot,
                                                     int c_off) {
  const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y;
  const int k = blockIdx.z % Do, b = blockIdx.z / Do;
  if (i >= Wo || j >= Ho) return;
  resize_source(s0, y, b, k, j, i, Do, Ho, Wo, Ctot, c_off);
  if (s1.C > 0) resize_source(s1, y, b, k, j, i, Do, Ho, Wo, Ctot, c_off + s0.C);
}

// two sources -> channels [0, C0 + C1) of y in one launch (s1.C = 0: one source, s1 is not read)
void launch_resize2(const RSrc& s0, const RSrc& s1, float* y, int B, int Do, int Ho, int Wo, hipStream_t s) {
  const dim3 grid((Wo + 63) / 64, (Ho + 3) / 4, B * Do), block(64, 4);
  resize_kernel<<<grid, block, 0, s>>>(s0, s1, y, B, Do, Ho, Wo, s0.C + s1.C, 0);
}

}  // namespace

// ---- what the training unit (fnx_cnn_train.hip) uses of the plan and the launchers above ----
void packed_offsets(int l, bool is3d, size_t* taps, size_t* bias) { *taps = plan(is3d)[l].im.taps; *bias = plan(is3d)[l].im.bias; }
void pack_mfma_images(bool is3d, const float* w, const float* bias, int cin, int cout, float* base, const MfmaImages& im, hipStream_t s) {
  const int kd = is3d ? 3 : 1;
  pack_layer_mfma_kernel<<<64, 256, 0, s>>>(w, bias, base + im.taps, base + im.bias, cin, cout, 9 * kd);
  pack_layer_wino_kernel<<<64, 256, 0, s>>>(w, base + im.wino2, cin, cout, kd);
  repack_wino3_kernel<<<64, 256, 0, s>>>(base + im.wino2, base + im.wino3, cin, cout, kd, wino3_rw(cout));
  if (im.wide) {
    pack_wbf_kernel<<<256, 256, 0, s>>>(base + im.wino2, (unsigned*)(base + im.wbf), cin, cout, kd);
    pack_layer_wino4g_kernel<<<64, 256, 0, s>>>(w, base + im.wino4, cin, cout, kd);
  }
}
bool conv_mfma_images(bool is3d, const MfmaImages& im, const float* base, int cin, int cout, int relu, int mode, const float* x, float* y,
                      int B, int D, int H, int W, hipStream_t s) {
  const ConvArgs a{x, y, base + im.taps, base + im.bias, B, cin, cout, D, H, W, relu, cout / co_tile(cout), nullptr, nullptr};
  return launch_conv_mfma_family(a, is3d, mode, im.wide, base + im.wbf, base + im.wino4, base + im.wino3, s);
}

size_t scalenet_weight_floats(bool is3d) { return blob_offsets(is3d).total; }

constexpr size_t packed_bytes(bool is3d) {
  return al256((PLAN[is3d].layer[N_LAYERS - 1].im.bias + LAYERS[N_LAYERS - 1].cout + 64) * sizeof(float));
}
static_assert(packed_bytes(false) == 12622080 && packed_bytes(true) == 38030592, "the packed images' sizes are part of the ABI");
size_t scalenet_packed_bytes(bool is3d) { return packed_bytes(is3d); }

void scalenet_pack(bool is3d, const float* blob, void* packed, hipStream_t s) {
  const BlobOff bo = blob_offsets(is3d);
  float* pk = (float*)packed;
  for (int l = 0; l < N_LAYERS; ++l) {
    const ConvLayer& L = LAYERS[l];
    const LayerPlan& P = plan(is3d)[l];
    const float *w = blob + bo.w[l], *bias = blob + bo.b[l];
    switch (P.fam) {
      case Family::MFMA: pack_mfma_images(is3d, w, bias, L.cin, L.cout, pk, P.im, s); break;
      case Family::PAIR:
        pack_layer_pair_kernel<<<64, 256, 0, s>>>(w, bias, pk + P.im.taps, pk + P.im.bias, L.cin, L.cout, is3d ? 5 : 1, pad_to(L.cin, 4));
        break;
      case Family::KPACK:
        pack_layer_kpack_kernel<<<64, 256, 0, s>>>(w, bias, pk + P.im.taps, pk + P.im.bias, L.cin, L.cout, is3d ? 5 : 1, pad_to(L.cout, 16));
        break;
      default:
        pack_layer_kernel<<<64, 256, 0, s>>>(w, bias, pk + P.im.taps, pk + P.im.bias, L.cin, L.cout, layer_taps(L, is3d), co_tile(L.cout));
    }
  }
}

MultiscaleWs multiscale_ws_layout(const GridDims& g, bool is3d, void* base) {
  const Towers t = tower_sizes(is3d, g.D, g.H, g.W);
  const size_t full = (size_t)g.B * g.DHW, half = (size_t)g.B * vol(t.h), quart = (size_t)g.B * vol(t.q);
  size_t off = 0;
  auto take = [&](size_t bytes) { float* r = base ? (float*)((char*)base + off) : nullptr; off += al256(bytes); return r; };
  MultiscaleWs w{};
  w.bufA = take(full * 128 * 4);
  w.bufB = take(full * 128 * 4);
  w.in1 = take(full * 3 * 4);
  w.in2 = take(half * 3 * 4);
  w.xq = take(quart * 2 * 4);
  w.c2 = take(half * 4);
  w.c4 = take(quart * 4);
  w.bytes = off;
  return w;
}

// The windows of a walk on NESTED z-crops (multiscale_forward_crop): x covers t.f.D planes; the quarter-resolution tower runs on all of
// them, the half-resolution tower on planes [trim[2], D - trim[3]) and the full-resolution tower on [trim[0], D - trim[1]); p and the full
// tower's tensors hold D - trim[0] - trim[1] planes.  Everything else is the arithmetic of the untrimmed pass: the resampling runs in the
// untrimmed grids' coordinates.
static_assert(family_of(LAYERS[15]) == Family::PAIR, "TowerWalk: layer 15 takes the final 1x1 into its epilogue and writes p");
void tower_walk(bool is3d, int B, const Towers& t, const void* packed, int mode, const TowerWalk& w, hipStream_t s) {
  const float* pk = (const float*)packed;
  const Dims q = t.q, h = t.h, f = t.f;
  auto tower = [&](int l0, int n, const float* in, int D, int H, int W) {
    const float* cur = in;
    for (int l = l0; l < l0 + n; ++l) {
      // the last 5x5 layer takes the final 1x1 into its epilogue (multi_scale_net.py:116): one launch, no 8-channel tensor
      float* dst = plan(is3d)[l].fam == Family::PAIR ? w.p : w.out[l];
      launch_conv(l, is3d, mode, pk, cur, dst, B, D, H, W, s);
      cur = dst;
    }
  };
  // windows (planes of each tower's own grid)
  const int f_lo = w.trim[0], f_n = f.D - w.trim[0] - w.trim[1];              // full-resolution tower
  const int h_lo = w.trim[2] / 2, h_n = h.D - w.trim[2] / 2 - w.trim[3] / 2;  // half-resolution tower
  // multi_scale_net.py:119-126
  const ZWin x_to_q{f.D, 0, q.D, 0};
  launch_resize2(RSrc{w.x, 2, f.D, f.H, f.W, x_to_q}, RSrc{nullptr, 0, 1, 1, 1, x_to_q}, w.in[0], B, q.D, q.H, q.W, s);
  tower(0, 4, w.in[0], q.D, q.H, q.W);
  const ZWin x_to_h{f.D, 0, h.D, h_lo}, q_to_h{q.D, 0, h.D, h_lo};
  launch_resize2(RSrc{w.x, 2, f.D, f.H, f.W, x_to_h}, RSrc{w.out[3], 1, q.D, q.H, q.W, q_to_h}, w.in[1], B, h_n, h.H, h.W, s);
  tower(4, 6, w.in[1], h_n, h.H, h.W);
  const ZWin x_to_f{f.D, 0, f.D, f_lo}, h_to_f{h.D, h_lo, f.D, f_lo};
  launch_resize2(RSrc{w.x, 2, f.D, f.H, f.W, x_to_f}, RSrc{w.out[9], 1, h_n, h.H, h.W, h_to_f}, w.in[2], B, f_n, f.H, f.W, s);
  // convN_1 (6 layers), the last one with the final 1x1: it writes p
  tower(10, 6, w.in[2], f_n, f.H, f.W);
}

void multiscale_forward(const GridDims& g, bool is3d, const void* packed, const float* x, float* p, int precision_mode, void* ws,
                        hipStream_t s) {
  const int none[4] = {0, 0, 0, 0};
  multiscale_forward_crop(g, is3d, packed, x, p, precision_mode, ws, s, none);
}

// The forward pass on nested z-crops (the z-slab driver's CNN projection, fnx_slab.hip; the windows: tower_walk): trims are full-resolution
// plane counts, multiples of 4 so that every window starts on a plane of each coarser grid; trim[2] <= trim[0], trim[3] <= trim[1].  A
// tower whose window ends at an artificial face computes garbage within its receptive radius of that face (8 / 14 / 16 full-resolution
// planes for the full / half / quarter tower) -- the caller sizes the windows so that this never reaches what it uses
// (SlabSimulator.NET_TRIMS).  The activations ping-pong between the two large buffers; a tower's last layer writes its output.
void multiscale_forward_crop(const GridDims& g, bool is3d, const void* packed, const float* x, float* p, int precision_mode,
                             void* ws, hipStream_t s, const int trim[4]) {
  const MultiscaleWs m = multiscale_ws_layout(g, is3d, ws);
  TowerWalk w{x, {m.xq, m.in2, m.in1}, {}, p, {trim[0], trim[1], trim[2], trim[3]}};
  for (int l = 0; l < 15; ++l) w.out[l] = (l & 1) ? m.bufB : m.bufA;     // (every tower starts at an even layer)
  w.out[3] = m.c4;
  w.out[9] = m.c2;
  tower_walk(is3d, g.B, tower_sizes(is3d, g.D, g.H, g.W), packed, precision_mode, w, s);
}

// The checks the CNN entry points share (fnx_cnn.h)
int check_net_call(const char* fn, const FnxGrid* g, bool args, int precision_mode, int* mode, size_t (*need)(const GridDims&, bool),
                   size_t ws_bytes) {
  if (!g || !args) return set_error(FNX_EINVAL, "%s: null argument", fn);
  *mode = net_mode(precision_mode);
  if (*mode < 0)
    return set_error(FNX_EINVAL, "%s: unknown precision_mode %d (FNX_PRECISION_FP32, _FP32_DIRECT, _BF16X6, _BF16X3, _FP32_F4 or "
                     "_FP32_F2)", fn, precision_mode);
  if (g->H < 4 || g->W < 4 || (g->is3D && g->D < 4))
    return set_error(FNX_EINVAL, "%s: the three-scale net needs at least 4 cells per axis (D %d, H %d, W %d)", fn, g->D, g->H, g->W);
  if (ws_bytes < need(make_dims(g->B, g->D, g->H, g->W, g->z_offset, g->D_global), g->is3D))
    return set_error(FNX_EWORKSPACE, "%s: workspace of %zu bytes is too small", fn, ws_bytes);
  return FNX_OK;
}

// the ScaleNet as FluidNet.forward's wrapper runs it (fnx_fluidnet.h): a grid's dims carry its z-slab view
static GridDims dims_of(const FnxGrid* g) { return make_dims(g->B, g->D, g->H, g->W, g->z_offset, g->D_global); }
static size_t scalenet_ws(const FnxGrid* g) { return multiscale_ws_bytes(dims_of(g), g->is3D); }
static void scalenet_forward(const FnxGrid* g, const void* packed, const float* x, float* p, int mode, void* ws, hipStream_t s) {
  multiscale_forward(dims_of(g), g->is3D, packed, x, p, mode, ws, s);
}
const Net& scalenet_net(bool is3d) {
  static const Net nets[2] = {{2, FNX_NET_SCALENET, [] { return launch_status(false); }, scalenet_ws, scalenet_forward},
                              {3, FNX_NET_SCALENET, [] { return launch_status(true); }, scalenet_ws, scalenet_forward}};
  return nets[is3d];
}
}  // namespace fnx

// ---------------------------------------------------------------------------------------------------
// C ABI (include/fluidnet_hip.h)
// ---------------------------------------------------------------------------------------------------

extern "C" {

size_t fnx_scalenet_weight_floats(int is3D) { return fnx::scalenet_weight_floats(is3D != 0); }
size_t fnx_scalenet_packed_bytes(int is3D) { return fnx::scalenet_packed_bytes(is3D != 0); }

int fnx_scalenet_pack(int is3D, const float* weights_blob, void* packed, void* stream) {
  if (!weights_blob || !packed) return fnx::set_error(FNX_EINVAL, "%s: null argument", __func__);
  fnx::scalenet_pack(is3D != 0, weights_blob, packed, (hipStream_t)stream);
  return fnx::launch_status(is3D != 0);
}

int fnx_multiscale_forward(const FnxGrid* g, const void* packed, const float* x, float* p, int precision_mode, void* ws,
                           size_t ws_bytes, void* stream) {
  int mode;
  if (int rc = fnx::check_net_call(__func__, g, packed && x && p && ws, precision_mode, &mode, fnx::multiscale_ws_bytes, ws_bytes)) return rc;
  const GridDims d = make_dims(g->B, g->D, g->H, g->W, g->z_offset, g->D_global);
  fnx::multiscale_forward(d, g->is3D, packed, x, p, mode, ws, (hipStream_t)stream);
  return fnx::launch_status(g->is3D);
}

int fnx_multiscale_forward_crop(const FnxGrid* g, const void* packed, const float* x, float* p, int precision_mode,
                                const int trim[4], void* ws, size_t ws_bytes, void* stream) {
  int mode;
  if (int rc = fnx::check_net_call(__func__, g, packed && x && p && ws && trim, precision_mode, &mode, fnx::multiscale_ws_bytes, ws_bytes)) return rc;
  if (!g->is3D && (trim[0] | trim[1] | trim[2] | trim[3])) return fnx::set_error(FNX_EINVAL, "multiscale_forward_crop: z windows need a 3D grid");
  for (int a = 0; a < 4; ++a)
    if (trim[a] < 0 || trim[a] % 4) return fnx::set_error(FNX_EINVAL, "multiscale_forward_crop: trim[%d] = %d must be a non-negative multiple of 4", a, trim[a]);
  if (trim[2] > trim[0] || trim[3] > trim[1]) return fnx::set_error(FNX_EINVAL, "multiscale_forward_crop: the half-resolution window must contain the full-resolution one");
  if ((trim[0] | trim[1] | trim[2] | trim[3]) && (g->D % 4 || g->D - trim[0] - trim[1] < 4))
    return fnx::set_error(FNX_EINVAL, "multiscale_forward_crop: D = %d must be a multiple of 4 and leave at least 4 planes (trims %d + %d)", g->D, trim[0], trim[1]);
  const GridDims d = make_dims(g->B, g->D, g->H, g->W, g->z_offset, g->D_global);
  fnx::multiscale_forward_crop(d, g->is3D, packed, x, p, mode, ws, (hipStream_t)stream, trim);
  return fnx::launch_status(g->is3D);
}

}  // extern "C"
