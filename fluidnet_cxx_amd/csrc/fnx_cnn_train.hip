// Training of the MultiScale pressure net in 2D and 3D: a forward that keeps every layer's input ("tape", (B,C,D,H,W) tensors) and the
// backward of the conv stack with respect to the 34 parameter tensors (lib/multi_scale_net.py:118-127 under loss.backward(),
// fluid_net_train.py:356-375).  One code for both dimensions: the grid is {D, H, W} with D = 1 in 2D, `is3d` goes down as in the
// inference forward, and the kernels that differ by the z axis take the dimension as a template parameter, so that the 2D
// instantiations have no z loop, no z tap and no plane arithmetic.
//
//   forward   every layer through the inference launchers (conv_layer), so p has the inference forward's bits; the 8-channel tensor
//             between the last 5x5(x5) layer and the final 1x1(x1), which the fused tail never writes, comes from one extra launch.
//   backward  towers in reverse.  Per layer: ReLU mask (saved output > 0), bias gradient, weight gradient, input gradient.
//             weight gradient of the 3x3(x3) layers between 32, 64 and 128 channels: wgrad_mfma_kernel, a GEMM with M = Cout, N = Cin x 9
//             taps (of one dz in 3D), K = B D H W on v_mfma_f32_32x32x2_f32 (exact fp32), split over the pixel tiles; thin layers:
//             wgrad_small_kernel (fp64, in 3D sliced by dz).
//             input gradient of those 3x3(x3) layers: the forward's own launchers on the transposed, tap-flipped weights (packed_t).
// No atomics: every cross-workgroup sum goes through per-workgroup partials that one kernel adds in index order, so two calls on the
// same inputs give the same bits.
#include "fnx_cnn.h"
#include <assert.h>
#include <stdio.h>
#include "fnx_fluidnet.h"
#include "fnx_kernels.h"
#include "../../include/fluidnet_hip.h"

namespace fnx {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr bool is_mfma(const ConvLayer& L) { return is_mfma_layer(L.cin, L.cout, L.k); }   // Family::MFMA, also transposed

// packed_t: [blob | 128 zeros (the transposed convolutions' bias) | staging for one transposed weight | images per MFMA layer]
constexpr size_t stage_floats(bool is3d) {              // the largest transposed 3x3(x3) weight of LAYERS
  size_t n = 0;
  for (int l = 0; l < N_LAYERS; ++l)
    if (is_mfma(LAYERS[l]) && layer_weight_floats(LAYERS[l], is3d) > n)
      n = layer_weight_floats(LAYERS[l], is3d);
  return n;
}
// (the 2D image keeps the 128 x 128 x 9 floats it has always had, twice what its largest weight (128 x 64 x 9) needs: callers see its size)
constexpr size_t STAGE_FLOATS_2D = (size_t)128 * 128 * 9;
static_assert(STAGE_FLOATS_2D >= stage_floats(false), "the 2D staging area");
struct PackedT { size_t zeros, stage, floats; MfmaImages im[N_LAYERS]; };
inline PackedT packed_t_plan(bool is3d) {
  PackedT P{};
  size_t off = al64(blob_offsets(is3d).total);
  P.zeros = off; off += 128;
  P.stage = off; off += is3d ? stage_floats(true) : STAGE_FLOATS_2D;
  for (int l = 0; l < N_LAYERS; ++l)
    if (is_mfma(LAYERS[l])) { P.im[l] = mfma_images(is3d, LAYERS[l].cout, LAYERS[l].cin, off); off = P.im[l].end; }
  P.floats = off + 64;
  return P;
}

// w (Cout,Cin,taps) -> wt (Cin,Cout,taps) with the taps reversed (on every axis): the weight of the input-gradient convolution
__global__ void transpose_flip_kernel(const float* __restrict__ w, float* __restrict__ wt, int cin, int cout, int taps) {
  const int n = cin * cout * taps;
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) {
    const int co = q / (cin * taps), r = q - co * cin * taps;
    const int ci = r / taps, t = r - ci * taps;
    wt[((size_t)ci * cout + co) * taps + (taps - 1 - t)] = w[q];
  }
}
__global__ void fill_zero_kernel(float* __restrict__ p, int n) {
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) p[q] = 0.f;
}

// ---------------------------------------------------------------------------------------------------
// Thin convolutions (the 8-channel tensor of the forward; the input gradients through the 32->1 3x3, 32->8 5x5, 8->1 1x1 layers and
// into channel 2 of the 3->32 5x5 layers): one thread per voxel, CO outputs, the weight of (output o, input i, tap z, r, c) at
// w[w_base + o s_o + i s_i + z s_z + r s_r + c s_c] -- any of the layouts these layers' weights sit in, transposed and flipped by the
// strides.  IS3D = false: one z tap (z = 0) on the one plane of a sample, grid z = B.
// ---------------------------------------------------------------------------------------------------
struct SmallConv { const float* x; float* y; const float* w; const float* bias; int B, cin, D, H, W; long w_base, s_o, s_i, s_z, s_r, s_c; };
template <int K, int CO, bool IS3D>
__global__ __launch_bounds__(256) void conv_small_kernel(SmallConv a) {
  const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y;
  const int k = IS3D ? blockIdx.z % a.D : 0, b = IS3D ? blockIdx.z / a.D : blockIdx.z;
  if (i >= a.W || j >= a.H) return;
  constexpr int PAD = K / 2, KZ = IS3D ? K : 1, PADZ = KZ / 2;
  const size_t plane = (size_t)a.H * a.W, volume = IS3D ? plane * a.D : plane;
  float acc[CO];
#pragma unroll
  for (int o = 0; o < CO; ++o) acc[o] = a.bias ? a.bias[o] : 0.f;
  for (int ci = 0; ci < a.cin; ++ci) {
    const float* xc = a.x + ((size_t)b * a.cin + ci) * volume;
    for (int z = 0; z < KZ; ++z) {
      const int zz = k + z - PADZ;
      if (IS3D && (zz < 0 || zz >= a.D)) continue;
#pragma unroll
      for (int r = 0; r < K; ++r) {
        const int yy = j + r - PAD;
        const bool yin = yy >= 0 && yy < a.H;
#pragma unroll
        for (int c = 0; c < K; ++c) {
          const int xx = i + c - PAD;
          const bool in = yin && xx >= 0 && xx < a.W;
          const float v = in ? xc[(size_t)zz * plane + (size_t)yy * a.W + xx] : 0.f;
          const float* wp = a.w + a.w_base + ci * a.s_i + z * a.s_z + r * a.s_r + c * a.s_c;
#pragma unroll
          for (int o = 0; o < CO; ++o) acc[o] = fmaf(v, wp[o * a.s_o], acc[o]);
        }
      }
    }
  }
  float* yb = a.y + (size_t)b * CO * volume + (size_t)k * plane + (size_t)j * a.W + i;
#pragma unroll
  for (int o = 0; o < CO; ++o) yb[(size_t)o * volume] = acc[o];
}
template <int K, int CO>
void launch_conv_small(bool is3d, const SmallConv& a, hipStream_t s) {
  const dim3 grid((a.W + 63) / 64, (a.H + 3) / 4, a.B * a.D), block(64, 4);
  if (is3d) conv_small_kernel<K, CO, true><<<grid, block, 0, s>>>(a);
  else conv_small_kernel<K, CO, false><<<grid, block, 0, s>>>(a);
}

// gz = gy where the layer's saved output is positive (torch's ReLU rule), else 0; in place
__global__ __launch_bounds__(256) void relu_mask_kernel(float* __restrict__ g, const float* __restrict__ y, size_t n) {
  for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (size_t)gridDim.x * 256) g[q] = y[q] > 0.f ? g[q] : 0.f;
}

// sum of a double over the block's 256 threads in a fixed order (lanes by shuffle, then the four waves in order); result in thread 0
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// The cross-workgroup sums: workgroup (., split) handles the rows [split R / nsplit, (split + 1) R / nsplit) of the R = B D H image rows
// and writes its partial; reduce_partials_kernel adds the nsplit partials of every output in split order.
__device__ __forceinline__ void split_rows(long R, int nsplit, int split, int& r0, int& r1) {
  r0 = (int)(R * split / nsplit);
  r1 = (int)(R * (split + 1) / nsplit);
}
__global__ __launch_bounds__(256) void reduce_partials_kernel(const double* __restrict__ partial, float* __restrict__ out, int n, int nsplit) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  double v = 0.0;
  for (int s = 0; s < nsplit; ++s) v += partial[(size_t)s * n + q];
  out[q] = (float)v;
}

// bias gradient: gb[co] = sum over b, z, y, x of gz.  grid (Cout, nsplit); H here is D H (the planes of a channel are contiguous)
__global__ __launch_bounds__(256) void bias_grad_kernel(const float* __restrict__ gz, double* __restrict__ partial, int B, int cout, int H, int W) {
  __shared__ double red[4];
  const int co = blockIdx.x;
  int r0, r1;
  split_rows((long)B * H, gridDim.y, blockIdx.y, r0, r1);
  double acc = 0.0;
  // wave w takes the rows r0 + w, r0 + w + 4, ..., a lane the columns lane, lane + 64, ...
  for (int row = r0 + (threadIdx.x >> 6); row < r1; row += 4) {
    const int b = row / H, y = row - b * H;
    const float* gr = gz + (((size_t)b * cout + co) * H + y) * W;
    for (int x = threadIdx.x & 63; x < W; x += 64) acc += (double)gr[x];
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) partial[(size_t)blockIdx.y * cout + co] = acc;
}

// weight gradient, plain: gW[co][ci][dz][dy][dx] = sum over b, z, y, x of gz[b,co,z,y,x] a[b,ci,z+dz-r,y+dy-r,x+dx-r].
// grid (Cout Cin, KZ, nsplit) with KZ = K z taps in 3D and 1 in 2D: a workgroup owns one (co, ci) pair and the K x K taps of ONE dz
// over its rows (the 125 taps of a 5x5x5 layer do not fit in fp64 registers; 25 do); a thread reads gz once per voxel and the K x K
// neighbours of a from cache.  The partial of (split, pair, dz, tap) sits at the gradient's own index behind split * n, so
// reduce_partials_kernel finishes it.
template <int K, bool IS3D>
__global__ __launch_bounds__(256) void wgrad_small_kernel(const float* __restrict__ gz, const float* __restrict__ a, double* __restrict__ partial,
                                                          int B, int cin, int cout, int D, int H, int W) {
  __shared__ double red[4];
  constexpr int PAD = K / 2, KK = K * K, KZ = IS3D ? K : 1;
  const int co = blockIdx.x / cin, ci = blockIdx.x - co * cin, dz = IS3D ? blockIdx.y : 0;
  int r0, r1;
  split_rows((long)B * (IS3D ? D : 1) * H, gridDim.z, blockIdx.z, r0, r1);
  const size_t plane = (size_t)H * W, volume = IS3D ? plane * D : plane;
  double acc[KK];
#pragma unroll
  for (int t = 0; t < KK; ++t) acc[t] = 0.0;
  // wave w takes the rows r0 + w, r0 + w + 4, ..., a lane the columns lane, lane + 64, ...
  for (int row = r0 + (threadIdx.x >> 6); row < r1; row += 4) {
    const int y = row % H, bz = row / H, z = IS3D ? bz % D : 0, b = IS3D ? bz / D : bz;
    const int zz = IS3D ? z + dz - PAD : 0;
    if (IS3D && (zz < 0 || zz >= D)) continue;             // the plane of a is padding: zero terms
    const float* gr = gz + ((size_t)b * cout + co) * volume + (size_t)z * plane + (size_t)y * W;
    const float* ap = a + ((size_t)b * cin + ci) * volume + (size_t)zz * plane;
    for (int x = threadIdx.x & 63; x < W; x += 64) {
      const double g = (double)gr[x];
#pragma unroll
      for (int dy = 0; dy < K; ++dy) {
        const int yy = y + dy - PAD;
        const bool yin = yy >= 0 && yy < H;
#pragma unroll
        for (int dx = 0; dx < K; ++dx) {
          const int xx = x + dx - PAD;
          const bool in = yin && xx >= 0 && xx < W;
          const float v = in ? ap[(size_t)yy * W + xx] : 0.f;
          acc[dy * K + dx] += g * (double)v;
        }
      }
    }
  }
  const size_t base = ((size_t)blockIdx.z * gridDim.x + blockIdx.x) * (KK * KZ) + (size_t)dz * KK;
#pragma unroll
  for (int t = 0; t < KK; ++t) {
    const double v = block_sum(acc[t], red);
    if (threadIdx.x == 0) partial[base + t] = v;
  }
}
template <int K>
void launch_wgrad_small(bool is3d, dim3 grid, const float* gz, const float* a, double* partial, int B, int cin, int cout, Dims d, hipStream_t s) {
  if (is3d) wgrad_small_kernel<K, true><<<grid, 256, 0, s>>>(gz, a, partial, B, cin, cout, d.D, d.H, d.W);
  else wgrad_small_kernel<K, false><<<grid, 256, 0, s>>>(gz, a, partial, B, cin, cout, d.D, d.H, d.W);
}

// ---------------------------------------------------------------------------------------------------
// Weight gradient of a 3x3(x3) layer with Cin % 32 == 0 and Cout % 32 == 0 on the matrix cores, exact fp32 (v_mfma_f32_32x32x2_f32).
// In 3D it is sliced by z tap: twenty-seven 32x32 accumulators would be 432 registers per lane, nine fit at two workgroups per CU.
//   D[co 32][ci 32] += A[co][k] * B[k][ci],  k = two neighbouring pixels of a row, one D per tap (dy, dx) of the workgroup's dz
//   A: lane -> gz[co0 + (lane&31)][z][y][x0 + 2 kk + (lane>>5)]                         from the LDS tile sg[32][4 x 32]
//   B: lane -> a[ci0 + (lane&31)][z + dz - 1][y + dy - 1][x0 + 2 kk + (lane>>5) + dx - 1]  from the LDS halo tile sa[32][6 x 34]
// Both tensors are channel-planar in memory; the tiles go through LDS so that a lane can read "its" channel (channel stride odd: the
// 32 channels of a half-wave fall into 32 banks).  Workgroup = 4 waves, pixel tile = 4 rows x 32 columns of one plane, wave w owns row
// w; one A read and nine B reads feed nine MFMAs (576 matrix-core cycles).  grid (Cout/32 * Cin/32, NZ, nsplit) with NZ = 3 z taps in 3D
// and 1 in 2D (dz = 0, no z offset): workgroup (pair, dz, split) marches over the tiles split, split + nsplit, ... of all (b, z) planes
// with its nine accumulators in registers (144 VGPRs); in 3D a tile whose activation plane z + dz - 1 lies outside [0, D) contributes
// zeros and is passed over, and gz is read three times (once per dz).  It adds its four waves' accumulators through LDS in wave order
// and writes partial[split][pair][dz][tap][co][ci]; wgrad_mfma_reduce_kernel adds the splits in order in fp64.
// ---------------------------------------------------------------------------------------------------
constexpr int WG_ROWS = 4, WG_SG = WG_ROWS * 32 + 1, WG_AT = (WG_ROWS + 2) * 34, WG_SA = WG_AT + 1;
template <bool IS3D>
__global__ __launch_bounds__(256, 2) void wgrad_mfma_kernel(const float* __restrict__ gz, const float* __restrict__ a,
                                                            float* __restrict__ partial, int B, int cin, int cout, int D, int H, int W,
                                                            int ntx, int nty) {
  __shared__ float sg[32 * WG_SG];
  __shared__ float sa[32 * WG_SA];
  static_assert(32 * WG_SA >= 4 * 1024, "the wave reduction reuses sa");
  constexpr int NZ = IS3D ? 3 : 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 31, k = lane >> 5;
  const int nib = cin / 32, pair = blockIdx.x, cb = pair / nib, ib = pair - cb * nib;
  const int dz = IS3D ? blockIdx.y : 0, split = blockIdx.z, nsplit = gridDim.z;
  const int ntile = B * (IS3D ? D : 1) * nty * ntx;
  const size_t plane = (size_t)H * W, volume = IS3D ? plane * D : plane;
  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  for (int tile = split; tile < ntile; tile += nsplit) {
    const int tx = tile % ntx, ty = (tile / ntx) % nty, bz = tile / (ntx * nty), z = IS3D ? bz % D : 0, b = IS3D ? bz / D : bz;
    const int za = IS3D ? z + dz - 1 : 0;
    if (IS3D && (za < 0 || za >= D)) continue;         // (uniform over the workgroup: the same tile for every thread)
    const int x0 = tx * 32, y0 = ty * WG_ROWS;
    __syncthreads();                                   // the previous tile's operand reads are done
    {
      const int x = tid & 31, row = (tid >> 5) & 3, c0 = tid >> 7;
      const int yy = y0 + row, xx = x0 + x;
      const bool in = yy < H && xx < W;
      const float* gp = gz + ((size_t)b * cout + cb * 32) * volume + (size_t)z * plane + (in ? (size_t)yy * W + xx : 0);
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int c = c0 + 2 * j;
        sg[c * WG_SG + row * 32 + x] = in ? gp[(size_t)c * volume] : 0.f;
      }
    }
    const float* ab = a + ((size_t)b * cin + ib * 32) * volume + (size_t)za * plane;
    for (int q = tid; q < 32 * WG_AT; q += 256) {
      const int c = q / WG_AT, rem = q - c * WG_AT;
      const int row = rem / 34, col = rem - row * 34;
      const int yy = y0 + row - 1, xx = x0 + col - 1;
      const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
      sa[c * WG_SA + rem] = in ? ab[(size_t)c * volume + (size_t)yy * W + xx] : 0.f;
    }
    __syncthreads();
    const float* sgp = sg + m * WG_SG + wave * 32 + k;
    const float* sap = sa + m * WG_SA + wave * 34 + k;
#pragma unroll 2
    for (int kk = 0; kk < 16; ++kk) {
      const float av = sgp[2 * kk];
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx)
          acc[dy * 3 + dx] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, sap[dy * 34 + 2 * kk + dx], acc[dy * 3 + dx], 0, 0, 0);
    }
  }
  float* red = sa;
  const size_t pbase = (((size_t)split * gridDim.x + pair) * NZ + dz) * 9 * 1024;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave * 1024 + ((r & 3) + 8 * (r >> 2) + 4 * k) * 32 + m] = acc[t][r];
    __syncthreads();
    for (int q = tid; q < 1024; q += 256)
      partial[pbase + (size_t)t * 1024 + q] = (red[q] + red[1024 + q]) + (red[2048 + q] + red[3072 + q]);
  }
}
// taps: 9 or 27 (t = dz * 9 + dy * 3 + dx)
__global__ __launch_bounds__(256) void wgrad_mfma_reduce_kernel(const float* __restrict__ partial, float* __restrict__ out, int cin, int cout,
                                                                int taps, int nsplit) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= cout * cin * taps) return;
  const int co = q / (cin * taps), r = q - co * cin * taps, ci = r / taps, t = r - ci * taps;
  const int nib = cin / 32, npairs = (cout / 32) * nib, pair = (co / 32) * nib + ci / 32;
  const size_t at = ((size_t)pair * taps + t) * 1024 + (co % 32) * 32 + ci % 32, stride = (size_t)npairs * taps * 1024;
  double v = 0.0;
  for (int s = 0; s < nsplit; ++s) v += (double)partial[(size_t)s * stride + at];
  out[q] = (float)v;
}
constexpr int WGRAD_MAX_WG = 512;                                        // workgroups of a wgrad_mfma_kernel launch (two per CU)
constexpr size_t PARTIAL_BYTES = (size_t)WGRAD_MAX_WG * 9 * 1024 * 4;    // 18.9 MB; the plain kernels' double partials are smaller

// Adjoint of the bi- / trilinear upsampling of ONE channel (resize_kernel: a gather through src_index), as a gather on the source side:
// a source voxel adds, in index order (x, then y, then z), the destination voxels whose i0 / i1 name it.  The index map is monotone per
// axis, so they lie in a window around (source + 0.5) / scale that is found by inverting the map with a margin and testing each
// candidate exactly with the forward's own src_index.  That also covers an axis of one plane on both sides (2D: Di = Do = 1): the window
// is {0}, i0 = i1 = 0 and the weight l0 + l1 is exactly 1, so the z step is fmaf(1, pl, 0) = pl.
__device__ __forceinline__ void adjoint_window(int src, int in, int out, int& lo, int& hi) {
  const float inv = (float)out / (float)in;
  lo = (int)floorf(((float)src - 0.5f) * inv - 0.5f) - 2;
  hi = (int)ceilf(((float)src + 1.5f) * inv - 0.5f) + 2;
  lo = lo < 0 ? 0 : lo;
  hi = hi > out - 1 ? out - 1 : hi;
}
__device__ __forceinline__ float adjoint_weight(int dst, int src, int in, int out) {
  int i0, i1; float l0, l1;
  src_index(dst, in, out, i0, i1, l0, l1);
  return (i0 == src ? l0 : 0.f) + (i1 == src ? l1 : 0.f);
}
__global__ __launch_bounds__(256) void resize_adjoint_kernel(const float* __restrict__ gd, float* __restrict__ gs, int Di, int Hi, int Wi,
                                                             int Do, int Ho, int Wo) {
  const int xs = blockIdx.x * 64 + threadIdx.x, ys = blockIdx.y * 4 + threadIdx.y;
  const int zs = blockIdx.z % Di, b = blockIdx.z / Di;
  if (xs >= Wi || ys >= Hi) return;
  int xlo, xhi, ylo, yhi, zlo, zhi;
  adjoint_window(xs, Wi, Wo, xlo, xhi);
  adjoint_window(ys, Hi, Ho, ylo, yhi);
  adjoint_window(zs, Di, Do, zlo, zhi);
  const float* g = gd + (size_t)b * Do * Ho * Wo;
  float acc = 0.f;
  for (int zd = zlo; zd <= zhi; ++zd) {
    const float wz = adjoint_weight(zd, zs, Di, Do);
    if (wz == 0.f) continue;
    float pl = 0.f;
    for (int yd = ylo; yd <= yhi; ++yd) {
      const float wy = adjoint_weight(yd, ys, Hi, Ho);
      if (wy == 0.f) continue;
      float row = 0.f;
      for (int xd = xlo; xd <= xhi; ++xd) {
        const float wx = adjoint_weight(xd, xs, Wi, Wo);
        if (wx != 0.f) row = fmaf(wx, g[((size_t)zd * Ho + yd) * Wo + xd], row);
      }
      pl = fmaf(wy, row, pl);
    }
    acc = fmaf(wz, pl, acc);
  }
  gs[(((size_t)b * Di + zs) * Hi + ys) * Wi + xs] = acc;
}

// out[b,c,:] = scale[b] * a[b,c,:] (+ addend[b,c,:])
__global__ __launch_bounds__(256) void scale_mul_kernel(size_t n1, int nc, const float* __restrict__ scale, const float* __restrict__ a,
                                                        const float* __restrict__ addend, float* __restrict__ out) {
  const int b = blockIdx.y;
  const float sc = scale[b];
  const size_t n = n1 * nc, base = (size_t)b * n;
  for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (size_t)gridDim.x * 256) {
    const float v = sc * a[base + q];
    out[base + q] = addend ? v + addend[base + q] : v;
  }
}

// about 4096 workgroups per launch (16 per CU: the plain kernels wait on their loads, so they want every wave slot), at least one
// image row each
inline int split_count(long outputs, long rows) {
  long n = (4096 + outputs - 1) / outputs;
  if (n > rows) n = rows;
  return n < 1 ? 1 : (int)n;
}

}  // namespace

TapeLayout tape_layout(bool is3d, int B, int D, int H, int W) {
  static const char* const names[N_TAPE] = {"xq", "y0", "y1", "y2", "y3", "in2", "y4", "y5", "y6", "y7", "y8", "y9", "in1", "y10", "y11", "y12",
                                            "y13", "y14", "y15"};
  const Towers t = tower_sizes(is3d, D, H, W);
  TapeLayout T{};
  size_t off = 0;
  int n = 0;
  auto add = [&](int C, Dims d) {
    T.e[n] = TapeEntry{names[n], off, C, d.D, d.H, d.W};
    off = al64(off + (size_t)B * C * vol(d));
    ++n;
  };
  add(2, t.q);
  for (int l = 0; l < 4; ++l) add(LAYERS[l].cout, t.q);
  add(3, t.h);
  for (int l = 4; l < 10; ++l) add(LAYERS[l].cout, t.h);
  add(3, t.f);
  for (int l = 10; l < 16; ++l) add(LAYERS[l].cout, t.f);
  assert(n == N_TAPE);
  T.floats = off + 1024;     // (slack behind the last entry, as the inference workspace has behind its buffers)
  return T;
}

void launch_resize3d_adjoint(const float* gd, float* gs, int B, int Di, int Hi, int Wi, int Do, int Ho, int Wo, hipStream_t s) {
  resize_adjoint_kernel<<<dim3((Wi + 63) / 64, (Hi + 3) / 4, B * Di), dim3(64, 4), 0, s>>>(gd, gs, Di, Hi, Wi, Do, Ho, Wo);
}

size_t scalenet_packed_t_bytes(bool is3d) { return al256(packed_t_plan(is3d).floats * sizeof(float)); }

void scalenet_pack_t(bool is3d, const float* blob, void* packed_t, hipStream_t s) {
  const PackedT P = packed_t_plan(is3d);
  const BlobOff bo = blob_offsets(is3d);
  float* pt = (float*)packed_t;
  hipMemcpyAsync(pt, blob, bo.total * sizeof(float), hipMemcpyDeviceToDevice, s);
  fill_zero_kernel<<<1, 128, 0, s>>>(pt + P.zeros, 128);
  for (int l = 0; l < N_LAYERS; ++l) {
    const ConvLayer& L = LAYERS[l];
    if (!is_mfma(L)) continue;
    // (the staging weight is reused by the next layer: the stream orders the launches)
    transpose_flip_kernel<<<64, 256, 0, s>>>(blob + bo.w[l], pt + P.stage, L.cin, L.cout, layer_taps(L, is3d));
    pack_mfma_images(is3d, pt + P.stage, pt + P.zeros, L.cout, L.cin, pt, P.im[l], s);
  }
}

void multiscale_forward_train(bool is3d, int B, int D, int H, int W, const void* packed, const float* x, float* p, float* tape, int mode,
                              hipStream_t s) {
  const TapeLayout T = tape_layout(is3d, B, D, H, W);
  const float* pk = (const float*)packed;
  auto out = [&](int l) { return tape + T.e[tape_output_index(l)].off; };
  // the inference forward's launches (tower_walk) with every tensor in the tape and no crop
  TowerWalk w{x, {}, {}, p, {0, 0, 0, 0}};
  for (int tw = 0; tw < 3; ++tw) w.in[tw] = tape + T.e[tape_input_index(tw)].off;
  for (int l = 0; l < 15; ++l) w.out[l] = out(l);
  tower_walk(is3d, B, tower_sizes(is3d, D, H, W), packed, mode, w, s);
  // the 8-channel tensor that launch never writes, from the same packed weights ([dz][r][wx 0..5][Cin][dx * 8 + co], dx = 0: tap (dz, r, wx))
  size_t taps, bias;
  packed_offsets(15, is3d, &taps, &bias);
  const long cin_pad = (LAYERS[15].cin + 3) / 4 * 4;
  launch_conv_small<5, 8>(is3d, SmallConv{out(14), out(15), pk + taps, pk + bias, B, LAYERS[15].cin, D, H, W, 0, 1, 16, 30 * cin_pad * 16,
                                          6 * cin_pad * 16, cin_pad * 16}, s);
}

size_t multiscale_backward_ws_bytes(bool is3d, int B, int D, int H, int W) {
  const Towers t = tower_sizes(is3d, D, H, W);
  const size_t full = (size_t)B * vol(t.f);
  return 2 * al256(full * 128 * 4) + al256(full * 4) + al256((size_t)B * vol(t.h) * 4) + al256((size_t)B * vol(t.q) * 4) + al256(PARTIAL_BYTES);
}

bool multiscale_backward(bool is3d, int B, int D, int H, int W, const void* packed_t, const float* grad_p, const float* tape,
                         float* grad_blob, int mode, void* ws, hipStream_t s, bool wgrad_mfma) {
  bool launched = true;                         // false: an input-gradient convolution the forward's launchers refused
  const TapeLayout T = tape_layout(is3d, B, D, H, W);
  const PackedT P = packed_t_plan(is3d);
  const BlobOff bo = blob_offsets(is3d);
  const float* pt = (const float*)packed_t;     // the blob sits at its front
  const Towers t = tower_sizes(is3d, D, H, W);
  const Dims q = t.q, h = t.h, f = t.f;
  const size_t full = (size_t)B * vol(f);
  char* w = (char*)ws;
  float* bufA = (float*)w; w += al256(full * 128 * 4);
  float* bufB = (float*)w; w += al256(full * 128 * 4);
  float* g1 = (float*)w; w += al256(full * 4);                            // gradient of in1's channel 2 (the upsampled c2)
  float* gh = (float*)w; w += al256((size_t)B * vol(h) * 4);              // gradient of c2
  float* gq = (float*)w; w += al256((size_t)B * vol(q) * 4);              // gradient of c4
  void* partial = w;
  auto out = [&](int l) { return tape + T.e[tape_output_index(l)].off; };

  auto bias_grad = [&](const float* gz, int l, Dims d) {
    const int cout = LAYERS[l].cout, ns = split_count(cout, (long)B * d.D * d.H);
    bias_grad_kernel<<<dim3(cout, ns), 256, 0, s>>>(gz, (double*)partial, B, cout, d.D * d.H, d.W);
    reduce_partials_kernel<<<(cout + 255) / 256, 256, 0, s>>>((const double*)partial, grad_blob + bo.b[l], cout, ns);
  };
  auto weight_grad = [&](const float* gz, const float* a, int l, Dims d) {
    const ConvLayer& L = LAYERS[l];
    float* gw = grad_blob + bo.w[l];
    const int kz = is3d ? L.k : 1;                                        // z taps: the y extent of both weight-gradient grids
    if (wgrad_mfma && is_mfma(L) && L.cin % 32 == 0) {
      const int ntx = (d.W + 31) / 32, nty = (d.H + WG_ROWS - 1) / WG_ROWS, npairs = (L.cout / 32) * (L.cin / 32);
      const long ntile = (long)B * d.D * ntx * nty;
      int ns = WGRAD_MAX_WG / (kz * npairs);
      if (ns > ntile) ns = (int)ntile;
      const dim3 grid(npairs, kz, ns);
      if (is3d) wgrad_mfma_kernel<true><<<grid, 256, 0, s>>>(gz, a, (float*)partial, B, L.cin, L.cout, d.D, d.H, d.W, ntx, nty);
      else wgrad_mfma_kernel<false><<<grid, 256, 0, s>>>(gz, a, (float*)partial, B, L.cin, L.cout, d.D, d.H, d.W, ntx, nty);
      const int n = L.cout * L.cin * 9 * kz;
      wgrad_mfma_reduce_kernel<<<(n + 255) / 256, 256, 0, s>>>((const float*)partial, gw, L.cin, L.cout, 9 * kz, ns);
      return;
    }
    const int pairs = L.cout * L.cin, ns = split_count((long)pairs * kz, (long)B * d.D * d.H), n = pairs * layer_taps(L, is3d);
    assert((size_t)ns * n * sizeof(double) <= PARTIAL_BYTES);
    const dim3 grid(pairs, kz, ns);
    if (L.k == 5) launch_wgrad_small<5>(is3d, grid, gz, a, (double*)partial, B, L.cin, L.cout, d, s);
    else if (L.k == 3) launch_wgrad_small<3>(is3d, grid, gz, a, (double*)partial, B, L.cin, L.cout, d, s);
    else launch_wgrad_small<1>(is3d, grid, gz, a, (double*)partial, B, L.cin, L.cout, d, s);
    reduce_partials_kernel<<<(n + 255) / 256, 256, 0, s>>>((const double*)partial, gw, n, ns);
  };
  // gradient of layer l's input from the gradient gz of its (pre-activation) output
  auto input_grad = [&](int l, const float* gz, float* ga, Dims d) {
    const ConvLayer& L = LAYERS[l];
    const long taps = layer_taps(L, is3d);
    if (is_mfma(L)) {
      launched = conv_mfma_images(is3d, P.im[l], pt, L.cout, L.cin, 0, mode, gz, ga, B, d.D, d.H, d.W, s) && launched;
      return;
    }
    // W (Cout,Cin,(k,)k,k) read as (output = ci, input = co, taps reversed)
    const SmallConv a{gz, ga, pt + bo.w[l], nullptr, B, L.cout, d.D, d.H, d.W, taps - 1, taps, L.cin * taps, -(long)(L.k * L.k), -(long)L.k, -1};
    if (L.k == 3 && L.cin == 32) launch_conv_small<3, 32>(is3d, a, s);
    else if (L.k == 5 && L.cin == 32) launch_conv_small<5, 32>(is3d, a, s);
    else { assert(L.k == 1 && L.cin == 8); launch_conv_small<1, 8>(is3d, a, s); }
  };
  // One tower in reverse: layers l0 .. l0 + n - 1 with input tape entry `tin`; g: the gradient of the last layer's output (modified);
  // gin2: where the gradient of the input's channel 2 goes (the upsampled output of the coarser tower), or null
  auto tower_bwd = [&](int tin, int l0, int n, float* g, Dims d, float* gin2) {
    float* cur = g;
    for (int l = l0 + n - 1; l >= l0; --l) {
      const ConvLayer& L = LAYERS[l];
      const float* a = l == l0 ? tape + T.e[tin].off : out(l - 1);
      if (L.relu) {
        const size_t cnt = (size_t)B * L.cout * vol(d);
        size_t blocks = (cnt + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        relu_mask_kernel<<<(unsigned)blocks, 256, 0, s>>>(cur, out(l), cnt);
      }
      bias_grad(cur, l, d);
      weight_grad(cur, a, l, d);
      if (l > l0) {
        float* nxt = cur == bufA ? bufB : bufA;
        input_grad(l, cur, nxt, d);
        cur = nxt;
      } else if (gin2) {
        // channel 2 of the 3->32 5x5(x5) layer's input: 32 -> 1, W[co][2][.] with the taps reversed
        assert(L.k == 5 && L.cin == 3);
        const long taps = layer_taps(L, is3d);
        launch_conv_small<5, 1>(is3d, SmallConv{cur, gin2, pt + bo.w[l], nullptr, B, L.cout, d.D, d.H, d.W, 2 * taps + taps - 1, 0, 3 * taps,
                                                -25, -5, -1}, s);
      }
    }
  };
  // the final 1x1(x1) (8 -> 1): its own gradients, then the gradient of the 8-channel tensor in bufA
  bias_grad(grad_p, 16, f);
  weight_grad(grad_p, out(15), 16, f);
  input_grad(16, grad_p, bufA, f);
  tower_bwd(tape_input_index(2), 10, 6, bufA, f, g1);
  launch_resize3d_adjoint(g1, gh, B, h.D, h.H, h.W, D, H, W, s);
  tower_bwd(tape_input_index(1), 4, 6, gh, h, g1);        // (g1 is free again: the half-resolution in2's channel 2)
  launch_resize3d_adjoint(g1, gq, B, q.D, q.H, q.W, h.D, h.H, h.W, s);
  tower_bwd(tape_input_index(0), 0, 4, gq, q, nullptr);
  return launched;
}

void launch_scale_mul(size_t n1, int nc, int B, const float* scale, const float* a, const float* addend, float* out, hipStream_t s) {
  size_t blocks = (n1 * nc + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  scale_mul_kernel<<<dim3((unsigned)blocks, B), 256, 0, s>>>(n1, nc, scale, a, addend, out);
}


// The adjoint of what follows a taped net in FluidNet.forward (fnx_cnn.h): one statement for the ScaleNet and the bank model.
FluidnetTrainBwdWs fluidnet_train_bwd_ws(int nc, const FnxGrid* g, void* base) {
  const size_t full = (size_t)g->B * g->D * g->H * g->W;
  char* w = (char*)base;
  FluidnetTrainBwdWs f{};
  f.gU = (float*)w; w += al256(full * nc * 4);
  f.gU_in = (float*)w; w += al256(full * nc * 4);
  f.gp = (float*)w; w += al256(full * 4);
  f.gnet = (float*)w; w += al256(full * 4);
  f.net = w;
  f.bytes = (size_t)(w - (char*)base);
  return f;
}
int fluidnet_train_gnet(int nc, const FnxGrid* g, const float* flags, const float* scale, const float* grad_p, const float* grad_U,
                        const FluidnetTrainBwdWs& w, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const size_t n1 = (size_t)g->D * g->H * g->W;
  launch_scale_mul(n1, nc, g->B, scale, grad_U, nullptr, w.gU, s);
  if (int rc = fnx_set_wall_bcs(g, w.gU, flags, stream)) return rc;
  if (int rc = fnx_velocity_update_backward(g, w.gU, flags, w.gU_in, w.gp, stream)) return rc;
  launch_scale_mul(n1, 1, g->B, scale, grad_p, w.gp, w.gnet, s);
  return FNX_OK;
}

}  // namespace fnx

// ---------------------------------------------------------------------------------------------------
// C ABI (include/fluidnet_hip.h): the fnx_multiscale_* / fnx_fluidnet_* entry points take a 2D grid, the fnx_multiscale3d_* /
// fnx_fluidnet3d_* ones a 3D grid and the byte size of the weight image they are given; both families are wrappers of one body each.
// ---------------------------------------------------------------------------------------------------
namespace {
// a whole 3D grid (no compute window, no z-slab view), the net's smallest grid and the ranges the kernels index with 32 bits
int check_grid3d(const char* fn, const FnxGrid* g) {
  if (!g->is3D || g->D < 4)
    return fnx::set_error(FNX_EINVAL, "%s: this entry point is 3D only (is3D = %d, D = %d; the 2D net trains through fnx_multiscale_* / "
                          "fnx_fluidnet_*)", fn, g->is3D, g->D);
  if (g->B < 1) return fnx::set_error(FNX_EINVAL, "%s: the batch size must be at least 1 (B = %d)", fn, g->B);
  if (g->H < 4 || g->W < 4)
    return fnx::set_error(FNX_EINVAL, "%s: the three-scale net needs at least 4 cells per axis (H %d, W %d)", fn, g->H, g->W);
  if (g->k_begin || g->k_end || g->z_offset || g->D_global)
    return fnx::set_error(FNX_EINVAL, "%s: training takes a whole domain, not a compute window or a z-slab view (k_begin %d, k_end %d, "
                          "z_offset %d, D_global %d)", fn, g->k_begin, g->k_end, g->z_offset, g->D_global);
  const size_t cells = (size_t)g->D * g->H * g->W;
  if (cells >= ((size_t)1 << 26) || (size_t)g->B * g->D * g->H >= ((size_t)1 << 30) || (size_t)g->B * g->D > 65535)
    return fnx::set_error(FNX_EINVAL, "%s: D * H * W = %zu cells per sample (B * D = %zu planes) is beyond the training kernels' ranges "
                          "(2^26 cells, 65535 planes)", fn, cells, (size_t)g->B * g->D);
  // (the weight-gradient kernel counts its 4 x 32 pixel tiles over all (b, z) planes in an int)
  const size_t tiles = (size_t)g->B * g->D * ((g->H + 3) / 4) * ((g->W + 31) / 32);
  if (tiles >= ((size_t)1 << 31))
    return fnx::set_error(FNX_EINVAL, "%s: %zu pixel tiles (B * D * ceil(H / 4) * ceil(W / 32)) are beyond the training kernels' ranges "
                          "(2^31 tiles)", fn, tiles);
  return FNX_OK;
}
inline bool is_grid2d(const FnxGrid* g) { return !g->is3D && g->D == 1; }
// The checks the training entry points share, before any device call, in the order each family has always made them: null arguments,
// the grid's dimension (3D: all of check_grid3d), an fp32 precision mode (*mode as the launchers dispatch on it), then in 2D the net's
// smallest grid and the ranges the kernels index with 32 bits.
int check_train_call(const char* fn, bool is3d, const FnxGrid* g, bool args, int precision_mode, int* mode) {
  if (!g || !args) return fnx::set_error(FNX_EINVAL, "%s: null argument", fn);
  if (is3d) {
    if (int rc = check_grid3d(fn, g)) return rc;
  } else if (!is_grid2d(g)) {
    return fnx::set_error(FNX_EINVAL, "%s: training is 2D only (is3D = %d, D = %d)", fn, g->is3D, g->D);
  }
  *mode = fnx::net_mode(precision_mode);
  if (*mode < 0)
    return fnx::set_error(FNX_EINVAL, "%s: unknown precision_mode %d (FNX_PRECISION_FP32, _FP32_DIRECT, _BF16X6, _BF16X3, _FP32_F4 or "
                          "_FP32_F2)", fn, precision_mode);
  if (*mode == FNX_PRECISION_BF16X6 || *mode == FNX_PRECISION_BF16X3)
    return fnx::set_error(FNX_EINVAL, "%s: training runs in fp32 arithmetic only (FNX_PRECISION_FP32, _FP32_F4, _FP32_F2 or _FP32_DIRECT), "
                          "not in the bf16 modes (precision_mode %d)", fn, precision_mode);
  if (is3d) return FNX_OK;
  if (g->B < 1 || g->H < 4 || g->W < 4)
    return fnx::set_error(FNX_EINVAL, "%s: the three-scale net needs at least 4 cells per axis (H %d, W %d)", fn, g->H, g->W);
  if ((size_t)g->H * g->W >= ((size_t)1 << 26) || (size_t)g->B * g->H >= ((size_t)1 << 30))
    return fnx::set_error(FNX_EINVAL, "%s: H * W = %zu cells per sample is beyond the training kernels' ranges", fn, (size_t)g->H * g->W);
  return FNX_OK;
}
// 3D entry points: packed (fnx_scalenet_pack(1, ..)) and packed3d_t look alike and differ in size: a swapped pair must not reach the
// device.  The 2D entry points take no size.
int check_image(const char* fn, bool is3d, size_t bytes, bool transposed) {
  if (!is3d) return FNX_OK;
  const size_t fwd = fnx::scalenet_packed_bytes(true), bwd = fnx::scalenet_packed_t_bytes(true);
  const size_t want = transposed ? bwd : fwd;
  if (bytes == want) return FNX_OK;
  return fnx::set_error(FNX_EINVAL, "%s: the weight image has %zu bytes, not the %zu of %s%s", fn, bytes, want,
                        transposed ? "fnx_scalenet3d_pack_t" : "fnx_scalenet_pack(is3D = 1)",
                        bytes == (transposed ? fwd : bwd) ? " (packed and packed3d_t are swapped)" : "");
}
int train_status(bool is3d) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? FNX_OK : fnx::set_error(FNX_EHIP, "HIP error in a %sCNN training launch: %s", is3d ? "3D " : "", hipGetErrorString(e));
}
int not_launched(const char* fn, bool is3d) {
  return fnx::set_error(FNX_EINVAL, "%s: an input-gradient convolution was not launched (%sH * W beyond the MFMA kernels' range)", fn,
                        is3d ? "D * " : "");
}
int too_small(const char* fn, size_t ws_bytes) { return fnx::set_error(FNX_EWORKSPACE, "%s: workspace of %zu bytes is too small", fn, ws_bytes); }

int pack_t_call(const char* fn, bool is3d, const float* weights_blob, void* packed_t, void* stream) {
  if (!weights_blob || !packed_t) return fnx::set_error(FNX_EINVAL, "%s: null argument", fn);
  fnx::scalenet_pack_t(is3d, weights_blob, packed_t, (hipStream_t)stream);
  return train_status(is3d);
}

int forward_train_call(const char* fn, bool is3d, const FnxGrid* g, const void* packed, size_t packed_bytes, const float* x, float* p,
                       float* tape, int precision_mode, void* stream) {
  int mode;
  if (int rc = check_train_call(fn, is3d, g, packed && x && p && tape, precision_mode, &mode)) return rc;
  if (int rc = check_image(fn, is3d, packed_bytes, false)) return rc;
  fnx::multiscale_forward_train(is3d, g->B, g->D, g->H, g->W, packed, x, p, tape, mode, (hipStream_t)stream);
  return train_status(is3d);
}

int backward_call(const char* fn, bool is3d, const FnxGrid* g, const void* packed_t, size_t packed_t_bytes, const float* grad_p,
                  const float* tape, float* grad_blob, int precision_mode, bool wgrad_mfma, void* ws, size_t ws_bytes, void* stream) {
  int mode;
  if (int rc = check_train_call(fn, is3d, g, packed_t && grad_p && tape && grad_blob && ws, precision_mode, &mode)) return rc;
  if (int rc = check_image(fn, is3d, packed_t_bytes, true)) return rc;
  if (ws_bytes < fnx::multiscale_backward_ws_bytes(is3d, g->B, g->D, g->H, g->W)) return too_small(fn, ws_bytes);
  if (!fnx::multiscale_backward(is3d, g->B, g->D, g->H, g->W, packed_t, grad_p, tape, grad_blob, mode, ws, (hipStream_t)stream, wgrad_mfma))
    return not_launched(fn, is3d);
  return train_status(is3d);
}

// The two ScaleNets' records for FluidNet.forward's wrapper (fnx_fluidnet.h): x is rebuilt from the tape, so none is kept or read
template <bool IS3D>
constexpr fnx::NetTrain scalenet_train() {
  return {IS3D ? 3 : 2, [] { return train_status(IS3D); },
          [](const FnxGrid* g, const void* packed, const float* x, float* p, float* tape, int mode, hipStream_t s) {
            fnx::multiscale_forward_train(IS3D, g->B, g->D, g->H, g->W, packed, x, p, tape, mode, s);
          },
          [](const FnxGrid* g, const void* packed_t, const float*, const float* grad_p, const float* tape, float* grad_blob, int mode, void* ws,
             hipStream_t s) { return fnx::multiscale_backward(IS3D, g->B, g->D, g->H, g->W, packed_t, grad_p, tape, grad_blob, mode, ws, s); },
          [](const FnxGrid* g) { return fnx::multiscale_backward_ws_bytes(IS3D, g->B, g->D, g->H, g->W); }, nullptr};
}
constexpr fnx::NetTrain NET_TRAIN[2] = {scalenet_train<false>(), scalenet_train<true>()};

// FluidNet.forward for training around the ScaleNet: this family's checks, then fnx_fluidnet.hip's bodies
int whole_forward_train_call(const char* fn, bool is3d, const FnxGrid* g, const void* packed, size_t packed_bytes, const float* input,
                             float normalize_threshold, float* p_out, float* U_out, float* flags_out, float* scale_out, float* tape,
                             int precision_mode, void* ws, size_t ws_bytes, void* stream) {
  int mode;
  if (int rc = check_train_call(fn, is3d, g, packed && input && p_out && U_out && flags_out && scale_out && tape && ws, precision_mode, &mode))
    return rc;
  if (int rc = check_image(fn, is3d, packed_bytes, false)) return rc;
  if (ws_bytes < fnx::fluidnet_train_ws_bytes(NET_TRAIN[is3d], g)) return too_small(fn, ws_bytes);
  return fnx::fluidnet_forward_train(NET_TRAIN[is3d], g, packed, input, normalize_threshold, p_out, U_out, flags_out, scale_out, tape, mode, ws,
                                     stream);
}

int whole_backward_call(const char* fn, bool is3d, const FnxGrid* g, const void* packed_t, size_t packed_t_bytes, const float* flags,
                        const float* scale, const float* grad_p, const float* grad_U, const float* tape, float* grad_blob, int precision_mode,
                        void* ws, size_t ws_bytes, void* stream) {
  int mode;
  if (int rc = check_train_call(fn, is3d, g, packed_t && flags && scale && grad_p && grad_U && tape && grad_blob && ws, precision_mode, &mode))
    return rc;
  if (int rc = check_image(fn, is3d, packed_t_bytes, true)) return rc;
  if (ws_bytes < fnx::fluidnet_train_ws_bytes(NET_TRAIN[is3d], g)) return too_small(fn, ws_bytes);
  bool launched;
  const int rc = fnx::fluidnet_backward(NET_TRAIN[is3d], g, packed_t, flags, scale, grad_p, grad_U, tape, grad_blob, mode, ws, stream, &launched);
  return launched ? rc : not_launched(fn, is3d);
}

// the tape layout of a checked grid into one of the two ABI structs (FnxTapeEntry has no D); either may be null
size_t fill_tape_entries(bool is3d, const FnxGrid* g, FnxTapeEntry* e2, FnxTapeEntry3D* e3) {
  const fnx::TapeLayout T = fnx::tape_layout(is3d, g->B, g->D, g->H, g->W);
  for (int i = 0; i < fnx::N_TAPE; ++i) {
    const fnx::TapeEntry& t = T.e[i];
    if (e2) { snprintf(e2[i].name, sizeof(e2[i].name), "%s", t.name); e2[i].offset = t.off; e2[i].C = t.C; e2[i].H = t.H; e2[i].W = t.W; }
    if (e3) { snprintf(e3[i].name, sizeof(e3[i].name), "%s", t.name); e3[i].offset = t.off; e3[i].C = t.C; e3[i].D = t.D; e3[i].H = t.H; e3[i].W = t.W; }
  }
  return T.floats;
}
// the 3D size queries: 0 with the refusal's text, or 1 for a grid that passes
bool grid3d_ok(const char* fn, const FnxGrid* g) {
  if (!g) { fnx::set_error(FNX_EINVAL, "%s: null argument", fn); return false; }
  return check_grid3d(fn, g) == FNX_OK;
}
bool grid2d_ok(const char* fn, const FnxGrid* g) {
  if (g && is_grid2d(g)) return true;
  fnx::set_error(FNX_EINVAL, "%s: a 2D grid is needed", fn);
  return false;
}
}  // namespace

extern "C" {

int fnx_multiscale_tape_entries(void) { return fnx::N_TAPE; }

size_t fnx_multiscale_tape_layout(const FnxGrid* g, FnxTapeEntry* entries) {
  if (!g || !is_grid2d(g) || g->B < 1 || g->H < 4 || g->W < 4) {
    fnx::set_error(FNX_EINVAL, "%s: a 2D grid of at least 4 cells per axis is needed", __func__);
    return 0;
  }
  return fill_tape_entries(false, g, entries, nullptr);
}
size_t fnx_multiscale3d_tape_layout(const FnxGrid* g, FnxTapeEntry3D* entries) {
  return grid3d_ok(__func__, g) ? fill_tape_entries(true, g, nullptr, entries) : 0;
}

int fnx_trilinear_upsample_backward(int B, int Di, int Hi, int Wi, int Do, int Ho, int Wo, const float* grad_dst, float* grad_src,
                                    void* stream) {
  if (!grad_dst || !grad_src) return fnx::set_error(FNX_EINVAL, "%s: null argument", __func__);
  if (B < 1 || Di < 1 || Hi < 1 || Wi < 1 || Do < 1 || Ho < 1 || Wo < 1 || (size_t)B * Di > 65535 ||
      (size_t)Do * Ho * Wo >= ((size_t)1 << 31) || (size_t)Di * Hi * Wi >= ((size_t)1 << 31))
    return fnx::set_error(FNX_EINVAL, "%s: sizes (%d; %d, %d, %d <- %d, %d, %d) outside the kernel's range (1 .. 65535 planes B * Di, "
                          "2^31 cells per sample)", __func__, B, Di, Hi, Wi, Do, Ho, Wo);
  fnx::launch_resize3d_adjoint(grad_dst, grad_src, B, Di, Hi, Wi, Do, Ho, Wo, (hipStream_t)stream);
  return train_status(true);
}

size_t fnx_scalenet_packed_t_bytes(void) { return fnx::scalenet_packed_t_bytes(false); }
size_t fnx_scalenet3d_packed_t_bytes(void) { return fnx::scalenet_packed_t_bytes(true); }

int fnx_scalenet_pack_t(const float* weights_blob, void* packed_t, void* stream) {
  return pack_t_call(__func__, false, weights_blob, packed_t, stream);
}
int fnx_scalenet3d_pack_t(const float* weights_blob, void* packed_t, void* stream) {
  return pack_t_call(__func__, true, weights_blob, packed_t, stream);
}

size_t fnx_multiscale_backward_ws_bytes(const FnxGrid* g) {
  return grid2d_ok(__func__, g) ? fnx::multiscale_backward_ws_bytes(false, g->B, 1, g->H, g->W) : 0;
}
size_t fnx_multiscale3d_backward_ws_bytes(const FnxGrid* g) {
  return grid3d_ok(__func__, g) ? fnx::multiscale_backward_ws_bytes(true, g->B, g->D, g->H, g->W) : 0;
}

int fnx_multiscale_forward_train(const FnxGrid* g, const void* packed, const float* x, float* p, float* tape, int precision_mode,
                                 void* stream) {
  return forward_train_call(__func__, false, g, packed, 0, x, p, tape, precision_mode, stream);
}
int fnx_multiscale3d_forward_train(const FnxGrid* g, const void* packed, size_t packed_bytes, const float* x, float* p, float* tape,
                                   int precision_mode, void* stream) {
  return forward_train_call(__func__, true, g, packed, packed_bytes, x, p, tape, precision_mode, stream);
}

int fnx_multiscale_backward(const FnxGrid* g, const void* packed_t, const float* grad_p, const float* tape, float* grad_blob,
                            int precision_mode, void* ws, size_t ws_bytes, void* stream) {
  return backward_call(__func__, false, g, packed_t, 0, grad_p, tape, grad_blob, precision_mode, true, ws, ws_bytes, stream);
}
int fnx_multiscale_backward_plain(const FnxGrid* g, const void* packed_t, const float* grad_p, const float* tape, float* grad_blob,
                                  int precision_mode, void* ws, size_t ws_bytes, void* stream) {
  return backward_call(__func__, false, g, packed_t, 0, grad_p, tape, grad_blob, precision_mode, false, ws, ws_bytes, stream);
}
int fnx_multiscale3d_backward(const FnxGrid* g, const void* packed_t, size_t packed_t_bytes, const float* grad_p, const float* tape,
                              float* grad_blob, int precision_mode, void* ws, size_t ws_bytes, void* stream) {
  return backward_call(__func__, true, g, packed_t, packed_t_bytes, grad_p, tape, grad_blob, precision_mode, true, ws, ws_bytes, stream);
}
int fnx_multiscale3d_backward_plain(const FnxGrid* g, const void* packed_t, size_t packed_t_bytes, const float* grad_p, const float* tape,
                                    float* grad_blob, int precision_mode, void* ws, size_t ws_bytes, void* stream) {
  return backward_call(__func__, true, g, packed_t, packed_t_bytes, grad_p, tape, grad_blob, precision_mode, false, ws, ws_bytes, stream);
}

size_t fnx_fluidnet_train_ws_bytes(const FnxGrid* g) { return grid2d_ok(__func__, g) ? fnx::fluidnet_train_ws_bytes(NET_TRAIN[0], g) : 0; }
size_t fnx_fluidnet3d_train_ws_bytes(const FnxGrid* g) { return grid3d_ok(__func__, g) ? fnx::fluidnet_train_ws_bytes(NET_TRAIN[1], g) : 0; }

int fnx_fluidnet_forward_train(const FnxGrid* g, const void* packed, const float* input, float normalize_threshold, float* p_out,
                               float* U_out, float* flags_out, float* scale_out, float* tape, int precision_mode, void* ws, size_t ws_bytes,
                               void* stream) {
  return whole_forward_train_call(__func__, false, g, packed, 0, input, normalize_threshold, p_out, U_out, flags_out, scale_out, tape,
                                  precision_mode, ws, ws_bytes, stream);
}
int fnx_fluidnet3d_forward_train(const FnxGrid* g, const void* packed, size_t packed_bytes, const float* input, float normalize_threshold,
                                 float* p_out, float* U_out, float* flags_out, float* scale_out, float* tape, int precision_mode, void* ws,
                                 size_t ws_bytes, void* stream) {
  return whole_forward_train_call(__func__, true, g, packed, packed_bytes, input, normalize_threshold, p_out, U_out, flags_out, scale_out,
                                  tape, precision_mode, ws, ws_bytes, stream);
}

int fnx_fluidnet_backward(const FnxGrid* g, const void* packed_t, const float* flags, const float* scale, const float* grad_p,
                          const float* grad_U, const float* tape, float* grad_blob, int precision_mode, void* ws, size_t ws_bytes,
                          void* stream) {
  return whole_backward_call(__func__, false, g, packed_t, 0, flags, scale, grad_p, grad_U, tape, grad_blob, precision_mode, ws, ws_bytes,
                             stream);
}
int fnx_fluidnet3d_backward(const FnxGrid* g, const void* packed_t, size_t packed_t_bytes, const float* flags, const float* scale,
                            const float* grad_p, const float* grad_U, const float* tape, float* grad_blob, int precision_mode, void* ws,
                            size_t ws_bytes, void* stream) {
  return whole_backward_call(__func__, true, g, packed_t, packed_t_bytes, flags, scale, grad_p, grad_U, tape, grad_blob, precision_mode, ws,
                             ws_bytes, stream);
}

}  // extern "C"
