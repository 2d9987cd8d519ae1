// MultiScale pressure-net (lib/multi_scale_net.py:21-127) -- internal interface of the conv stack.
#pragma once
#include <hip/hip_runtime.h>
#include "fnx_device.h"

struct FnxGrid;
namespace fnx {

struct ConvLayer { int cin, cout, k, relu; };

// channel plan, multi_scale_net.py:111-116 (Dropout = identity in eval)
constexpr int N_LAYERS = 17;
constexpr ConvLayer LAYERS[N_LAYERS] = {
    // convN_4 (quarter resolution)
    {2, 32, 3, 1}, {32, 64, 3, 1}, {64, 32, 3, 0}, {32, 1, 3, 0},
    // convN_2 (half resolution)
    {3, 32, 5, 1}, {32, 64, 3, 1}, {64, 128, 3, 1}, {128, 64, 3, 1}, {64, 32, 3, 0}, {32, 1, 3, 0},
    // convN_1 (full resolution)
    {3, 32, 5, 1}, {32, 64, 3, 1}, {64, 128, 3, 1}, {128, 64, 3, 1}, {64, 32, 3, 0}, {32, 8, 5, 0},
    // final 1x1
    {8, 1, 1, 0}};

constexpr int layer_taps(const ConvLayer& L, bool is3d) { return L.k * L.k * (is3d ? L.k : 1); }
constexpr size_t layer_weight_floats(const ConvLayer& L, bool is3d) { return (size_t)L.cout * L.cin * layer_taps(L, is3d); }

// float offsets of the layers' weights and biases in the blob (and in the gradient blob): per layer the weight, then the bias
struct BlobOff { size_t w[N_LAYERS], b[N_LAYERS], total; };
constexpr BlobOff blob_offsets(bool is3d) {
  BlobOff o{};
  size_t off = 0;
  for (int l = 0; l < N_LAYERS; ++l) {
    o.w[l] = off; off += layer_weight_floats(LAYERS[l], is3d);
    o.b[l] = off; off += LAYERS[l].cout;
  }
  o.total = off;
  return o;
}

// Family::MFMA: the 3x3(x3) layers the matrix-core kernels take (the bf16 pieces, F(4x4), F(2x2) or the implicit GEMM by launch_conv's rule)
constexpr bool is_mfma_layer(int cin, int cout, int k) { return k == 3 && cin % 16 == 0 && cout % 32 == 0; }
// Where a layer's images sit, as float offsets into the packed buffer.  Every family has `taps` (its tap image) and `bias`; `end` is where the
// next layer starts.  The images of one Family::MFMA weight at float offset `off` of a buffer are what scalenet_pack writes for such a
// layer, for any weight tensor -- the backward's transposed, tap-flipped weights go through the forward's launchers.
struct MfmaImages {
  size_t taps;      // the family's tap image (MFMA: [taps][Cin][Cout], the implicit GEMM's A operand)
  size_t wino2;     // MFMA: G g G^T as [dz][16][Cin][Cout] (read by the pack kernels only)
  size_t wino3;     // MFMA: the same values stage-contiguous (conv3_wino3_kernel)
  size_t wbf;       // wide: G g G^T cut into three bf16 pieces in conv3_wbf_kernel's operand layout (1.5x the fp32 image)
  size_t wino4;     // wide: the nine taps in conv3_wino4_kernel's lane order ([Cin/4][Cout/64][9][4][4][16] per z tap)
  size_t bias, end;
  bool wide;        // MFMA with Cout % 64 == 0: also has the bf16 and F(4x4) images
};
constexpr size_t al64(size_t x) { return (x + 63) & ~(size_t)63; }
constexpr MfmaImages mfma_images(bool is3d, int cin, int cout, size_t off) {
  MfmaImages im{};
  const size_t kd = is3d ? 3 : 1, nw = 9 * kd * cin * cout, nwino = 16 * kd * cin * cout;
  im.wide = cout % 64 == 0;
  im.taps = off; im.wino2 = off + nw; im.wino3 = im.wino2 + nwino;
  off = im.wino3 + nwino;
  if (im.wide) { im.wbf = off; im.wino4 = im.wbf + nwino * 3 / 2; off = im.wino4 + nw; }
  im.bias = off;
  im.end = al64(off + cout);
  return im;
}
// w (Cout,Cin,(3,)3,3), bias (Cout) -> the images at base + im.*
void pack_mfma_images(bool is3d, const float* w, const float* bias, int cin, int cout, float* base, const MfmaImages& im, hipStream_t s);
// y = conv3x3(x3)(x, the packed weight) [+ ReLU] by launch_conv's mode rule; false: nothing launched (D * H * W beyond the MFMA kernels'
// range)
bool conv_mfma_images(bool is3d, const MfmaImages& im, const float* base, int cin, int cout, int relu, int mode, const float* x, float* y,
                      int B, int D, int H, int W, hipStream_t s);
// float offsets of layer l's tap image and bias in the packed buffer
void packed_offsets(int l, bool is3d, size_t* taps, size_t* bias);

size_t scalenet_weight_floats(bool is3d);
size_t scalenet_packed_bytes(bool is3d);
void scalenet_pack(bool is3d, const float* blob, void* packed, hipStream_t s);

// The three towers' grids {D, H, W}: quarter, half and full resolution, the reference's int(n * 0.25) / int(n * 0.5) (D stays 1 in 2D,
// which is D = 1: one plane in every tensor)
struct Dims { int D, H, W; };
inline size_t vol(Dims d) { return (size_t)d.D * d.H * d.W; }
struct Towers { Dims q, h, f; };
inline Towers tower_sizes(bool is3d, int D, int H, int W) {
  return Towers{{is3d ? (int)(D * 0.25) : 1, (int)(H * 0.25), (int)(W * 0.25)}, {is3d ? (int)(D * 0.5) : 1, (int)(H * 0.5), (int)(W * 0.5)},
                {D, H, W}};
}

// The inference workspace, in this order, each region rounded up to 256 bytes: two ping-pong activation buffers of 128 channels at full
// resolution, then the small tower I/O.  base == nullptr: the sizes only.
struct MultiscaleWs { float *bufA, *bufB, *in1, *in2, *xq, *c2, *c4; size_t bytes; };
MultiscaleWs multiscale_ws_layout(const GridDims& g, bool is3d, void* base);
inline size_t multiscale_ws_bytes(const GridDims& g, bool is3d) { return multiscale_ws_layout(g, is3d, nullptr).bytes; }

// The forward itself (multi_scale_net.py:119-126): resize, quarter tower, resize, half tower, resize, full tower, the last 5x5(x5) layer
// with the final 1x1(x1) in its epilogue -- 19 launches, and where their tensors live: the three tower inputs (xq, in2, in1), the output
// of layer l = 0..14 and p, the output of layers 15 + 16.  trim: multiscale_forward_crop's (zeros: whole tensors).
struct TowerWalk { const float* x; float* in[3]; float* out[15]; float* p; int trim[4]; };
void tower_walk(bool is3d, int B, const Towers& t, const void* packed, int mode, const TowerWalk& w, hipStream_t s);

// x (B,2,D,H,W) -> p (B,1,D,H,W)
void multiscale_forward(const GridDims& g, bool is3d, const void* packed, const float* x, float* p, int precision_mode, void* ws,
                        hipStream_t s);
// the same on nested z-crops (fnx_cnn.hip): trim = {full-tower low, high, half-tower low, high} in full-resolution planes,
// multiples of 4; p receives g.D - trim[0] - trim[1] planes.  Workspace: multiscale_ws_bytes(g)
void multiscale_forward_crop(const GridDims& g, bool is3d, const void* packed, const float* x, float* p, int precision_mode,
                             void* ws, hipStream_t s, const int trim[4]);
// (every error return sets the thread's message: the Python layer raises fnx_last_error(), which would otherwise be an earlier call's text)
int launch_status(bool is3d);
// The checks the CNN entry points share, before any device call: null arguments (`args`), the precision mode (*mode: as the launchers
// dispatch on it, net_mode), the net's smallest grid and the workspace, which must hold need(dims of g, g->is3D) bytes
int check_net_call(const char* fn, const FnxGrid* g, bool args, int precision_mode, int* mode, size_t (*need)(const GridDims&, bool),
                   size_t ws_bytes);


// ---- training (fnx_cnn_train.hip: 2D and 3D, fp32 modes) --------------------------------------------------------------------------
// torch upsample_{bi,tri}linear(align_corners=False): src = scale*(dst+0.5)-0.5, clamped at 0
__device__ __forceinline__ void src_index(int dst, int in, int out, int& i0, int& i1, float& l0, float& l1) {
  const float scale = (float)in / (float)out;
  float sidx = scale * ((float)dst + 0.5f) - 0.5f;
  if (sidx < 0.f) sidx = 0.f;
  i0 = (int)sidx;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = sidx - (float)i0;
  l0 = 1.f - l1;
}

// tape_layout, multiscale_forward_train, multiscale_backward and its workspace size below take `is3d` and a grid {D, H, W}; 2D is D = 1.

// One entry of the tape of the training forward: a (B,C,D,H,W) tensor at float offset `off`.  The layout is a function of the
// dimension and (B,D,H,W) alone.
constexpr int N_TAPE = 19;   // xq, y0..y3, in2, y4..y9, in1, y10..y15   (y_l: the output of LAYERS[l], after its ReLU)
struct TapeEntry { const char* name; size_t off; int C, D, H, W; };
struct TapeLayout { TapeEntry e[N_TAPE]; size_t floats; };
TapeLayout tape_layout(bool is3d, int B, int D, int H, int W);
inline int tape_input_index(int tower) { return tower == 0 ? 0 : (tower == 1 ? 5 : 12); }   // xq, in2, in1
inline int tape_output_index(int l) { return l < 4 ? 1 + l : (l < 10 ? 2 + l : 3 + l); }    // y_l, l = 0..15

// packed_t: the blob itself followed by the images of the ten transposed, tap-flipped 3x3(x3) weights between 32, 64 and 128 channels
size_t scalenet_packed_t_bytes(bool is3d);
void scalenet_pack_t(bool is3d, const float* blob, void* packed_t, hipStream_t s);
size_t multiscale_backward_ws_bytes(bool is3d, int B, int D, int H, int W);
// x (B,2,D,H,W) -> p (B,1,D,H,W) bit-identical to multiscale_forward in the same mode, and every layer's input in `tape`
void multiscale_forward_train(bool is3d, int B, int D, int H, int W, const void* packed, const float* x, float* p, float* tape, int mode,
                              hipStream_t s);
// grad_p (B,1,D,H,W), the tape of the forward -> grad_blob in the blob's own layout (per layer: weight gradient, bias gradient).
// No atomics; every sum in a fixed order.  wgrad_mfma = false: the plain weight-gradient kernel for every layer (cross-checks).
// false: an input-gradient convolution was not launched (see conv_mfma_images).
bool multiscale_backward(bool is3d, int B, int D, int H, int W, const void* packed_t, const float* grad_p, const float* tape,
                         float* grad_blob, int mode, void* ws, hipStream_t s, bool wgrad_mfma = true);
// gd (B,1,Do,Ho,Wo) -> gs (B,1,Di,Hi,Wi): the adjoint of resize_kernel's resampling of one channel from (Di,Hi,Wi) to (Do,Ho,Wo)
void launch_resize3d_adjoint(const float* gd, float* gs, int B, int Di, int Hi, int Wi, int Do, int Ho, int Wo, hipStream_t s);
// g_net = scale[b] * grad_p + velocity_update_backward_p(scale[b] * setWallBcs(grad_U))   (the adjoint of model.py:213-226)
void launch_scale_mul(size_t n1, int nc, int B, const float* scale, const float* a, const float* addend, float* out, hipStream_t s);
}  // namespace fnx
