// MultiScale pressure-net (lib/multi_scale_net.py:21-127) -- internal interface of the conv stack.
#pragma once
#include <hip/hip_runtime.h>
#include "fnx_device.h"

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

size_t scalenet_weight_floats(bool is3d);
size_t scalenet_packed_bytes(bool is3d);
void scalenet_pack(bool is3d, const float* blob, void* packed, hipStream_t s);

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
size_t multiscale_ws_bytes(const GridDims& g, bool is3d);
size_t fluidnet_ws_bytes(const GridDims& g, bool is3d);

// x (B,2,D,H,W) -> p (B,1,D,H,W)
void multiscale_forward(const GridDims& g, bool is3d, const void* packed, const float* x, float* p, int precision_mode, void* ws,
                        hipStream_t s);
// the same on nested z-crops (fnx_cnn.hip): trim = {full-tower low, high, half-tower low, high} in full-resolution planes,
// multiples of 4; p receives g.D - trim[0] - trim[1] planes.  Workspace: multiscale_ws_bytes(g)
void multiscale_forward_crop(const GridDims& g, bool is3d, const void* packed, const float* x, float* p, int precision_mode,
                             void* ws, hipStream_t s, const int trim[4]);

// pieces of FluidNet.forward (lib/model.py:76-227)
size_t scale_std_scratch_bytes(int B);      // `partial` of launch_scale_std (fixed-order fp64 partial sums, no atomics)
void launch_scale_std(const GridDims& g, int nc, const float* U, float thr, double* partial,
                      float* scale /*B*/, hipStream_t s);
void launch_pack_input(const GridDims& g, int nc, const float* div, const float* flags, const float* scale, float* U,
                       float* x, hipStream_t s);
void launch_unscale(const GridDims& g, int nc, const float* scale, float* p, float* U, hipStream_t s);
void launch_gather_input(const GridDims& g, int nc, const float* input, float* U, float* flags, hipStream_t s);

// pieces of the CNN projection on a z-slab (fnx_slab_step with method 1; fnx_slab.hip)
size_t window_sums_scratch_bytes(int B);                       // `partial` of launch_window_sums_encode
// this rank's fp64 (sum, sumsq) of U over the planes [k0, k1) of every channel, as 3 floats per double in ITS slots of
// red[nranks][B][2][3] (all other slots zero): a float all-reduce(sum) over the ranks then is an exact all-gather
void launch_window_sums_encode(const GridDims& g, int nc, int k0, int k1, const float* U, int rank, int nranks, double* partial,
                               float* red, hipStream_t s);
// scale[b] = clamp(unbiased std over n elements, thr) from the gathered sums, added in rank order
void launch_scale_from_sums(int nranks, int B, double n, float thr, const float* red, float* scale, hipStream_t s);
// x[b,0] = div(U / scale[b]), x[b,1] = occupancy(flags) on the planes of g's compute window (U is not modified)
void launch_pack_div(const GridDims& g, bool is3d, const float* U, const float* flags, const float* scale, float* x, hipStream_t s);


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


// what the training unit uses of the forward's launchers (fnx_cnn.hip).  These hooks, and tape_layout, multiscale_forward_train,
// multiscale_backward and its workspace size below, take `is3d` and a grid {D, H, W}; 2D is D = 1 (one plane in every tensor).
// layer l of the net from x into y, exactly the launch the inference forward makes (launch_conv)
void conv_layer(int l, bool is3d, int mode, const float* packed, const float* x, float* y, int B, int D, int H, int W, hipStream_t s);
// float offsets of layer l's tap image and bias in the packed buffer
void packed_offsets(int l, bool is3d, size_t* taps, size_t* bias);
// the net's tower sizes: q, h = {D, H, W} at quarter and half resolution, the reference's int(n * 0.25) / int(n * 0.5) (D stays 1 in 2D)
void net_sizes(bool is3d, int D, int H, int W, int q[3], int h[3]);
// the resampling of multi_scale_net.py:119-125: x0 (B,C0,D0,H0,W0) and, if C1 > 0, x1 (B,C1,D1,H1,W1) -> channels [0, C0 + C1) of
// y (B,.,Do,Ho,Wo)
void resize(const float* x0, int C0, int D0, int H0, int W0, const float* x1, int C1, int D1, int H1, int W1, float* y, int B, int Do,
            int Ho, int Wo, hipStream_t s);
// The images of one Family::MFMA weight (3x3(x3), Cin % 16 == 0, Cout % 32 == 0) at float offset `off` of a buffer: what scalenet_pack
// writes for such a layer, for any weight tensor -- the backward's transposed, tap-flipped weights go through the forward's launchers.
struct MfmaImages { size_t taps, wino2, wino3, wbf, wino4, bias, end; bool wide; };
MfmaImages mfma_images(bool is3d, int cin, int cout, size_t off);
// w (Cout,Cin,(3,)3,3), bias (Cout) -> the images at base + im.*
void pack_mfma_images(bool is3d, const float* w, const float* bias, int cin, int cout, float* base, const MfmaImages& im, hipStream_t s);
// y = conv3x3(x3)(x, the packed weight) [+ ReLU] by launch_conv's mode rule; false: nothing launched (D * H * W beyond the MFMA kernels'
// range)
bool conv_mfma_images(bool is3d, const MfmaImages& im, const float* base, int cin, int cout, int relu, int mode, const float* x, float* y,
                      int B, int D, int H, int W, hipStream_t s);

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

struct FnxGrid;
struct FnxState;
namespace fnx {
// precision_mode (FNX_PRECISION_*) as the CNN launchers dispatch on it: FNX_PRECISION_FP32_F4 names what FNX_PRECISION_FP32 runs and
// becomes it; -1: no such mode.  The C ABI entry points map it once; everything below them takes the mapped value.
int net_mode(int precision_mode);
// FluidNet.forward around a net, whichever net it is (the ScaleNet, the bank nets and the two trainers call these).
// The scratch behind the flags copy, in this order, each region rounded up to 256 bytes: the divergence (the fused step keeps the net's p
// there), the net's input, scale_std's partial sums, the per-sample scales, `net_bytes` for the net's own workspace.  cells: D * H * W.
// base == nullptr: the sizes only.  head: the bytes in front of `scale`, all a training forward takes (its scales go to the caller).
// A whole-forward entry point puts its contiguous (B,1,..) copy of the flags channel, fluidnet_flags_bytes, in front of it.
struct FluidnetWs { float* div; float* x; double* partial; float* scale; void* net; size_t head, bytes; };
FluidnetWs fluidnet_ws_layout(int B, size_t cells, size_t net_bytes, void* base);
inline size_t fluidnet_flags_bytes(int B, size_t cells) { return al256((size_t)B * cells * 4); }
inline size_t fluidnet_whole_ws_bytes(int B, size_t cells, size_t net_bytes) {
  return fluidnet_flags_bytes(B, cells) + fluidnet_ws_layout(B, cells, net_bytes, nullptr).bytes;
}
// the channel split of model.py:104-119 (input -> U, flags), the launches of :125-168 in front of the net and those of :213-226 behind
// it.  The velocity components, 2 or 3, follow from g->is3D.
void fluidnet_split(const FnxGrid* g, const float* input, float* U, float* flags, void* stream);
int fluidnet_pre(const FnxGrid* g, float thr, float* U, const float* flags, float* scale, const FluidnetWs& w, void* stream);
int fluidnet_post(const FnxGrid* g, float* p, float* U, const float* flags, const float* scale, void* stream);
// The backward's scratch (the wall-masked scaled grad_U, the update's grad_U and grad_p, g_net, then the net's own workspace at `net`) and
// g_net = s grad_p + velocity_update_backward_p(s setWallBcs(grad_U)) (fnx_cnn_train.hip).  nc: 2 or 3 velocity components.
struct FluidnetTrainBwdWs { float *gU, *gU_in, *gp, *gnet; void* net; size_t bytes; };   // bytes: in front of `net`
FluidnetTrainBwdWs fluidnet_train_bwd_ws(int nc, const FnxGrid* g, void* base);
int fluidnet_train_gnet(int nc, const FnxGrid* g, const float* flags, const float* scale, const float* grad_p, const float* grad_U,
                        const FluidnetTrainBwdWs& w, void* stream);
// The net in the middle, by its kind (FNX_NET_SCALENET or FNX_NET_BANK, the 2D bank net; FNX_NET_BANK3D is not built into the step):
// `packed` is the image of that kind.  The bank unit exports its net for it (fnx_banknet.hip): the workspace of the net alone, its
// launches, and check_bank_call's refusals of a grid or a precision mode under the caller's name (no argument or workspace check).
size_t bank_net_ws_bytes(const FnxGrid* g);
void bank_net_forward(const FnxGrid* g, const void* packed, const float* x, float* p, void* ws, hipStream_t s);
int check_bank_grid(const char* fn, const FnxGrid* g, int precision_mode);
// what fluidnet_core and fluidnet_pressure take at `ws` for a net of this kind: fluidnet_ws_layout with the net's own workspace
size_t fluidnet_core_ws_bytes(const FnxGrid* g, int net_kind);
// the net's un-normalised pressure alone (model.py:125-175, :221-222) for the hybrid projection: p_out = scale * net(div(U) / scale, occupancy);
// U is read only.  ws: fluidnet_core_ws_bytes.
int fluidnet_pressure(const FnxGrid* g, const void* packed, int net_kind, const float* flags, float thr, int precision_mode, float* p_out,
                      const float* U, void* ws, void* stream);
// bcs != nullptr: the fused step's form -- the last setConstVals of the step (simulate.py:168) is part of the pass behind the
// net (bcs supplies density, the BC arrays, bc_class and density_bc_applied; p_out must not be the workspace)
int fluidnet_core(const FnxGrid* g, const void* packed, int net_kind, const float* flags, float thr, int precision_mode, float* p_out,
                  float* U, void* ws, void* stream, const FnxState* bcs = nullptr);
}
