// FluidNet.forward (lib/model.py:76-227) around a pressure net, whichever net it is -- internal interface of the glue (fnx_fluidnet.hip):
// the _ScaleNet std, the packing of the net's input, the un-normalisation, and the same pieces on a z-slab.
#pragma once
#include <hip/hip_runtime.h>
#include "fnx_device.h"

struct FnxGrid;
struct FnxState;
namespace fnx {
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
// fnx_fluidnet_forward's workspace: the above with the MultiScale net's own
size_t fluidnet_ws_bytes(const GridDims& g, bool is3d);
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
// The net in the middle, x (B,2,..) -> p (B,1,..), as the wrapper sees it.  Each unit defines its net's records next to its launchers:
// fnx_cnn.hip / fnx_cnn_train.hip the two ScaleNets, the four bank units theirs.  mode: net_mode's value (the bank nets have one
// arithmetic and ignore it).  status: the unit's wording of a HIP error after its launches.
struct Net {
  int ndim, kind;                                            // 2 or 3; FNX_NET_*
  int (*status)();
  size_t (*ws_bytes)(const FnxGrid* g);                      // the workspace of the net alone
  void (*forward)(const FnxGrid* g, const void* packed, const float* x, float* p, int mode, void* ws, hipStream_t s);
};
const Net& scalenet_net(bool is3d);   // fnx_cnn.hip
const Net& banknet_net();             // fnx_banknet.hip
const Net& banknet3d_net();           // fnx_banknet3d.hip
// kind: FNX_NET_SCALENET (either dimension), FNX_NET_BANK (2D) or FNX_NET_BANK3D (3D), as the caller has checked it
const Net& net_of(int kind, bool is3d);
// The net for training: the forward that keeps every layer's input in `tape`, the backward (false: a convolution was not launched, which
// the caller refuses; x: the net's input, for a net that reads it again) and the backward's workspace.  tape_x: the float offset inside
// the tape at which the net wants its input kept by the whole forward; nullptr: it does not.
struct NetTrain {
  int ndim;
  int (*status)();
  void (*forward)(const FnxGrid* g, const void* packed, const float* x, float* p, float* tape, int mode, hipStream_t s);
  bool (*backward)(const FnxGrid* g, const void* packed_t, const float* x, const float* grad_p, const float* tape, float* grad_blob, int mode,
                   void* ws, hipStream_t s);
  size_t (*backward_ws_bytes)(const FnxGrid* g);
  size_t (*tape_x)(const FnxGrid* g);
};
// FluidNet.forward around a net, everything behind an entry point's checks.  ws: fluidnet_whole_ws_bytes with the net's own (whole
// forward); fluidnet_train_ws_bytes, one size for the training forward and the backward.  fluidnet_backward: *launched = false where the
// net's backward was not launched (nothing is reported then: the entry point words the refusal).
int fluidnet_whole_forward(const Net& n, const FnxGrid* g, const void* packed, const float* input, float thr, float* p_out, float* U_out,
                           int mode, void* ws, void* stream);
size_t fluidnet_train_ws_bytes(const NetTrain& n, const FnxGrid* g);
int fluidnet_forward_train(const NetTrain& n, const FnxGrid* g, const void* packed, const float* input, float thr, float* p_out, float* U_out,
                           float* flags_out, float* scale_out, float* tape, int mode, void* ws, void* stream);
int fluidnet_backward(const NetTrain& n, const FnxGrid* g, const void* packed_t, const float* flags, const float* scale, const float* grad_p,
                      const float* grad_U, const float* tape, float* grad_blob, int mode, void* ws, void* stream, bool* launched);
// the bank net's refusals of a grid or a precision mode under the caller's name, for the step (check_bank_call without an argument or
// workspace check; fnx_banknet.hip)
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
}  // namespace fnx
