// What the two training units of the 16-channel bank net share (fnx_banknet_train.hip: 2D; fnx_banknet3d_train.hip: 3D): the tape's
// layout, the arithmetic of packed_t, the tail's partial sums and their place in the gradient blob, the launcher of the one tail
// backward kernel, and the checks of the training entry points over the net's record.  The forward and backward launchers, the
// level parts of the launch plans and every kernel but the tail's differ by algorithm and stay in their units.
#pragma once
#include "fnx_banknet3d_tile.h"
#include <stdio.h>

namespace fnx {

// fnx_banknet_train.hip: bank_tail_bwd_kernel (see there) over N flattened cells of a sample, for either dimension.  tail_t: the 1x1
// block of packed_t (W2T; W3T at + 256, WO at + 512, both images alike); tt, c2a, c2b, c3: the tape's entries; g_t (B,16,N) and
// partial [split][TAIL_P] are written.
void bank_tail_backward(const float* tail_t, const float* grad_p, const float* tt, const float* c2a, const float* c2b, const float* c3,
                        float* g_t, float* partial, int N, int ups, int nunits, int split, hipStream_t s);

namespace {

// ---- the tape: every ReLU output, contiguous (B,C,[d,]h,w) tensors; a2, a4 are the pooled relu(conv1) the coarser levels start from; x
// is the net's input, which only fnx_fluidnet_bank*_forward_train writes (it builds x itself; fnx_banknet*_backward is given x) ----
constexpr int N_BANK_TAPE = 14;
enum { TP_A, TP_H1, TP_B1, TP_A2, TP_H2, TP_B2, TP_A4, TP_H4, TP_B4, TP_T, TP_C2A, TP_C2B, TP_C3, TP_X };
struct BankTapeEntry { const char* name; size_t off; int C, D, H, W; };
struct BankTapeLayout { BankTapeEntry e[N_BANK_TAPE]; size_t floats; };
inline size_t al64(size_t x) { return (x + 63) & ~(size_t)63; }
inline BankTapeLayout bank_tape_layout(int ndim, int B, int D, int H, int W) {
  static const char* const names[N_BANK_TAPE] = {"a", "h1", "b1", "a2", "h2", "b2", "a4", "h4", "b4", "t", "c2a", "c2b", "c3", "x"};
  BankTapeLayout T{};
  size_t off = 0;
  for (int n = 0; n < N_BANK_TAPE; ++n) {
    const int R = n < TP_A2 || n >= TP_T ? 1 : (n < TP_A4 ? 2 : 4), C = n == TP_C3 ? 8 : (n == TP_X ? 2 : 16);
    const int d = ndim == 3 ? D / R : 1;
    T.e[n] = BankTapeEntry{names[n], off, C, d, H / R, W / R};
    off = al64(off + (size_t)B * C * d * (H / R) * (W / R));
  }
  T.floats = off;
  return T;
}
// into one of the two ABI structs (FnxTapeEntry has no D); either may be null
inline size_t bank_fill_tape(const BankTapeLayout& T, FnxTapeEntry* e2, FnxTapeEntry3D* e3) {
  for (int i = 0; i < N_BANK_TAPE; ++i) {
    const BankTapeEntry& t = T.e[i];
    if (e2) { snprintf(e2[i].name, sizeof(e2[i].name), "%s", t.name); e2[i].offset = t.off; e2[i].C = t.C; e2[i].H = t.H; e2[i].W = t.W; }
    if (e3) { snprintf(e3[i].name, sizeof(e3[i].name), "%s", t.name); e3[i].offset = t.off; e3[i].C = t.C; e3[i].D = t.D; e3[i].H = t.H; e3[i].W = t.W; }
  }
  return T.floats;
}

// ---- packed_t: what the backward reads of the weights (floats), for a bank convolution of `taps` taps (9 in 2D, 27 in 3D) ----
//   wb0t, wb2t  [tap][kc 4][lane 64] = W[cout = 4 kc + (lane >> 4)][cin = lane & 15][taps - 1 - tap]: the A operand of the transposed,
//               tap-flipped convolution in the forward kernel's order (block.0, block.2)
//   zero        16 zeros: its bias
//   w2t, w3t    [r 4][lane 64] = W[cout = 4 (lane >> 4) + r][cin = lane & 15]  (conv3: zero for cout >= 8)
//   wo          16: convOut's weight of input channel c, zero for c >= 8
struct BankPtOffsets { int wb0t, wb2t, zero, w2t, w3t, wo, floats; };
constexpr BankPtOffsets bank_pt_offsets(int taps) {
  return BankPtOffsets{0, 256 * taps, 512 * taps, 512 * taps + 16, 512 * taps + 272, 512 * taps + 528, 512 * taps + 544};
}
constexpr BankPtOffsets PT2 = bank_pt_offsets(9), PT3 = bank_pt_offsets(27);
constexpr int PT_WB0T = PT2.wb0t, PT_WB2T = PT2.wb2t, PT_ZERO = PT2.zero, PT_W2T = PT2.w2t, PT_W3T = PT2.w3t, PT_WO = PT2.wo,
              PT_FLOATS = PT2.floats;
constexpr int PT3_WB0T = PT3.wb0t, PT3_WB2T = PT3.wb2t, PT3_ZERO = PT3.zero, PT3_W2T = PT3.w2t, PT3_W3T = PT3.w3t, PT3_WO = PT3.wo,
              PT3_FLOATS = PT3.floats;
static_assert(PT_FLOATS == 5152 && PT3_FLOATS == 14368, "the sizes fnx_banknet*_packed_t_bytes has always answered");

// A pack kernel's body: element blockIdx.x * blockDim.x + threadIdx.x of the image, from the blob with block.0's weight at wb0, block.2's
// at wb2 and conv2's at w2 (conv3 and convOut follow conv2 at the 2D blob's distances in both blobs: bank_pack_tail).
__device__ __forceinline__ void bank_pack_t(const float* __restrict__ blob, float* __restrict__ pt, int taps, int wb0, int wb2, int w2) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int wb2t = 256 * taps, zero = 2 * wb2t, w2t = zero + 16, w3t = w2t + 256, wo = w3t + 256;
  if (i >= wo + 16) return;
  float v = 0.f;
  if (i < zero) {
    const int j = i % wb2t, src = i < wb2t ? wb0 : wb2;
    const int lane = j & 63, kc = (j >> 6) & 3, tap = j >> 8;
    v = blob[src + ((4 * kc + (lane >> 4)) * 16 + (lane & 15)) * taps + taps - 1 - tap];
  } else if (i >= w2t && i < wo) {
    const bool third = i >= w3t;
    const int j = i - (third ? w3t : w2t), lane = j & 63, r = j >> 6;
    const int cout = 4 * (lane >> 4) + r, cin = lane & 15;
    if (!third || cout < 8) v = blob[(third ? w2 + BLOB_W3 - BLOB_W2 : w2) + cout * 16 + cin];
  } else if (i >= wo && i - wo < 8) {
    v = blob[w2 + BLOB_WO - BLOB_W2 + i - wo];
  }
  pt[i] = v;
}

// ---- the tail's and conv1's launches: units of 64 flattened cells of a sample, strided over min(units, MAX_SPLIT) workgroups ----
constexpr int MAX_SPLIT = 512;            // workgroups of such a launch: two per CU of the largest part, a constant
constexpr int TAIL_P = 816;               // floats of a tail workgroup's partial sums: convOut [16][16] (row 0), conv3 [16][16] (rows 0..7),
                                          // conv2 [16][16]; then their biases, 16 each
inline int split_of(long items) { return items < MAX_SPLIT ? (int)items : MAX_SPLIT; }
struct BankUnits { int ups, nunits, split; };      // units per sample, in all (< 2^31: see the entry points' range checks), workgroups
inline BankUnits bank_units(int B, size_t cells) {
  BankUnits u{};
  u.ups = (int)((cells + 63) / 64);
  u.nunits = B * u.ups;
  u.split = split_of(u.nunits);
  return u;
}
// where a tail workgroup's partial sums hold element q2 of the gradient blob, q2 >= BLOB_W2 an index at the 2D blob's distances
__device__ __forceinline__ int bank_tail_partial_at(int q2) {
  int at;
  if (q2 < BLOB_B2) at = 512 + (q2 - BLOB_W2);
  else if (q2 < BLOB_W3) at = 800 + (q2 - BLOB_B2);
  else if (q2 < BLOB_B3) at = 256 + (q2 - BLOB_W3);
  else if (q2 < BLOB_WO) at = 784 + (q2 - BLOB_B3);
  else if (q2 < BLOB_BO) at = q2 - BLOB_WO;
  else at = 768;
  return at;
}

// ---- the training entry points: one body each, over the net's record (fnx_fluidnet.h's NetTrain) and the grids its unit answers for ----
struct BankTrainDim {
  const NetTrain& net;
  bool (*sized)(const FnxGrid*);           // the grids the size queries answer for (not null, the dimension's kind, at least 4 cells an axis)
  bool (*range_ok)(const FnxGrid*);        // the backward's own launch range behind check_bank_call's; nullptr: that one is all
};

// check_bank_call's want_of is a plain function: the backward's workspace, and the one size of the whole training forward and backward
template <const BankTrainDim& DIM>
size_t bank_bwd_ws(const FnxGrid* g) { return DIM.net.backward_ws_bytes(g); }
template <const BankTrainDim& DIM>
size_t bank_train_ws(const FnxGrid* g) { return fluidnet_train_ws_bytes(DIM.net, g); }
// a size query: 0 for a grid outside `sized` or the backward's range
template <const BankTrainDim& DIM>
size_t bank_size_query(const FnxGrid* g, size_t (*bytes_of)(const FnxGrid*)) {
  if (!DIM.sized(g) || (DIM.range_ok && !DIM.range_ok(g))) return 0;
  return bytes_of(g);
}

// check_bank_call and, behind it, the backward's own range
template <const BankTrainDim& DIM>
int check_bank_bwd_call(const char* fn, const FnxGrid* g, bool args, int precision_mode, size_t (*want_of)(const FnxGrid*), size_t ws_bytes) {
  if (DIM.range_ok && args && DIM.sized(g) && !DIM.range_ok(g))
    return set_error(FNX_EINVAL, "%s: B * D * H * W = %d * %zu cells is beyond the bank backward's launch range", fn, g->B,
                     (size_t)g->D * g->H * g->W);
  return check_bank_call(fn, DIM.net.ndim, g, args, precision_mode, want_of, ws_bytes);
}

template <const BankTrainDim& DIM>
int bank_forward_train(const char* fn, const FnxGrid* g, const void* packed, const float* x, float* p, float* tape, int precision_mode,
                       void* stream) {
  if (int rc = check_bank_call(fn, DIM.net.ndim, g, packed && x && p && tape, precision_mode, nullptr, 0)) return rc;
  DIM.net.forward(g, packed, x, p, tape, precision_mode, (hipStream_t)stream);
  return bank_status();
}

template <const BankTrainDim& DIM>
int bank_backward(const char* fn, const FnxGrid* g, const void* packed_t, const float* x, const float* grad_p, const float* tape,
                  float* grad_blob, int precision_mode, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_bank_bwd_call<DIM>(fn, g, packed_t && x && grad_p && tape && grad_blob && ws, precision_mode, bank_bwd_ws<DIM>, ws_bytes))
    return rc;
  DIM.net.backward(g, packed_t, x, grad_p, tape, grad_blob, precision_mode, ws, (hipStream_t)stream);
  return bank_status();
}

// FluidNet.forward for training with the bank net in the middle: the checks, then fnx_fluidnet.hip's bodies
template <const BankTrainDim& DIM>
int bank_whole_forward_train(const char* fn, const FnxGrid* g, const void* packed, const float* input, float normalize_threshold,
                             float* p_out, float* U_out, float* flags_out, float* scale_out, float* tape, int precision_mode, void* ws,
                             size_t ws_bytes, void* stream) {
  if (int rc = check_bank_bwd_call<DIM>(fn, g, packed && input && p_out && U_out && flags_out && scale_out && tape && ws, precision_mode,
                                        bank_train_ws<DIM>, ws_bytes))
    return rc;
  return fluidnet_forward_train(DIM.net, g, packed, input, normalize_threshold, p_out, U_out, flags_out, scale_out, tape, precision_mode, ws,
                                stream);
}

template <const BankTrainDim& DIM>
int bank_whole_backward(const char* fn, const FnxGrid* g, const void* packed_t, const float* flags, const float* scale, const float* grad_p,
                        const float* grad_U, const float* tape, float* grad_blob, int precision_mode, void* ws, size_t ws_bytes,
                        void* stream) {
  if (int rc = check_bank_bwd_call<DIM>(fn, g, packed_t && flags && scale && grad_p && grad_U && tape && grad_blob && ws, precision_mode,
                                        bank_train_ws<DIM>, ws_bytes))
    return rc;
  bool launched;
  return fluidnet_backward(DIM.net, g, packed_t, flags, scale, grad_p, grad_U, tape, grad_blob, precision_mode, ws, stream, &launched);
}

}  // namespace
}  // namespace fnx
