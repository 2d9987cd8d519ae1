// The 3D step glue's stage word: what stage3d_kernel and post_projection_kernel<true, .> read of `flags` and of the BC class map at a
// cell and its six neighbours, folded into one uint32 per cell.  Both are functions of `flags` and of the BC arrays alone, so where the
// caller promises those static (FnxStepParams.static_flags) the word is built once (stage_word_kernel, fnx_step.hip) and the two passes
// load it instead of seven flags and seven class bytes.  Pure functions, no HIP call: the kernels and a host-only program share them.
//
//   bits  0- 1   flag code of the cell                     codes: 1 = fluid, 2 = obstacle, 3 = empty, 0 = any other value (NaN included).
//   bits  2- 7   flag codes of the -1 neighbours x, y, z   The stage sequence, addGravity's condition, the wall BCs, the divergence and the
//   bits  8-13   flag codes of the +1 neighbours x, y, z   velocity update compare flags for equality with these three constants only.
//   bits 14-15   the cell's class byte (bit 0: velocity BCs are the identity, bit 1: density)
//   bits 16-18   bit 1 of the class of the -1 neighbours x, y, z
//   bits 19-21   "class == 3" of the +1 neighbours x, y, z
// Neighbours are those of the local array (a z-slab's or a whole domain's), by the kernels' convention: a -1 neighbour that does not exist is
// the cell itself; a +1 neighbour that does not exist is never used and is the cell itself here as well (what the float kernels load).
#pragma once
#include <stddef.h>

#include "../../include/fluidnet_hip.h"

#if defined(__HIPCC__)
#define FNX_WORD_FN __host__ __device__ inline
#else
#define FNX_WORD_FN inline
#endif

namespace fnx {

enum : unsigned { FLAG_CODE_OTHER = 0, FLAG_CODE_FLUID = 1, FLAG_CODE_OBST = 2, FLAG_CODE_EMPTY = 3 };

FNX_WORD_FN unsigned stage_flag_code(float f) {
  return f == (float)FNX_TYPE_FLUID ? FLAG_CODE_FLUID : f == (float)FNX_TYPE_OBSTACLE ? FLAG_CODE_OBST : f == (float)FNX_TYPE_EMPTY ? FLAG_CODE_EMPTY : FLAG_CODE_OTHER;
}

// What the stages compare a flag with, as a value and as a code: the kernels are written once over either (`f == FlagConst<F>::fluid`).
// (Constants and not predicate functions: through functions the float instances of the kernels came out with other branches.)
template <class F> struct FlagConst;
template <> struct FlagConst<float> { static constexpr float fluid = (float)FNX_TYPE_FLUID, obst = (float)FNX_TYPE_OBSTACLE, empty = (float)FNX_TYPE_EMPTY; };
template <> struct FlagConst<unsigned> { static constexpr unsigned fluid = FLAG_CODE_FLUID, obst = FLAG_CODE_OBST, empty = FLAG_CODE_EMPTY; };

// element offsets of the -1 neighbours (subtracted) and of the +1 neighbours (added) of cell (i, j, k) in a (D, H, W) array; 0: none
FNX_WORD_FN void stage_word_offsets(int i, int j, int k, int W, int H, int D, int* minus, int* plus) {
  const int HW = H * W;
  minus[0] = i > 0 ? 1 : 0; minus[1] = j > 0 ? W : 0; minus[2] = k > 0 ? HW : 0;
  plus[0] = i + 1 < W ? 1 : 0; plus[1] = j + 1 < H ? W : 0; plus[2] = k + 1 < D ? HW : 0;
}

// from the values themselves: fc / fm / fp the flags of the cell, its -1 and its +1 neighbours, cc / cm / cp their class bytes
FNX_WORD_FN unsigned stage_word_encode(float fc, const float* fm, const float* fp, unsigned cc, const unsigned* cm, const unsigned* cp) {
  unsigned w = stage_flag_code(fc) | ((cc & 3u) << 14);
  for (int a = 0; a < 3; ++a) {
    w |= stage_flag_code(fm[a]) << (2 + 2 * a);
    w |= stage_flag_code(fp[a]) << (8 + 2 * a);
    w |= ((cm[a] >> 1) & 1u) << (16 + a);
    w |= (cp[a] == 3u ? 1u : 0u) << (19 + a);
  }
  return w;
}

// the word of cell (i, j, k) of one sample: `flags` and `cls` are that sample's (D, H, W) arrays
FNX_WORD_FN unsigned stage_word_at(const float* flags, const unsigned char* cls, int W, int H, int D, int i, int j, int k) {
  int om[3], op[3];
  stage_word_offsets(i, j, k, W, H, D, om, op);
  const size_t o = ((size_t)k * H + j) * W + i;
  float fm[3], fp[3];
  unsigned cm[3], cp[3];
  for (int a = 0; a < 3; ++a) { fm[a] = flags[o - om[a]]; fp[a] = flags[o + op[a]]; cm[a] = cls[o - om[a]]; cp[a] = cls[o + op[a]]; }
  return stage_word_encode(flags[o], fm, fp, cls[o], cm, cp);
}

FNX_WORD_FN unsigned stage_word_cell(unsigned w) { return w & 3u; }
FNX_WORD_FN unsigned stage_word_minus(unsigned w, int a) { return (w >> (2 + 2 * a)) & 3u; }
FNX_WORD_FN unsigned stage_word_plus(unsigned w, int a) { return (w >> (8 + 2 * a)) & 3u; }
FNX_WORD_FN unsigned stage_word_class(unsigned w) { return (w >> 14) & 3u; }
// The stage's test for "this cell needs no BC entry": its class is 3, its -1 neighbours' densities are identity cells and, where the
// divergence re-derives the +1 neighbours (with_plus), those are of class 3 too.
FNX_WORD_FN bool stage_word_ident(unsigned w, bool with_plus) {
  const unsigned need = (3u << 14) | (7u << 16) | (with_plus ? 7u << 19 : 0u);
  return (w & need) == need;
}

}  // namespace fnx
