// What the host decides about a Jacobi call before it launches anything, as pure functions: no HIP call, the compute-unit count is an
// argument.  fnx_jacobi.hip launches by them, fnx_api.hip sizes workspaces and schedules solves by them, and a host-only program can
// include this file alone: it needs nothing but a GridDims with the fields B, D, H, W, HW, DHW declared before it (fnx_device.h).
#pragma once
#include <stddef.h>

namespace fnx {
// ---- the launch schedule of a run of sweeps ---------------------------------------------------------------------------------------
constexpr int KMAX_2D = 8, KLARGE_2D = 10, KDEEP_2D = 28;
// 64 x 64 tiles with an output window of (64 - 2K)^2: how many a launch of K sweeps needs
inline long tiles_2d(const GridDims& g, int K) {
  const int o = 64 - 2 * K;
  return (long)((g.W + o - 1) / o) * ((g.H + o - 1) / o) * g.B;
}

// 2D: the most sweeps one launch runs when the solve has `total` (>= 1) to run
inline int jacobi_max_sweeps_per_launch(const GridDims& g, bool is3d, int total, int cus) {
  if (is3d || g.D != 1) return 1;

  // Small grids are launch-latency bound (a launch costs ~5 us + ~0.35 us per sweep whatever the halo does to the work, as
  // long as every tile has a CU to itself): the fewest launches whose tiles all run at once, the sweeps dealt evenly.
  if (total > KMAX_2D) {
    int kcap = 0;
    for (int K = KDEEP_2D; K > KMAX_2D; --K) if (tiles_2d(g, K) <= cus) { kcap = K; break; }
    if (kcap) {
      const int nl = (total + kcap - 1) / kcap;
      return (total + nl - 1) / nl;
    }
  }
  // a wave's chain per sweep is its 8 rows whatever K, so the halo (2K of the 64 columns and rows of a tile) is what limits K:
  // 7 where launches are still short (28 sweeps = 4 launches); on large grids at most 10, the sweeps dealt evenly over the
  // launches (measured at 2048^2 x 100 sweeps, ms per step: 13 launches of <= 8 0.584, 12 of <= 9 0.607, 10 of 10 0.574, 9 of <= 12
  // 0.615, 8 of <= 14 0.630)
  if ((long)g.W * g.H * g.B <= (2l << 20)) return 7;
  const int nl = (total + KLARGE_2D - 1) / KLARGE_2D;
  const int k = (total + nl - 1) / nl;
  return k < 1 ? 1 : k;
}

constexpr int Z2R = 4, Z2NW = 1, Z2WPS = 4;   // the two-sweep march: rows a wave, waves a workgroup, waves per SIMD of its register budget
// can the two-sweep passes of this grid hand each other p in the row-quad layout (`lay`: bit 0 = p_in, bit 1 = p_out is in it)?
inline bool jacobi3d_quad_ok(const GridDims& g) { return g.H % 4 == 0 && Z2R == 4 && Z2NW == 1; }

// `total` sweeps as launches of at most kmax: 2 in 3D (the two-sweep march; an odd remainder is one single-sweep pass), else
// jacobi_max_sweeps_per_launch, taken once from the total.  Launch l runs min(what is left, kmax) sweeps.  3D: consecutive two-sweep
// passes hand each other p in the row-quad layout (fewer, wider vector-memory instructions); the last of them writes rows.
struct JacobiLaunch { int sweeps, lay; };
struct JacobiSchedule {
  int n, kmax, total; bool quad;           // n launches
  int sweeps(int l) const { const int left = total - l * kmax; return left < kmax ? left : kmax; }
  // launch l writes the row-quad layout: it and the next are both two-sweep passes
  bool out_quad(int l) const { return quad && l >= 0 && l + 1 < n && sweeps(l) == 2 && sweeps(l + 1) == 2; }
  JacobiLaunch at(int l) const { return {sweeps(l), (out_quad(l - 1) ? 1 : 0) | (out_quad(l) ? 2 : 0)}; }
};
inline JacobiSchedule jacobi_schedule(const GridDims& g, bool is3d, int nsweeps, int cus) {
  JacobiSchedule s{0, 1, nsweeps > 0 ? nsweeps : 0, is3d && jacobi3d_quad_ok(g)};
  if (s.total == 0) return s;              // (the solve of one sweep whose caller wants the residual fuses none)
  s.kmax = is3d ? 2 : jacobi_max_sweeps_per_launch(g, false, s.total, cus);
  s.n = s.total / s.kmax + (s.total % s.kmax != 0);
  return s;
}
constexpr int JACOBI_MAX_LAUNCHES = 1022;  // of one fnx_jacobi call
// The launches ping-pong between two buffers, launch l writing buffer (first + l) & 1.  A solve numbers them 0 = p, 1 = the
// workspace's, and starts so that its last launch -- the extra single sweep of a caller who wants the residual included -- writes p.
inline int jacobi_solve_first_buffer(const JacobiSchedule& s, bool residual) { return (s.n + (residual ? 1 : 0) - 1) & 1; }

// ---- the 3D two-sweep march.  Its tiles: 60 output columns (a wave's lanes 2..61) by Z2NW * Z2R rows; ntiles over all samples; kwords = 32-plane words of a tile's
// "same as the plane below" bits
struct Jacobi3dTiles { int nxt, nyt; long ntiles; int kwords; };
inline Jacobi3dTiles jacobi3d_tiles(const GridDims& g) {
  const int nxt = (g.W + 59) / 60, nyt = (g.H + Z2NW * Z2R - 1) / (Z2NW * Z2R);
  return {nxt, nyt, (long)nxt * nyt * g.B, (g.D + 31) / 32};
}
inline int jacobi3d_wave_slots(int cus) { return (Z2WPS * 4 / Z2NW) * cus; }   // resident waves: Z2WPS per SIMD (<= 128 VGPRs each)
// a segment of np planes and the planes around it that it reads stay inside the march's 32-bit buffer offsets
inline bool jacobi3d_offsets_fit(const GridDims& g, int np) { return (size_t)(np + 4) * g.HW < 0x3fffffffu; }

// The mask allocation of the 3D launches: B*D*H*W neighbour-mask bytes (`rows`), the same bytes in row groups of four (`quads`), one
// "same as the plane below" bit per (sample, tile, plane), 32 planes to a word (`same`); each rounded up to 256 bytes.  base == nullptr: the size.
struct JacobiMaskLayout { unsigned char* rows; unsigned* quads; unsigned* same; size_t bytes; };
inline JacobiMaskLayout jacobi3d_mask_layout(const GridDims& g, void* base) {
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  auto at = [&](size_t off) { return base ? (char*)base + off : nullptr; };
  const Jacobi3dTiles t = jacobi3d_tiles(g);
  const size_t quads = al((size_t)g.B * g.DHW), same = al(quads + (size_t)g.B * g.D * ((g.H + 3) / 4) * g.W * 4);
  return {(unsigned char*)at(0), (unsigned*)at(quads), (unsigned*)at(same), al(same + (size_t)t.ntiles * t.kwords * 4)};
}

// One two-sweep launch over np output planes (of one plane range, or of each of two ranges of np planes).
struct Jacobi3dX2Plan {
  int zchunk;        // planes a wave marches; 0 with `split`
  bool split;        // more tiles than wave slots: the (tile, plane) space is dealt evenly over G workgroups (the kernel's SPLIT)
  long long G;       // workgroups of a launch
  bool serial;       // two plane ranges that do not fit one resident set: two launches of this plan, one range each
  int lay;           // the layout the kernel runs with: a launch from zero reads no input, so bit 0 is dropped
};
inline Jacobi3dX2Plan jacobi3d_x2_plan(const GridDims& g, int np, bool two_ranges, bool from_zero, int lay, int cus) {
  // Smallest plane chunk.  Every (tile, chunk) wave is resident at once, so a launch lasts (chunk + 2 lead-in steps) x
  // the per-step time of one wave, whatever the occupancy: small plane ranges (the slab driver's edge parts, small
  // grids) are cut as finely as the wave slots allow (measured 20 -> 14 us for 14 planes of 512^2).
  constexpr int zmin = 2;
  const long slots = jacobi3d_wave_slots(cus), ntiles = jacobi3d_tiles(g).ntiles;
  Jacobi3dX2Plan p{};
  p.lay = from_zero ? lay & 2 : lay;
  // as many equal plane chunks per tile as fit one resident set, which two plane ranges share
  int nzc = (int)(slots / ntiles);
  if (two_ranges) nzc /= 2;
  if (nzc < 1) nzc = 1;
  p.zchunk = (np + nzc - 1) / nzc;
  if (p.zchunk < zmin) p.zchunk = zmin;
  // more tiles than slots: an even split of the (tile, plane) space -- unless a segment's 32-bit offsets would pass 4 GB
  if (ntiles > slots) p.zchunk = jacobi3d_offsets_fit(g, np) ? 0 : 64;
  p.split = p.zchunk == 0;
  if (two_ranges && (p.split || 2 * ntiles > slots)) {     // no room for both ranges at once: one after the other
    p = jacobi3d_x2_plan(g, np, false, from_zero, lay, cus);
    p.serial = true;
    return p;
  }
  if (!p.split) {
    p.G = (long long)ntiles * ((np + p.zchunk - 1) / p.zchunk) * (two_ranges ? 2 : 1);
    p.G = ((p.G + 7) / 8) * 8;
  } else {
    p.G = (long long)ntiles * np / 8;
    if (p.G > slots) p.G = slots;
    p.G = (p.G / 8) * 8;
    if (p.G < 8) p.G = 8;
  }
  return p;
}
// ---- the 64-column tiling of the two-sweep march (the kernel's X64): a workgroup is the ceil(W / 64) waves of one (row group, plane
// chunk), which hand each other their edge columns through LDS instead of recomputing a two-column halo a side.
constexpr int X64_MAXW = 8;                // waves a workgroup: W <= 512 (wider rows keep the 60-column tiles)
enum { JACOBI3D_X_AUTO = 0, JACOBI3D_X_60 = 1, JACOBI3D_X_64 = 2 };   // the request: FnxGrid.ref_quirks bits 8-9 force a tiling (A/B timing, tests)
inline int jacobi3d_x64_waves(const GridDims& g) { return (g.W + 63) / 64; }
// whole workgroups resident at once: a compute unit holds Z2WPS * 4 waves of the march, i.e. floor(16 / nw) workgroups of nw waves
// (5 of 3 waves, not 16 / 3: measured at 192^3, where the 64 workgroups that did not fit cost the pass 10 %)
inline long jacobi3d_x64_slots(int nw, int cus) { return (long)(Z2WPS * 4 / nw) * cus; }
// can the 64-column kernel run this launch at all?  Whole-domain passes of one plane range without a mirror, H % 4 == 0, at most
// X64_MAXW waves a row, and every row group with a workgroup in one resident set.
inline bool jacobi3d_x64_ok(const GridDims& g, int np, bool two_ranges, bool mirror, int cus) {
  if (two_ranges || mirror || np != g.D || g.H % 4 != 0 || !jacobi3d_quad_ok(g)) return false;
  const int nw = jacobi3d_x64_waves(g);
  if (nw > X64_MAXW || !jacobi3d_offsets_fit(g, np)) return false;
  return (long)(g.H / 4) * g.B <= jacobi3d_x64_slots(nw, cus);
}
// its launch: `nw` waves a workgroup, G workgroups (a multiple of 8), each marching `zchunk` planes of one row group; the chunk
// count is what one resident set holds of the (fewer) waves.  Call only where jacobi3d_x64_ok.
struct Jacobi3dX64Plan { int nw, zchunk; long long G; int lay; };
inline Jacobi3dX64Plan jacobi3d_x64_plan(const GridDims& g, int np, bool from_zero, int lay, int cus) {
  constexpr int zmin = 2;
  Jacobi3dX64Plan p{};
  p.nw = jacobi3d_x64_waves(g);
  p.lay = from_zero ? lay & 2 : lay;
  const long groups = (long)(g.H / 4) * g.B;
  int nzc = (int)(jacobi3d_x64_slots(p.nw, cus) / groups);
  if (nzc < 1) nzc = 1;
  p.zchunk = (np + nzc - 1) / nzc;
  if (p.zchunk < zmin) p.zchunk = zmin;
  p.G = groups * ((np + p.zchunk - 1) / p.zchunk);
  p.G = ((p.G + 7) / 8) * 8;
  return p;
}
// THE rule: which tiling a two-sweep launch runs with.  Every wave of either launch is resident and marches its chunk plus two
// lead-in steps, so a pass costs (waves x steps) wave-steps at a rate the tiling sets.  The hand-over (a barrier a step, one more
// VALU instruction per obstacle-free row update) lowers that rate by 13 to 19 % (docs/history/r34_jacobi_x64.md), so the 64-column
// tiling is taken where it issues at least X64_MARGIN_PCT per cent fewer wave-steps -- 256^3: 4096 x 18 against 3840 x 24, 20 %;
// 128 wide: about 29 % -- and its chunks are at least X64_MIN_CHUNK planes: shorter ones are lead-in and launch latency (a tie).
constexpr int X64_MARGIN_PCT = 19, X64_MIN_CHUNK = 8;
inline bool jacobi3d_x64_pick(const GridDims& g, int np, bool two_ranges, bool mirror, int request, int cus) {
  if (request == JACOBI3D_X_60 || !jacobi3d_x64_ok(g, np, two_ranges, mirror, cus)) return false;
  if (request == JACOBI3D_X_64) return true;
  const Jacobi3dX2Plan a = jacobi3d_x2_plan(g, np, false, false, 0, cus);
  if (a.split) return false;                               // (the 60-column tiles overflow the wave slots, e.g. 2048 x 512: unmeasured, left alone)
  const Jacobi3dX64Plan b = jacobi3d_x64_plan(g, np, false, 0, cus);
  if (b.zchunk < X64_MIN_CHUNK) return false;
  const long long w60 = jacobi3d_tiles(g).ntiles * ((np + a.zchunk - 1) / a.zchunk) * (a.zchunk + 2);
  const long long w64 = (long long)(g.H / 4) * g.B * ((np + b.zchunk - 1) / b.zchunk) * b.nw * (b.zchunk + 2);
  return w64 * 100 <= w60 * (100 - X64_MARGIN_PCT);
}

// may a two-sweep launch of these plane ranges mirror its output (launch_jacobi3d_x2's `mirror`)?  One resident set of waves, both
// arrays in the same layout, not the from-zero pass
inline bool jacobi3d_mirror_ok(const GridDims& g, int np, bool two_ranges, bool from_zero, int lay, int cus) {
  if (from_zero || (lay != 0 && lay != 3) || np < 1) return false;
  const Jacobi3dX2Plan p = jacobi3d_x2_plan(g, np, two_ranges, false, lay, cus);
  return !p.serial && !p.split && jacobi3d_offsets_fit(g, np);
}

}  // namespace fnx
