// 3x3(x3) convolution in the Winograd F(2x2, 3x3) domain, exact fp32 on v_mfma_f32_32x32x2_f32, and the two pack kernels of its weight
// images (included by fnx_cnn.hip inside its anonymous namespace, after its DMA helpers and ConvArgs).
// ---------------------------------------------------------------------------------------------------
// 3x3(x3) convolution in the Winograd domain, F(2x2, 3x3), fp32 on v_mfma_f32_32x32x2_f32:
//   Y = A^T [ sum_cin (G g G^T) . (B^T d B) ] A      (Lavin & Gray; d = 4x4 input patch of a 2x2 output block)
// 16 multiplies per 4 outputs instead of 36: the contraction over input channels becomes 16 independent GEMMs (one per
// position p of the 4x4 transform domain)
//   D_p[cout 32][block 32] += Wt_p[cout][k] * Xt_p[k][block],   k = two consecutive input channels
//   raw halo tile  global -> registers (fetched three stages ahead) -> LDS at the start of the next phase
//                  (8-wave variant: global -> LDS by DMA into a ring of four copies, HDMA below)
//   B^T d B        per (channel, block) half patch by all threads, LDS -> LDS [position pair][c][block][2]
//   G g G^T        precomputed at pack time; the stage's slice goes global -> LDS by buffer_load_dwordx4 ... lds (DMA, one stage ahead)
// and the epilogue applies A^T . A per output channel register, adds the bias, clamps (ReLU) and stores pixel pairs.
// The 16 positions of a (32 output channels x 32 blocks) tile are split over TWO waves (8 positions = 128 accumulator
// registers each), so that a wave fits a 256-register budget and two waves share a SIMD: while one is between its barriers
// the other one's MFMAs keep the matrix cores busy (all 16 positions in one 512-register wave, one wave per SIMD, exposes
// every such gap: measured 2.78 vs 2.42 ms per 1024^2 forward).  Workgroup = 2 position halves x NCG output-channel groups
// x NPG pixel groups stacked in y (4 or 8 waves); stage = 4 input channels.  Each wave ends with partial outputs (A^T . A
// is linear in the positions); the two halves swap half of their 16 output-channel registers through LDS and each finishes
// (bias, ReLU, store) its own 8.
// Numerics: not the summation order of a direct convolution; the transforms are exact in binary up to the roundings of
// their additions (measured against the CPU oracle: max |d| 7.1e-8 at |ref| <= 7.7e-2, the direct kernel 7.5e-8;
// tools/cnn_error_probe.py, tests/test_parity_gpu.py::test_cnn_winograd_layers_vs_oracle).  FNX_PRECISION_FP32_DIRECT
// (fnx_multiscale_forward's precision_mode) keeps every layer on the direct kernels instead.
// The kernel is a PERSISTENT software pipeline (the round-1 kernel serialised every stage -- halo tile -> LDS, barrier,
// transform, barrier, operand reads, MFMAs -- and paid a full prologue and epilogue per 256-pixel tile: time = rounds x
// (5.5 us + stages x 1.31 us) against 0.91 us of MFMA work per stage, 47 % of the MFMA peak at 1024^2):
//  * every LDS image has two copies and a phase has ONE barrier.  Between two barriers a wave issues
//      registers -> LDS      halo tile of stage s+2, fetched during the phase before (into the copy the transform of stage s read
//                            one phase ago), then
//      global -> registers   halo tile of stage s+3          (it has until this point of the NEXT phase to land; the barrier
//                            in between waits for vmcnt(NLD): these loads stay in flight, the weight DMA issued before them lands)
//      global -> LDS (DMA)   transformed weights of stage s+1
//      LDS -> LDS            input transform of stage s+1 (halo tile s+1 -> xt[s+1]) in the gaps of the MFMA stream
//      16 MFMAs              second k-step of stage s-1, then first k-step of stage s: the stream is rotated by half a
//                            stage against the barriers and each k-step's operands are read half a phase before its
//                            MFMAs, so a wave leaves a barrier with its next 8 MFMAs' operands already in registers
//  * a workgroup walks over tiles (tile = blockIdx.x, += gridDim.x) and the three streams -- halo fetch (three stages ahead),
//    weights + transform (one ahead), MFMAs -- each carry their own tile: the fetches run on into the next tile while the
//    MFMAs finish the current one, so only the first tile of a workgroup pays a prologue.  Between tiles: the last
//    k-step, the output transform + half-exchange (its own LDS buffer: the xt copies already hold the next tile), stores.
//  * the transform work is dealt out in half patches (two of the four rows of B^T d B: 4 ds_read2_b64, 4 xor, 16 adds,
//    4 ds_write2) so that all threads carry the same share, with no per-lane selects.
//  * the transformed weights a workgroup DMAs per stage are one contiguous 16*4*RW-float block (repack_wino3_kernel).
// ---------------------------------------------------------------------------------------------------
// Output stores carry the non-temporal hint (the next layer reads them after this launch is through; measured 2.345 ->
// 2.312 ms per 1024^2 forward).  The same hint on the halo fetch (aux = 2) measured 4 % SLOWER.  Neither changes the
// L2 picture (PMC: 10.8 M hits / 7.9 M misses per launch): the streamed activations flush an XCD's 4 MB L2 about once per
// tile period, so about half of the transformed-weight reads miss it and are served by the Infinity Cache -- that, not
// HBM, is the "traffic beyond the activations" FETCH_SIZE shows for these launches (it counts Infinity-Cache hits).
#define W3_ST(p, v) do { const float2 v_ = (v); __builtin_nontemporal_store((f32x2){v_.x, v_.y}, (f32x2*)(p)); } while (0)
#ifndef W3_ABL
#define W3_ABL 0
#endif
constexpr int WCOLS = 34;                              // halo tile row: 32 pixels + halo
constexpr int W3C = 4;                                 // input channels per stage of conv3_wino3_kernel
inline int wino3_rw(int cout) { return cout % 64 == 0 ? 64 : 32; }   // its output channels per workgroup
template <int NCG, int NPG, bool IS3D = false>
__global__ __launch_bounds__(128 * NCG * NPG, 2) void conv3_wino3_kernel(ConvArgs a, const float* __restrict__ wt, int ntx,
                                                                         int nty, int ntiles) {
  constexpr int C = W3C;
  constexpr int NWV = 2 * NCG * NPG, NT = 64 * NWV;
  constexpr int ROWS = 4 * NPG + 2;
  constexpr int NB = 32 * NPG;
  constexpr int RW = 32 * NCG;
  constexpr int WROWS = 16 * C;
  constexpr int WD = NCG * NPG == 4 ? 2 : 1;             // stages the weight DMA runs ahead (two 4-wave workgroups per CU: no room for four copies)
  constexpr int NWI = WROWS * RW / 256, NDMA = NWI / NWV;       // 1-KiB DMA instructions per stage / per wave
  constexpr int NEL = C * ROWS * WCOLS, NLD = (NEL + NT - 1) / NT;
  constexpr int NUNIT = 2 * C * NB, UPT = NUNIT / NT;          // half patches per stage / per thread
  static_assert(NUNIT % NT == 0 && (C * NB) % 64 == 0, "half patches must deal out evenly, wave-uniform in the half");
  static_assert(NWI % NWV == 0 && UPT <= 4, "stage shape");
  // HDMA (the 8-wave variant: one workgroup per CU has the LDS): the halo tile goes global -> LDS by DMA into a ring of four copies;
  // the 4-wave variants (two workgroups per CU, 80 KB each) take it through registers into two
  constexpr bool HDMA = NCG * NPG == 4;
  constexpr int RAWN = HDMA ? NLD * NT : NEL;            // (DMA: the lanes of the last instruction beyond the tile land in the padding)
  __shared__ __attribute__((aligned(16))) float raw0[RAWN];
  __shared__ __attribute__((aligned(16))) float raw1[RAWN];
  __shared__ __attribute__((aligned(16))) float raw2[HDMA ? RAWN : 4];
  __shared__ __attribute__((aligned(16))) float raw3[HDMA ? RAWN : 4];
  __shared__ __attribute__((aligned(16))) float xt0[16 * C * NB];
  __shared__ __attribute__((aligned(16))) float xt1[16 * C * NB];
  __shared__ __attribute__((aligned(16))) float wbuf0[WROWS * RW];
  __shared__ __attribute__((aligned(16))) float wbuf1[WROWS * RW];
  __shared__ __attribute__((aligned(16))) float wbuf2[WD == 2 ? WROWS * RW : 4];
  __shared__ __attribute__((aligned(16))) float wbuf3[WD == 2 ? WROWS * RW : 4];
  __shared__ __attribute__((aligned(16))) float exch[NWV * 16 * 64];   // epilogue: 4 registers x 4 outputs x 64 lanes per wave
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int half = lane >> 5, l31 = lane & 31;
  const int h = wave & 1, g = wave >> 1;
  const int cg = g % NCG, pg = g / NCG;
  const int ngrp = a.cout / RW, nchunk = a.cin / C;
  const size_t plane = (size_t)a.H * a.W, vol = plane * a.D;
  const unsigned stage_bytes = (unsigned)((size_t)C * vol * 4 - 1) + 1u;
  const int tstep = gridDim.x;
  const float relu_lo = a.relu ? 0.f : -__builtin_inff();   // max(v, -inf) == v: the ReLU without a select per value

  // Tiles are numbered x fastest, then y, output-channel group, z, sample.  A workgroup's tiles are blockIdx.x + k*gridDim.x:
  // the tile's digits are advanced by the digits of the step with carries (one integer division chain per workgroup, not
  // three per tile: scalar division is a ~30-instruction dependent chain).
  struct Tile { int tx, ty, grp, z, b; };
  auto decode = [&](int t) __attribute__((always_inline)) {
    Tile T;
    T.tx = t % ntx; t /= ntx;
    T.ty = t % nty; t /= nty;
    T.grp = t % ngrp; t /= ngrp;
    T.z = t % a.D; T.b = t / a.D;
    return T;
  };
  const Tile T0 = decode(blockIdx.x), TS = decode(tstep);
  auto next_tile = [&](Tile T) __attribute__((always_inline)) {
    int c;
    T.tx += TS.tx;        c = T.tx >= ntx;   T.tx -= c ? ntx : 0;
    T.ty += TS.ty + c;    c = T.ty >= nty;   T.ty -= c ? nty : 0;
    T.grp += TS.grp + c;  c = T.grp >= ngrp; T.grp -= c ? ngrp : 0;
    T.z += TS.z + c;      c = T.z >= a.D;    T.z -= c ? a.D : 0;
    T.b += TS.b + c;
    return T;
  };
  auto dz_lo_of = [&](const Tile& T) __attribute__((always_inline)) { return IS3D && T.z == 0 ? 1 : 0; };
  auto dz_hi_of = [&](const Tile& T) __attribute__((always_inline)) { return IS3D ? (T.z == a.D - 1 ? 2 : 3) : 1; };

  // ---- halo-fetch stream (three stages ahead of the MFMAs): its tile is (xR, rz), cursor (rdz, rc0) ----
  const float* xR;                                      // sample base of the stream's tile
  int rz, rdz, rc0 = 0;
  // per-thread slots of the [C][ROWS][34] halo tile: the tile-independent part of the byte offset and (row, col); a slot
  // outside the image gets an out-of-range offset (the buffer load then returns 0)
  unsigned uoff[NLD], ubase[NLD], urc[NLD];
#pragma unroll
  for (int t = 0; t < NLD; ++t) {
    const int idx = threadIdx.x + NT * t;
    const int cc = idx / (ROWS * WCOLS);
    const int rem = idx - cc * ROWS * WCOLS;
    const int row = rem / WCOLS, col = rem - row * WCOLS;
    ubase[t] = (unsigned)(((size_t)cc * vol + (size_t)row * a.W + col) * 4);
    urc[t] = idx < NEL ? (unsigned)(row << 16 | col) : 0xffffffffu;
  }
  auto enter_R = [&](const Tile& T) __attribute__((always_inline)) {
    xR = a.x + (size_t)T.b * a.cin * vol; rz = T.z; rdz = dz_lo_of(T); rc0 = 0;
    const int tx0 = T.tx * 32, ty0 = T.ty * (4 * NPG);
    const unsigned toff = (unsigned)(((size_t)(ty0 - 1) * a.W + (tx0 - 1)) * 4);      // (wraps for the first row/column: those slots are out of the image)
#pragma unroll
    for (int t = 0; t < NLD; ++t) {
      const int gx = tx0 - 1 + (int)(urc[t] & 0xffff), gy = ty0 - 1 + (int)(urc[t] >> 16);
      const bool ok = (gx >= 0) & (gx < a.W) & (gy >= 0) & (gy < a.H);
      uoff[t] = ok ? ubase[t] + toff : 0xfffffff0u;
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  enter_R(T0);
  float stage[NLD];
  // HDMA: straight into `rawdst` (buffer_load_dword ... lds: 64 consecutive floats per wave instruction, zeros for the out-of-range
  // offsets) -- no registers, no LDS store, and nothing waits for it before the barrier of the NEXT phase
  auto prefetch = [&](float* rawdst = nullptr) __attribute__((always_inline)) {
    const int zz = IS3D ? rz + rdz - 1 : 0;
    const BufRsrcC r = (W3_ABL & 128) ? make_rsrc_c(a.x, 1u << 20)
                                      : make_rsrc_c(xR + (size_t)rc0 * vol + (size_t)zz * plane, stage_bytes - (unsigned)((size_t)zz * plane * 4));
#pragma unroll
    for (int t = 0; t < NLD; ++t) {
      const unsigned vo = (W3_ABL & 128) ? (unsigned)(threadIdx.x * 4 + t * 2048) : uoff[t];
      if (HDMA) dma4_to_lds(r, (LdsF)&rawdst[0] + wave * 64 + NT * t, vo);
      else stage[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, vo, 0, 0));
    }
    rc0 += C;
    if (rc0 >= a.cin) { rc0 = 0; ++rdz; }
  };
  auto store_raw = [&](float* rawdst) __attribute__((always_inline)) {
#pragma unroll
    for (int t = 0; t < NLD; ++t)
      if (threadIdx.x + NT * t < NEL) rawdst[threadIdx.x + NT * t] = stage[t];
  };
  // ---- weight stream (one stage ahead): the stage's [16][C][RW] image is one contiguous block of the packed weights
  // ([dz][Cin/C][Cout/RW] blocks); DMA instruction q of this wave moves its floats [wi*256, (wi+1)*256), wi = wave + NWV*q
  // (buffer_load_dwordx4 ... lds, not global_load_lds: the compiler counts a FLAT-encoded DMA as a flat access that may return
  // out of order and turns every later wait -- the halo registers, the transform's LDS reads -- into a wait for ALL of them)
  const BufRsrcC wrs = make_rsrc_c(wt, 0x7ffffff0u);
  const unsigned wlane = (unsigned)(wave * 256 + lane * 4) * 4u;   // per-lane byte offset inside a DMA instruction's 1 KiB x NWV
  unsigned wgrp;                                        // byte offset of block (dz 0, chunk 0) of the stream's output-channel group
  int wblk;                                             // (dz, chunk) block index of the cursor
  const unsigned wstep = (unsigned)ngrp * (16 * C * RW) * 4u;
  auto enter_W = [&](const Tile& T) __attribute__((always_inline)) {
    wgrp = (unsigned)T.grp * (16 * C * RW) * 4u; wblk = dz_lo_of(T) * nchunk;
    __builtin_amdgcn_sched_barrier(0);
  };
  enter_W(T0);
  auto stage_weights = [&](float* wdst) __attribute__((always_inline)) {
    const unsigned sb = wgrp + (unsigned)wblk * wstep;
#pragma unroll
    for (int q = 0; q < NDMA; ++q)
      dma16_to_lds(wrs, (LdsF)&wdst[0] + (wave + NWV * q) * 256, wlane, sb + (unsigned)(NWV * 256 * q) * 4u);
    ++wblk;
  };
  // ---- input transform.  Half patch u = threadIdx.x + NT*i: block n = u % NB, channel c = (u / NB) % C, row half
  // hp = u / (NB*C) (wave-uniform).
  //   hp 0 -> rows 0,1 of B^T d B:  t0 = d0 - d2, t1 = d1 + d2        hp 1 -> rows 2,3:  t2 = d2 - d1, t3 = d1 - d3
  // as ONE instruction stream: t_a = P - Q, t_b = R + (S ^ sign) with (P,Q,R,S) = (d0,d2,d1,d2) or (d2,d1,d1,d3) and
  // sign = 0 or the sign bit (x + (-y) == x - y bit for bit).
  int rd_off[UPT][4], wr_off[UPT];
  unsigned sgn[UPT];
#pragma unroll
  for (int i = 0; i < UPT; ++i) {
    const int u = threadIdx.x + NT * i;
    const int n = u % NB, c = (u / NB) % C, hp = u / (NB * C);
    const int bx = n & 15, by = n >> 4;
    const int d = c * ROWS * WCOLS + (2 * by) * WCOLS + 2 * bx;
    rd_off[i][0] = d + (hp ? 2 : 0) * WCOLS; rd_off[i][1] = d + (hp ? 1 : 2) * WCOLS;
    rd_off[i][2] = d + 1 * WCOLS;            rd_off[i][3] = d + (hp ? 3 : 2) * WCOLS;
    wr_off[i] = 2 * ((4 * hp) * C * NB + c * NB + n);   // xt is [position pair][channel][block][2]
    sgn[i] = hp ? 0x80000000u : 0u;
  }
  float2 e[4][2];
  float tc[2][4];
  auto xf_load = [&](int i, const float* rawsrc) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      e[j][0] = *(const float2*)(rawsrc + rd_off[i][j]); e[j][1] = *(const float2*)(rawsrc + rd_off[i][j] + 2);
    }
  };
  // hpk: the row half where the caller knows it at compile time (0 / 1: a plain add or subtract), 2: by the sign mask
  auto xf_cols = [&](int i, int hpk = 2) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float P = s & 1 ? e[0][s >> 1].y : e[0][s >> 1].x, Q = s & 1 ? e[1][s >> 1].y : e[1][s >> 1].x;
      const float R = s & 1 ? e[2][s >> 1].y : e[2][s >> 1].x, S = s & 1 ? e[3][s >> 1].y : e[3][s >> 1].x;
      tc[0][s] = P - Q;
      tc[1][s] = hpk == 0 ? R + S : hpk == 1 ? R - S : R + __builtin_bit_cast(float, __builtin_bit_cast(unsigned, S) ^ sgn[i]);
    }
  };
  auto xf_rows_store = [&](int i, float* xtdst) __attribute__((always_inline)) {
    float* o = xtdst + wr_off[i];
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {                      // row 2 hp + rr of B^T d B: positions 4 row + 0..3 = pairs 2 row, 2 row + 1
      *(float2*)(o + (2 * rr + 0) * 2 * C * NB) = make_float2(tc[rr][0] - tc[rr][2], tc[rr][1] + tc[rr][2]);
      *(float2*)(o + (2 * rr + 1) * 2 * C * NB) = make_float2(tc[rr][2] - tc[rr][1], tc[rr][1] - tc[rr][3]);
    }
  };

  // ---- prologue (first tile of the workgroup only): halo tiles of stages 0 and 1, weights of stage 0, transform of stage 0
  if (HDMA) {
    prefetch(raw0);
    stage_weights(wbuf0);
    if (WD == 2) stage_weights(wbuf1);
    prefetch(raw1);
    prefetch(raw2);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < UPT; ++i) { xf_load(i, raw0); xf_cols(i); xf_rows_store(i, xt0); }
    __syncthreads();
  } else {
    prefetch();
    stage_weights(wbuf0);
    if (WD == 2) stage_weights(wbuf1);
    store_raw(raw0);
    prefetch();
    __syncthreads();
#pragma unroll
    for (int i = 0; i < UPT; ++i) { xf_load(i, raw0); xf_cols(i); xf_rows_store(i, xt0); }
    store_raw(raw1);
    prefetch();
    __syncthreads();
  }

  // ---- MFMA stream ----
  f32x16 acc[8];
  // both LDS images keep the two positions of a pair next to each other ([pair][channel][RW or NB][2]): one ds_read_b64
  // per operand and position PAIR (half the LDS time of two 4-byte reads)
  const int wlo = 2 * ((4 * h * C + half) * RW + cg * 32 + l31), tlo = 2 * ((4 * h * C + half) * NB + pg * 32 + l31);
  float av[2][8], bv[2][8];
  auto load_k = [&](int ks, const float* wcur, const float* xcur) __attribute__((always_inline)) {
#pragma unroll
    for (int p2 = 0; p2 < 4; ++p2) {
      const float2 wa = *(const float2*)(wcur + wlo + 2 * (p2 * C + 2 * ks) * RW), xb = *(const float2*)(xcur + tlo + 2 * (p2 * C + 2 * ks) * NB);
      av[ks][2 * p2] = wa.x; av[ks][2 * p2 + 1] = wa.y; bv[ks][2 * p2] = xb.x; bv[ks][2 * p2 + 1] = xb.y;
    }
  };
  // One phase (between two barriers), stage s of the MFMA stream's tile.  M0: a stage s-1 exists in this tile (its second
  // k-step is issued first; without it the accumulators start from zero).  The weight/transform stream (stage s+1) and the
  // halo stream (stage s+3) are always live: behind a workgroup's last tile they run on a stand-in tile whose results
  // nobody reads, which keeps every phase the same straight-line code.
  auto phase_sched = [&](auto m0, auto late_, auto hpw_, const float* wcur, float* wnext, const float* xcur, float* xnext,
                         const float* rawnext, float* rawfree) __attribute__((always_inline)) {
    constexpr bool M0 = decltype(m0)::value;
    constexpr bool LATE = decltype(late_)::value;
    constexpr int HPW = decltype(hpw_)::value;            // the row half of this wave's half patches (UPT == 1); with UPT == 2 it is i         // the second wave of each SIMD runs its fillers half a phase later
    // (the fetches of the phase are issued BEHIND its first MFMAs, whose operands are already in registers: the matrix
    // pipe restarts right behind the barrier instead of idling through ~40 address/VMEM/LDS instructions per wave)
    constexpr int S_XF = LATE ? 4 : 0, S_DMA = LATE ? 5 : 1, S_K0 = LATE ? 6 : 2, S_K1 = LATE ? 11 : 7;
#pragma unroll
    for (int slot = 0; slot < 16; ++slot) {
      const int ks = slot < 8 ? 1 : 0, p = slot & 7;
      if (!(W3_ABL & 2) && (slot >= 8 || M0)) {
        if (slot >= 8 && !M0) {
          const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ks][p], bv[ks][p], zero, 0, 0, 0);
        } else {
          acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ks][p], bv[ks][p], acc[p], 0, 0, 0);
        }
      }
      if ((W3_ABL & 2) && (slot >= 8 || M0)) asm volatile("; keep" :: "v"(av[ks][p]), "v"(bv[ks][p]));
      __builtin_amdgcn_sched_barrier(0);
      if (!(W3_ABL & 4) && slot == S_XF) xf_load(0, rawnext);
      if (!(W3_ABL & 16) && slot == S_DMA) stage_weights(wnext);
      if (!(W3_ABL & 8) && slot == S_DMA + 1) {
        if (HDMA) prefetch(rawfree);                      // (behind the weights: the barrier waits for those, not for these)
        else { store_raw(rawfree); prefetch(); }          // the halo tile fetched one phase ago; then the next one
      }
      if (!(W3_ABL & 32) && slot == S_K0) load_k(0, wcur, xcur);
      // half patch i: loaded at slot S_XF + 4i, columns 3 slots later, rows + stores 4 slots later
      const int rel = slot - S_XF, ui = rel / 4, us = rel % 4;
      if (!(W3_ABL & 4) && rel >= 0) {
        if (us == 0 && ui > 0 && ui < UPT) xf_load(ui, rawnext);
        if (us == 3 && ui < UPT) xf_cols(ui, UPT == 2 ? ui : HPW);
        if (us == 0 && ui > 0 && ui - 1 < UPT) xf_rows_store(ui - 1, xnext);
      }
      if (!(W3_ABL & 32) && slot == S_K1) load_k(1, wcur, xcur);             // the registers of k-step 1 are free: its MFMAs have all been issued
      __builtin_amdgcn_sched_barrier(0);
    }
    // the phase's own weight DMA (stage s+2) may still be in flight; everything older -- the DMA of stage s+1, the halo loads --
    // has landed: vmcnt(NDMA), lgkmcnt(0)
    asm volatile("" ::: "memory");
    constexpr int NFLY = NLD + (WD == 2 ? NDMA : 0);
    __builtin_amdgcn_s_waitcnt((NFLY & 15) | ((NFLY >> 4) << 14) | 0x70);
    if (!(W3_ABL & 1)) __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };
  using T_ = std::integral_constant<bool, true>;
  using F_ = std::integral_constant<bool, false>;

  // The two waves of a SIMD (waves w and w + 4 of an 8-wave workgroup) would otherwise run the same instruction at the same
  // time and wait at the same points, leaving the matrix pipe idle together: the second one runs the whole tile loop with
  // the late filler schedule (ONE branch around two copies of the loop: a branch per phase made the register allocator
  // spill 600 registers at the joins).
  // (2D only: with the 3D layers' 48 stages per tile the late schedule measured 5 % slower, 82 -> 86 ms at 256^3)
  constexpr bool STAGGER = NWV == 8 && UPT == 1 && !IS3D;
  auto run = [&](auto late_, auto hpw_) __attribute__((always_inline)) {
    auto phase = [&](auto m0, const float* wcur, float* wnext, const float* xcur, float* xnext, const float* rawnext,
                     float* rawfree) __attribute__((always_inline)) {
      phase_sched(m0, late_, hpw_, wcur, wnext, xcur, xnext, rawnext, rawfree);
    };
    int tM = blockIdx.x;
    Tile TM = T0;
    for (;;) {
      const int niter = (dz_hi_of(TM) - dz_lo_of(TM)) * nchunk;   // even, >= 4 (the host checks Cin % (4 C))
      const bool more = tM + tstep < ntiles;
      const Tile TN = more ? next_tile(TM) : TM;          // the streams' next tile (stand-in behind the last one: this tile again)
      // four stages per round: stage s computes on weight copy s % 4 and DMAs stage s+2 into copy (s+2) % 4
      auto group = [&](auto m0, bool last) __attribute__((always_inline)) {
        // (halo copies: stage s transforms copy (s+1) % 4 and DMAs the tile of stage s+3 into copy (s+3) % 4; through registers:
        // transforms copy (s+1) % 2 and stores the tile of stage s+2 into copy s % 2)
        phase(m0, wbuf0, WD == 2 ? wbuf2 : wbuf1, xt0, xt1, raw1, HDMA ? raw3 : raw0);
        if (last) enter_R(TN);                            // stage niter-3 fetches the halo tile of the next tile's stage 0
        phase(T_{}, wbuf1, WD == 2 ? wbuf3 : wbuf0, xt1, xt0, HDMA ? raw2 : raw0, HDMA ? raw0 : raw1);
        if (last && WD == 2) enter_W(TN);                 // ... and stage niter-WD its weights
        phase(T_{}, WD == 2 ? wbuf2 : wbuf0, WD == 2 ? wbuf0 : wbuf1, xt0, xt1, HDMA ? raw3 : raw1, HDMA ? raw1 : raw0);
        if (last && WD == 1) enter_W(TN);
        phase(T_{}, WD == 2 ? wbuf3 : wbuf1, WD == 2 ? wbuf1 : wbuf0, xt1, xt0, raw0, HDMA ? raw2 : raw1);
      };
      group(F_{}, niter == 4);
      for (int it = 4; it < niter; it += 4) group(T_{}, it + 4 == niter);
      // the second k-step of the last stage
#pragma unroll
      for (int p = 0; p < 8; ++p) acc[p] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1][p], bv[1][p], acc[p], 0, 0, 0);
      if (W3_ABL & 64) {
#pragma unroll
        for (int p = 0; p < 8; ++p) asm volatile("; keep" :: "v"(acc[p]));
        if (!more) break;
        tM += tstep; TM = TN; continue;
      }

      // Output transform A^T M A (A^T = [1 1 1 0; 0 1 -1 -1]); this wave holds rows 2h, 2h+1 of M (acc[4*(row-2h) + s]):
      //   h = 0:  t0 = M0 + M1, t1 = M1          h = 1:  t0 = M2, t1 = -M2 - M3
      // Register r belongs to half (r >> 3): the partial outputs of the other half's registers go through LDS to the
      // partner wave, the own ones are completed with the partner's, then bias, ReLU, store.  All of it on register PAIRS
      // (r, r+1) as packed fp32 (v_pk_add_f32: the same IEEE additions, two per instruction); the barriers of the
      // exchange wait for LDS only (a __syncthreads() would also wait for the stores of the round before to be acknowledged).
      {
        const int bx = l31 & 15, byl = l31 >> 4;
        const int tx0 = TM.tx * 32, ty0 = TM.ty * (4 * NPG);
        const int x = tx0 + 2 * bx, y = ty0 + 2 * (2 * pg + byl);
        // channel of register r = 8 hh + 4 round + 2 j (+1):  cg*32 + 2 j + 8 (2 hh + round) + 4 half
        const int co_own = TM.grp * RW + cg * 32 + 16 * h + 4 * half;
        f32x2 bias2[2][2];
#pragma unroll
        for (int round = 0; round < 2; ++round)
#pragma unroll
          for (int j = 0; j < 2; ++j) bias2[round][j] = *(const f32x2*)&a.bias[co_own + 8 * round + 2 * j];
        float* obase = a.y + ((size_t)TM.b * a.cout + co_own) * vol + (size_t)TM.z * plane + (size_t)y * a.W + x;
        // full tiles store through a buffer resource on the wave's 16 channels: one 32-bit lane offset per pixel row (the
        // channel quad of the lane's half included) and the channel in the scalar offset -- no 64-bit address arithmetic on
        // the vector ALU, which runs in the matrix pipe's time (tools/ubench/mfma_coexec.hip)
        typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
        const BufRsrcC yrs = (W3_ABL & 256) ? make_rsrc_c(a.y + (size_t)blockIdx.x * 65536, 1u << 20)
                                            : make_rsrc_c(a.y + ((size_t)TM.b * a.cout + TM.grp * RW + cg * 32 + 16 * h) * vol, (unsigned)(16 * vol * 4 - 1) + 1u);
        const unsigned yoff0 = (W3_ABL & 256) ? threadIdx.x * 8u : (unsigned)(((size_t)(4 * half) * vol + (size_t)TM.z * plane + (size_t)y * a.W + x) * 4),
                       yoff1 = (W3_ABL & 256) ? yoff0 + 4096u : yoff0 + (unsigned)a.W * 4u;
        const unsigned chan_bytes = (W3_ABL & 256) ? 8192u : (unsigned)(vol * 4);
        const bool inx = x < a.W, iny = y < a.H, inx1 = x + 1 < a.W, iny1 = y + 1 < a.H;
        const bool full = (tx0 + 32 <= a.W) & (ty0 + 4 * NPG <= a.H);       // (wave-uniform) no clipped pixel in the tile
        f32x2* ex_out = (f32x2*)&exch[wave * 16 * 64] + lane;
        const f32x2* ex_in = (const f32x2*)&exch[(wave ^ 1) * 16 * 64] + lane;
        auto out_part = [&](auto hh_, int r, f32x2 (&pt)[4]) __attribute__((always_inline)) {
          constexpr int HH = decltype(hh_)::value;           // this wave's position half
          f32x2 t0[4], t1[4];
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const f32x2 a0 = {acc[s][r], acc[s][r + 1]}, a1 = {acc[4 + s][r], acc[4 + s][r + 1]};
            if (HH == 0) { t0[s] = a0 + a1; t1[s] = a1; }
            else { t0[s] = a0; t1[s] = (-a0) - a1; }
          }
          pt[0] = (t0[0] + t0[1]) + t0[2]; pt[1] = (t0[1] - t0[2]) - t0[3];
          pt[2] = (t1[0] + t1[1]) + t1[2]; pt[3] = (t1[1] - t1[2]) - t1[3];
        };
        auto send = [&](auto hh_, int round) __attribute__((always_inline)) {
          constexpr int HH = decltype(hh_)::value;
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            f32x2 pt[4];
            out_part(hh_, 8 * (1 - HH) + 4 * round + 2 * j, pt);
#pragma unroll
            for (int q = 0; q < 4; ++q) ex_out[(j * 4 + q) * 64] = pt[q];
          }
        };
        auto finish = [&](auto hh_, int round) __attribute__((always_inline)) {
          constexpr int HH = decltype(hh_)::value;
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            f32x2 pt[4], v[4];
            out_part(hh_, 8 * HH + 4 * round + 2 * j, pt);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              v[q] = (pt[q] + ex_in[(j * 4 + q) * 64]) + bias2[round][j];
              v[q] = __builtin_elementwise_max(v[q], (f32x2){relu_lo, relu_lo});
            }
            float* o0 = obase + (size_t)(8 * round + 2 * j) * vol;
            float* o1 = o0 + vol;
            if (full) {
              const unsigned c0 = (unsigned)(8 * round + 2 * j) * chan_bytes, c1 = c0 + chan_bytes;
              __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, (f32x2){v[0].x, v[1].x}), yrs, yoff0, c0, 2);   // (aux 2: non-temporal)
              __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, (f32x2){v[2].x, v[3].x}), yrs, yoff1, c0, 2);
              __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, (f32x2){v[0].y, v[1].y}), yrs, yoff0, c1, 2);
              __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, (f32x2){v[2].y, v[3].y}), yrs, yoff1, c1, 2);
            } else if (inx & iny) {
              if (inx1) {
                *(float2*)o0 = make_float2(v[0].x, v[1].x); *(float2*)o1 = make_float2(v[0].y, v[1].y);
                if (iny1) { *(float2*)(o0 + a.W) = make_float2(v[2].x, v[3].x); *(float2*)(o1 + a.W) = make_float2(v[2].y, v[3].y); }
              } else {
                o0[0] = v[0].x; o1[0] = v[0].y;
                if (iny1) { o0[a.W] = v[2].x; o1[a.W] = v[2].y; }
              }
            }
          }
        };
        using H0 = std::integral_constant<int, 0>;
        using H1 = std::integral_constant<int, 1>;
#pragma unroll
        for (int round = 0; round < 2; ++round) {            // 4 of a half's 8 registers per round (16 values each way)
          // (round 0: the previous tile's reads of the exchange buffer are many barriers back)
          if (round) { __builtin_amdgcn_s_waitcnt(0xc07f); __builtin_amdgcn_s_barrier(); }       // lgkmcnt(0) only
          if (h == 0) send(H0{}, round); else send(H1{}, round);
          __builtin_amdgcn_s_waitcnt(0xc07f); __builtin_amdgcn_s_barrier();
          if (h == 0) finish(H0{}, round); else finish(H1{}, round);
        }
      }
      if (!more) break;
      tM += tstep; TM = TN;
    }
  };
  // (the same split serves the input transform: with one half patch per thread the upper half of the waves has the rows 2, 3
  // of B^T d B, and each copy of the loop knows its half at compile time)
  static_assert(UPT == 2 || NB * C == NT / 2, "row half = upper half of the waves");
  if (UPT == 1 && wave >= NWV / 2) run(std::integral_constant<bool, STAGGER>{}, std::integral_constant<int, 1>{});
  else run(std::integral_constant<bool, false>{}, std::integral_constant<int, 0>{});
}

// blob: (Cout,Cin,3x3) -> G g G^T as [16][Cin][Cout], G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1]
// (3D: per z tap dz, [dz][16][Cin][Cout])
__global__ void pack_layer_wino_kernel(const float* __restrict__ w, float* __restrict__ pw, int cin, int cout, int kd) {
  const int n = cin * cout * kd;
  for (int q0 = blockIdx.x * blockDim.x + threadIdx.x; q0 < n; q0 += gridDim.x * blockDim.x) {
    const int dz = q0 / (cin * cout), q = q0 - dz * cin * cout;
    const int co = q / cin, ci = q - co * cin;
    const float* g = w + ((size_t)q * kd + dz) * 9;
    float t[4][3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const float g0 = g[s], g1 = g[3 + s], g2 = g[6 + s];
      t[0][s] = g0; t[1][s] = 0.5f * ((g0 + g1) + g2); t[2][s] = 0.5f * ((g0 - g1) + g2); t[3][s] = g2;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float u[4] = { t[r][0], 0.5f * ((t[r][0] + t[r][1]) + t[r][2]), 0.5f * ((t[r][0] - t[r][1]) + t[r][2]), t[r][2] };
#pragma unroll
      for (int s = 0; s < 4; ++s) pw[((size_t)(dz * 16 + 4 * r + s) * cin + ci) * cout + co] = u[s];
    }
  }
}

// The same G g G^T values re-ordered for conv3_wino3_kernel: [dz][Cin/4][Cout/RW][8 position pairs][4][RW][2] -- the 16*4*RW floats one
// workgroup DMAs per stage are ONE contiguous block (every workgroup of the launch reads the same blocks at about the
// same time: 64 rows of RW floats strided over the [16][Cin][Cout] image land on half of an XCD's L2 channels, the
// contiguous block on all of them).  RW = 64 where Cout % 64 == 0, else 32 (the kernel's output channels per workgroup).
__global__ void repack_wino3_kernel(const float* __restrict__ src, float* __restrict__ dst, int cin, int cout, int kd, int rw) {
  const size_t n = (size_t)kd * 16 * cin * cout;
  const int nchunk = cin / W3C, ngrp = cout / rw;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (size_t)gridDim.x * blockDim.x) {
    const int co = (int)(q % cout);
    size_t r = q / cout;
    const int ci = (int)(r % cin); r /= cin;
    const int pp = (int)(r % 16), dz = (int)(r / 16);
    const size_t o = (((((((size_t)dz * nchunk + ci / W3C) * ngrp + co / rw) * 8 + pp / 2) * W3C + ci % W3C) * rw) + co % rw) * 2 + pp % 2;
    dst[o] = src[q];
  }
}
