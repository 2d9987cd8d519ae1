// 5x5(x5) convolution of the thin layers (3->32 packed over (tap, channel), 32->8 with the final 1x1 in its epilogue), exact fp32 on
// v_mfma_f32_16x16x4_f32 (included by fnx_cnn.hip inside its anonymous namespace, after its DMA helpers and ConvArgs).
// ---------------------------------------------------------------------------------------------------
// Implicit-GEMM 5x5(x5) convolution for the thin layers (3->32 and 32->8) on v_mfma_f32_16x16x4_f32 (exact fp32):
//   D[cout 16][pixel 16] += A[cout][k] * B[k][pixel],  k = four consecutive input channels of one tap
//   A: lane -> W[tap][c + (lane>>4)][m*16 + (lane&15)]       (LDS image [tap][CHS][CO], conflict-free)
//   B: lane -> X[c + (lane>>4)][y + r - 2][x + (lane&15) + s - 2]  from the LDS halo tile (the four 16-lane groups read
//      four channel planes whose stride, 12*68 floats, spreads them over disjoint banks)
//   D: lane holds pixel (lane&15) and output channels 4*(lane>>4)..+3
// Workgroup = 4 waves stacked in y; wave tile = 64 px (4 segments of 16) x 2 rows x MB*16 output channels.  A stage
// is one z plane x CHS input channels: the halo tile goes global -> registers -> LDS (prefetched during the previous
// stage's MFMAs), the stage's 25 x CHS x CO weights go global -> LDS by buffer_load_dwordx4 ... lds; both double-buffered,
// one barrier per stage (25*CHS/4*8*MB MFMAs per wave between barriers).  Padded output channels (32->8 uses half
// of the 16-row M block) cost MFMA cycles, not memory traffic.
// ---------------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));

// PAIR (Cout <= 8): the 16 rows of the M block are (dx, cout) for TWO x-adjacent output pixels, the 16 columns are pixel
// pairs, and k runs over a 6-wide window per tap row (weights zero where the tap falls outside an output's 5): 30
// k-positions per row-plane instead of 2 x 25 half-empty ones -- 0.6x the MFMAs of the plain mapping for 32->8.
// KPC (2 or 3 = Cin; 0: off): K packed over (tap, channel), see pack_layer_kpack_kernel.
template <int CHS, int MB, bool IS3D, bool PAIR, int KPC = 0>
__global__ __launch_bounds__(256, 2) void conv5_mfma16_kernel(ConvArgs a, int cin_pad) {
  constexpr int KS = 5, PAD = 2, PR = 2;
  static_assert(KPC == 0 || (CHS == 4 && !PAIR), "packed K: one stage per z plane, all (<= 3) channels in it");
  constexpr int NKP = (25 * KPC + 3) / 4, KROWS = NKP * 4;           // K-groups of four / weight rows per plane (KPC)
  constexpr int NX = PAIR ? 2 : 4;                                    // MFMA column blocks per wave row (64 px either way)
  constexpr int KW = PAIR ? KS + 1 : KS;                              // k positions along x per tap row
  constexpr int XSEG = PAIR ? 32 : 16, XSTEP = PAIR ? 2 : 1;          // pixels per column block, pixel stride of a lane
  static_assert(!PAIR || MB == 1, "pairs fill one M block");
  constexpr int ROWS = 4 * PR + KS - 1, COLS = 64 + KS - 1;           // 12 x 68 halo tile per channel
  constexpr int CO = 16 * MB;
  constexpr int NEL = CHS * ROWS * COLS, NLD = (NEL + 255) / 256;
  constexpr int TAPF = CHS * CO;                                      // floats per tap in a stage (128 or 64)
  static_assert(TAPF == 128 || TAPF == 64, "a wave-wide 16-byte load covers 2 or 4 taps");
  constexpr int TPI = 256 / TAPF, LPT = 64 / TPI;                     // taps per wave-instruction, lanes per tap
  constexpr int NTAP = KS * KW;                                       // k positions per plane (25, or 30 for PAIR)
  constexpr int NWI = KPC ? (KROWS * CO + 255) / 256 : (NTAP + TPI - 1) / TPI;   // wave-instructions per stage
  __shared__ __attribute__((aligned(16))) float tile2[2][NEL];
  __shared__ __attribute__((aligned(16))) float wbuf0[NWI * 256];       // (two separate arrays and out-of-range-zero buffer
  __shared__ __attribute__((aligned(16))) float wbuf1[NWI * 256];       //  loads: see conv3_mfma_kernel)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int seg = lane & 15, kq = lane >> 4;
  const int x0 = blockIdx.x * 64, y0 = blockIdx.y * (4 * PR);
  int zb = blockIdx.z;
  const int z = zb % a.D; const int b = zb / a.D;
  const size_t plane = (size_t)a.H * a.W, vol = plane * a.D;

  f32x4 acc[PR][NX][MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = PAIR ? (4 * kq + r) % 8 : mb * 16 + 4 * kq + r;
      const float bv = co < a.cout ? a.bias[co] : 0.f;
#pragma unroll
      for (int pr = 0; pr < PR; ++pr)
#pragma unroll
        for (int nx = 0; nx < NX; ++nx) acc[pr][nx][mb][r] = bv;
    }
  }

  const float* xb = a.x + (size_t)b * a.cin * vol;
  // per-thread staging slots of the [CHS][ROWS][COLS] halo tile (offsets and predicates are stage-invariant: Cin is a
  // multiple of CHS, or smaller than CHS with a single chunk whose missing channels read as zero)
  unsigned uoff[NLD];
#pragma unroll
  for (int t = 0; t < NLD; ++t) {
    const int idx = threadIdx.x + 256 * t;
    const int cc = idx / (ROWS * COLS);
    const int rem = idx - cc * ROWS * COLS;
    const int row = rem / COLS, col = rem - row * COLS;
    const int gx = x0 - PAD + col, gy = y0 - PAD + row;
    const bool ok = (idx < NEL) & (cc < a.cin) & (gx >= 0) & (gx < a.W) & (gy >= 0) & (gy < a.H);
    uoff[t] = ok ? (unsigned)(((size_t)cc * vol + (size_t)gy * a.W + gx) * 4) : 0xfffffff0u;
  }
  const unsigned stage_bytes = (unsigned)((size_t)CHS * vol * 4 - 1) + 1u;
  float stage[NLD];
  auto prefetch = [&](int dz, int c0) {
    const int zz = IS3D ? z + dz - PAD : 0;
    const BufRsrcC r = make_rsrc_c(xb + (size_t)c0 * vol + (size_t)zz * plane, stage_bytes - (unsigned)((size_t)zz * plane * 4));
#pragma unroll
    for (int t = 0; t < NLD; ++t) stage[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, uoff[t], 0, 0));
  };
  // (weights by buffer_load_dwordx4 ... lds with a fixed lane offset and the stage in the scalar offset: see conv3_mfma_kernel)
  const BufRsrcC wrs = make_rsrc_c(a.w, 0x7ffffff0u);
  constexpr int NWQ = (NWI + 3) / 4;
  unsigned wvoff[NWQ];
#pragma unroll
  for (int q = 0; q < NWQ; ++q) {
    if (KPC) {                                            // the plane's KROWS x CO floats are one linear block
      int f = (wave + 4 * q) * 256 + lane * 4;
      if (f > KROWS * CO - 4) f = KROWS * CO - 4;         // (the tail re-reads the last floats into slots nobody reads)
      wvoff[q] = (unsigned)f * 4u;
    } else {
      int tap = TPI * (wave + 4 * q) + lane / LPT;
      if (tap > NTAP - 1) tap = NTAP - 1;                 // the tail re-reads the last tap into slots nobody reads
      wvoff[q] = (unsigned)((size_t)tap * cin_pad * CO + (lane % LPT) * 4) * 4u;
    }
  }
  // packed K: the lane's element of K-group m is k = 4 m + kq = (tap, channel); its offset in the halo tile
  int boff[KPC ? NKP : 1];
  if (KPC) {
#pragma unroll
    for (int m = 0; m < NKP; ++m) {
      const int k = 4 * m + kq, tap = k / (KPC ? KPC : 1), ci = k - tap * KPC;
      const int r = tap / KS, sx = tap - r * KS;
      boff[m] = tap < 25 ? ci * ROWS * COLS + r * COLS + sx : 0;      // (padding: zero weights on a valid address)
    }
  }
  auto stage_weights = [&](int dz, int c0, float* wdst) {
    const unsigned soff = KPC ? (unsigned)((size_t)dz * KROWS * CO) * 4u : (unsigned)(((size_t)dz * NTAP * cin_pad + c0) * CO) * 4u;
#pragma unroll
    for (int q = 0; q < NWQ; ++q) {
      const int wi = wave + 4 * q;                        // wave-uniform
      if (wi < NWI) dma16_to_lds(wrs, (LdsF)&wdst[0] + wi * 256, wvoff[q], soff);
    }
  };
  const int nchunk = cin_pad / CHS;
  int dz_lo = 0, dz_hi = IS3D ? KS : 1;
  if (IS3D) { dz_lo = PAD - z > 0 ? PAD - z : 0; dz_hi = a.D + PAD - z < KS ? a.D + PAD - z : KS; }
  const int niter = (dz_hi - dz_lo) * nchunk;
  if (niter > 0) { prefetch(dz_lo, 0); stage_weights(dz_lo, 0, wbuf0); }
  auto stage_body = [&](int it, float* wcur, float* wnext) __attribute__((always_inline)) {
    float* tile = tile2[it & 1];
#pragma unroll
    for (int t = 0; t < NLD; ++t)
      if (threadIdx.x + 256 * t < NEL) tile[threadIdx.x + 256 * t] = stage[t];
    __syncthreads();                                     // tile stores + the stage's weight DMA visible to all
    if (it + 1 < niter) {
      prefetch(dz_lo + (it + 1) / nchunk, ((it + 1) % nchunk) * CHS);
      stage_weights(dz_lo + (it + 1) / nchunk, ((it + 1) % nchunk) * CHS, wnext);
    }
    const float* wl = &wcur[kq * CO + seg];
    const float* tl = &tile[kq * ROWS * COLS + (wave * PR) * COLS + XSTEP * seg];
    if (KPC) {
      const float* tb = &tile[(wave * PR) * COLS + XSTEP * seg];
#pragma unroll
      for (int m = 0; m < NKP; ++m) {
        float av[MB], bv[PR][NX];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) av[mb] = wl[(4 * m) * CO + mb * 16];
#pragma unroll
        for (int pr = 0; pr < PR; ++pr)
#pragma unroll
          for (int nx = 0; nx < NX; ++nx) bv[pr][nx] = tb[boff[m] + pr * COLS + nx * XSEG];
#pragma unroll
        for (int pr = 0; pr < PR; ++pr)
#pragma unroll
          for (int nx = 0; nx < NX; ++nx)
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
              acc[pr][nx][mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mb], bv[pr][nx], acc[pr][nx][mb], 0, 0, 0);
      }
      return;
    }
    // (an explicit operand pipeline as in conv3_mfma_kernel measured slower here: 2.27 -> 2.74 ms at 128^3)
#pragma unroll
    for (int r = 0; r < KS; ++r) {
#pragma unroll
      for (int s = 0; s < KW; ++s) {
#pragma unroll
        for (int ks = 0; ks < CHS / 4; ++ks) {
          float av[MB], bv[PR][NX];
#pragma unroll
          for (int mb = 0; mb < MB; ++mb) av[mb] = wl[((r * KW + s) * CHS + ks * 4) * CO + mb * 16];
#pragma unroll
          for (int pr = 0; pr < PR; ++pr)
#pragma unroll
            for (int nx = 0; nx < NX; ++nx) bv[pr][nx] = tl[(ks * 4) * ROWS * COLS + (pr + r) * COLS + nx * XSEG + s];
#pragma unroll
          for (int pr = 0; pr < PR; ++pr)
#pragma unroll
            for (int nx = 0; nx < NX; ++nx)
#pragma unroll
              for (int mb = 0; mb < MB; ++mb)
                acc[pr][nx][mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mb], bv[pr][nx], acc[pr][nx][mb], 0, 0, 0);
        }
      }
    }
  };
  for (int it = 0; it < niter; it += 2) {
    stage_body(it, wbuf0, wbuf1);
    if (it + 1 < niter) stage_body(it + 1, wbuf1, wbuf0);
  }
  if (PAIR && a.tail_w != nullptr) {
    // fused 1x1 tail: a lane holds channels (4 kq + r) % 8 of pixel x (kq 0, 1) or x + 1 (kq 2, 3); its four weighted values are
    // summed in the lane, the two halves of a pixel (lanes 16 apart) through a DPP row... the lanes sit in different rows of 16:
    // ds_swizzle / bpermute; the lane with even kq adds the bias and stores the ONE output channel
    float tw[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) tw[r] = a.tail_w[(4 * kq + r) % 8];
    const float tb = a.tail_b[0];
#pragma unroll
    for (int pr = 0; pr < PR; ++pr) {
      const int y = y0 + wave * PR + pr;
#pragma unroll
      for (int nx = 0; nx < NX; ++nx) {
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = acc[pr][nx][0][r];
          if (a.relu) v = fmaxf(v, 0.f);
          sum = fmaf(tw[r], v, sum);
        }
        const float other = __shfl_xor(sum, 16);             // (every lane takes part: no early exits above)
        const int x = x0 + nx * XSEG + XSTEP * seg + (kq >> 1);
        if ((kq & 1) == 0 && y < a.H && x < a.W)
          a.y[(size_t)b * vol + (size_t)z * plane + (size_t)y * a.W + x] = (sum + other) + tb;
      }
    }
    return;
  }
#pragma unroll
  for (int pr = 0; pr < PR; ++pr) {
    const int y = y0 + wave * PR + pr;
    if (y >= a.H) continue;
#pragma unroll
    for (int nx = 0; nx < NX; ++nx) {
      const int x = x0 + nx * XSEG + XSTEP * seg + (PAIR ? (kq >> 1) : 0);   // PAIR: rows 8..15 of the block are the +1 pixel
      if (x >= a.W) continue;
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int co = PAIR ? (4 * kq + r) % 8 : mb * 16 + 4 * kq + r;
          if (co < a.cout) {
            float v = acc[pr][nx][mb][r];
            if (a.relu) v = fmaxf(v, 0.f);
            a.y[((size_t)b * a.cout + co) * vol + (size_t)z * plane + (size_t)y * a.W + x] = v;
          }
        }
      }
    }
  }
}
