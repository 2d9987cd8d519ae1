// Vorticity confinement for gfx950: U_out = U_in + the confinement force of U_in, one launch, no intermediate field in memory.
//
// Per cell (fp32, no contraction, this order -- tests/vorticity_reference.py is the same statement in numpy):
//   c   = centred velocity                     c_a = 0.5 (U_a(cell) + U_a(cell + e_a))
//   w   = curl of c by central differences     w_z = 0.5 (d_x c_y - d_y c_x), ...;  n = |w|
//   F   = (grad n / |grad n|) x w * amp        grad n by central differences
//   U_a += 0.5 (F_a(cell - e_a) + F_a(cell))   where addGravity would write (fnx_step.hip: gravity_applies)
// Every one of c, w, n, F is 0 outside the interior cells.  A component of the output depends on U within three cells in every
// axis, so the pass is out of place.
//
// Shape: a workgroup owns a 64 x 16 (x, y) region -- a 59 x 11 tile of outputs with the halo the chain needs (3 cells towards -,
// 2 towards +; c itself is taken from global memory, so the region is the footprint of c) -- and marches in z over a chunk of
// ZCH planes.  Each of the 512 threads owns two cells of the region for the whole march, so everything the chain needs along z is
// in that thread's registers (three planes of c_x, c_y and n, two of w, three of F_z); LDS only carries the one plane of c, n and
// (F_x, F_y) whose in-plane neighbours the step reads.  In step s of the march the block
//   phase 1: turns the prefetched U of plane s into c(s); puts c(s-1), n(s-2), F_xy(s-3) into the LDS planes of parity s
//   barrier
//   phase 2: prefetches U of plane s+1; computes w(s-1), n(s-1); F(s-2); writes the output plane s-3.
// The LDS planes are double-buffered by the parity of s, so one barrier per step is enough: a wave that runs ahead into phase 1
// of step s+1 writes the other parity, and nobody reaches step s+2 before everyone is through the barrier of s+1.
// A chunk starts three planes early (its registers fill up with planes it does not write); in 2D the march is the four steps of
// the one plane.  48 KiB of LDS and < 128 VGPRs: two workgroups, 16 waves, per CU.
#include "fnx_device.h"
#include "fnx_kernels.h"

namespace {

constexpr int RX = 64, RY = 16;          // region (threads: RX x RY/2, two rows each)
constexpr int TY = RY / 2;
constexpr int HALO = 3;                  // region origin = tile origin - HALO
constexpr int OX = RX - 5, OY = RY - 5;  // outputs per tile: region cells [3, RX-3] x [3, RY-3]
constexpr int ZCH = 32;                  // planes per chunk of the march (3D)
constexpr float VC_EPS = 1e-6f;

__device__ __forceinline__ float vc_norm(float x, float y, float z) {
  const float s = (x * x + y * y) + z * z;
  return s > VC_EPS ? sqrtf(s) : 0.f;
}

__device__ __forceinline__ bool vc_applies(float fc, float fm) {     // gravity_applies of fnx_step.hip
  return (fc == FNX_FLUID || fc == FNX_EMPTY) && (fm == FNX_FLUID || (fm == FNX_EMPTY && fc == FNX_FLUID));
}

enum { L_CX = 0, L_CY, L_CZ, L_N, L_FX, L_FY, L_COUNT };

template <bool IS3D>
__global__ __launch_bounds__(RX* TY) void vorticity_confinement_kernel(GridDims g, const float* __restrict__ Uin,
                                                                      const float* __restrict__ flags,
                                                                      float* __restrict__ Uout, float amp, int nzc) {
  __shared__ float L[2][L_COUNT][RY][RX];
  constexpr int NC = IS3D ? 3 : 2;
  const int lx = threadIdx.x;
  const int i = (int)blockIdx.x * OX - HALO + lx;
  const int b = (int)blockIdx.z / nzc, zc = (int)blockIdx.z - b * nzc;
  const int k0 = IS3D ? zc * ZCH : 0;
  const int k1 = IS3D ? (k0 + ZCH < g.D ? k0 + ZCH : g.D) : 1;
  const float* Ub = Uin + (size_t)b * NC * g.DHW;
  float* Wb = Uout + (size_t)b * NC * g.DHW;
  const float* Fb = flags + (size_t)b * g.DHW;

  int ly[2], off[2];
  bool inxy[2], wok[2], fok[2], ook[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    ly[r] = (int)threadIdx.y + r * TY;
    const int j = (int)blockIdx.y * OY - HALO + ly[r];
    const bool ingrid = i >= 0 && i < g.W && j >= 0 && j < g.H;
    inxy[r] = i >= 1 && i <= g.W - 2 && j >= 1 && j <= g.H - 2;
    off[r] = ingrid ? j * g.W + i : 0;
    wok[r] = inxy[r] && lx >= 1 && lx <= RX - 2 && ly[r] >= 1 && ly[r] <= RY - 2;
    fok[r] = inxy[r] && lx >= 2 && lx <= RX - 3 && ly[r] >= 2 && ly[r] <= RY - 3;
    ook[r] = ingrid && lx >= 3 && lx <= RX - 3 && ly[r] >= 3 && ly[r] <= RY - 3;
  }
  // is plane q one whose cells can be interior?
  auto plane_in = [&](int q) { return IS3D ? (q >= 1 && q <= g.D - 2) : (q == 0); };

  // rolling state of the two cells (planes relative to the step s at the top of phase 2)
  float cxa[2] = {0.f, 0.f}, cxb[2] = {0.f, 0.f}, cxc[2] = {0.f, 0.f};      // c_x of planes s-2, s-1, s
  float cya[2] = {0.f, 0.f}, cyb[2] = {0.f, 0.f}, cyc[2] = {0.f, 0.f};
  float czb[2] = {0.f, 0.f}, czc[2] = {0.f, 0.f};                            // c_z of planes s-1, s
  float wa[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};                       // w of plane s-2
  float na[2] = {0.f, 0.f}, nb[2] = {0.f, 0.f};                              // n of planes s-2, s-3
  float fxp[2] = {0.f, 0.f}, fyp[2] = {0.f, 0.f};                            // F_x, F_y of plane s-3 (on their way to LDS)
  float fza[2] = {0.f, 0.f}, fzb[2] = {0.f, 0.f};                            // F_z of planes s-3, s-4
  float pu[2][6];                                                            // prefetched U of plane s: x, x+1, y, y+W, z, z+HW

  auto prefetch = [&](int q) {
    const bool pq = plane_in(q);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
      for (int t = 0; t < 6; ++t) pu[r][t] = 0.f;
      if (pq && inxy[r]) {
        const int o = q * g.HW + off[r];
        pu[r][0] = Ub[o]; pu[r][1] = Ub[o + 1];
        pu[r][2] = Ub[(size_t)g.DHW + o]; pu[r][3] = Ub[(size_t)g.DHW + o + g.W];
        if (IS3D) { pu[r][4] = Ub[(size_t)2 * g.DHW + o]; pu[r][5] = Ub[(size_t)2 * g.DHW + o + g.HW]; }
      }
    }
  };

  const int s0 = IS3D ? k0 - 3 : 0;
  prefetch(s0);
  for (int s = s0; s < k1 + 3; ++s) {
    float(*P)[RY][RX] = L[s & 1];
    // ---- phase 1
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      cxa[r] = cxb[r]; cxb[r] = cxc[r]; cya[r] = cyb[r]; cyb[r] = cyc[r]; czb[r] = czc[r];
      cxc[r] = 0.5f * (pu[r][0] + pu[r][1]);         // (all zero where the cell is not interior: the prefetch left zeros)
      cyc[r] = 0.5f * (pu[r][2] + pu[r][3]);
      czc[r] = IS3D ? 0.5f * (pu[r][4] + pu[r][5]) : 0.f;
      P[L_CX][ly[r]][lx] = cxb[r]; P[L_CY][ly[r]][lx] = cyb[r];
      if (IS3D) P[L_CZ][ly[r]][lx] = czb[r];
      P[L_N][ly[r]][lx] = na[r];
      P[L_FX][ly[r]][lx] = fxp[r]; P[L_FY][ly[r]][lx] = fyp[r];
    }
    __syncthreads();
    // ---- phase 2
    prefetch(s + 1);
    const int qo = s - 3;                              // the output plane
    const bool out_plane = qo >= k0 && qo < k1;        // (block-uniform, like every plane test)
    float ou[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}}, ofc[2] = {0.f, 0.f}, ofm[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
    bool oin[2] = {false, false};                      // the output cell is interior: its flags were read
    if (out_plane) {
      const bool qin = plane_in(qo);
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        if (!ook[r]) continue;
        const int o = qo * g.HW + off[r];
#pragma unroll
        for (int a = 0; a < NC; ++a) ou[r][a] = Ub[(size_t)a * g.DHW + o];
        if (qin && inxy[r]) {
          oin[r] = true;
          ofc[r] = Fb[o]; ofm[r][0] = Fb[o - 1]; ofm[r][1] = Fb[o - g.W];
          if (IS3D) ofm[r][2] = Fb[o - g.HW];
        }
      }
    }
    const bool pw = plane_in(s - 1), pf = plane_in(s - 2);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int y = ly[r];
      // w, n of plane s-1
      float wn[3] = {0.f, 0.f, 0.f}, nn = 0.f;
      if (pw && wok[r]) {
        const float dxcy = P[L_CY][y][lx + 1] - P[L_CY][y][lx - 1];
        const float dycx = P[L_CX][y + 1][lx] - P[L_CX][y - 1][lx];
        wn[2] = 0.5f * (dxcy - dycx);
        if (IS3D) {
          const float dycz = P[L_CZ][y + 1][lx] - P[L_CZ][y - 1][lx];
          const float dzcy = cyc[r] - cya[r];
          wn[0] = 0.5f * (dycz - dzcy);
          const float dzcx = cxc[r] - cxa[r];
          const float dxcz = P[L_CZ][y][lx + 1] - P[L_CZ][y][lx - 1];
          wn[1] = 0.5f * (dzcx - dxcz);
        }
        nn = vc_norm(wn[0], wn[1], wn[2]);
      }
      // F of plane s-2
      float fx = 0.f, fy = 0.f, fz = 0.f;
      if (pf && fok[r]) {
        float gx = 0.5f * (P[L_N][y][lx + 1] - P[L_N][y][lx - 1]);
        float gy = 0.5f * (P[L_N][y + 1][lx] - P[L_N][y - 1][lx]);
        float gz = IS3D ? 0.5f * (nn - nb[r]) : 0.f;
        const float m = vc_norm(gx, gy, gz);
        if (m > VC_EPS) { gx = gx / m; gy = gy / m; gz = gz / m; }
        else { gx = 0.f; gy = 0.f; gz = 0.f; }
        const float wx = wa[r][0], wy = wa[r][1], wz = wa[r][2];
        fx = (gy * wz - gz * wy) * amp;
        fy = (gz * wx - gx * wz) * amp;
        fz = (gx * wy - gy * wx) * amp;
      }
      // the output plane s-3
      if (out_plane && ook[r]) {
        const int o = qo * g.HW + off[r];
        float v[3] = {ou[r][0], ou[r][1], IS3D ? ou[r][2] : 0.f};
        if (oin[r]) {
          if (vc_applies(ofc[r], ofm[r][0])) v[0] = v[0] + 0.5f * (P[L_FX][y][lx - 1] + P[L_FX][y][lx]);
          if (vc_applies(ofc[r], ofm[r][1])) v[1] = v[1] + 0.5f * (P[L_FY][y - 1][lx] + P[L_FY][y][lx]);
          if (IS3D) { if (vc_applies(ofc[r], ofm[r][2])) v[2] = v[2] + 0.5f * (fzb[r] + fza[r]); }
        }
#pragma unroll
        for (int a = 0; a < NC; ++a) Wb[(size_t)a * g.DHW + o] = v[a];
      }
      // roll
      nb[r] = na[r]; na[r] = nn;
#pragma unroll
      for (int a = 0; a < 3; ++a) wa[r][a] = wn[a];
      fxp[r] = fx; fyp[r] = fy;
      fzb[r] = fza[r]; fza[r] = fz;
    }
  }
}

}  // namespace

namespace fnx {

void launch_vorticity_confinement(const GridDims& g, bool is3d, const float* U_in, const float* flags, float* U_out, float amp,
                                  hipStream_t s) {
  const int nzc = is3d ? (g.D + ZCH - 1) / ZCH : 1;
  const dim3 grid((g.W + OX - 1) / OX, (g.H + OY - 1) / OY, g.B * nzc), block(RX, TY);
  if (is3d) vorticity_confinement_kernel<true><<<grid, block, 0, s>>>(g, U_in, flags, U_out, amp, nzc);
  else vorticity_confinement_kernel<false><<<grid, block, 0, s>>>(g, U_in, flags, U_out, amp, nzc);
}

}  // namespace fnx
