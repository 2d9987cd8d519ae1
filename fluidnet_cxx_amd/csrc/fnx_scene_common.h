// What the 2D (fnx_scenes.hip) and 3D (fnx_scenes3d.hip) training scenes and losses share: the counter-based hash, the loss's
// coefficients and its one-workgroup finish, and the parameter checks.  Included once per unit; everything has internal linkage.
#pragma once
#include <stdio.h>
#include "fnx_device.h"
#include "fnx_kernels.h"
#include "../../include/fluidnet_hip.h"

namespace {

constexpr int BX = 64, BY = 4;

__host__ __device__ __forceinline__ unsigned mix32(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
__host__ __device__ __forceinline__ unsigned scene_key(unsigned seed, unsigned scene, unsigned stream) {
  return mix32(mix32(mix32(seed + 0x9e3779b9u) ^ scene) ^ stream);
}
__host__ __device__ __forceinline__ float uniform01(unsigned key, unsigned ctr) {
  return (float)(int)(mix32(key ^ ctr) >> 8) * 5.9604644775390625e-8f;      // 2^-24
}

struct LossCoef { float p2, p1, d2, d1; };     // 2 lambda / N resp. lambda / N of the four terms (the gradient's factors)

__device__ __forceinline__ float sign_of(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// terms[q] = sum of the partials in index order / N;  terms[4] = sum_q lambda_q terms[q]
__global__ __launch_bounds__(256) void train_loss_finish_kernel(size_t nblk, double n, const double* __restrict__ partial, float l0,
                                                                float l1, float l2, float l3, float* __restrict__ terms) {
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (size_t q = threadIdx.x; q < nblk; q += 256) {
#pragma unroll
    for (int c = 0; c < 4; ++c) s[c] += partial[q * 4 + c];
  }
  __shared__ double red[4][4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s[c] += __shfl_down(s[c], off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) red[threadIdx.x >> 6][c] = s[c];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double m[4];
    for (int c = 0; c < 4; ++c) m[c] = ((red[0][c] + red[1][c]) + (red[2][c] + red[3][c])) / n;
    for (int c = 0; c < 4; ++c) terms[c] = (float)m[c];
    terms[4] = (float)((((double)l0 * m[0] + (double)l1 * m[1]) + (double)l2 * m[2]) + (double)l3 * m[3]);
  }
}

int check_scene_params(const char* fn, const FnxSceneParams* p, bool obstacles) {
  if (obstacles) {
    if (p->n_max > FNX_SCENE_MAX_PRIMITIVES)
      return fnx::set_error(FNX_EINVAL, "%s: n_max %d is above the cap of %d primitives per scene", fn, p->n_max, FNX_SCENE_MAX_PRIMITIVES);
    if (p->n_min < 0 || p->n_min > p->n_max) return fnx::set_error(FNX_EINVAL, "%s: inverted range: n_min %d, n_max %d", fn, p->n_min, p->n_max);
    if (!(p->centre_min <= p->centre_max)) return fnx::set_error(FNX_EINVAL, "%s: inverted range: centre_min %g, centre_max %g", fn, p->centre_min, p->centre_max);
    if (!(p->size_min >= 0.f && p->size_min <= p->size_max)) return fnx::set_error(FNX_EINVAL, "%s: inverted range: size_min %g, size_max %g (0 <= min <= max)", fn, p->size_min, p->size_max);
  } else {
    if (p->octaves < 1 || p->octaves > FNX_SCENE_MAX_OCTAVES) return fnx::set_error(FNX_EINVAL, "%s: octaves %d outside 1 .. %d", fn, p->octaves, FNX_SCENE_MAX_OCTAVES);
    if (!(p->wavelength >= (float)(1 << (p->octaves - 1))))
      return fnx::set_error(FNX_EINVAL, "%s: wavelength %g cells is below 2^(octaves - 1) = %d (the finest octave needs a lattice of at least one cell)", fn,
                            p->wavelength, 1 << (p->octaves - 1));
    if (!(p->amplitude == p->amplitude) || !(p->density_scale == p->density_scale)) return fnx::set_error(FNX_EINVAL, "%s: amplitude or density_scale is NaN", fn);
  }
  return FNX_OK;
}

int scene_status(const char* fn) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? FNX_OK : fnx::set_error(FNX_EHIP, "%s: HIP error in a launch: %s", fn, hipGetErrorString(e));
}

}  // namespace
