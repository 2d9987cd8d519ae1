// FluidNet.forward (lib/model.py:76-227) around a pressure net for gfx950: the channel split, the _ScaleNet std, the net's input, the net
// by its record (fnx_fluidnet.h: the MultiScale net of fnx_cnn.hip or a bank net of fnx_banknet*.hip), velocityUpdate and the
// un-normalisation -- as the whole forward of every net (fluidnet_whole_forward), as the training forward and backward around a taped net,
// as the projection of the native step (fluidnet_core, fluidnet_pressure) and, on a z-slab, as the per-rank sums of the std over the whole
// domain.  All four nets, their trainers, the step and the slab driver call it.
// Built like fnx_cnn.hip (tolerance-checked, may contract a * b + c: the fp64 sums of squares of the std kernels do).
#include "fnx_fluidnet.h"
#include "fnx_cnn.h"
#include "fnx_kernels.h"
#include "../../include/fluidnet_hip.h"

namespace fnx {
namespace {

// _ScaleNet (model.py:8-23): unbiased std over C*D*H*W per sample, clamp(thr, inf).  Reproducible: every workgroup writes
// its own pair of fp64 partial sums (fixed element -> thread -> wave -> workgroup order, no atomics) and one workgroup per
// sample adds them up in index order.
constexpr int STD_MAXB = 1024;                              // partial pairs per sample
__device__ __forceinline__ void std_block_sum(double& s, double& ss, double (&red)[8]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { s += __shfl_down(s, off, 64); ss += __shfl_down(ss, off, 64); }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[2 * wave] = s; red[2 * wave + 1] = ss; }
  __syncthreads();
  s = (red[0] + red[2]) + (red[4] + red[6]);
  ss = (red[1] + red[3]) + (red[5] + red[7]);
}

__global__ __launch_bounds__(256) void std_partial_kernel(size_t n, const float* __restrict__ U, double* __restrict__ partial) {
  const int b = blockIdx.y;
  const float* u = U + (size_t)b * n;
  double s = 0.0, ss = 0.0;
  for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (size_t)gridDim.x * 256) {
    const double v = u[q];
    s += v; ss += v * v;
  }
  __shared__ double red[8];
  std_block_sum(s, ss, red);
  if (threadIdx.x == 0) {
    double* o = partial + 2 * ((size_t)b * STD_MAXB + blockIdx.x);
    o[0] = s; o[1] = ss;
  }
}

__global__ __launch_bounds__(256) void std_finish_kernel(int nb, size_t n, const double* __restrict__ partial, float thr,
                                                         float* __restrict__ scale) {
  const int b = blockIdx.x;
  const double* pb = partial + 2 * (size_t)b * STD_MAXB;
  double s = 0.0, ss = 0.0;
  for (int q = threadIdx.x; q < nb; q += 256) { s += pb[2 * q]; ss += pb[2 * q + 1]; }
  __shared__ double red[8];
  std_block_sum(s, ss, red);
  if (threadIdx.x == 0) {
    double var = (ss - s * s / (double)n) / (double)(n - 1);
    if (var < 0.0) var = 0.0;
    const float sd = (float)sqrt(var);
    scale[b] = sd < thr ? thr : sd;
  }
}

// x[b,0] = div/s ; x[b,1] = occupancy(flags) ; U /= s      (model.py:129-168)
__global__ __launch_bounds__(256) void pack_input_kernel(size_t n1, int nc, const float* __restrict__ div,
                                                         const float* __restrict__ flags,
                                                         const float* __restrict__ scale, float* __restrict__ U,
                                                         float* __restrict__ x) {
  const int b = blockIdx.y;
  const float s = scale[b];
  for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < n1; q += (size_t)gridDim.x * 256) {
    x[((size_t)b * 2) * n1 + q] = div[(size_t)b * n1 + q] / s;
    const float f = flags[(size_t)b * n1 + q];
    x[((size_t)b * 2 + 1) * n1 + q] = f == FNX_FLUID ? 0.f : (f == FNX_OBST ? 1.f : f);
    for (int c = 0; c < nc; ++c) {
      const size_t o = ((size_t)b * nc + c) * n1 + q;
      U[o] = U[o] / s;
    }
  }
}

// the fused step's variant: x[b,0] = velocityDivergence(U, flags) / s (velocity_divergence.py:46-74, the divergence_kernel's
// expression) ; x[b,1] = occupancy(flags); U is left as it is -- the pass behind the net divides and multiplies
// (launch_post_projection with `scale`).  x fastest: i = q % W.
template <bool IS3D>
__global__ __launch_bounds__(256) void pack_div_kernel(GridDims g, const float* __restrict__ U, const float* __restrict__ flags,
                                                       const float* __restrict__ scale, float* __restrict__ x) {
  const int b = blockIdx.y;
  const size_t n1 = (size_t)g.DHW;
  constexpr int NC = IS3D ? 3 : 2;
  const float s = scale[b];
  const float* u = U + (size_t)b * NC * n1;
  // (planes of the compute window only: a z-slab's last ghost plane has no +1 neighbour in the array)
  const size_t q0 = (size_t)g.K0 * g.HW, q1 = (size_t)(g.K0 + g.KN) * g.HW;
  for (size_t q = q0 + (size_t)blockIdx.x * 256 + threadIdx.x; q < q1; q += (size_t)gridDim.x * 256) {
    const int i = (int)(q % g.W), j = (int)((q / g.W) % g.H), k = (int)(q / g.HW);
    const float f = flags[(size_t)b * n1 + q];
    float d = 0.f;
    if (!is_border<IS3D>(g, i, j, k)) {
      d = ((u[q] - u[q + 1]) + u[n1 + q]) - u[n1 + q + g.W];
      if (IS3D) d = d + (u[2 * n1 + q] - u[2 * n1 + q + g.HW]);
    }
    if (f == FNX_OBST) d = 0.f;
    x[((size_t)b * 2) * n1 + q] = d / s;
    x[((size_t)b * 2 + 1) * n1 + q] = f == FNX_FLUID ? 0.f : (f == FNX_OBST ? 1.f : f);
  }
}

__global__ __launch_bounds__(256) void unscale_kernel(size_t n1, int nc, const float* __restrict__ scale,
                                                      float* __restrict__ p, float* __restrict__ U) {
  const int b = blockIdx.y;
  const float s = scale[b];
  for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < n1; q += (size_t)gridDim.x * 256) {
    p[(size_t)b * n1 + q] = p[(size_t)b * n1 + q] * s;
    for (int c = 0; c < nc; ++c) {
      const size_t o = ((size_t)b * nc + c) * n1 + q;
      U[o] = U[o] * s;
    }
  }
}

// input (B, nc+3, ...) = [p, U, flags, rho] -> U (B,nc,...), flags (B,1,...)
__global__ __launch_bounds__(256) void gather_input_kernel(size_t n1, int nc, const float* __restrict__ input,
                                                           float* __restrict__ U, float* __restrict__ flags) {
  const int b = blockIdx.y;
  const float* in = input + (size_t)b * (nc + 3) * n1;
  for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < n1; q += (size_t)gridDim.x * 256) {
    for (int c = 0; c < nc; ++c) U[((size_t)b * nc + c) * n1 + q] = in[(size_t)(1 + c) * n1 + q];
    flags[(size_t)b * n1 + q] = in[(size_t)(1 + nc) * n1 + q];
  }
}

// the grid of the streaming kernels above: at most 2048 blocks of 256 per sample
inline dim3 bgrid(size_t n1, int B) {
  size_t blocks = (n1 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  return dim3((unsigned)blocks, B);
}

// ---- _ScaleNet on a z-slab (fnx_slab_step, method 1): the std over the WHOLE domain from per-rank sums ----
constexpr int WIN_BLOCKS = 256;
// block q of sample b: sum and sum of squares (fp64) of its share of the planes [k0, k1) of every channel, in a fixed order
__global__ __launch_bounds__(256) void window_sums_partial_kernel(GridDims g, int nc, int k0, int k1, const float* __restrict__ U,
                                                                  double* __restrict__ partial) {
  const int b = blockIdx.y;
  const size_t per = (size_t)(k1 - k0) * g.HW, n = per * nc;
  const float* u = U + (size_t)b * nc * g.DHW;
  double s = 0.0, ss = 0.0;
  for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (size_t)gridDim.x * 256) {
    const size_t c = q / per, r = q - c * per;
    const double v = (double)u[c * g.DHW + (size_t)k0 * g.HW + r];
    s += v; ss += v * v;
  }
  __shared__ double red[8];
  std_block_sum(s, ss, red);
  if (threadIdx.x == 0) { partial[2 * ((size_t)b * WIN_BLOCKS + blockIdx.x)] = s; partial[2 * ((size_t)b * WIN_BLOCKS + blockIdx.x) + 1] = ss; }
}
// One block per sample: the partials in index order -> this rank's (sum, sumsq), written as three floats per double (exact:
// 24 + 24 + 5 bits) into ITS slots of `red` ([rank][sample][2][3]); every other slot is zeroed.  A float all-reduce(sum) over the
// ranks then IS an all-gather (x + 0 + ... + 0 is exact in any order), with the communicator's existing entry point.
__global__ __launch_bounds__(256) void window_sums_encode_kernel(int rank, int nranks, int B, const double* __restrict__ partial,
                                                                 float* __restrict__ red) {
  const int b = blockIdx.x;
  double s = 0.0, ss = 0.0;
  for (int q = threadIdx.x; q < WIN_BLOCKS; q += 256) { s += partial[2 * ((size_t)b * WIN_BLOCKS + q)]; ss += partial[2 * ((size_t)b * WIN_BLOCKS + q) + 1]; }
  __shared__ double sh[8];
  std_block_sum(s, ss, sh);
  for (int q = threadIdx.x; q < nranks * 6; q += 256) red[((size_t)(q / 6) * B + b) * 6 + q % 6] = 0.f;
  __syncthreads();
  if (threadIdx.x == 0) {
    float* o = red + ((size_t)rank * B + b) * 6;
    const double v[2] = {s, ss};
    for (int k = 0; k < 2; ++k) {
      const float f1 = (float)v[k]; const double r1 = v[k] - (double)f1;
      const float f2 = (float)r1; const float f3 = (float)(r1 - (double)f2);
      o[3 * k] = f1; o[3 * k + 1] = f2; o[3 * k + 2] = f3;
    }
  }
}
// the ranks' sums added in RANK ORDER (the same bits on every rank), unbiased std over n elements, clamp(thr, inf)   (model.py:14-21)
__global__ void scale_from_sums_kernel(int nranks, int B, double n, float thr, const float* __restrict__ red, float* __restrict__ scale) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double s = 0.0, ss = 0.0;
  for (int r = 0; r < nranks; ++r) {
    const float* o = red + ((size_t)r * B + b) * 6;
    s += ((double)o[0] + (double)o[1]) + (double)o[2];
    ss += ((double)o[3] + (double)o[4]) + (double)o[5];
  }
  double var = (ss - s * s / n) / (n - 1.0);
  if (var < 0.0) var = 0.0;
  const float sd = (float)sqrt(var);
  scale[b] = sd < thr ? thr : sd;
}

}  // namespace

size_t window_sums_scratch_bytes(int B) { return sizeof(double) * 2 * WIN_BLOCKS * (size_t)B; }
void launch_window_sums_encode(const GridDims& g, int nc, int k0, int k1, const float* U, int rank, int nranks, double* partial,
                               float* red, hipStream_t s) {
  window_sums_partial_kernel<<<dim3(WIN_BLOCKS, g.B), 256, 0, s>>>(g, nc, k0, k1, U, partial);
  window_sums_encode_kernel<<<g.B, 256, 0, s>>>(rank, nranks, g.B, partial, red);
}
void launch_scale_from_sums(int nranks, int B, double n, float thr, const float* red, float* scale, hipStream_t s) {
  scale_from_sums_kernel<<<(B + 63) / 64, 64, 0, s>>>(nranks, B, n, thr, red, scale);
}
void launch_pack_div(const GridDims& g, bool is3d, const float* U, const float* flags, const float* scale, float* x, hipStream_t s) {
  const dim3 grid = bgrid((size_t)g.KN * g.HW, g.B);
  if (is3d) pack_div_kernel<true><<<grid, 256, 0, s>>>(g, U, flags, scale, x);
  else pack_div_kernel<false><<<grid, 256, 0, s>>>(g, U, flags, scale, x);
}

size_t scale_std_scratch_bytes(int B) { return sizeof(double) * 2 * STD_MAXB * (size_t)B; }

void launch_scale_std(const GridDims& g, int nc, const float* U, float thr, double* partial, float* scale, hipStream_t s) {
  const size_t n = (size_t)nc * g.DHW;
  size_t nb = (n + 256 * 8 - 1) / (256 * 8);
  if (nb > STD_MAXB) nb = STD_MAXB;
  if (nb < 1) nb = 1;
  std_partial_kernel<<<dim3((unsigned)nb, g.B), 256, 0, s>>>(n, U, partial);
  std_finish_kernel<<<g.B, 256, 0, s>>>((int)nb, n, partial, thr, scale);
}

void launch_pack_input(const GridDims& g, int nc, const float* div, const float* flags, const float* scale, float* U,
                       float* x, hipStream_t s) {
  pack_input_kernel<<<bgrid(g.DHW, g.B), 256, 0, s>>>((size_t)g.DHW, nc, div, flags, scale, U, x);
}

void launch_unscale(const GridDims& g, int nc, const float* scale, float* p, float* U, hipStream_t s) {
  unscale_kernel<<<bgrid(g.DHW, g.B), 256, 0, s>>>((size_t)g.DHW, nc, scale, p, U);
}

void launch_gather_input(const GridDims& g, int nc, const float* input, float* U, float* flags, hipStream_t s) {
  gather_input_kernel<<<bgrid(g.DHW, g.B), 256, 0, s>>>((size_t)g.DHW, nc, input, U, flags);
}

FluidnetWs fluidnet_ws_layout(int B, size_t cells, size_t net_bytes, void* base) {
  const size_t full = (size_t)B * cells;
  size_t off = 0;
  auto take = [&](size_t bytes) { void* r = base ? (char*)base + off : nullptr; off += al256(bytes); return r; };
  FluidnetWs w{};
  w.div = (float*)take(full * 4);
  w.x = (float*)take(full * 2 * 4);
  w.partial = (double*)take(scale_std_scratch_bytes(B));
  w.head = off;
  w.scale = (float*)take(sizeof(float) * B);
  w.net = take(net_bytes);
  w.bytes = off;
  return w;
}

size_t fluidnet_ws_bytes(const GridDims& g, bool is3d) {
  return fluidnet_whole_ws_bytes(g.B, g.DHW, multiscale_ws_bytes(g, is3d));
}

int net_mode(int precision_mode) {
  if (precision_mode < FNX_PRECISION_FP32 || precision_mode > FNX_PRECISION_FP32_F2) return -1;
  return precision_mode == FNX_PRECISION_FP32_F4 ? FNX_PRECISION_FP32 : precision_mode;
}

void fluidnet_split(const FnxGrid* g, const float* input, float* U, float* flags, void* stream) {
  launch_gather_input(make_dims(g->B, g->D, g->H, g->W), g->is3D ? 3 : 2, input, U, flags, (hipStream_t)stream);   // model.py:104-119
}
int fluidnet_pre(const FnxGrid* g, float thr, float* U, const float* flags, float* scale, const FluidnetWs& w, void* stream) {
  const GridDims d = make_dims(g->B, g->D, g->H, g->W);          // (the launchers below read B and DHW alone)
  hipStream_t s = (hipStream_t)stream;
  const int nc = g->is3D ? 3 : 2;
  if (int rc = fnx_velocity_divergence(g, U, flags, w.div, stream)) return rc;   // model.py:125-126
  launch_scale_std(d, nc, U, thr, w.partial, scale, s);                          // model.py:129-144
  launch_pack_input(d, nc, w.div, flags, scale, U, w.x, s);                      // model.py:146-168
  return FNX_OK;
}
int fluidnet_post(const FnxGrid* g, float* p, float* U, const float* flags, const float* scale, void* stream) {
  if (int rc = fnx_velocity_update(g, p, U, flags, stream)) return rc;           // model.py:213-218
  launch_unscale(make_dims(g->B, g->D, g->H, g->W), g->is3D ? 3 : 2, scale, p, U, (hipStream_t)stream);   // model.py:221-223
  return fnx_set_wall_bcs(g, U, flags, stream);                                  // model.py:226
}

// the net by its kind and the grid's dimension (fnx_fluidnet.h)
const Net& net_of(int kind, bool is3d) {
  return kind == FNX_NET_BANK ? banknet_net() : (kind == FNX_NET_BANK3D ? banknet3d_net() : scalenet_net(is3d));
}
size_t fluidnet_core_ws_bytes(const FnxGrid* g, int net_kind) {
  return fluidnet_ws_layout(g->B, (size_t)g->D * g->H * g->W, net_of(net_kind, g->is3D).ws_bytes(g), nullptr).bytes;
}

// FluidNet.forward behind the channel split (model.py:120-227), U in place: U holds UDiv on entry and the projected velocity on exit.
// ws: fluidnet_ws_layout with the net's own workspace.  The caller reports the launch status.
static int fluidnet_around(const Net& n, const FnxGrid* g, const void* packed, const float* flags, float thr, int mode, float* p_out, float* U,
                           void* ws, void* stream) {
  const FluidnetWs w = fluidnet_ws_layout(g->B, (size_t)g->D * g->H * g->W, n.ws_bytes(g), ws);
  if (int rc = fluidnet_pre(g, thr, U, flags, w.scale, w, stream)) return rc;
  n.forward(g, packed, w.x, p_out, mode, w.net, (hipStream_t)stream);              // model.py:174-175 or :179-209
  return fluidnet_post(g, p_out, U, flags, w.scale, stream);
}

int fluidnet_whole_forward(const Net& n, const FnxGrid* g, const void* packed, const float* input, float thr, float* p_out, float* U_out,
                           int mode, void* ws, void* stream) {
  float* flags = (float*)ws;                       // contiguous (B,1,..) copy of the flags channel
  void* rest = (char*)ws + fluidnet_flags_bytes(g->B, (size_t)g->D * g->H * g->W);
  fluidnet_split(g, input, U_out, flags, stream);
  if (int rc = fluidnet_around(n, g, packed, flags, thr, mode, p_out, U_out, rest, stream)) return rc;
  return n.status();
}

int fluidnet_core(const FnxGrid* g, const void* packed, int net_kind, const float* flags, float thr, int precision_mode, float* p_out,
                  float* U, void* ws, void* stream, const FnxState* bcs) {
  const Net& n = net_of(net_kind, g->is3D);
  if (bcs) {
    // The fused step (fnx_simulate_step, convnet, no flags_stick): three launches around the net instead of eight, the same
    // arithmetic per value.  The divergence goes straight into the net's input, U is not rewritten before the net, and
    // velocityUpdate, the un-normalisation, setWallBcs and the step's last setConstVals (simulate.py:168) are one pass.
    const GridDims d = make_dims(g->B, g->D, g->H, g->W, g->z_offset, g->D_global);
    hipStream_t s = (hipStream_t)stream;
    const FluidnetWs w = fluidnet_ws_layout(d.B, d.DHW, n.ws_bytes(g), ws);
    launch_scale_std(d, g->is3D ? 3 : 2, U, thr, w.partial, w.scale, s);         // model.py:129-144
    launch_pack_div(d, g->is3D, U, flags, w.scale, w.x, s);                      // model.py:125-126, :146-168
    float* pnet = w.div;                                                         // (the divergence buffer is free here)
    n.forward(g, packed, w.x, pnet, precision_mode, w.net, s);
    ProfScope ps(FNX_PROF_STAGE, s);
    launch_post_projection(d, g->is3D, pnet, U, bcs->density, flags, bc_ptrs(bcs), s, bcs->density_bc_applied != 0, w.scale,
                           p_out);                                               // model.py:213-226, simulate.py:168
    return fnx::launch_status(g->is3D);
  }
  if (int rc = fluidnet_around(n, g, packed, flags, thr, precision_mode, p_out, U, ws, stream)) return rc;
  return fnx::launch_status(g->is3D);
}

// The hybrid projection's guess (fnx_simulate_step, method 3): the launches of the fused step in front of the net, the net straight
// into p_out, and the multiply launch_unscale applies to p (nc = 0: no velocity is touched).  The same arithmetic per value as
// fluidnet_core, so p_out holds the bits fnx_fluidnet_forward returns as p for this U.
int fluidnet_pressure(const FnxGrid* g, const void* packed, int net_kind, const float* flags, float thr, int precision_mode, float* p_out,
                      const float* U, void* ws, void* stream) {
  const Net& n = net_of(net_kind, g->is3D);
  const GridDims d = make_dims(g->B, g->D, g->H, g->W, g->z_offset, g->D_global);
  hipStream_t s = (hipStream_t)stream;
  const FluidnetWs w = fluidnet_ws_layout(d.B, d.DHW, n.ws_bytes(g), ws);        // (its divergence buffer is not used here)
  launch_scale_std(d, g->is3D ? 3 : 2, U, thr, w.partial, w.scale, s);           // model.py:129-144
  launch_pack_div(d, g->is3D, U, flags, w.scale, w.x, s);                        // model.py:125-126, :146-168
  n.forward(g, packed, w.x, p_out, precision_mode, w.net, s);
  launch_unscale(d, 0, w.scale, p_out, nullptr, s);                              // model.py:221-222
  return fnx::launch_status(g->is3D);
}

// ---- training: the same stages around a taped net, and their adjoints in front of the net's backward ----
size_t fluidnet_train_ws_bytes(const NetTrain& n, const FnxGrid* g) {
  // forward: div, x (2), std partials; backward: the wall-masked scaled grad_U, grad_U of the update, its grad_p, g_net, the net's own
  const size_t fwd = fluidnet_ws_layout(g->B, (size_t)g->D * g->H * g->W, 0, nullptr).head;
  const size_t bwd = fluidnet_train_bwd_ws(n.ndim, g, nullptr).bytes + n.backward_ws_bytes(g);
  return fwd > bwd ? fwd : bwd;
}

int fluidnet_forward_train(const NetTrain& n, const FnxGrid* g, const void* packed, const float* input, float thr, float* p_out, float* U_out,
                           float* flags_out, float* scale_out, float* tape, int mode, void* ws, void* stream) {
  FluidnetWs w = fluidnet_ws_layout(g->B, (size_t)g->D * g->H * g->W, 0, ws);      // (its head: the scales go to scale_out)
  if (n.tape_x) w.x = tape + n.tape_x(g);                                          // the backward reads the net's input again
  fluidnet_split(g, input, U_out, flags_out, stream);
  if (int rc = fluidnet_pre(g, thr, U_out, flags_out, scale_out, w, stream)) return rc;
  n.forward(g, packed, w.x, p_out, tape, mode, (hipStream_t)stream);
  if (int rc = fluidnet_post(g, p_out, U_out, flags_out, scale_out, stream)) return rc;
  return n.status();
}

int fluidnet_backward(const NetTrain& n, const FnxGrid* g, const void* packed_t, const float* flags, const float* scale, const float* grad_p,
                      const float* grad_U, const float* tape, float* grad_blob, int mode, void* ws, void* stream, bool* launched) {
  *launched = true;
  const FluidnetTrainBwdWs w = fluidnet_train_bwd_ws(n.ndim, g, ws);
  // g_net = s g_p + velocity_update_backward_p(s setWallBcs(g_U)): the adjoints of model.py:226, :221-223 and :213-218 in reverse
  if (int rc = fluidnet_train_gnet(n.ndim, g, flags, scale, grad_p, grad_U, w, stream)) return rc;
  *launched = n.backward(g, packed_t, n.tape_x ? tape + n.tape_x(g) : nullptr, w.gnet, tape, grad_blob, mode, w.net, (hipStream_t)stream);
  return *launched ? n.status() : FNX_OK;
}
}  // namespace fnx

// ---------------------------------------------------------------------------------------------------
// C ABI (include/fluidnet_hip.h)
// ---------------------------------------------------------------------------------------------------
extern "C" {

int fnx_fluidnet_forward(const FnxGrid* g, const void* packed, const float* input, float thr, float* p_out,
                         float* U_out, int precision_mode, void* ws, size_t ws_bytes, void* stream) {
  int mode;
  if (int rc = fnx::check_net_call(__func__, g, packed && input && p_out && U_out && ws, precision_mode, &mode, fnx::fluidnet_ws_bytes, ws_bytes))
    return rc;
  return fnx::fluidnet_whole_forward(fnx::scalenet_net(g->is3D), g, packed, input, thr, p_out, U_out, mode, ws, stream);
}

}  // extern "C"
