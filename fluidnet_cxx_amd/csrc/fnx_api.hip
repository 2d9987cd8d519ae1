// C-ABI of libfluidnet_hip.so (include/fluidnet_hip.h): argument checks, workspace carving and the launch
// sequences.  No allocation, no synchronisation (except fnx_jacobi with p_tol > 0), no CPU fallback.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "../../include/fluidnet_hip.h"
#include "fnx_fluidnet.h"
#include "fnx_kernels.h"
#include <algorithm>
#include <atomic>
#include <dlfcn.h>

namespace {
thread_local char g_err[512] = "";
}
// the thread's message (fnx_last_error) and the code to return, for every unit (fnx_kernels.h)
int fnx::set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

namespace {

constexpr auto fail = fnx::set_error;      // (this unit's older name for it)

#define HIP_OK(expr)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess) return fail(FNX_EHIP, "HIP error: %s (%s)", hipGetErrorString(e_), #expr); \
  } while (0)

int check_grid(const FnxGrid* g) {
  if (!g) return fail(FNX_EINVAL, "grid descriptor is NULL");
  if (g->B < 1 || g->D < 1 || g->H < 3 || g->W < 3) return fail(FNX_EINVAL, "Dimension mismatch: B=%d D=%d H=%d W=%d", g->B, g->D, g->H, g->W);
  if (!g->is3D && g->D != 1) return fail(FNX_EINVAL, "2D velocity field but zdepth > 1");
  if (g->is3D && g->D < 3) return fail(FNX_EINVAL, "3D domain needs D >= 3");
  if ((long long)g->D * g->H * g->W >= (1ll << 31)) return fail(FNX_EINVAL, "more than 2^31 cells per sample");
  if ((long long)g->B * g->D > 65535) return fail(FNX_EINVAL, "B*D > 65535 not supported");
  if (!g->is3D && (g->W > 65535 || g->H > 65535)) return fail(FNX_EINVAL, "2D grids wider or taller than 65535 are not supported");
  if (g->k_end != 0 || g->k_begin != 0) {
    if (!g->is3D || g->k_begin < 0 || g->k_end > g->D || g->k_end <= g->k_begin)
      return fail(FNX_EINVAL, "bad compute window [%d, %d) for D=%d", g->k_begin, g->k_end, g->D);
  }
  if (g->D_global != 0 && (!g->is3D || g->z_offset < 0 || g->z_offset + g->D > g->D_global))
    return fail(FNX_EINVAL, "bad z-slab: z_offset=%d D=%d D_global=%d", g->z_offset, g->D, g->D_global);
  return FNX_OK;
}

inline GridDims dims(const FnxGrid* g) {
  GridDims d = make_dims(g->B, g->D, g->H, g->W, g->z_offset, g->D_global);
  if (g->is3D && g->k_end > g->k_begin) { d.K0 = g->k_begin; d.KN = g->k_end - g->k_begin; }
  return d;
}
inline bool quirks(const FnxGrid* g) { return g->is3D && (g->ref_quirks & 1); }
inline int jacobi3d_x(const FnxGrid* g) { return (g->ref_quirks >> FNX_JACOBI3D_X_SHIFT) & 3; }   // the forced tiling of the two-sweep march, if any
inline size_t ncell(const FnxGrid* g) { return (size_t)g->B * g->D * g->H * g->W; }
inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

struct Carver {
  char* base; size_t off;
  explicit Carver(void* p) : base((char*)p), off(0) {}
  void* take(size_t bytes) { void* r = base ? base + off : nullptr; off += al(bytes); return r; }
};

// advection: the forward fields of `what` and the tile kernels' fix-up bitmaps (the layout is fnx::advect_workspace's)
size_t ws_advect(const FnxGrid* g, int what) { return fnx::advect_workspace(dims(g), g->is3D, what, nullptr).bytes; }
// 3D solver: the neighbour mask by rows and by row groups and the planes-alike bits (the layout is fnx::jacobi3d_mask_layout's)
size_t ws_mask(const FnxGrid* g) { return g->is3D ? fnx::jacobi3d_mask_layout(dims(g), nullptr).bytes : 0; }
// Jacobi workspace: ping-pong pressure, the residual's fixed-order partial sums, one result float, the 3D neighbour mask.  Returns
// the bytes it takes; ws == nullptr: the size only.
struct JacobiWs { float* tmp; double* partials; float* res; fnx::JacobiMaskLayout mask; };
size_t carve_jacobi(const FnxGrid* g, void* ws, JacobiWs* out) {
  Carver c(ws);
  out->tmp = (float*)c.take(ncell(g) * 4);
  out->partials = (double*)c.take(fnx::residual_scratch_bytes(g->B));
  out->res = (float*)c.take(4);
  out->mask = fnx::jacobi3d_mask_layout(dims(g), g->is3D ? c.take(ws_mask(g)) : nullptr);
  return c.off;
}
size_t ws_jacobi(const FnxGrid* g) { JacobiWs W; return carve_jacobi(g, nullptr, &W); }
// PCG: the multigrid hierarchy (kept between steps by fnx_simulate_step), then the solver's vectors
size_t ws_pcg_kept(const FnxGrid* g) { return al(fnx::pcg_kept_bytes(dims(g), g->is3D)); }
size_t ws_pcg(const FnxGrid* g) { return ws_pcg_kept(g) + al(fnx::pcg_scratch_bytes(dims(g), g->is3D)); }
// neither a whole domain nor all of its planes: a compute window or a z-slab view
inline bool is_view(const FnxGrid* g) { return g->k_begin != 0 || g->k_end != 0 || g->z_offset != 0 || g->D_global != 0; }
// The step's workspace (the layout is fnx::step_layout's).  Its tail serves, one after the other, the users named here.
fnx::StepLayout carve_step(const FnxGrid* g, void* ws) {
  const GridDims d = dims(g);
  const size_t advect = ws_advect(g, fnx::ADVECT_BOTH);              // the fused advection launches keep both forward fields at once
  const size_t jacobi = ws_jacobi(g);                               // sized as the stand-alone solve (its 3D mask is the kept one)
  const size_t net = fnx::fluidnet_ws_bytes(d, g->is3D);            // the convnet projection, the hybrid's guess
  const size_t pcg = al(fnx::pcg_scratch_bytes(d, g->is3D));        // the PCG solve's vectors
  const size_t periodic = fnx::periodic_save_bytes(d);              // the patches' source row and column around the post-projection pass
  const size_t tail_need = std::max({advect, jacobi, net, pcg, periodic});
  return fnx::step_layout(ncell(g), g->is3D ? 3 : 2, g->is3D != 0, ws_mask(g), ws_pcg_kept(g), tail_need, ws);
}
size_t ws_step(const FnxGrid* g) { return carve_step(g, nullptr).bytes; }
// the step's workspace with, in 3D, room for the stage word map behind it (fnx_step_plan.h)
size_t ws_step_static(const FnxGrid* g) {
  const fnx::StepLayout L = carve_step(g, nullptr);
  return g->is3D ? fnx::stage_word_offset(L) + al(fnx::stage_word_bytes(ncell(g), true)) : L.bytes;
}

}  // namespace

// ---- event-pair profiler ----------------------------------------------------------------------------
namespace fnx {
namespace {
constexpr int PROF_MAX = 16384;
struct Prof {
  bool on = false;
  bool runs = false;               // fnx_profile_enable(2): ONE event pair around a run of consecutive launches of a class on a stream
  int n = 0;
  hipEvent_t ev[PROF_MAX][2];
  int tag[PROF_MAX];
  int count[PROF_MAX];             // launches between the pair
  hipStream_t stream[PROF_MAX];
  int created = 0;
  int open_idx[FNX_PROF_NTAGS];
  double work[FNX_PROF_NTAGS];     // what the recorded launches of a class issued (MFMA FLOPs for the conv classes)
} g_prof;
}  // namespace

// roctx ranges around the same phases (the reference has no tracing hooks; rocprofv3 --marker-trace shows
// them).  The marker library is resolved on request (fnx_roctx_enable), never linked: without it the ranges are no-ops.
namespace {
struct Roctx { int (*push)(const char*) = nullptr; int (*pop)() = nullptr; std::atomic<bool> on{false}; } g_roctx;
const char* const kProfNames[FNX_PROF_NTAGS] = {"fnx:jacobi", "fnx:conv_mfma", "fnx:advect", "fnx:stage", "fnx:conv_direct", "fnx:conv_mfma16", "fnx:conv_bf16"};
}  // namespace

// A scope pops the range it pushed and no other: fnx_roctx_enable may be toggled (from another thread, or inside an open scope
// such as the pTol loop of a solve) between a scope's begin and end.
bool prof_begin(int tag, hipStream_t s) {
  const bool pushed = g_roctx.on.load(std::memory_order_acquire);
  if (pushed) g_roctx.push(kProfNames[tag]);
  if (!g_prof.on || g_prof.n >= PROF_MAX) { if (g_prof.on) g_prof.open_idx[tag] = -1; return pushed; }
  if (g_prof.runs && g_prof.n > 0 && g_prof.tag[g_prof.n - 1] == tag && g_prof.stream[g_prof.n - 1] == s) {
    // the launch before this one on the stream was of the same class: extend its pair (prof_end records the end event again) -- events between
    // back-to-back launches keep the next kernel from starting behind the one before it, and each then reads 3-5 % long
    g_prof.open_idx[tag] = g_prof.n - 1;
    ++g_prof.count[g_prof.n - 1];
    return pushed;
  }
  const int i = g_prof.n++;
  if (i >= g_prof.created) {
    hipEventCreate(&g_prof.ev[i][0]); hipEventCreate(&g_prof.ev[i][1]);
    g_prof.created = i + 1;
  }
  g_prof.tag[i] = tag;
  g_prof.count[i] = 1;
  g_prof.stream[i] = s;
  g_prof.open_idx[tag] = i;
  hipEventRecord(g_prof.ev[i][0], s);
  return pushed;
}

void prof_add_work(int tag, double amount) {
  if (g_prof.on && g_prof.open_idx[tag] >= 0) g_prof.work[tag] += amount;
}

void prof_end(int tag, hipStream_t s, bool pushed) {
  if (pushed) g_roctx.pop();
  if (!g_prof.on) return;
  const int i = g_prof.open_idx[tag];
  if (i >= 0) hipEventRecord(g_prof.ev[i][1], s);
}
}  // namespace fnx

extern "C" {

int fnx_profile_enable(int on) {
  fnx::g_prof.on = on != 0;
  fnx::g_prof.runs = on == 2;
  if (on) { fnx::g_prof.n = 0; for (int t = 0; t < FNX_PROF_NTAGS; ++t) { fnx::g_prof.open_idx[t] = -1; fnx::g_prof.work[t] = 0.0; } }
  return FNX_OK;
}

int fnx_roctx_enable(int on) {
  if (!on) { fnx::g_roctx.on.store(false, std::memory_order_release); return FNX_OK; }
  if (!fnx::g_roctx.push) {
    void* h = nullptr;
    for (const char* name : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"}) {
      h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (h) break;
    }
    if (!h) return fail(FNX_EINVAL, "roctx_enable: no roctx library found (librocprofiler-sdk-roctx.so / libroctx64.so)");
    fnx::g_roctx.push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
    fnx::g_roctx.pop = (int (*)())dlsym(h, "roctxRangePop");
    if (!fnx::g_roctx.push || !fnx::g_roctx.pop) { fnx::g_roctx.push = nullptr; return fail(FNX_EINVAL, "roctx_enable: roctxRangePushA / roctxRangePop not found"); }
  }
  fnx::g_roctx.on.store(true, std::memory_order_release);
  return FNX_OK;
}

int fnx_profile_read_work(int tag, double* work) {
  if (tag < 0 || tag >= FNX_PROF_NTAGS || !work) return fail(FNX_EINVAL, "profile_read_work: bad tag");
  *work = fnx::g_prof.work[tag];
  return FNX_OK;
}

int fnx_profile_read(int tag, double* total_ms, int* launches) {
  double tot = 0.0; int cnt = 0;
  for (int i = 0; i < fnx::g_prof.n; ++i) {
    if (fnx::g_prof.tag[i] != tag) continue;
    if (hipEventSynchronize(fnx::g_prof.ev[i][1]) != hipSuccess) continue;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, fnx::g_prof.ev[i][0], fnx::g_prof.ev[i][1]) == hipSuccess) { tot += ms; cnt += fnx::g_prof.count[i]; }
  }
  if (total_ms) *total_ms = tot;
  if (launches) *launches = cnt;
  return FNX_OK;
}

const char* fnx_last_error(void) { return g_err; }
int fnx_abi_version(void) { return FNX_ABI_VERSION; }

const char* fnx_device_name(void) {
  static thread_local char name[256];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { fail(FNX_EHIP, "no HIP device"); return nullptr; }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) { fail(FNX_EHIP, "no HIP device"); return nullptr; }
  snprintf(name, sizeof(name), "%s (%s)", prop.name, prop.gcnArchName);
  return name;
}

size_t fnx_workspace_bytes(const FnxGrid* g, int op) {
  if (check_grid(g) != FNX_OK) return 0;
  switch (op) {
    case FNX_OP_ADVECT_SCALAR: return ws_advect(g, fnx::ADVECT_RHO);
    case FNX_OP_ADVECT_VEL: return ws_advect(g, fnx::ADVECT_VEL);
    case FNX_OP_JACOBI: return ws_jacobi(g);
    case FNX_OP_STEP: return ws_step(g);
    case FNX_OP_FLUIDNET: return fnx::fluidnet_ws_bytes(dims(g), g->is3D);
    case FNX_OP_ADVECT_STEP: return ws_advect(g, fnx::ADVECT_BOTH);
    case FNX_OP_STEP_STATIC: return ws_step_static(g);
  }
  fail(FNX_EINVAL, "unknown op %d", op);
  return 0;
}

// What the three advection entry points do after their argument checks: plan, carve, launch.  The stand-alone operators take the
// LDS tile kernels of the pair with their part only (3D default semantics; 2D from 1.5 M cells): same bits as one thread per cell
// (fnx_advect_march.h), ~1.5x faster in 3D.
static int advect_run(const char* name, const FnxGrid* g, int what, int method, int plan, const fnx::AdvectArgs& a, void* ws,
                      size_t ws_bytes, void* stream) {
  const fnx::AdvectPlan p = fnx::advect_plan(dims(g), g->is3D, quirks(g), what, a.orig == a.U, method, plan);
  fnx::AdvectWs w{};
  if (p.maccormack) {                                    // Euler writes dst directly and takes no workspace
    w = fnx::advect_workspace(p.g, g->is3D, what, ws);
    if (!ws || w.bytes > ws_bytes) return fail(FNX_EWORKSPACE, "%s: workspace too small (%zu < %zu)", name, ws_bytes, w.bytes);
  }
  hipStream_t s = (hipStream_t)stream;
  fnx::ProfScope ps(FNX_PROF_ADVECT, s);
  fnx::launch_advect(p, a, w, s);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

int fnx_advect_scalar(const FnxGrid* g, float dt, const float* src, const float* U, const float* flags, float* dst,
                      int method, int bnd, int sample_outside, float strength, void* ws, size_t ws_bytes,
                      void* stream) {
  return fnx_advect_scalar_plan(g, dt, src, U, flags, dst, method, bnd, sample_outside, strength, FNX_ADVECT_PLAN_AUTO, ws, ws_bytes, stream);
}

int fnx_advect_scalar_plan(const FnxGrid* g, float dt, const float* src, const float* U, const float* flags, float* dst,
                           int method, int bnd, int sample_outside, float strength, int plan, void* ws, size_t ws_bytes,
                           void* stream) {
  if (int rc = check_grid(g)) return rc;
  if (plan < FNX_ADVECT_PLAN_AUTO || plan > FNX_ADVECT_PLAN_TILES_SPLIT) return fail(FNX_EINVAL, "advect_scalar: unknown plan %d", plan);
  if (!src || !U || !flags || !dst) return fail(FNX_EINVAL, "advect_scalar: NULL tensor");
  if (dst == src) return fail(FNX_EINVAL, "advect_scalar: dst must not alias src");
  if (method != FNX_ADVECT_EULER && method != FNX_ADVECT_MACCORMACK) return fail(FNX_EMETHOD, "Advection method not supported");
  if (bnd != 1) return fail(FNX_EINVAL, "advect_scalar: only boundary_width == 1 is supported (the reference's MAC sampling strips exactly one border cell)");
  const fnx::AdvectArgs a{dt, strength * 0.5f, sample_outside != 0, src, U, U, flags, dst, nullptr};
  return advect_run("advect_scalar", g, fnx::ADVECT_RHO, method, plan, a, ws, ws_bytes, stream);
}

int fnx_advect_vel(const FnxGrid* g, float dt, const float* orig, const float* U, const float* flags, float* dst,
                   int method, int bnd, float strength, void* ws, size_t ws_bytes, void* stream) {
  return fnx_advect_vel_plan(g, dt, orig, U, flags, dst, method, bnd, strength, FNX_ADVECT_PLAN_AUTO, ws, ws_bytes, stream);
}

int fnx_advect_vel_plan(const FnxGrid* g, float dt, const float* orig, const float* U, const float* flags, float* dst,
                        int method, int bnd, float strength, int plan, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_grid(g)) return rc;
  if (plan < FNX_ADVECT_PLAN_AUTO || plan > FNX_ADVECT_PLAN_TILES_SPLIT) return fail(FNX_EINVAL, "advect_vel: unknown plan %d", plan);
  if (!orig || !U || !flags || !dst) return fail(FNX_EINVAL, "advect_vel: NULL tensor");
  if (dst == orig || dst == U) return fail(FNX_EINVAL, "advect_vel: dst must not alias orig or U");
  if (method != FNX_ADVECT_EULER && method != FNX_ADVECT_MACCORMACK) return fail(FNX_EMETHOD, "Advection method not supported");
  if (bnd != 1) return fail(FNX_EINVAL, "advect_vel: only boundary_width == 1 is supported");
  const fnx::AdvectArgs a{dt, strength * 0.5f, false, nullptr, orig, U, flags, nullptr, dst};
  return advect_run("advect_vel", g, fnx::ADVECT_VEL, method, plan, a, ws, ws_bytes, stream);
}

int fnx_advect_step(const FnxGrid* g, float dt, const float* density, const float* U, const float* flags,
                    float* density_dst, float* U_dst, int sample_outside, float strength, void* ws, size_t ws_bytes,
                    void* stream) {
  return fnx_advect_step_plan(g, dt, density, U, flags, density_dst, U_dst, sample_outside, strength, FNX_ADVECT_PLAN_AUTO, ws, ws_bytes, stream);
}

int fnx_advect_step_plan(const FnxGrid* g, float dt, const float* density, const float* U, const float* flags,
                         float* density_dst, float* U_dst, int sample_outside, float strength, int plan, void* ws,
                         size_t ws_bytes, void* stream) {
  if (int rc = check_grid(g)) return rc;
  if (plan < FNX_ADVECT_PLAN_AUTO || plan > FNX_ADVECT_PLAN_TILES_SPLIT) return fail(FNX_EINVAL, "advect_step: unknown plan %d", plan);
  if (!density || !U || !flags || !density_dst || !U_dst) return fail(FNX_EINVAL, "advect_step: NULL tensor");
  if (density_dst == density || U_dst == U) return fail(FNX_EINVAL, "advect_step: dst must not alias the inputs");
  const fnx::AdvectArgs a{dt, strength * 0.5f, sample_outside != 0, density, U, U, flags, density_dst, U_dst};
  return advect_run("advect_step", g, fnx::ADVECT_BOTH, FNX_ADVECT_MACCORMACK, plan, a, ws, ws_bytes, stream);
}

// passive scalars (fnx_scalars.hip): every refusal comes before a pointer is read
static int check_scalars_grid(const FnxGrid* g, int channels) {
  if (int rc = check_grid(g)) return rc;
  if (channels < 1) return fail(FNX_EINVAL, "advect_scalars: channels < 1 (%d)", channels);
  if (is_view(g)) return fail(FNX_EINVAL, "advect_scalars: no compute window or z-slab view (single-domain only)");
  if ((g->H + 3) / 4 > 65535) return fail(FNX_EINVAL, "advect_scalars: H/4 > 65535 not supported");
  // the 3D clamp-bounds launch carries the channels in its grid's z extent
  if (g->is3D && (long long)g->B * channels * fnx::advect_scalars_box_chunks(dims(g)) > 65535)
    return fail(FNX_EINVAL, "advect_scalars: B*channels*ceil(D/16) > 65535 not supported");
  return FNX_OK;
}

size_t fnx_advect_scalars_workspace_bytes(const FnxGrid* g, int channels) {
  if (check_scalars_grid(g, channels) != FNX_OK) return 0;
  return fnx::advect_scalars_workspace(dims(g), g->is3D != 0, channels, nullptr).bytes;
}

int fnx_advect_scalars(const FnxGrid* g, float dt, int channels, const float* src, const float* U, const float* flags, float* dst,
                       int method, int bnd, int sample_outside, float strength, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_scalars_grid(g, channels)) return rc;
  if (!src || !U || !flags || !dst) return fail(FNX_EINVAL, "advect_scalars: NULL tensor");
  if (dst == src) return fail(FNX_EINVAL, "advect_scalars: dst must not alias src");
  if (method != FNX_ADVECT_EULER && method != FNX_ADVECT_MACCORMACK) return fail(FNX_EMETHOD, "Advection method not supported");
  if (bnd != 1) return fail(FNX_EINVAL, "advect_scalars: only boundary_width == 1 is supported (the reference's MAC sampling strips exactly one border cell)");
  const bool mac = method == FNX_ADVECT_MACCORMACK;
  fnx::AdvectScalarsWs w{};
  if (mac) {                                             // Euler writes dst directly and takes no workspace
    w = fnx::advect_scalars_workspace(dims(g), g->is3D != 0, channels, ws);
    if (!ws || w.bytes > ws_bytes) return fail(FNX_EWORKSPACE, "advect_scalars: workspace too small (%zu < %zu)", ws ? ws_bytes : (size_t)0, w.bytes);
  }
  hipStream_t s = (hipStream_t)stream;
  fnx::ProfScope ps(FNX_PROF_ADVECT, s);
  fnx::launch_advect_scalars(dims(g), g->is3D != 0, quirks(g), mac, sample_outside != 0, dt, strength * 0.5f, channels, src, U, flags, dst,
                             w, s);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

int fnx_velocity_divergence(const FnxGrid* g, const float* U, const float* flags, float* div, void* stream) {
  if (int rc = check_grid(g)) return rc;
  if (!U || !flags || !div) return fail(FNX_EINVAL, "velocity_divergence: NULL tensor");
  fnx::launch_divergence(dims(g), g->is3D, U, flags, div, (hipStream_t)stream);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

// Jacobi (the decisions are fnx_jacobi_plan.h's).  What every entry point does after its argument checks: carve the workspace, refusing
// under its name, and in 3D build the neighbour mask unless the one in place is current (kept_mask: it lives there, not in the workspace)
static int jacobi_begin(const char* name, const FnxGrid* g, const float* flags, void* ws, size_t ws_bytes, bool reuse_mask,
                        hipStream_t s, JacobiWs* W, unsigned char* kept_mask = nullptr) {
  const size_t need = carve_jacobi(g, ws, W);
  if (!ws || need > ws_bytes) return fail(FNX_EWORKSPACE, "%s: workspace too small (%zu < %zu)", name, ws_bytes, need);
  if (g->is3D && kept_mask) W->mask = fnx::jacobi3d_mask_layout(dims(g), kept_mask);
  if (g->is3D && !reuse_mask) fnx::launch_jacobi3d_mask(dims(g), quirks(g), flags, W->mask, s);
  return FNX_OK;
}

// the output planes [kb, ke) of a 3D pass (whole_ok: ke == 0 stands for all planes) and its second range [kb2, kb2 + ke - kb), if any
static int check_plane_ranges(const char* name, const FnxGrid* g, int kb, int ke, int kb2, bool whole_ok) {
  if (kb < 0 || ke > g->D || ((ke != 0 || !whole_ok) && ke <= kb)) return fail(FNX_EINVAL, "%s: bad plane range", name);
  const int n = ke - kb;
  if (kb2 >= 0 && (ke == 0 || kb2 + n > g->D || (kb2 < ke && kb < kb2 + n)))
    return fail(FNX_EINVAL, "%s: bad or overlapping second plane range", name);
  return FNX_OK;
}

// Issues the launches of a schedule, one profiler scope each: launch l reads what launch l - 1 wrote (the first: `in`, NULL = all zeros,
// not read) and writes buf[(first + l) & 1].  Returns where the result lies.  The one place that chooses between the 2D and 3D launches.
static const float* run_jacobi_launches(const FnxGrid* g, const fnx::JacobiSchedule& sch, const float* flags, const float* div,
                                        const fnx::JacobiMaskLayout& mask, const float* in, float* const buf[2], int first,
                                        hipStream_t s) {
  const GridDims d = dims(g);
  for (int l = 0; l < sch.n; ++l) {
    const fnx::JacobiLaunch L = sch.at(l);
    float* out = buf[(first + l) & 1];
    fnx::ProfScope ps(FNX_PROF_JACOBI, s);
    if (!g->is3D) fnx::launch_jacobi(d, flags, div, in, out, L.sweeps, in == nullptr, s);
    else if (L.sweeps == 2) fnx::launch_jacobi3d_x2(d, mask, div, in, out, s, 0, 0, in == nullptr, -1, L.lay, nullptr, jacobi3d_x(g));
    else fnx::launch_jacobi3d(d, mask, div, in, out, in == nullptr, s);
    in = out;
  }
  return in;
}

static int jacobi_solve(const FnxGrid* g, const float* flags, const float* div, float* p, float* residual, float p_tol,
                        int max_iter, int* iters_done, void* ws, size_t ws_bytes, unsigned char* kept_mask, bool reuse_mask,
                        void* stream, int verbose) {
  if (int rc = check_grid(g)) return rc;
  if (!flags || !div || !p) return fail(FNX_EINVAL, "solve_linear_system: NULL tensor");
  if (max_iter < 1) return fail(FNX_EINVAL, "At least 1 iteration is needed (maxIter < 1)");
  hipStream_t s = (hipStream_t)stream;
  const GridDims d = dims(g);
  JacobiWs W;                                           // kept_mask: a slot nothing else in the step scribbles on; only such a mask can be current
  if (int rc = jacobi_begin("solve_linear_system", g, flags, ws, ws_bytes, reuse_mask && kept_mask, s, &W, kept_mask)) return rc;
  float* const buf[2] = {p, W.tmp};
  const int cus = cu_count();
  const fnx::JacobiSchedule one = fnx::jacobi_schedule(d, g->is3D, 1, cus);      // the residual's sweep, the per-sweep test's
  // ||a - b||_2 per sample, max over the batch, reproducible (fixed-order fp64 partial sums, no atomics)
  const size_t per = (size_t)g->D * g->H * g->W;
  auto residual_of = [&](const float* a, const float* b, float* out) { fnx::launch_residual(g->B, per, 0, per, a, b, W.partials, nullptr, out, s); };
  const bool per_sweep = p_tol > 0.f || verbose;        // the reference's per-sweep host test / per-sweep print
  if (!per_sweep) {
    // When the caller wants the residual ||p_n - p_(n-1)||, the last sweep runs on its own so that both iterates are in memory.
    const fnx::JacobiSchedule sch = fnx::jacobi_schedule(d, g->is3D, residual ? max_iter - 1 : max_iter, cus);
    if (sch.n > fnx::JACOBI_MAX_LAUNCHES) return fail(FNX_EINVAL, "solve_linear_system: max_iter too large for one call (%d)", max_iter);
    const float* in = run_jacobi_launches(g, sch, flags, div, W.mask, nullptr, buf, fnx::jacobi_solve_first_buffer(sch, residual != nullptr), s);
    if (residual) {
      run_jacobi_launches(g, one, flags, div, W.mask, in, buf, 0, s);
      residual_of(p, in, residual);
    }
    if (iters_done) *iters_done = max_iter;
  } else {
    // the reference's own per-sweep convergence test (fluids_init.cpp:961-979): one host read per sweep
    const float* in = nullptr;
    int sweeps = 0;
    float r = 0.f;
    for (;;) {
      const float* out = run_jacobi_launches(g, one, flags, div, W.mask, in, buf, sweeps & 1, s);
      residual_of(out, in, W.res);
      HIP_OK(hipMemcpyAsync(&r, W.res, 4, hipMemcpyDeviceToHost, s));
      HIP_OK(hipStreamSynchronize(s));
      in = out;
      ++sweeps;
      if (verbose) printf("Jacobi iteration %d: residual %g\n", sweeps, (double)r);      // fluids_init.cpp:968-971
      if (r < p_tol) {
        if (verbose) printf("Jacobi max residual fell below p_tol (%g) (terminating)\n", (double)p_tol);          // :973-978
        break;
      }
      if (sweeps >= max_iter) {
        if (verbose) printf("Jacobi max iteration count (%d) reached (terminating)\n", max_iter);                 // :982-987
        break;
      }
    }
    if (verbose) fflush(stdout);
    if (in != p) HIP_OK(hipMemcpyAsync(p, in, ncell(g) * 4, hipMemcpyDeviceToDevice, s));
    if (residual) HIP_OK(hipMemcpyAsync(residual, W.res, 4, hipMemcpyDeviceToDevice, s));
    if (iters_done) *iters_done = sweeps;
  }
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

int fnx_jacobi(const FnxGrid* g, const float* flags, const float* div, float* p, float* residual, float p_tol,
               int max_iter, int* iters_done, void* ws, size_t ws_bytes, void* stream) {
  return jacobi_solve(g, flags, div, p, residual, p_tol, max_iter, iters_done, ws, ws_bytes, nullptr, false, stream, 0);
}

int fnx_jacobi_verbose(const FnxGrid* g, const float* flags, const float* div, float* p, float* residual, float p_tol,
                       int max_iter, int* iters_done, void* ws, size_t ws_bytes, void* stream) {
  return jacobi_solve(g, flags, div, p, residual, p_tol, max_iter, iters_done, ws, ws_bytes, nullptr, false, stream, 1);
}

int fnx_jacobi_sweeps(const FnxGrid* g, const float* flags, const float* div, float* p, int nsweeps, void* ws,
                      size_t ws_bytes, void* stream) {
  return fnx_jacobi_sweeps_ex(g, flags, div, p, nsweeps, ws, ws_bytes, 0, stream);
}

int fnx_jacobi_sweeps_ex(const FnxGrid* g, const float* flags, const float* div, float* p, int nsweeps, void* ws,
                         size_t ws_bytes, int reuse_mask, void* stream) {
  if (int rc = check_grid(g)) return rc;
  if (!flags || !div || !p) return fail(FNX_EINVAL, "jacobi_sweeps: NULL tensor");
  if (nsweeps < 1) return fail(FNX_EINVAL, "At least 1 iteration is needed (maxIter < 1)");
  hipStream_t s = (hipStream_t)stream;
  JacobiWs W;
  if (int rc = jacobi_begin("jacobi_sweeps", g, flags, ws, ws_bytes, (reuse_mask & 1) != 0, s, &W)) return rc;
  const bool from_zero = (reuse_mask & 2) != 0;
  // ping-pong p -> tmp -> p ...; an odd number of launches ends in tmp and is copied back
  float* const buf[2] = {p, W.tmp};
  const fnx::JacobiSchedule sch = fnx::jacobi_schedule(dims(g), g->is3D, nsweeps, cu_count());
  const float* in = run_jacobi_launches(g, sch, flags, div, W.mask, from_zero ? nullptr : p, buf, 1, s);
  if (in != p) HIP_OK(hipMemcpyAsync(p, in, ncell(g) * 4, hipMemcpyDeviceToDevice, s));
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

int fnx_jacobi_pass2(const FnxGrid* g, const float* flags, const float* div, const float* p_in, float* p_out,
                     int nsweeps, int k_begin, int k_end, int k_begin2, void* ws, size_t ws_bytes, int reuse_mask,
                     void* stream) {
  return fnx_jacobi_pass_layout(g, flags, div, p_in, p_out, nsweeps, k_begin, k_end, k_begin2, 0, ws, ws_bytes, reuse_mask, stream);
}

int fnx_jacobi_quad_ok(const FnxGrid* g) {
  if (check_grid(g) != FNX_OK || !g->is3D) return 0;
  return fnx::jacobi3d_quad_ok(dims(g)) ? 1 : 0;
}

int fnx_jacobi_pass_layout(const FnxGrid* g, const float* flags, const float* div, const float* p_in, float* p_out,
                           int nsweeps, int k_begin, int k_end, int k_begin2, int layout, void* ws, size_t ws_bytes,
                           int reuse_mask, void* stream) {
  if (int rc = check_grid(g)) return rc;
  if (layout < 0 || layout > 3) return fail(FNX_EINVAL, "jacobi_pass: layout must be 0..3");
  if (layout != 0 && (nsweeps != 2 || !g->is3D || !fnx::jacobi3d_quad_ok(dims(g))))
    return fail(FNX_EINVAL, "jacobi_pass: the row-quad layout needs a two-sweep pass on a grid fnx_jacobi_quad_ok accepts");
  if (!flags || !div || !p_out || p_in == p_out) return fail(FNX_EINVAL, "jacobi_pass: NULL or aliased tensor");
  if (!g->is3D) return fail(FNX_EINVAL, "jacobi_pass: 3D only (2D uses fnx_jacobi_sweeps)");
  const bool from_zero = p_in == nullptr;                 // the first pass of a solve: p = 0 everywhere, nothing to read
  if (nsweeps < 1 || nsweeps > 2) return fail(FNX_EINVAL, "jacobi_pass: nsweeps must be 1 or 2");
  if (int rc = check_plane_ranges("jacobi_pass", g, k_begin, k_end, k_begin2, true)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const GridDims d = dims(g);
  JacobiWs W;
  if (int rc = jacobi_begin("jacobi_pass", g, flags, ws, ws_bytes, reuse_mask != 0, s, &W)) return rc;
  fnx::ProfScope ps(FNX_PROF_JACOBI, s);
  if (nsweeps == 2) fnx::launch_jacobi3d_x2(d, W.mask, div, p_in, p_out, s, k_begin, k_end, from_zero, k_begin2, layout, nullptr, jacobi3d_x(g));
  else {
    fnx::launch_jacobi3d(d, W.mask, div, p_in, p_out, from_zero, s, k_begin, k_end);
    if (k_begin2 >= 0) fnx::launch_jacobi3d(d, W.mask, div, p_in, p_out, from_zero, s, k_begin2, k_begin2 + (k_end - k_begin));
  }
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

int fnx_jacobi_pass_mirror_ok(const FnxGrid* g, int planes, int two_ranges, int layout) {
  if (check_grid(g) != FNX_OK || !g->is3D || planes < 1) return 0;
  return fnx::jacobi3d_mirror_ok(dims(g), planes, two_ranges != 0, false, layout, cu_count()) ? 1 : 0;
}

int fnx_jacobi_pass_mirror(const FnxGrid* g, const float* flags, const float* div, const float* p_in, float* p_out, int k_begin,
                           int k_end, int k_begin2, int layout, const FnxPlaneMirror* mirror, void* ws, size_t ws_bytes,
                           int reuse_mask, void* stream) {
  if (int rc = check_grid(g)) return rc;
  if (!g->is3D || !flags || !div || !p_in || !p_out || p_in == p_out || !mirror) return fail(FNX_EINVAL, "jacobi_pass_mirror: NULL or aliased argument");
  if (int rc = check_plane_ranges("jacobi_pass_mirror", g, k_begin, k_end, k_begin2, false)) return rc;
  const GridDims d = dims(g);
  if ((layout == 3 && !fnx::jacobi3d_quad_ok(d)) || !fnx::jacobi3d_mirror_ok(d, k_end - k_begin, k_begin2 >= 0, false, layout, cu_count()))
    return fail(FNX_EINVAL, "jacobi_pass_mirror: this launch cannot mirror its output (fnx_jacobi_pass_mirror_ok)");
  if (mirror->planes < 1 || !mirror->out[0][0] || (mirror->slot_select[0] && !mirror->out[0][1]) ||
      (k_begin2 >= 0 && (!mirror->out[1][0] || (mirror->slot_select[1] && !mirror->out[1][1]))))
    return fail(FNX_EINVAL, "jacobi_pass_mirror: bad mirror");
  hipStream_t s = (hipStream_t)stream;
  JacobiWs W;
  if (int rc = jacobi_begin("jacobi_pass_mirror", g, flags, ws, ws_bytes, reuse_mask != 0, s, &W)) return rc;
  fnx::ProfScope ps(FNX_PROF_JACOBI, s);
  fnx::JacobiMirror m{};
  for (int r = 0; r < 2; ++r) { m.out[r][0] = mirror->out[r][0]; m.out[r][1] = mirror->out[r][1]; m.sel[r] = mirror->slot_select[r]; }
  m.k[0] = mirror->k_first[0]; m.k[1] = mirror->k_first[1]; m.n = mirror->planes;
  m.bstride = mirror->sample_stride; m.clock = mirror->start_clock;
  fnx::launch_jacobi3d_x2(d, W.mask, div, p_in, p_out, s, k_begin, k_end, false, k_begin2, layout, &m);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

int fnx_jacobi_pass(const FnxGrid* g, const float* flags, const float* div, const float* p_in, float* p_out,
                    int nsweeps, int k_begin, int k_end, void* ws, size_t ws_bytes, int reuse_mask, void* stream) {
  return fnx_jacobi_pass2(g, flags, div, p_in, p_out, nsweeps, k_begin, k_end, -1, ws, ws_bytes, reuse_mask, stream);
}

int fnx_residual(const FnxGrid* g, const float* a, const float* b, float* sumsq, float* residual, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_grid(g)) return rc;
  if (!a || (!sumsq && !residual)) return fail(FNX_EINVAL, "residual: NULL tensor");
  if (!ws || ws_bytes < fnx::residual_scratch_bytes(g->B)) return fail(FNX_EWORKSPACE, "residual: workspace too small (%zu < %zu)", ws_bytes, fnx::residual_scratch_bytes(g->B));
  const GridDims d = dims(g);
  const size_t per = (size_t)g->D * g->H * g->W;
  fnx::launch_residual(g->B, per, (size_t)d.K0 * d.HW, (size_t)d.KN * d.HW, a, b, (double*)ws, sumsq, residual, (hipStream_t)stream);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

size_t fnx_pcg_workspace_bytes(const FnxGrid* g) {
  if (check_grid(g) != FNX_OK) return 0;
  return ws_pcg(g);
}

namespace {
int check_pcg_grid(const FnxGrid* g, const char* who) {
  if (int rc = check_grid(g)) return rc;
  if (is_view(g))
    return fail(FNX_EINVAL, "%s: no compute window or z-slab view (the solve is single-domain)", who);
  return FNX_OK;
}

// min_iter: the smallest max_iter the entry point takes (fnx_pcg 1, fnx_pcg_from 0)
int pcg_entry(const FnxGrid* g, const float* flags, const float* div, const float* p0, float* p, float* residual, float p_tol, int max_iter,
              int min_iter, int* iters_done, void* ws, size_t ws_bytes, void* stream, bool verbose) {
  if (int rc = check_pcg_grid(g, "pcg")) return rc;
  if (!flags || !div || !p) return fail(FNX_EINVAL, "pcg: NULL tensor");
  if (div == p) return fail(FNX_EINVAL, "pcg: p must not alias div");
  if (min_iter > 0 && max_iter < 1) return fail(FNX_EINVAL, "At least 1 iteration is needed (maxIter < 1)");
  if (max_iter < 0) return fail(FNX_EINVAL, "pcg_from: max_iter must not be negative (maxIter < 0)");
  if (!ws || ws_bytes < ws_pcg(g)) return fail(FNX_EWORKSPACE, "pcg: workspace too small (%zu < %zu)", ws_bytes, ws_pcg(g));
  hipStream_t s = (hipStream_t)stream;
  const GridDims d = dims(g);
  char* kept = (char*)ws;
  fnx::launch_pcg_build(d, g->is3D, quirks(g), flags, kept, s);
  HIP_OK(hipGetLastError());
  if (int rc = fnx::pcg_solve(d, g->is3D, kept, kept + ws_pcg_kept(g), div, p0, p, residual, p_tol, max_iter, iters_done, verbose, s)) return rc;
  HIP_OK(hipGetLastError());
  return FNX_OK;
}
}  // namespace

int fnx_pcg(const FnxGrid* g, const float* flags, const float* div, float* p, float* residual, float p_tol, int max_iter,
            int* iters_done, void* ws, size_t ws_bytes, void* stream) {
  return pcg_entry(g, flags, div, nullptr, p, residual, p_tol, max_iter, 1, iters_done, ws, ws_bytes, stream, false);
}

int fnx_pcg_verbose(const FnxGrid* g, const float* flags, const float* div, float* p, float* residual, float p_tol, int max_iter,
                    int* iters_done, void* ws, size_t ws_bytes, void* stream) {
  return pcg_entry(g, flags, div, nullptr, p, residual, p_tol, max_iter, 1, iters_done, ws, ws_bytes, stream, true);
}

int fnx_pcg_from(const FnxGrid* g, const float* flags, const float* div, const float* p0, float* p, float* residual, float p_tol,
                 int max_iter, int* iters_done, void* ws, size_t ws_bytes, void* stream) {
  return pcg_entry(g, flags, div, p0, p, residual, p_tol, max_iter, 0, iters_done, ws, ws_bytes, stream, false);
}

int fnx_pcg_from_verbose(const FnxGrid* g, const float* flags, const float* div, const float* p0, float* p, float* residual, float p_tol,
                         int max_iter, int* iters_done, void* ws, size_t ws_bytes, void* stream) {
  return pcg_entry(g, flags, div, p0, p, residual, p_tol, max_iter, 0, iters_done, ws, ws_bytes, stream, true);
}

int fnx_poisson_apply(const FnxGrid* g, const float* flags, const float* p, float* Ap, void* stream) {
  if (int rc = check_pcg_grid(g, "poisson_apply")) return rc;
  if (!flags || !p || !Ap) return fail(FNX_EINVAL, "poisson_apply: NULL tensor");
  if (p == Ap) return fail(FNX_EINVAL, "poisson_apply: Ap must not alias p");
  fnx::launch_poisson_apply(dims(g), g->is3D, quirks(g), flags, p, Ap, (hipStream_t)stream);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

int fnx_pcg_precondition(const FnxGrid* g, const float* flags, const float* r, float* z, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_pcg_grid(g, "pcg_precondition")) return rc;
  if (!flags || !r || !z) return fail(FNX_EINVAL, "pcg_precondition: NULL tensor");
  if (r == z) return fail(FNX_EINVAL, "pcg_precondition: z must not alias r");
  if (!ws || ws_bytes < ws_pcg(g)) return fail(FNX_EWORKSPACE, "pcg_precondition: workspace too small (%zu < %zu)", ws_bytes, ws_pcg(g));
  hipStream_t s = (hipStream_t)stream;
  const GridDims d = dims(g);
  char* kept = (char*)ws;
  fnx::launch_pcg_build(d, g->is3D, quirks(g), flags, kept, s);
  fnx::launch_pcg_precondition(d, g->is3D, kept, kept + ws_pcg_kept(g), r, z, s);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

int fnx_velocity_update(const FnxGrid* g, const float* p, float* U, const float* flags, void* stream) {
  if (int rc = check_grid(g)) return rc;
  if (!p || !U || !flags) return fail(FNX_EINVAL, "velocity_update: NULL tensor");
  fnx::launch_velocity_update(dims(g), g->is3D, p, U, flags, (hipStream_t)stream);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

int fnx_add_gravity(const FnxGrid* g, float* U, const float* flags, const float gravity[3], float dt, void* stream) {
  if (int rc = check_grid(g)) return rc;
  if (!U || !flags || !gravity) return fail(FNX_EINVAL, "add_gravity: NULL tensor");
  fnx::launch_add_gravity(dims(g), g->is3D, U, flags, gravity[0] * dt, gravity[1] * dt, gravity[2] * dt,
                          (hipStream_t)stream);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

int fnx_correct_scalar(const FnxGrid* g, float dt, float* src, const float* div, const float* flags, void* stream) {
  if (int rc = check_grid(g)) return rc;
  if (!src || !div || !flags) return fail(FNX_EINVAL, "correct_scalar: NULL tensor");
  fnx::launch_correct_scalar(dims(g), g->is3D, dt * 0.5f, src, div, flags, (hipStream_t)stream);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

int fnx_add_viscosity(const FnxGrid* g, float dt, const float* U_in, float* U_out, const float* flags, float viscosity,
                      void* stream) {
  if (int rc = check_grid(g)) return rc;
  if (!U_in || !U_out || !flags) return fail(FNX_EINVAL, "add_viscosity: NULL tensor");
  if (quirks(g))
    return fail(FNX_EINVAL, "add_viscosity: no 3D form with ref_quirks (the reference's 3D branch cannot run, viscosity.py never defines "
                            "mask_fluid_k: there is nothing to reproduce)");
  if (g->is3D && is_view(g)) return fail(FNX_EINVAL, "add_viscosity: no compute window or z-slab view (whole grids only)");
  if (U_in == U_out) return fail(FNX_EINVAL, "add_viscosity: U_out must not alias U_in");
  if (!(viscosity >= 0.f)) return fail(FNX_EINVAL, "add_viscosity: viscosity must be positive");
  const float coef = (float)((double)dt * (double)viscosity);
  if (g->is3D) fnx::launch_add_viscosity3d(dims(g), U_in, U_out, flags, coef, (hipStream_t)stream);
  else fnx::launch_add_viscosity(dims(g), U_in, U_out, flags, coef, (hipStream_t)stream);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

int fnx_add_vorticity_confinement(const FnxGrid* g, const float* U_in, float* U_out, const float* flags, float amp, void* stream) {
  if (!U_in || !U_out || !flags) return fail(FNX_EINVAL, "add_vorticity_confinement: NULL tensor");
  if (U_in == U_out) return fail(FNX_EINVAL, "add_vorticity_confinement: U_out must not alias U_in (a cell reads U_in three cells around it)");
  if (int rc = check_grid(g)) return rc;
  if (is_view(g))
    return fail(FNX_EINVAL, "add_vorticity_confinement: no compute window or z-slab view (whole grids only)");
  if (!(amp == amp)) return fail(FNX_EINVAL, "add_vorticity_confinement: the amplitude is NaN");
  hipStream_t s = (hipStream_t)stream;
  if (amp == 0.f) HIP_OK(hipMemcpyAsync(U_out, U_in, ncell(g) * 4 * (g->is3D ? 3 : 2), hipMemcpyDeviceToDevice, s));
  else fnx::launch_vorticity_confinement(dims(g), g->is3D, U_in, flags, U_out, amp, s);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

namespace {
int check_render(const FnxGrid* g, const FnxRenderParams* prm) {
  if (!prm) return fail(FNX_EINVAL, "render_volume: NULL parameters");
  if (int rc = check_grid(g)) return rc;
  if (is_view(g))
    return fail(FNX_EINVAL, "render_volume: no compute window or z-slab view (whole grids only)");
  if (prm->view_dir < 0 || prm->view_dir > 5 || prm->light_dir < 0 || prm->light_dir > 5)
    return fail(FNX_EINVAL, "render_volume: direction outside 0..5 (view_dir=%d light_dir=%d)", prm->view_dir, prm->light_dir);
  if (prm->bnd < 0) return fail(FNX_EINVAL, "render_volume: bnd < 0 (%d)", prm->bnd);
  const float k[2] = {prm->k_view, prm->k_light};
  for (float v : k)
    if (!(v >= 0.f) || !(v - v == 0.f))
      return fail(FNX_EINVAL, "render_volume: absorption must be finite and not negative (k_view=%g k_light=%g)", prm->k_view, prm->k_light);
  return FNX_OK;
}
}  // namespace

size_t fnx_render_volume_ws_bytes(const FnxGrid* g, const FnxRenderParams* prm) {
  if (check_render(g, prm) != FNX_OK) return 0;
  return prm->view_dir == prm->light_dir ? 0 : al(ncell(g) * 4);
}

int fnx_render_volume(const FnxGrid* g, const float* density, const float* flags, const FnxRenderParams* prm, float* image,
                      void* ws, size_t ws_bytes, void* stream) {
  if (!density || !flags || !image) return fail(FNX_EINVAL, "render_volume: NULL tensor");
  if (int rc = check_render(g, prm)) return rc;
  const size_t need = prm->view_dir == prm->light_dir ? 0 : al(ncell(g) * 4);
  if (need && (!ws || ws_bytes < need)) return fail(FNX_EINVAL, "render_volume: workspace too small (%zu < %zu)", ws ? ws_bytes : (size_t)0, need);
  const fnx::RenderConsts c = {prm->k_view, prm->k_light, prm->ambient, prm->one_minus_ambient, prm->albedo_smoke, prm->albedo_obstacle,
                               prm->bnd};
  fnx::launch_render_volume(dims(g), prm->view_dir, prm->light_dir, c, density, flags, (float*)ws, image, (hipStream_t)stream);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

int fnx_add_buoyancy(const FnxGrid* g, float* U, const float* flags, const float* density, const float gravity[3],
                     float rho_star, float dt, void* stream) {
  if (int rc = check_grid(g)) return rc;
  if (!U || !flags || !density || !gravity) return fail(FNX_EINVAL, "add_buoyancy: NULL tensor");
  const float sx = gravity[0] * dt, sy = gravity[1] * dt, sz = gravity[2] * dt;   // strength = gravity * dt
  fnx::launch_add_buoyancy(dims(g), g->is3D, quirks(g), U, flags, density, sx, sy, sz, rho_star, (hipStream_t)stream);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

int fnx_set_wall_bcs(const FnxGrid* g, float* U, const float* flags, void* stream) {
  if (int rc = check_grid(g)) return rc;
  if (!U || !flags) return fail(FNX_EINVAL, "set_wall_bcs: NULL tensor");
  fnx::launch_set_wall_bcs(dims(g), g->is3D, U, flags, (hipStream_t)stream);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

int fnx_set_wall_bcs_stick(const FnxGrid* g, const float* U_in, float* U_out, const float* flags, const float* flags_stick,
                           void* stream) {
  if (int rc = check_grid(g)) return rc;
  if (!U_in || !U_out || !flags || !flags_stick) return fail(FNX_EINVAL, "set_wall_bcs_stick: NULL tensor");
  if (quirks(g))
    return fail(FNX_EINVAL, "set_wall_bcs_stick: no 3D form with ref_quirks (the reference's 3D branch cannot run, "
                            "set_wall_bcs_stick.py:85-86: there is nothing to reproduce)");
  if (U_in == U_out) return fail(FNX_EINVAL, "set_wall_bcs_stick: U_out must not alias U_in");
  if (g->is3D) fnx::launch_set_wall_bcs_stick3d(dims(g), U_in, U_out, flags, flags_stick, (hipStream_t)stream);
  else fnx::launch_set_wall_bcs_stick(dims(g), U_in, U_out, flags, flags_stick, (hipStream_t)stream);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

int fnx_set_const_vals(const FnxGrid* g, float* U, const float* UBC, const float* UBCInvMask, float* density,
                       const float* densityBC, const float* densityBCInvMask, void* stream) {
  if (int rc = check_grid(g)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (U && UBC && UBCInvMask) fnx::launch_set_const_vals(ncell(g) * (g->is3D ? 3 : 2), U, UBC, UBCInvMask, s);
  if (density && densityBC && densityBCInvMask) fnx::launch_set_const_vals(ncell(g), density, densityBC, densityBCInvMask, s);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

int fnx_flags_to_occupancy(const FnxGrid* g, const float* flags, float* occupancy, void* stream) {
  if (int rc = check_grid(g)) return rc;
  if (!flags || !occupancy) return fail(FNX_EINVAL, "flags_to_occupancy: NULL tensor");
  fnx::launch_flags_to_occupancy(ncell(g), flags, occupancy, (hipStream_t)stream);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

int fnx_max_abs(const FnxGrid* g, const float* x, int channels, float* out_max, void* stream) {
  if (int rc = check_grid(g)) return rc;
  if (!x || !out_max || channels < 1) return fail(FNX_EINVAL, "max_abs: NULL tensor or channels < 1");
  if (((size_t)x & 15) != 0) return fail(FNX_EINVAL, "max_abs: the field must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  HIP_OK(hipMemsetAsync(out_max, 0, 4, s));
  fnx::launch_max_abs(ncell(g) * (size_t)channels, x, out_max, s);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

int fnx_empty_domain(const FnxGrid* g, float* flags, int boundary_width, void* stream) {
  if (int rc = check_grid(g)) return rc;
  if (!flags) return fail(FNX_EINVAL, "empty_domain: NULL tensor");
  if (boundary_width < 1) return fail(FNX_EINVAL, "Boundary width must be greater than zero!");
  fnx::launch_empty_domain(dims(g), g->is3D, flags, boundary_width, (hipStream_t)stream);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

int fnx_create_cylinder(const FnxGrid* g, float* flags, double center_x, double center_y, double radius, void* stream) {
  if (int rc = check_grid(g)) return rc;
  if (!flags) return fail(FNX_EINVAL, "create_cylinder: NULL tensor");
  // the reference squares the radius as a python double and the comparison casts it to fp32 (geometry_utils.py:31)
  const float r2 = (float)(radius * radius);
  fnx::launch_create_cylinder(dims(g), flags, (float)center_x, (float)center_y, r2, (hipStream_t)stream);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

int fnx_create_box2d(const FnxGrid* g, float* flags, float x0, float x1, float y0, float y1, void* stream) {
  if (int rc = check_grid(g)) return rc;
  if (!flags) return fail(FNX_EINVAL, "create_box2d: NULL tensor");
  fnx::launch_create_box2d(dims(g), flags, x0, x1, y0, y1, (hipStream_t)stream);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

// 3D obstacles from geometry (fnx_voxelize.hip): whole 3D domains only, any batch; sample -1 = every sample
static int check_geometry3d(const char* name, const FnxGrid* g, const float* flags, int sample) {
  if (int rc = check_grid(g)) return rc;
  if (!g->is3D) return fail(FNX_EINVAL, "%s: 3D grids only (a 2D obstacle is createCylinder's or createBox2D's)", name);
  if (is_view(g)) return fail(FNX_EINVAL, "%s: whole domains only, not a compute window or a z-slab view", name);
  if (!flags) return fail(FNX_EINVAL, "%s: NULL tensor", name);
  if (sample < -1 || sample >= g->B) return fail(FNX_EINVAL, "%s: sample %d out of range for B=%d", name, sample, g->B);
  return FNX_OK;
}

int fnx_create_sphere(const FnxGrid* g, float* flags, double center_x, double center_y, double center_z, double radius, int sample,
                      void* stream) {
  if (int rc = check_geometry3d("create_sphere", g, flags, sample)) return rc;
  const float r2 = (float)(radius * radius);               // as fnx_create_cylinder
  fnx::launch_create_sphere(dims(g), flags, sample < 0 ? 0 : sample, sample < 0 ? g->B : 1, (float)center_x, (float)center_y,
                            (float)center_z, r2, (hipStream_t)stream);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

int fnx_create_box3d(const FnxGrid* g, float* flags, float x0, float x1, float y0, float y1, float z0, float z1, int sample,
                     void* stream) {
  if (int rc = check_geometry3d("create_box3d", g, flags, sample)) return rc;
  fnx::launch_create_box3d(dims(g), flags, sample < 0 ? 0 : sample, sample < 0 ? g->B : 1, x0, x1, y0, y1, z0, z1, (hipStream_t)stream);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

static int check_voxelize_grid(const FnxGrid* g) {
  if (int rc = check_grid(g)) return rc;
  if (!g->is3D) return fail(FNX_EINVAL, "voxelize_mesh: 3D grids only");
  if (is_view(g)) return fail(FNX_EINVAL, "voxelize_mesh: whole domains only, not a compute window or a z-slab view");
  return FNX_OK;
}

size_t fnx_voxelize_mesh_ws_bytes(const FnxGrid* g) {
  if (check_voxelize_grid(g) != FNX_OK) return 0;
  return (fnx::voxel_words(dims(g)) + 2) * 4;
}

int fnx_voxelize_mesh(const FnxGrid* g, float* flags, const float* vertices, int n_vertices, const int* faces, int n_faces, int sample,
                      int* report, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = check_voxelize_grid(g)) return rc;
  if (n_vertices < 0 || n_faces < 0) return fail(FNX_EINVAL, "voxelize_mesh: n_vertices=%d n_faces=%d must not be negative", n_vertices, n_faces);
  // (an empty array may have no address: a mesh without faces marks nothing, a mesh without vertices has bad faces only)
  if (!flags || (!vertices && n_vertices > 0) || (!faces && n_faces > 0)) return fail(FNX_EINVAL, "voxelize_mesh: NULL tensor");
  if (sample < -1 || sample >= g->B) return fail(FNX_EINVAL, "voxelize_mesh: sample %d out of range for B=%d", sample, g->B);
  const GridDims d = dims(g);
  const size_t words = fnx::voxel_words(d), need = (words + 2) * 4;
  if (!ws || need > ws_bytes) return fail(FNX_EWORKSPACE, "voxelize_mesh: workspace too small (%zu < %zu)", ws ? ws_bytes : (size_t)0, need);
  if (((size_t)ws & 3) != 0) return fail(FNX_EINVAL, "voxelize_mesh: the workspace must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  unsigned* bits = (unsigned*)ws;
  int* counters = (int*)(bits + words);                    // {open rows, bad faces}
  HIP_OK(hipMemsetAsync(ws, 0, need, s));
  fnx::launch_voxelize_mesh(d, flags, sample < 0 ? 0 : sample, sample < 0 ? g->B : 1, vertices, n_vertices, faces, n_faces, bits, counters, s);
  HIP_OK(hipGetLastError());
  if (report) HIP_OK(hipMemcpyAsync(report, counters, 8, hipMemcpyDeviceToDevice, s));
  return FNX_OK;
}

int fnx_get_centered(const FnxGrid* g, const float* U, float* centered, void* stream) {
  // a pure per-cell average: any block of a field is a valid input (the drivers pass interior blocks, plume.py:351), so
  // only the launch limits are checked, not the operators' minimum domain size
  if (!g) return fail(FNX_EINVAL, "grid descriptor is NULL");
  if (g->B < 1 || g->D < 1 || g->H < 1 || g->W < 1) return fail(FNX_EINVAL, "Dimension mismatch: B=%d D=%d H=%d W=%d", g->B, g->D, g->H, g->W);
  if (!g->is3D && g->D != 1) return fail(FNX_EINVAL, "2D velocity field but zdepth > 1");
  if ((long long)g->D * g->H * g->W >= (1ll << 31)) return fail(FNX_EINVAL, "more than 2^31 cells per sample");
  if ((long long)g->B * g->D > 65535 || (g->H + 3) / 4 > 65535) return fail(FNX_EINVAL, "B*D or H/4 > 65535 not supported");
  if (!U || !centered) return fail(FNX_EINVAL, "get_centered: NULL tensor");
  if ((const float*)centered == U) return fail(FNX_EINVAL, "get_centered: the output must not alias U");
  fnx::launch_get_centered(make_dims(g->B, g->D, g->H, g->W), g->is3D, U, centered, (hipStream_t)stream);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

int fnx_velocity_divergence_backward(const FnxGrid* g, const float* grad_div, const float* flags, float* grad_U, void* stream) {
  if (int rc = check_grid(g)) return rc;
  if (!grad_div || !flags || !grad_U) return fail(FNX_EINVAL, "velocity_divergence_backward: NULL tensor");
  fnx::launch_divergence_bwd(make_dims(g->B, g->D, g->H, g->W, g->z_offset, g->D_global), g->is3D, grad_div, flags, grad_U, (hipStream_t)stream);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

int fnx_velocity_update_backward(const FnxGrid* g, const float* grad_U_out, const float* flags, float* grad_U, float* grad_p,
                                 void* stream) {
  if (int rc = check_grid(g)) return rc;
  if (!grad_U_out || !flags || !grad_U || !grad_p) return fail(FNX_EINVAL, "velocity_update_backward: NULL tensor");
  if (grad_U == grad_U_out) return fail(FNX_EINVAL, "velocity_update_backward: grad_U must not alias grad_U_out (a cell reads its +1 neighbours)");
  fnx::launch_velocity_update_bwd(make_dims(g->B, g->D, g->H, g->W, g->z_offset, g->D_global), g->is3D, grad_U_out, flags, grad_U, grad_p, (hipStream_t)stream);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

// The stage by its plan, for fnx_pre_projection and fnx_simulate_step.  One fused pass writes the staged fields and the divergence (each
// cell re-derives the staged component of its +1 neighbours), unless the periodic patches have to go between the stages and the
// divergence: then staging, patches, a divergence pass.  With the confinement, which reads the field three cells around a cell and so
// cannot join the radius-1 recompute, the stage is cut in three around it.
// word: the step's stage word map (3D, with st->bc_class), or nullptr
static int pre_projection(const FnxGrid* g, const fnx::StagePlan& sp, const FnxState* st, const float* U_adv, const float* rho_adv,
                          float* div, void* stream, const unsigned* word = nullptr) {
  // a cell reads the advected fields of its +1 / -1 neighbours while other threads write theirs: no in-place use
  if (U_adv == st->U || (rho_adv && rho_adv == st->density)) return fail(FNX_EINVAL, "pre_projection: the advected fields must not alias the state");
  if (sp.confine && is_view(g))
    return fail(FNX_EINVAL, "pre_projection: vorticity confinement takes no compute window or z-slab view (single domain only)");
  hipStream_t s = (hipStream_t)stream;
  fnx::ProfScope ps(FNX_PROF_STAGE, s);
  const GridDims d = dims(g);
  const fnx::BcPtrs bc = fnx::bc_ptrs(st, word);
  // the uncut stage: every operation of the plan, the divergence in the same pass unless the patches come between
  const fnx::StageIO io{U_adv, rho_adv, st->flags, bc, st->U, st->density, sp.periodic ? nullptr : div};
  const fnx::StageOps all{quirks(g), true, sp.buoy, {sp.s[0], sp.s[1], sp.s[2]}, sp.rho_star, sp.grav, {sp.g[0], sp.g[1], sp.g[2]},
                          sp.wall, sp.second_bcs, d.K0 + d.KN};
  if (!sp.confine) {
    // the staging covers one plane more than the divergences asked for where there is one (3D ranges): the divergence of the last
    // plane reads the advected fields of that plane, and the callers of plane ranges expect it staged as well
    GridDims ds = d;
    if (g->is3D && div && ds.K0 + ds.KN < ds.D) ds.KN += 1;
    fnx::launch_pre_projection(ds, g->is3D, io, all, s);
    if (sp.periodic) fnx::launch_periodic_pre(ds, g->is3D, U_adv, bc.UBC, bc.UBCInvMask, st->U, sp.px, sp.py, s, false);
  } else {
    // (1) setConstVals, addBuoyancy, addGravity: U_adv -> st->U; the density is through with it but for its second setConstVals
    fnx::StageIO io1 = io;
    io1.div = nullptr;
    fnx::StageOps upto_gravity = all;
    upto_gravity.wall = false; upto_gravity.second_bcs = false; upto_gravity.div_k_end = 0;
    fnx::launch_pre_projection(d, g->is3D, io1, upto_gravity, s);
    // (2) the confinement: st->U -> U_adv, which is scratch from here on
    float* U_scr = const_cast<float*>(U_adv);
    fnx::launch_vorticity_confinement(d, g->is3D, st->U, st->flags, U_scr, sp.amp, s);
    // (3) setWallBcs (+ periodic patches), setConstVals, divergence: U_adv -> st->U, the velocity alone
    fnx::StageIO io3 = io;
    io3.rho_adv = nullptr; io3.rho = nullptr; io3.bc.rhoBC = nullptr; io3.bc.rhoBCInvMask = nullptr;
    fnx::StageOps from_walls = all;
    from_walls.first_bcs = false; from_walls.buoy = false; from_walls.grav = false;
    fnx::launch_pre_projection(d, g->is3D, io3, from_walls, s);
    if (sp.periodic) fnx::launch_periodic_pre(d, g->is3D, U_scr, bc.UBC, bc.UBCInvMask, st->U, sp.px, sp.py, s, true);
  }
  if (sp.periodic && div) fnx::launch_divergence(d, g->is3D, st->U, st->flags, div, s);
  if (sp.confine && rho_adv && bc.rhoBC && sp.second_bcs) fnx::launch_set_const_vals(ncell(g), st->density, bc.rhoBC, bc.rhoBCInvMask, s);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

int fnx_pre_projection(const FnxGrid* g, const FnxStepParams* prm, const FnxState* st, const float* U_adv,
                       const float* rho_adv, float* div, void* stream) {
  if (int rc = check_grid(g)) return rc;
  if (!prm || !st || !st->U || !st->flags || !U_adv) return fail(FNX_EINVAL, "pre_projection: NULL state");
  if (rho_adv && !st->density) return fail(FNX_EINVAL, "pre_projection: rho_adv given but state has no density");
  return pre_projection(g, fnx::stage_plan(prm, rho_adv != nullptr, st->flags_stick != nullptr), st, U_adv, rho_adv, div, stream);
}

static int post_projection(const FnxGrid* g, const FnxState* st, void* stream, const unsigned* word) {
  if (int rc = check_grid(g)) return rc;
  if (!st || !st->U || !st->flags || !st->p) return fail(FNX_EINVAL, "post_projection: NULL state");
  fnx::ProfScope ps(FNX_PROF_STAGE, (hipStream_t)stream);
  fnx::launch_post_projection(dims(g), g->is3D, st->p, st->U, st->density, st->flags, fnx::bc_ptrs(st, word), (hipStream_t)stream,
                              st->density_bc_applied != 0);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

int fnx_post_projection(const FnxGrid* g, const FnxState* st, void* stream) { return post_projection(g, st, stream, nullptr); }

int fnx_bc_classify(const FnxGrid* g, const FnxState* st, unsigned char* bc_class, void* stream) {
  if (int rc = check_grid(g)) return rc;
  if (!st || !bc_class) return fail(FNX_EINVAL, "bc_classify: NULL argument");
  fnx::launch_bc_classify(dims(g), g->is3D, fnx::bc_ptrs(st), bc_class, (hipStream_t)stream);
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

int fnx_simulate_step(const FnxGrid* g, const FnxStepParams* prm, const FnxState* st, void* ws, size_t ws_bytes,
                      void* stream) {
  return fnx_simulate_step_net(g, prm, st, FNX_NET_SCALENET, ws, ws_bytes, stream);
}

// What the bank net (FNX_NET_BANK) in methods 1 and 3 adds to the step's refusals, before the first launch and in the bank unit's own
// words (check_bank_call): the kind against the grid's dimension, the precision mode, the axes, a view.  The Conv3d bank net has a kind
// of its own, which the step does not take yet.
static int check_step_net(const char* fn, const FnxGrid* g, const FnxStepParams* prm, int net_kind) {
  if (net_kind == FNX_NET_SCALENET) return FNX_OK;
  if (net_kind == FNX_NET_BANK3D)
    return fail(FNX_EINVAL, "%s: FNX_NET_BANK3D is not built into the step (the Conv3d bank net runs through fnx_fluidnet_bank3d_forward, "
                            "around the operators)", fn);
  if (net_kind != FNX_NET_BANK)
    return fail(FNX_EINVAL, "%s: unknown net_kind %d (FNX_NET_SCALENET, FNX_NET_BANK or FNX_NET_BANK3D)", fn, net_kind);
  if (int rc = fnx::check_bank_grid(fn, g, prm->precision_mode)) return rc;
  if (is_view(g)) return fail(FNX_EINVAL, "%s: the bank nets take no compute window or z-slab view (single domain only)", fn);
  return FNX_OK;
}

// One whole step: the argument checks, the workspace (carve_step), the plan (fnx::step_plan), then the sequence the plan names.
// net_kind: the net of methods 1 and 3 (the other methods do not look at it).
int fnx_simulate_step_net(const FnxGrid* g, const FnxStepParams* prm, const FnxState* st, int net_kind, void* ws, size_t ws_bytes,
                          void* stream) {
  using fnx::StepAdvect; using fnx::StepClassMap; using fnx::StepProjection; using fnx::StepStageWord; using fnx::StepTail;
  if (int rc = check_grid(g)) return rc;
  if (!prm || !st || !st->p || !st->U || !st->flags) return fail(FNX_EINVAL, "simulate_step: NULL state");
  if (prm->method < 0 || prm->method > 4) return fail(FNX_EINVAL, "Simulation method not supported. Choose convnet, jacobi, pcg or hybrid.");
  if (prm->method != 1 && prm->method != 3) net_kind = FNX_NET_SCALENET;      // no net: the kind is not looked at
  if (int rc = check_step_net(__func__, g, prm, net_kind)) return rc;
  const bool pcg = prm->method >= 2;                 // 2: cold, 3 ('hybrid'): from the net's pressure, 4: from st->p as it stands
  if (pcg && prm->pcg_iter < 1) return fail(FNX_EINVAL, "At least 1 iteration of the solver is needed (pcg_iter < 1)");
  if (pcg && is_view(g))
    return fail(FNX_EINVAL, "simulate_step: the PCG solve takes no compute window or z-slab view (single domain only)");
  if (prm->vorticity_confinement > 0.f && is_view(g))
    return fail(FNX_EINVAL, "simulate_step: vorticity confinement takes no compute window or z-slab view (single domain only)");
  if (prm->method == 1 && !st->net) return fail(FNX_EINVAL, "simulate_step: convnet method needs packed weights");
  if (prm->method == 3 && !st->net) return fail(FNX_EINVAL, "simulate_step: hybrid method needs packed weights");
  if (prm->method == 3 && fnx::net_mode(prm->precision_mode) < 0) return fail(FNX_EINVAL, "simulate_step: unknown precision_mode %d", prm->precision_mode);
  const fnx::StepLayout L = carve_step(g, ws);
  if (!ws || ws_bytes < L.bytes) return fail(FNX_EWORKSPACE, "simulate_step: workspace too small (%zu < %zu)", ws_bytes, L.bytes);
  // a bank net's scratch comes out of the tail as the ScaleNet's does; the tail is sized for the ScaleNet (carve_step) and is not grown
  if (net_kind != FNX_NET_SCALENET && fnx::fluidnet_core_ws_bytes(g, net_kind) > L.tail_bytes)
    return fail(FNX_EWORKSPACE, "%s: the step workspace's scratch tail is too small for the bank net (%zu < %zu)", __func__, L.tail_bytes,
                fnx::fluidnet_core_ws_bytes(g, net_kind));
  const bool has_rho = st->density != nullptr;
  const fnx::StepPlan plan = fnx::step_plan(prm, has_rho, st->flags_stick != nullptr, st->UBC || st->densityBC);
  if (prm->viscosity < 0.f) return fail(FNX_EINVAL, "Viscosity must be positive");
  if (prm->vorticity_confinement != prm->vorticity_confinement) return fail(FNX_EINVAL, "simulate_step: vorticity_confinement is NaN");
  // (the operators themselves take 3D grids since ABI 29; the step has no 3D viscous stage: the message's "2D only" speaks of the step)
  if (plan.viscous && g->is3D) return fail(FNX_EINVAL, "simulate_step: viscosity is 2D only (reference viscosity.py:5)");
  if (plan.projection == StepProjection::NET_STICK && g->is3D) return fail(FNX_EINVAL, "simulate_step: flags_stick is 2D only (set_wall_bcs_stick.py:85-86)");
  hipStream_t s = (hipStream_t)stream;
  const GridDims d = dims(g);
  const size_t nc = g->is3D ? 3 : 2;

  // simulate.py:66-93: advect density then velocity (both by the OLD U; the velocity advected is the viscous one)
  if (plan.viscous) {
    if (int rc = fnx_add_viscosity(g, prm->dt, st->U, L.orig, st->flags, prm->viscosity, stream)) return rc;
  }
  if (plan.advect == StepAdvect::PAIR) {
    // forward passes of both advections in one launch, backward/clamp passes in another (same cell functions)
    if (int rc = fnx_advect_step(g, prm->dt, st->density, st->U, st->flags, L.rho2, L.U2, prm->sample_outside_fluid,
                                 prm->maccormack_strength, L.tail, L.tail_bytes, stream)) return rc;
  } else {
    if (plan.advect == StepAdvect::RHO_THEN_VEL) {
      if (int rc = fnx_advect_scalar(g, prm->dt, st->density, st->U, st->flags, L.rho2, FNX_ADVECT_MACCORMACK, 1,
                                     prm->sample_outside_fluid, prm->maccormack_strength, L.tail, L.tail_bytes, stream)) return rc;
    }
    if (int rc = fnx_advect_vel(g, prm->dt, plan.viscous ? L.orig : st->U, st->U, st->flags, L.U2, FNX_ADVECT_MACCORMACK, 1,
                                prm->maccormack_strength, L.tail, L.tail_bytes, stream)) return rc;
  }
  if (plan.correct_scalar) {                   // simulate.py:79-81: by the divergence of the OLD U (st->U is still untouched)
    fnx::launch_divergence(d, g->is3D, st->U, st->flags, L.div, s);
    if (int rc = fnx_correct_scalar(g, prm->dt, L.rho2, L.div, st->flags, stream)) return rc;
  }
  // static BC arrays: the BC stages go by the class map kept in the workspace
  FnxState stc = *st;
  if (plan.class_map == StepClassMap::BUILD) { if (int rc = fnx_bc_classify(g, st, L.cls, stream)) return rc; }
  stc.bc_class = plan.class_map == StepClassMap::NONE ? nullptr : L.cls;
  stc.density_bc_applied = 1;                  // by the pre-projection stage below, with these BC arrays
  st = &stc;
  // static flags as well, 3D, and a workspace of FNX_OP_STEP_STATIC's size: the stage and the tail go by the stage word map behind the layout
  const StepStageWord sw = fnx::stage_word_plan(prm, g->is3D != 0, plan.class_map, L, ncell(g), ws_bytes);
  unsigned* word = sw == StepStageWord::NONE ? nullptr : (unsigned*)((char*)ws + fnx::stage_word_offset(L));
  if (sw == StepStageWord::BUILD) {
    fnx::ProfScope ps(FNX_PROF_STAGE, s);
    fnx::launch_stage_word(d, st->flags, L.cls, word, s);
  }
  // simulate.py:96-133 (+ :144 divergence) in one pass: BCs, buoyancy, gravity, wall BCs (+ periodic patches), BCs, -div
  if (int rc = pre_projection(g, plan.stage, st, L.U2, has_rho ? L.rho2 : nullptr, plan.solve ? L.div : nullptr, stream, word)) return rc;

  // setWallBcsStick is out of place: st->U -> U2 (free since the staging pass) and back; then the setConstVals behind it
  auto stick_then_bcs = [&]() -> int {
    if (int rc = fnx_set_wall_bcs_stick(g, st->U, L.U2, st->flags, st->flags_stick, stream)) return rc;
    HIP_OK(hipMemcpyAsync(st->U, L.U2, ncell(g) * 4 * nc, hipMemcpyDeviceToDevice, s));
    return fnx_set_const_vals(g, st->U, st->UBC, st->UBCInvMask, st->density, st->densityBC, st->densityBCInvMask, stream);
  };
  switch (plan.projection) {                   // simulate.py:136-152
    case StepProjection::JACOBI:
      if (int rc = jacobi_solve(g, st->flags, L.div, st->p, nullptr, prm->p_tol, prm->jacobi_iter, nullptr, L.tail, L.tail_bytes, L.mask,
                                plan.reuse_mask, stream, 0)) return rc;
      break;
    case StepProjection::PCG_COLD: case StepProjection::PCG_FROM_NET: case StepProjection::PCG_FROM_P: {
      if (plan.pcg_rebuild) fnx::launch_pcg_build(d, g->is3D, quirks(g), st->flags, L.pcg_kept, s);
      if (plan.projection == StepProjection::PCG_FROM_NET) {
        // the guess: the net's un-normalised pressure of this U, written into st->p.  The net's scratch and the solve's share the
        // tail: the net has finished (same stream) before the solve's first launch, and all the solve takes from it is st->p
        if (int rc = fnx::fluidnet_pressure(g, st->net, net_kind, st->flags, prm->normalize_threshold, fnx::net_mode(prm->precision_mode), st->p, st->U,
                                            L.tail, stream)) return rc;
      }
      const float* p0 = plan.projection == StepProjection::PCG_COLD ? nullptr : st->p;
      if (int rc = fnx::pcg_solve(d, g->is3D, L.pcg_kept, L.tail, L.div, p0, st->p, nullptr, prm->pcg_tol, prm->pcg_iter, nullptr, false, s)) return rc;
      break;
    }
    case StepProjection::NET_STICK:            // simulate.py:129-133: setWallBcsStick, then the second setConstVals
      if (int rc = stick_then_bcs()) return rc;
      [[fallthrough]];
    case StepProjection::NET_FUSED: {
      // simulate.py:136-142: p, U = net(cat(p, U, flags, density)) -- the net only reads U and flags (model.py:104-126),
      // so the concatenation is not materialised: U is projected in place.
      const int mode = fnx::net_mode(prm->precision_mode);
      if (mode < 0) return fail(FNX_EINVAL, "simulate_step: unknown precision_mode %d", prm->precision_mode);
      // without flags_stick the tail of the net's forward and the step's last setConstVals are one pass (fluidnet_core)
      if (int rc = fnx::fluidnet_core(g, st->net, net_kind, st->flags, prm->normalize_threshold, mode, st->p, st->U, L.tail, stream,
                                      plan.projection == StepProjection::NET_FUSED ? st : nullptr)) return rc;
      break;
    }
  }
  switch (plan.tail) {                         // simulate.py:154-168
    case StepTail::POST:
      if (int rc = post_projection(g, st, stream, word)) return rc;
      break;
    case StepTail::POST_PERIODIC: {
      // simulate.py:157-164: the patches read the field as it was before setWallBcs; their source row / column (border cells,
      // which velocityUpdate leaves alone) is saved ahead of the in-place pass.  The solve is through with the tail.
      const fnx::BcPtrs bc = fnx::bc_ptrs(st);
      fnx::launch_periodic_post(d, g->is3D, st->U, (float*)L.tail, nullptr, nullptr, plan.stage.px, plan.stage.py, 0, s);
      if (int rc = post_projection(g, st, stream, word)) return rc;
      fnx::launch_periodic_post(d, g->is3D, st->U, (float*)L.tail, bc.UBC, bc.UBCInvMask, plan.stage.px, plan.stage.py, 1, s);
      break;
    }
    case StepTail::STICK_BCS:                  // simulate.py:165-168
      if (int rc = stick_then_bcs()) return rc;
      break;
    case StepTail::NONE:
      break;
  }
  HIP_OK(hipGetLastError());
  return FNX_OK;
}

}  // extern "C"
