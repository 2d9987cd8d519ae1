// Host-side launch wrappers of the gfx950 kernels (internal to libfluidnet_hip.so).
#pragma once
#include <hip/hip_runtime.h>
#include "fnx_device.h"
#include "fnx_jacobi_plan.h"
#include "fnx_step_plan.h"

namespace fnx {

// sets the calling thread's fnx_last_error() message and returns `code` (fnx_api.hip)
int set_error(int code, const char* fmt, ...);

// event-pair timing of kernel classes (fnx_api.hip); no-ops unless fnx_profile_enable(1)
bool prof_begin(int tag, hipStream_t s);      // true: a roctx range was pushed (prof_end pops only then)
void prof_end(int tag, hipStream_t s, bool pushed);
void prof_add_work(int tag, double amount);   // adds to the class's work counter while a recorded launch of it is open
struct ProfScope {
  int tag; hipStream_t s; bool pushed;
  ProfScope(int t, hipStream_t st) : tag(t), s(st), pushed(prof_begin(t, st)) {}
  ~ProfScope() { prof_end(tag, s, pushed); }
};

// advection (fnx_advect.hip): a call is planned (advect_plan), given its workspace (advect_workspace) and launched (launch_advect)
enum { ADVECT_RHO = 1, ADVECT_VEL = 2, ADVECT_BOTH = 3 };   // `what`: the density by U, `orig` by U, or one step's pair (orig is U)
enum class AdvectPath { CELLS, TILES_2D, TILES_3D };        // one thread per cell; LDS tiles (2D); z-marching LDS tiles (3D)
struct AdvectPlan {
  GridDims g, gfwd;        // the compute window; the window of the forward pass (MacCormack: widened by what the backward pass reads)
  bool is3d, quirks;
  int what;
  bool maccormack;         // false: Euler, the forward pass writes dst and nothing follows
  AdvectPath fwd, bwd;     // 2D: both tiles or both cells; 3D: see advect_plan
  bool bwd_fused;          // TILES_3D backward pass of a pair: one march for density and velocity instead of two
  bool cells_pair;         // CELLS passes: the pair's fused kernels instead of the stand-alone scalar / velocity kernels
};
// request: FNX_ADVECT_PLAN_*; method: FNX_ADVECT_EULER / _MACCORMACK; orig_is_U: what the velocity advection advects is U itself
AdvectPlan advect_plan(const GridDims& g, bool is3d, bool quirks, int what, bool orig_is_U, int method, int request);
// Workspace of a MacCormack call, in this order: forward density, traced cell, 3D clamp bounds (the density's three), forward
// velocity, the tile kernels' four fix-up bitmaps (2D and 3D); each rounded up to 256 bytes.  base == nullptr: the size only.
struct AdvectWs { float* rho_fwd; int* cell; float2* box; float* U_fwd; unsigned long long* fix; size_t bytes; };
AdvectWs advect_workspace(const GridDims& g, bool is3d, int what, void* base);
struct AdvectArgs {
  float dt, half_s; bool sample_outside;
  const float *rho, *orig, *U, *flags;
  float *rho_dst, *U_dst;
};
void launch_advect(const AdvectPlan& p, const AdvectArgs& a, const AdvectWs& ws, hipStream_t s);
// the 3D clamp bounds of the planes [K0, K0 + KN) of `channels` fields per sample (src, box: B * channels plane stacks; flags: B), the
// reduction both launch_advect (channels = 1) and launch_advect_scalars run; its grid's z extent is B * channels * ceil(KN / 16)
void launch_box_minmax(const GridDims& g, int channels, bool sample_outside, const float* src, const float* flags, float2* box,
                       hipStream_t s);

// passive scalars (fnx_scalars.hip): `channels` fields (B, C, D, H, W) through one pair of line traces, one thread per cell, whole
// single domains only.  Workspace of a MacCormack call: the C forward fields, the traced cell, in 3D the C clamp-bounds fields; each
// rounded up to 256 bytes (base == nullptr: the size only).  Euler writes dst directly and takes none.
struct AdvectScalarsWs { float* fwd; int* cell; float2* box; size_t bytes; };
AdvectScalarsWs advect_scalars_workspace(const GridDims& g, bool is3d, int channels, void* base);
// z chunks of the 3D clamp-bounds launch: its grid's z extent is B * channels * this
inline int advect_scalars_box_chunks(const GridDims& g) { return (g.D + 15) / 16; }
void launch_advect_scalars(const GridDims& g, bool is3d, bool quirks, bool maccormack, bool sample_outside, float dt, float half_s,
                           int channels, const float* src, const float* U, const float* flags, float* dst, const AdvectScalarsWs& w,
                           hipStream_t s);

// stencils (fnx_stencils.hip)
void launch_divergence(const GridDims& g, bool is3d, const float* U, const float* flags, float* div, hipStream_t s);
void launch_velocity_update(const GridDims& g, bool is3d, const float* p, float* U, const float* flags, hipStream_t s);
void launch_add_gravity(const GridDims& g, bool is3d, float* U, const float* flags, float fx, float fy, float fz,
                        hipStream_t s);
void launch_correct_scalar(const GridDims& g, bool is3d, float half_dt, float* src, const float* div, const float* flags,
                           hipStream_t s);
void launch_add_viscosity(const GridDims& g, const float* Uin, float* Uout, const float* flags, float coef,
                          hipStream_t s);
void launch_add_buoyancy(const GridDims& g, bool is3d, bool quirks, float* U, const float* flags, const float* rho,
                         float sx, float sy, float sz, float rho_star, hipStream_t s);
void launch_set_wall_bcs(const GridDims& g, bool is3d, float* U, const float* flags, hipStream_t s);
void launch_set_wall_bcs_stick(const GridDims& g, const float* Uin, float* Uout, const float* flags, const float* stick,
                               hipStream_t s);
void launch_set_const_vals(size_t n, float* x, const float* bc, const float* inv_mask, hipStream_t s);
void launch_flags_to_occupancy(size_t n, const float* flags, float* occ, hipStream_t s);
void launch_max_abs(size_t n, const float* x, float* out, hipStream_t s);
void launch_empty_domain(const GridDims& g, bool is3d, float* flags, int bnd, hipStream_t s);
void launch_create_cylinder(const GridDims& g, float* flags, float cx, float cy, float r2, hipStream_t s);
void launch_create_box2d(const GridDims& g, float* flags, float x0, float x1, float y0, float y1, hipStream_t s);
void launch_get_centered(const GridDims& g, bool is3d, const float* U, float* out, hipStream_t s);
void launch_divergence_bwd(const GridDims& g, bool is3d, const float* gdiv, const float* flags, float* gU, hipStream_t s);
void launch_velocity_update_bwd(const GridDims& g, bool is3d, const float* gout, const float* flags, float* gU, float* gp,
                                hipStream_t s);

// 3D obstacles from geometry (fnx_voxelize.hip): whole 3D domains; the samples [b0, b0 + nb) are written.  The mesh voxeliser's
// workspace is one toggle bit per (k, j, i0), i0 in 0..W, in 32-bit words by rows, then two counters (open rows, bad faces); the
// caller zeroes all of it before the launch.
inline int voxel_words_per_row(const GridDims& g) { return g.W / 32 + 1; }                       // ceil((W + 1) / 32)
inline size_t voxel_words(const GridDims& g) { return (size_t)g.D * g.H * voxel_words_per_row(g); }
void launch_create_sphere(const GridDims& g, float* flags, int b0, int nb, float cx, float cy, float cz, float r2, hipStream_t s);
void launch_create_box3d(const GridDims& g, float* flags, int b0, int nb, float x0, float x1, float y0, float y1, float z0, float z1,
                         hipStream_t s);
void launch_voxelize_mesh(const GridDims& g, float* flags, int b0, int nb, const float* vertices, int n_vertices, const int* faces,
                          int n_faces, unsigned* bits, int* counters, hipStream_t s);

// the viscous-flow operators in 3D (fnx_viscous.hip; default semantics only: the reference has no 3D form to reproduce).  Both are out
// of place, Uout must not alias Uin.  addViscosity marches whole grids along z; setWallBcsStick honours a compute window and a z-slab view
void launch_add_viscosity3d(const GridDims& g, const float* Uin, float* Uout, const float* flags, float coef, hipStream_t s);
void launch_set_wall_bcs_stick3d(const GridDims& g, const float* Uin, float* Uout, const float* flags, const float* stick,
                                 hipStream_t s);

// fused step stages (fnx_step.hip)
// The BC arrays of a state as the stages take them: a pair counts only with both of its halves (bc_ptrs); cls: the optional class map
// word: the optional stage word map of a 3D array (fnx_stage_word.h; needs cls): the 3D stage and the unscaled 3D post-projection pass then
// read it instead of flags and cls.  Only fnx_simulate_step has one (the map lives in its workspace).
struct BcPtrs { const float *UBC, *UBCInvMask, *rhoBC, *rhoBCInvMask; const unsigned char* cls; const unsigned* word; };
inline BcPtrs bc_ptrs(const FnxState* st, const unsigned* word = nullptr) {
  const bool ubc = st->UBC && st->UBCInvMask, rbc = st->densityBC && st->densityBCInvMask;
  return BcPtrs{ubc ? st->UBC : nullptr, ubc ? st->UBCInvMask : nullptr, rbc ? st->densityBC : nullptr, rbc ? st->densityBCInvMask : nullptr,
                st->bc_class, st->bc_class ? word : nullptr};
}
// The stage between the advection and the projection: U_adv, rho_adv (may be null) -> U, rho and, with `div`, the divergence of the
// staged field (the staged value of a cell's +1 neighbours is re-derived in the same pass; their advected inputs must be valid)
struct StageIO {
  const float *U_adv, *rho_adv, *flags;
  BcPtrs bc;
  float *U, *rho, *div;
};
struct StageOps {
  bool quirks;
  bool first_bcs;              // false leaves out the setConstVals of simulate.py:96 (U_adv is a field that has been through it already)
  bool buoy; float s[3];       // strengths gravity * dt
  float rho_star;
  bool grav; float g[3];       // forces gravity * dt
  bool wall;
  bool second_bcs;             // false leaves out the setConstVals of simulate.py:133
  int div_k_end;               // 3D with div: the divergence is written for the planes [g.K0, div_k_end) of the staged range
};
void launch_pre_projection(const GridDims& g, bool is3d, const StageIO& io, const StageOps& ops, hipStream_t s);
// periodic patches of the Jacobi branch (simulate.py:121-128, :157-164); `save`: periodic_save_bytes(g), mode 0 = save the
// source row / column before the post-projection pass, 1 = write the destinations after it
void launch_periodic_pre(const GridDims& g, bool is3d, const float* U_adv, const float* UBC, const float* UBCInvMask, float* U,
                         bool px, bool py, hipStream_t s, bool staged = false);   // staged: U_adv is the field ahead of setWallBcs itself
size_t periodic_save_bytes(const GridDims& g);
void launch_periodic_post(const GridDims& g, bool is3d, float* U, float* save, const float* UBC, const float* UBCInvMask,
                          bool px, bool py, int mode, hipStream_t s);
void launch_post_projection(const GridDims& g, bool is3d, const float* p, float* U, float* rho, const float* flags, const BcPtrs& bc,
                            hipStream_t s, bool rho_bc_applied = false, const float* scale = nullptr, float* p_scaled = nullptr);
// scale (B device floats) / p_scaled: the tail of FluidNet.forward in the same pass (u = U / s into the update, u * s and
// p_scaled = p * s out of it); p_scaled must not alias p (a cell reads p of its -1 neighbours)
void launch_bc_classify(const GridDims& g, bool is3d, const BcPtrs& bc, unsigned char* cls, hipStream_t s);
// the stage word of every cell of a 3D array (all D planes, whatever the compute window) from flags and the class map
void launch_stage_word(const GridDims& g, const float* flags, const unsigned char* cls, unsigned* word, hipStream_t s);

// vorticity confinement (fnx_vorticity.hip): U_out = U_in + the confinement force of U_in scaled by amp; whole grids only (no
// compute window, no z-slab view); U_out must not alias U_in
void launch_vorticity_confinement(const GridDims& g, bool is3d, const float* U_in, const float* flags, float* U_out, float amp,
                                  hipStream_t s);

// volume rendering (fnx_render.hip): density + flags -> image (B, 2, R, Cc), channel 0 radiance, channel 1 transmittance.  Directions
// 0..5 = +x -x +y -y +z -z (the way rays / light travel).  Lws: B*D*H*W floats, unused (may be NULL) when view_dir == light_dir.
struct RenderConsts { float k_view, k_light, ambient, one_minus_ambient, albedo_smoke, albedo_obstacle; int bnd; };
void launch_render_volume(const GridDims& g, int view_dir, int light_dir, const RenderConsts& c, const float* density, const float* flags,
                          float* Lws, float* image, hipStream_t s);

// Jacobi (fnx_jacobi.hip).  What a call decides before it launches is fnx_jacobi_plan.h, pure functions: the schedule of a run of sweeps,
// the tile geometry, mask layout, launch plan and mirror predicate of the 3D two-sweep march.  The launches:
// 2D: `nsweeps` sweeps (1..jacobi_max_sweeps_per_launch) from p_in into p_out; from_zero: p_in is all zeros and is not read
void launch_jacobi(const GridDims& g, const float* flags, const float* div, const float* p_in, float* p_out, int nsweeps,
                   bool from_zero, hipStream_t s);
// 3D: flags -> 7-bit neighbour mask (once per solve), then z-marching passes of two sweeps (one for an odd remainder)
void launch_jacobi3d_mask(const GridDims& g, bool quirks, const float* flags, const JacobiMaskLayout& mask, hipStream_t s);
// kb/ke: restrict the OUTPUT to planes [kb, ke) (0,0 = all planes); inputs are read from kb-1 (kb-2 for x2) on
void launch_jacobi3d(const GridDims& g, const JacobiMaskLayout& mask, const float* div, const float* p_in, float* p_out,
                     bool from_zero, hipStream_t s, int kb = 0, int ke = 0);
// mirror of a two-sweep launch's output: planes [k[r], k[r] + n) of plane range r also go to out[r][q] + sample * bstride (floats),
// q = (*sel[r] + 1) & 1 read on the device (sel NULL: q = 0)
struct JacobiMirror { float* out[2][2]; const unsigned* sel[2]; int k[2]; int n; unsigned long long bstride; unsigned long long* clock; };
// plans (jacobi3d_x2_plan) and launches: once, or once per plane range when the two (kb2 >= 0: [kb2, kb2 + ke - kb)) do not fit together
void launch_jacobi3d_x2(const GridDims& g, const JacobiMaskLayout& mask, const float* div, const float* p_in, float* p_out,
                        hipStream_t s, int kb = 0, int ke = 0, bool from_zero = false, int kb2 = -1, int lay = 0,
                        const JacobiMirror* mirror = nullptr, int x_request = 0);   // x_request: JACOBI3D_X_* (fnx_jacobi_plan.h)
// Reproducible residual (no atomics): per sample b the squared differences of a[b*per_sample + first + q] - b[...] (b == null:
// zeros), q < count, summed in a fixed order in fp64 through `partials` (residual_scratch_bytes(B)); sumsq (B floats, may be
// null) receives the sums, res (1 float, may be null) max_b sqrt(sum)
size_t residual_scratch_bytes(int B);
void launch_residual(int B, size_t per_sample, size_t first, size_t count, const float* a, const float* b, double* partials,
                     float* sumsq, float* res, hipStream_t s);
void launch_residual_root(int B, const float* sumsq, float* res, hipStream_t s);   // res = max_b sqrt(sumsq[b])

// Multigrid-preconditioned CG (fnx_pcg.hip).  `kept`: the hierarchy built from flags (pcg_kept_bytes, reusable while flags do not
// change); `scratch`: vectors, partial sums and per-sample scalars (pcg_scratch_bytes).
size_t pcg_kept_bytes(const GridDims& g, bool is3d);
size_t pcg_scratch_bytes(const GridDims& g, bool is3d);
void launch_pcg_build(const GridDims& g, bool is3d, bool quirks, const float* flags, void* kept, hipStream_t s);
void launch_poisson_apply(const GridDims& g, bool is3d, bool quirks, const float* flags, const float* x, float* y, hipStream_t s);
void launch_pcg_precondition(const GridDims& g, bool is3d, const void* kept, void* scratch, const float* r, float* z, hipStream_t s);
// returns FNX_OK or an FNX_E* code (set_error); synchronises only for tol > 0, iters_done != null or verbose.  p0: a starting guess or
// null (the cold solve, launch for launch); it may be p.  With p0, max_iter 0 returns the line-searched guess.
int pcg_solve(const GridDims& g, bool is3d, const void* kept, void* scratch, const float* div, const float* p0, float* p, float* residual,
              float tol, int max_iter, int* iters_done, bool verbose, hipStream_t s);

}  // namespace fnx
