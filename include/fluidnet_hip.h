/*
 * fluidnet_hip.h -- C ABI of libfluidnet_hip.so, the MI355X (gfx950) fluid time-step library.
 *
 * This is the drop-in boundary for fluidnet_cxx's operator surface.  Each entry point cites the
 * reference interface it replaces (paths relative to the reference repo root).  The torch
 * cpp-extension `fluidnet_cpp` (fluidnet_cxx_amd/csrc/fluidnet_cpp.cpp) binds these 1:1 behind
 * the reference's three pybind names (pytorch/lib/fluid/cpp/fluids_init.cpp:1009-1014) plus the
 * operators the reference implements in Python; INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - every tensor is a caller-owned DEVICE pointer on the current HIP device, fp32, contiguous
 *    (B,C,D,H,W) with x fastest; 2D == D=1 with 2 velocity channels, 3D has 3.  `flags` is fp32
 *    holding Manta cell types exactly as the reference passes them (cpp/cell_type.h:7-18).
 *  - nothing is allocated, retained or freed; scratch comes from the caller's `ws` buffer
 *    (size from fnx_workspace_bytes); outputs are caller-allocated.
 *  - every call only ENQUEUES work on `stream` (a hipStream_t, may be NULL = default stream) and
 *    returns without synchronising, except fnx_jacobi with p_tol > 0 (the reference's own
 *    per-sweep host test, fluids_init.cpp:973).
 *  - return value: FNX_OK or an FNX_E* code; fnx_last_error() gives the message (thread local).
 *    There is no CPU fallback: without a HIP device every compute entry point fails.
 */
#ifndef FLUIDNET_HIP_H
#define FLUIDNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FNX_ABI_VERSION 36

enum {
  FNX_OK = 0,
  FNX_EINVAL = 1,    /* bad argument (shape, bnd != 1, null pointer, max_iter < 1 ...) */
  FNX_EMETHOD = 2,   /* "Advection method not supported" (cpp/advect_type.cpp:14) */
  FNX_EWORKSPACE = 3,/* workspace too small */
  FNX_EHIP = 4,      /* HIP runtime error / no device */
  FNX_ECFL = 5,      /* z-slab step: max |U| dt > 1 cell (the decomposition's ghost widths rest on CFL <= 1) */
  FNX_ECOMM = 6      /* communicator error (RCCL call failed, librccl not loadable, peer missing) */
};

/* Cell types, cpp/cell_type.h:7-18 and lib/fluid/cell_type.py:5-14 */
enum { FNX_TYPE_NONE = 0, FNX_TYPE_FLUID = 1, FNX_TYPE_OBSTACLE = 2, FNX_TYPE_EMPTY = 4,
       FNX_TYPE_INFLOW = 8, FNX_TYPE_OUTFLOW = 16, FNX_TYPE_OPEN = 32, FNX_TYPE_STICK = 128 };

/* Advection methods, cpp/advect_type.cpp:5-16 ("eulerFluidNet", "maccormackFluidNet") */
enum { FNX_ADVECT_EULER = 0, FNX_ADVECT_MACCORMACK = 1 };

enum { FNX_JACOBI3D_X_SHIFT = 8, FNX_JACOBI3D_X_AUTO = 0, FNX_JACOBI3D_X_60 = 1, FNX_JACOBI3D_X_64 = 2 };   /* FnxGrid.ref_quirks bits 8-9 */

typedef struct FnxGrid {
  int B, D, H, W;   /* batch, depth (1 for 2D), height, width */
  int is3D;         /* 0: U has 2 channels and D must be 1; 1: U has 3 channels */
  int ref_quirks;   /* 3D only.  Bit 0: 1 reproduces the reference's 3D defects bit-for-bit,
                       0 (default) gives the intended 3D semantics.  Ignored in 2D.
                       Bits 8-9 (FNX_JACOBI3D_X_*  << FNX_JACOBI3D_X_SHIFT; A/B timing and tests, the results are the same bits):
                       the column tiling of the 3D two-sweep Jacobi march -- 0 the plan's choice, 1 the 60-column tiles,
                       2 the 64-column tiles wherever that kernel can run. */
  /* z-slab decomposition (3D, multi-GPU): the arrays hold planes [z_offset, z_offset + D) of a domain that is
     D_global planes deep; only the domain-border test uses them.  0 / 0 = a whole domain (the default). */
  int z_offset, D_global;
  /* Compute window (z-slab driver): the cell-parallel operators -- advection, the BC/buoyancy/wall/divergence stage,
     velocity update and the stand-alone stencils -- only produce local planes [k_begin, k_end); planes outside keep
     their old contents.  They still READ outside the window.  MacCormack advection evaluates its forward pass on the
     window widened by 2 planes, which covers what the backward pass and the clamp read while |U dt| <= 1 cell (the
     same bound the ghost width of the decomposition rests on).  0 / 0 = all planes (the default).  The Jacobi entry
     points take their own plane range. */
  int k_begin, k_end;
} FnxGrid;

/* Workspace sizing. */
enum { FNX_OP_ADVECT_SCALAR = 0, FNX_OP_ADVECT_VEL = 1, FNX_OP_JACOBI = 2, FNX_OP_STEP = 3, FNX_OP_FLUIDNET = 4,
       FNX_OP_ADVECT_STEP = 5,
       FNX_OP_STEP_STATIC = 6   /* ABI 33: FNX_OP_STEP plus, in 3D, 4 bytes per cell for the stage word map that fnx_simulate_step keeps
                                   behind the step's layout when flags and BC arrays are promised static (FnxStepParams.static_flags).
                                   FNX_OP_STEP stays what it was and stays enough for every call; in 2D the two are equal */
};
size_t fnx_workspace_bytes(const FnxGrid* g, int op);

const char* fnx_last_error(void);
int fnx_abi_version(void);
/* name of the HIP device the library would run on, or NULL (and FNX_EHIP set) when there is none */
const char* fnx_device_name(void);

/* advectScalar: pybind `advect_scalar`, cpp/fluids_init.cpp:265-382 (wrapper cpp/advection.py:14-66).
 * dst must not alias src.  MacCormack in 3D default semantics, and in 2D from 1.5 M cells, runs the LDS tile kernels of the fused pair
 * below with its density part only (ABI 19; FNX_OP_ADVECT_SCALAR grew by the tiles' fix-up bitmaps); quirks mode, Euler and small 2D
 * grids run one thread per cell.  Same bits either way. */
int fnx_advect_scalar(const FnxGrid* g, float dt, const float* src, const float* U, const float* flags,
                      float* dst, int method, int bnd, int sample_outside_fluid, float maccormack_strength,
                      void* ws, size_t ws_bytes, void* stream);

/* advectVel: pybind `advect_vel`, cpp/fluids_init.cpp:656-807 (wrapper cpp/advection.py:68-118).
 * orig may alias U (self-advection); dst must alias neither.  Self-advection (orig == U, what lib/simulate.py:93 passes unless
 * viscosity > 0) takes the LDS tile kernels under the same conditions as fnx_advect_scalar (ABI 19); same bits either way. */
int fnx_advect_vel(const FnxGrid* g, float dt, const float* orig, const float* U, const float* flags,
                   float* dst, int method, int bnd, float maccormack_strength,
                   void* ws, size_t ws_bytes, void* stream);

/* The two advections of one time step (lib/simulate.py:75-93): density by U and U by itself, both MacCormack, both
 * from the OLD U, as one fused pair of launches (forward passes together, backward/clamp passes together).  Results
 * are bit-identical to fnx_advect_scalar + fnx_advect_vel.  dst buffers must not alias the inputs. */
int fnx_advect_step(const FnxGrid* g, float dt, const float* density, const float* U, const float* flags,
                    float* density_dst, float* U_dst, int sample_outside, float strength, void* ws, size_t ws_bytes,
                    void* stream);
/* The same with the kernel family chosen by the caller instead of by grid size (same bits either way): */
enum { FNX_ADVECT_PLAN_AUTO = 0,      /* what fnx_advect_step does: LDS tile kernels in 3D and on 2D grids of >= 1.5 M cells */
       FNX_ADVECT_PLAN_TILES = 1,     /* LDS tile kernels + fix-up launches (CFL < 1 is their fast path, any CFL is correct) */
       FNX_ADVECT_PLAN_CELLS = 2,     /* one thread per cell, gathers from global memory */
       FNX_ADVECT_PLAN_TILES_SPLIT = 3 };  /* TILES with the 3D backward pass of fnx_advect_step as two marches (density, velocity) instead of the
                                              fused one (same bits, 1 % slower: a timing aid) */
int fnx_advect_step_plan(const FnxGrid* g, float dt, const float* density, const float* U, const float* flags,
                         float* density_dst, float* U_dst, int sample_outside, float strength, int plan, void* ws,
                         size_t ws_bytes, void* stream);
/* ... and the stand-alone operators with the kernel family chosen by the caller (ABI 19; TILES is honoured where tiles exist: MacCormack,
 * default 3D semantics or 2D, fnx_advect_vel with orig == U -- elsewhere the call runs one thread per cell): */
int fnx_advect_scalar_plan(const FnxGrid* g, float dt, const float* src, const float* U, const float* flags,
                           float* dst, int method, int bnd, int sample_outside_fluid, float maccormack_strength, int plan,
                           void* ws, size_t ws_bytes, void* stream);
int fnx_advect_vel_plan(const FnxGrid* g, float dt, const float* orig, const float* U, const float* flags,
                        float* dst, int method, int bnd, float maccormack_strength, int plan,
                        void* ws, size_t ws_bytes, void* stream);

/* Passive scalar transport (ABI 28; no reference counterpart): `channels` fields, src and dst (B, channels, D, H, W) contiguous, advected
 * by U through ONE forward and ONE backward line trace -- the trace, the interpolation weights, the corners' fluid bits and the clamp
 * neighbourhood's validity depend on U, flags and dt alone.  Channel c of dst has the bits fnx_advect_scalar gives for channel c alone
 * (any plan), so a caller may mix the two freely.  One thread per cell; no atomics.  Whole single domains only: a compute window or a
 * z-slab view is FNX_EINVAL ("single-domain only"); ref_quirks is honoured.  dst must not alias src; channels >= 1; bnd == 1.
 * Workspace (MacCormack; Euler takes none): channels forward fields, one traced-cell field and, in 3D, channels clamp-bounds fields
 * (8 bytes a cell); 3D also needs B * channels * ceil(D/16) <= 65535. */
size_t fnx_advect_scalars_workspace_bytes(const FnxGrid* g, int channels);
int fnx_advect_scalars(const FnxGrid* g, float dt, int channels, const float* src, const float* U, const float* flags,
                       float* dst, int method, int bnd, int sample_outside_fluid, float maccormack_strength,
                       void* ws, size_t ws_bytes, void* stream);

/* velocityDivergence, lib/fluid/velocity_divergence.py:4-74 */
int fnx_velocity_divergence(const FnxGrid* g, const float* U, const float* flags, float* div, void* stream);

/* solveLinearSystemJacobi: pybind `solve_linear_system`, cpp/fluids_init.cpp:809-1004.
 * p: output (B,1,D,H,W).  residual: DEVICE pointer to 1 float (max over batch of ||p - p_prev||_2 of the
 * last sweep) or NULL.  iters_done: HOST pointer or NULL.  p_tol <= 0 never synchronises.
 * The residual is reproducible: squared differences summed in a fixed order in fp64 (no atomics), so the sweep at which a
 * p_tol > 0 solve stops is the same run to run.  With residual != NULL the last sweep runs as its own launch (both
 * iterates must be in memory); fnx_simulate_step passes NULL. */
int fnx_jacobi(const FnxGrid* g, const float* flags, const float* div, float* p, float* residual,
               float p_tol, int max_iter, int* iters_done, void* ws, size_t ws_bytes, void* stream);
/* The same with `verbose` of the reference (cpp/fluids_init.cpp:968-987): "Jacobi iteration N: residual R" on stdout after
 * EVERY sweep and the two termination messages -- one sweep per launch and one host synchronisation per sweep. */
int fnx_jacobi_verbose(const FnxGrid* g, const float* flags, const float* div, float* p, float* residual,
                       float p_tol, int max_iter, int* iters_done, void* ws, size_t ws_bytes, void* stream);
/* ||a - b||_2 per sample over the compute window of g (b == NULL: zeros), reproducible as above: sumsq (B DEVICE floats, may be
 * NULL) receives the sums of squares, residual (1 DEVICE float, may be NULL) max_b sqrt(sum).  ws: B * 4096 bytes.  What the
 * z-slab driver all-reduces over the ranks for p_tol > 0. */
int fnx_residual(const FnxGrid* g, const float* a, const float* b, float* sumsq, float* residual, void* ws, size_t ws_bytes, void* stream);

/* `nsweeps` more Jacobi sweeps starting from the pressure already in `p` (in place).  Same per-sweep arithmetic as
 * fnx_jacobi (cpp/fluids_init.cpp:858-994); used by the z-slab driver, which exchanges ghost planes of p between
 * blocks of sweeps.  No residual. */
int fnx_jacobi_sweeps(const FnxGrid* g, const float* flags, const float* div, float* p, int nsweeps,
                      void* ws, size_t ws_bytes, void* stream);
/* Same, for callers that keep `ws` alive between calls on the SAME flags: bit 0 of reuse_mask skips rebuilding the 3D
 * neighbour mask that an earlier call (without it) left in `ws`.  Bit 1: the solve starts from p = 0 -- `p` is not read
 * (it need not be zeroed), the first launch is the from-zero instantiation: a whole solve without the residual of
 * fnx_jacobi, which is what the z-slab driver runs on a single rank. */
int fnx_jacobi_sweeps_ex(const FnxGrid* g, const float* flags, const float* div, float* p, int nsweeps,
                         void* ws, size_t ws_bytes, int reuse_mask, void* stream);

/* One pass of 1 or 2 sweeps (3D) from p_in into p_out restricted to the output planes [k_begin, k_end)
 * (0,0 = all); explicit buffers, no ping-pong.  p_in == NULL: the pressure is 0 everywhere (first pass of a solve).  Lets the z-slab driver compute the planes its neighbours need
 * first, start the ghost exchange, and compute the interior while the exchange is in flight.  `ws` as for
 * fnx_jacobi_sweeps_ex (holds the neighbour mask). */
int fnx_jacobi_pass(const FnxGrid* g, const float* flags, const float* div, const float* p_in, float* p_out,
                    int nsweeps, int k_begin, int k_end, void* ws, size_t ws_bytes, int reuse_mask, void* stream);
/* The same for TWO disjoint plane ranges of equal length in one launch: [k_begin, k_end) and [k_begin2, k_begin2 +
 * k_end - k_begin) (k_begin2 < 0: one range).  The slab driver's edge parts at the lower and the upper internal face. */
int fnx_jacobi_pass2(const FnxGrid* g, const float* flags, const float* div, const float* p_in, float* p_out,
                     int nsweeps, int k_begin, int k_end, int k_begin2, void* ws, size_t ws_bytes, int reuse_mask,
                     void* stream);
/* The same with the pressure arrays in the solver's ROW-QUAD layout p[b][k][j/4][i][j%4] (a plane is the same H*W floats as
 * in the row layout p[b][k][j][i]: ghost-plane exchanges do not care): layout bit 0 = p_in, bit 1 = p_out is row-quad.
 * Two-sweep passes only, on grids fnx_jacobi_quad_ok() accepts (3D, H % 4 == 0).  A chain of passes reads the pressure with
 * 3 instead of 8 and writes it with 1 instead of 4 vector-memory instructions per step of the march when its passes hand each
 * other this layout; the first pass of a solve has no input, the last one writes rows (layout 1).  fnx_jacobi and
 * fnx_jacobi_sweeps do this internally. */
int fnx_jacobi_quad_ok(const FnxGrid* g);
int fnx_jacobi_pass_layout(const FnxGrid* g, const float* flags, const float* div, const float* p_in, float* p_out,
                           int nsweeps, int k_begin, int k_end, int k_begin2, int layout, void* ws, size_t ws_bytes,
                           int reuse_mask, void* stream);

/* A two-sweep pass that ALSO stores some of the planes it finishes to a second destination ("mirror"): the planes
 * [k_first[r], k_first[r] + planes) of plane range r (0: [k_begin, k_end); 1: the second range) go to out[r][q] + sample * sample_stride
 * floats, plane after plane, each in the layout of p_out.  The destination is double buffered: q = (*slot_select[r] + 1) & 1, read ON
 * THE DEVICE when the launch starts (slot_select[r] NULL: q = 0) -- whose turn it is may depend on how often a captured graph has been
 * replayed.  What the z-slab driver's last edge part of a sweep block uses to write the planes its neighbours need next straight into
 * their mapped mailboxes (FnxSlabComm.direct_begin): the transport then has nothing left to copy on the sending side.  layout 0 (rows in
 * and out) or 3 (row-quad in and out); p_in != NULL; only launches fnx_jacobi_pass_mirror_ok accepts (every (tile, plane chunk) wave
 * resident at once). */
typedef struct FnxPlaneMirror {
  float* out[2][2]; const unsigned* slot_select[2]; int k_first[2]; int planes; size_t sample_stride;
  unsigned long long* start_clock;   /* optional DEVICE word: the launch stores the device clock (wall_clock64) there when it starts */
} FnxPlaneMirror;
int fnx_jacobi_pass_mirror_ok(const FnxGrid* g, int planes_per_range, int two_ranges, int layout);
int fnx_jacobi_pass_mirror(const FnxGrid* g, const float* flags, const float* div, const float* p_in, float* p_out, int k_begin,
                           int k_end, int k_begin2, int layout, const FnxPlaneMirror* mirror, void* ws, size_t ws_bytes,
                           int reuse_mask, void* stream);

/* ---- Converged pressure solve (ABI 20; the reference has none: its README names PCG as what FluidNet replaces) ----
 * The system is the fixed point of fnx_jacobi, in the same semantics (FnxGrid.ref_quirks included): on an ACTIVE cell (neither
 * border nor TypeObstacle)  (denom - n_obs) p_i - sum_{active nbr j} p_j = div_i,  denom 4 (2D) / 6 (3D), n_obs the obstacle
 * neighbours (Neumann: the Jacobi substitutes p_i; with ref_quirks in 3D the z obstacle neighbours count 0 instead),
 * a non-obstacle border neighbour 0 (Dirichlet); every other cell gets p = 0.  A is symmetric positive semi-definite.  A sample none
 * of whose active cells touches a Dirichlet cell (every closed box) is singular: div is projected onto mean zero over the active
 * cells, and p is returned with active-cell mean zero (velocityUpdate ignores constants).  Several closed fluid components (a pocket
 * sealed inside obstacles) keep one null vector each of which only the global mean is removed: such a solve may stop at max_iter
 * without converging (finite output, residual above p_tol).
 * Method: conjugate gradients from p = 0, preconditioned by one symmetric V-cycle of an aggregation multigrid (2:1 in every axis,
 * Galerkin coarse operators built from flags on the device, damped Jacobi 2 + 2, coarse correction x 1.8).  Per sample it stops at
 * ||r||_2 <= p_tol ||b||_2 (b: the projected div) and is frozen from then on.  residual: DEVICE float, max over the batch of that
 * relative residual from the recurrence (may be NULL); iters_done: HOST int[B] or NULL.  p_tol <= 0 runs exactly max_iter
 * iterations without a host synchronisation (capturable in a HIP graph); p_tol > 0 reads one device flag every 4 iterations.
 * Dot products: fp64 partial sums added in a fixed order, no atomics -- the same bits run to run.  No compute window, no z-slab view. */
size_t fnx_pcg_workspace_bytes(const FnxGrid* g);
int fnx_pcg(const FnxGrid* g, const float* flags, const float* div, float* p, float* residual, float p_tol, int max_iter,
            int* iters_done, void* ws, size_t ws_bytes, void* stream);
/* The same with one line per iteration on stdout ("PCG iteration N: residual R") and the termination reason: one host
 * synchronisation per iteration. */
int fnx_pcg_verbose(const FnxGrid* g, const float* flags, const float* div, float* p, float* residual, float p_tol, int max_iter,
                    int* iters_done, void* ws, size_t ws_bytes, void* stream);
/* ABI 27: the same solve from a starting guess p0 (DEVICE, the shape of p; it may BE p: it is read before p is written).
 * p0 == NULL is fnx_pcg.  Let d = p0 on the active cells and 0 elsewhere.  The solve starts from x = a0 d with the line-search scale
 *   a0 = (d . b) / (d . A d),
 * b the projected div: one steepest-descent step along d.  a0 = 0 is among the candidates, so in the energy norm the start is never
 * worse than the cold one, and a guess of the wrong magnitude (an un-normalised or under-trained net) is repaired for free.  A d,
 * d . b and d . A d do not change when a constant is added to d on a singular sample, so d needs no mean removal (p is returned
 * with active-cell mean zero as above).  The stopping test is unchanged, ||r|| <= p_tol ||b||, with r0 = b - a0 A d the true fp32
 * residual; a sample that meets it at the start reports 0 iterations.  Per sample the guess is REJECTED when d . A d is not > 0 or
 * a dot product is not finite (a zero, NaN or Inf guess): that sample runs the cold solve bit for bit, no value of the guess reaches
 * p.  max_iter >= 0 here: 0 returns the scaled guess (zeros where it was rejected).  With p_tol > 0 the start costs one more host
 * read of the stop flag.  Same workspace, same determinism, no compute window, no z-slab view. */
int fnx_pcg_from(const FnxGrid* g, const float* flags, const float* div, const float* p0, float* p, float* residual, float p_tol,
                 int max_iter, int* iters_done, void* ws, size_t ws_bytes, void* stream);
/* The same with fnx_pcg_verbose's lines, preceded (with a guess) by one line "PCG warm start: a0 <per sample> , residual R". */
int fnx_pcg_from_verbose(const FnxGrid* g, const float* flags, const float* div, const float* p0, float* p, float* residual, float p_tol,
                         int max_iter, int* iters_done, void* ws, size_t ws_bytes, void* stream);
/* Ap = A p (the operator above; p is read on active cells only, Ap is 0 elsewhere).  No workspace. */
int fnx_poisson_apply(const FnxGrid* g, const float* flags, const float* p, float* Ap, void* stream);
/* z = M^-1 r, one V-cycle of the preconditioner (a fixed symmetric linear map; r is read on active cells only, z is 0 elsewhere).
 * ws: fnx_pcg_workspace_bytes. */
int fnx_pcg_precondition(const FnxGrid* g, const float* flags, const float* r, float* z, void* ws, size_t ws_bytes, void* stream);

/* velocityUpdate (in place on U), lib/fluid/velocity_update.py:6-162 */
int fnx_velocity_update(const FnxGrid* g, const float* p, float* U, const float* flags, void* stream);

/* addBuoyancy (in place on U), lib/fluid/source_terms.py:6-116.  gravity: 3 HOST floats. */
int fnx_add_buoyancy(const FnxGrid* g, float* U, const float* flags, const float* density,
                     const float gravity[3], float rho_star, float dt, void* stream);

/* addGravity (in place on U), lib/fluid/source_terms.py:122-219.  gravity: 3 HOST floats. */
int fnx_add_gravity(const FnxGrid* g, float* U, const float* flags, const float gravity[3], float dt, void* stream);

/* correctScalar (in place on src), lib/fluid/cpp/advection.py:9-12: src += (dt * 0.5) * src * div on fluid cells. */
int fnx_correct_scalar(const FnxGrid* g, float dt, float* src, const float* div, const float* flags, void* stream);

/* addViscosity, lib/fluid/viscosity.py:7-70.  The reference updates U in place from a fully evaluated right-hand side; here U_in
 * is the old field and U_out (a distinct buffer) receives the result.  2D: the reference's bits (its fourth neighbour is (i-1, j-1)).
 * 3D (ABI 29; the reference's 3D branch cannot run, so default semantics only: with FnxGrid.ref_quirks it is FNX_EINVAL): on an
 * interior cell and component c, fp32, uncontracted, in this order,
 *   s = u(x+e_x) + u(x+e_y) + u(x+e_z);  s += u(x-e_x);  s += u(x-e_y);  s += u(x-e_z);  s -= 6 u(x)
 *   U_out = m * (u(x) + coef * s),  coef = (float)((double)dt * viscosity),  m = 1 if the cell and its -e_c neighbour are fluid, else 0
 * and the one-cell border is copied.  Stable for coef <= 1/6 (1/4 in 2D); not checked, as the reference checks nothing.  3D takes whole
 * grids only (no compute window, no z-slab view).
 * The reference multiplies dt and viscosity as Python doubles and rounds the product once; two doubles rounded to float first give a
 * coef that is an ulp off for about a third of all pairs (dt = 0.1 with viscosity = 0.05 is one).  A caller that holds the doubles
 * gets the reference's coef by passing dt = (float)(dt * viscosity), viscosity = 1 (the Python layer does). */
int fnx_add_viscosity(const FnxGrid* g, float dt, const float* U_in, float* U_out, const float* flags,
                      float viscosity, void* stream);

/* Vorticity confinement (ABI 22; no runnable reference counterpart -- the reference tree only keeps its per-cell statement as
 * dead code): U_out = U_in + the confinement force of U_in.  fp32, uncontracted, in this order, every field below being 0
 * outside the interior cells (1 <= i <= W-2, 1 <= j <= H-2, in 3D 1 <= k <= D-2):
 *   c_a = 0.5 (U_a(cell) + U_a(cell + e_a))                                  centred velocity (c_z = 0 in 2D)
 *   w   = curl c by central differences, w_z = 0.5 (d_x c_y - d_y c_x) ...   with d_a f = f(cell + e_a) - f(cell - e_a)
 *   n   = norm(w);  norm(v) = sqrt((v_x v_x + v_y v_y) + v_z v_z) if that sum > 1e-6, else 0
 *   g_a = 0.5 d_a n;  m = norm(g);  g = g / m if m > 1e-6 else 0;  F = (g x w) * amp
 *   U_a(cell) += 0.5 (F_a(cell - e_a) + F_a(cell))   on the interior cells and components addGravity writes (cell fluid or
 *                                                    empty, -e_a neighbour fluid, or empty under a fluid cell)
 * Every other value is copied.  A component depends on U_in within three cells in every axis, so U_out must be a distinct
 * buffer.  Whole grids only (no compute window, no z-slab view).  amp == 0 copies U_in. */
int fnx_add_vorticity_confinement(const FnxGrid* g, const float* U_in, float* U_out, const float* flags, float amp,
                                  void* stream);

/* Volume rendering (ABI 24; no reference counterpart): a density grid with its obstacles -> an image.  Axis-aligned and orthographic,
 * single scattering with self-shadowing from an axis-aligned light.  Axes x = W, y = H, z = D; a direction is the way rays or light
 * TRAVEL, 0..5 = +x -x +y -y +z -z; view_dir and light_dir are independent (equal: a headlight, opposite: backlit).
 * Per cell, fp32 add / subtract / multiply / compare in exactly this order (tests/render_reference.py is the same in numpy):
 *   rho = min(max(density, 0), 1);  obs = flags == FNX_TYPE_OBSTACLE
 *   a cell within bnd cells of a domain face is empty in both passes (not an obstacle, rho = 0); a 2D grid (D == 1) has no z faces
 *   light pass along light_dir, Lin = 1 before the first cell:  L[cell] = Lin;  Lin = obs ? 0 : Lin * (1 - min(k_light * rho, 1))
 *   view pass along view_dir, T = 1, C = 0:                     s = ambient + one_minus_ambient * L[cell]
 *     obs:   C = C + T * (albedo_obstacle * s);  T = 0
 *     else:  a = min(k_view * rho, 1);  C = C + (T * a) * (albedo_smoke * s);  T = T * (1 - a)
 * image: (B, 2, R, Cc) floats, channel 0 = C (radiance), channel 1 = T (what is left of the background).  Rows and columns are the two
 * axes the view does not travel along, in (z, y, x) order -- view along z: (y, x), along y: (z, x), along x: (z, y) -- index 0 is
 * coordinate 0, nothing is mirrored for the negative directions.
 * ws: fnx_render_volume_ws_bytes() bytes (L, one float per cell); 0 when view_dir == light_dir, which runs as one march with no L in
 * memory.  density and flags are only read.  Everything is launched on `stream`, nothing synchronises.  Whole grids only (no compute
 * window, no z-slab view). */
typedef struct FnxRenderParams {
  int view_dir, light_dir;      /* 0..5: +x -x +y -y +z -z */
  float k_view, k_light;        /* absorption per cell of rho = 1 */
  float ambient, one_minus_ambient, albedo_smoke, albedo_obstacle;
  int bnd;
} FnxRenderParams;
size_t fnx_render_volume_ws_bytes(const FnxGrid* g, const FnxRenderParams* prm);   /* 0 also for a grid or params that are refused */
int fnx_render_volume(const FnxGrid* g, const float* density, const float* flags, const FnxRenderParams* prm, float* image,
                      void* ws, size_t ws_bytes, void* stream);

/* setWallBcs (in place on U), lib/fluid/set_wall_bcs.py:4-86 */
int fnx_set_wall_bcs(const FnxGrid* g, float* U, const float* flags, void* stream);

/* setWallBcsStick, lib/fluid/set_wall_bcs_stick.py:5-157 (no-slip walls: `flags_stick` is a copy of flags with the
 * no-slip obstacle cells set to 128, cylinder.py:76).  As shipped the reference function raises NameError
 * on three unbound names (:62 ff.); with them bound its 2D body runs, and that is what the 2D form reproduces bit for bit
 * (tests/golden/stick.npz).  The reference updates U in place from gathered copies; here U_in is the old field and
 * U_out (a distinct buffer) receives the result.
 * 3D (ABI 29; the reference's 3D branch cannot run, :85-87, so default semantics only: with FnxGrid.ref_quirks it is FNX_EINVAL).
 * Every value is a function of U_in:
 *   slip value s_c(x): 0 on an obstacle cell; else 0 where the cell is fluid or stick, x_c > 0 and flags(x - e_c) is an obstacle; else U_in
 *   on a stick cell, component c: the fluid neighbours y = x -+ e_a inside the domain, a != c ascending, low before high, contribute
 *     s_c(y): t = -s_c(y_1), t = t - s_c(y_k), value t / (float)n (an IEEE division).  It is written unless x_c > 0 and
 *     flags(x - e_c) is fluid (a wall face: the normal component keeps its slip value, 0 on an obstacle); n = 0 keeps the slip value
 *   every other cell gets its slip value.
 * A compute window and a z-slab view are honoured as fnx_set_wall_bcs honours them (plane 0 of the domain has no -e_z rule). */
int fnx_set_wall_bcs_stick(const FnxGrid* g, const float* U_in, float* U_out, const float* flags,
                           const float* flags_stick, void* stream);

/* setConstVals (in place), lib/simulate.py:4-26.  Either triple may be NULL (key absent in batch_dict). */
int fnx_set_const_vals(const FnxGrid* g, float* U, const float* UBC, const float* UBCInvMask,
                       float* density, const float* densityBC, const float* densityBCInvMask, void* stream);

/* flagsToOccupancy, lib/fluid/flags_to_occupancy.py:6-19 */
int fnx_flags_to_occupancy(const FnxGrid* g, const float* flags, float* occupancy, void* stream);

/* max |x| over a (B,channels,D,H,W) field into *out_max (DEVICE float; overwritten).  No reference counterpart: the
 * z-slab driver's CFL guard (max |U| dt <= 1 is what its ghost widths rest on) and any caller that wants the CFL number
 * without a host-side reduction.  NaNs are ignored. */
int fnx_max_abs(const FnxGrid* g, const float* x, int channels, float* out_max, void* stream);

/* emptyDomain (writes flags), lib/fluid/util.py:5-47 */
int fnx_empty_domain(const FnxGrid* g, float* flags, int boundary_width, void* stream);

/* createCylinder, lib/fluid/geometry_utils.py:4-34: cells with (x - center_x)^2 + (y - center_y)^2 <= radius^2 (integer
 * cell indices against the float centre, fp32 arithmetic as the reference's tensor expression evaluates it) become
 * obstacles on every z plane.  The scalars are doubles like the python floats the reference takes: radius is squared in
 * double and then rounded to fp32, the centre is rounded to fp32 (what the tensor iterator does).  In place on flags. */
int fnx_create_cylinder(const FnxGrid* g, float* flags, double center_x, double center_y, double radius, void* stream);
/* createBox2D, lib/fluid/geometry_utils.py:36-63: cells with x0 <= x < x1 and y0 <= y < y1 become obstacles.  The
 * reference's body cannot run (it tests Y against y1 twice and names an undefined mask, :59-62); this is the box its
 * docstring describes.  In place on flags. */
int fnx_create_box2d(const FnxGrid* g, float* flags, float x0, float x1, float y0, float y1, void* stream);

/* 3D obstacles from geometry (ABI 36; no reference counterpart).  Cell (i, j, k) sits at the point (x, y, z) = (i, j, k), as for
 * fnx_create_cylinder.  Each call writes FNX_TYPE_OBSTACLE into the cells it finds inside, whatever they held, and touches no other
 * cell.  flags is (B,1,D,H,W) with B >= 1; sample = -1 applies the shape to every sample, sample = b to that one alone.  3D only: a
 * 2D grid, a compute window and a z-slab view are each refused, and every refusal comes before a pointer is read.
 * Sphere: dx*dx + dy*dy + dz*dz <= r*r in fp32, summed in that order -- fnx_create_cylinder's arithmetic with a third term (the
 * slice k == center_z is the cylinder's disc bit for bit).  Box: half open, x0 <= i < x1 and the same for y and z. */
int fnx_create_sphere(const FnxGrid* g, float* flags, double center_x, double center_y, double center_z, double radius, int sample,
                      void* stream);
int fnx_create_box3d(const FnxGrid* g, float* flags, float x0, float x1, float y0, float y1, float z0, float z1, int sample,
                     void* stream);
/* Triangle-mesh voxeliser: marks the cells whose point lies inside the closed surface, by the even-odd rule along x (overlapping closed
 * components cancel; for a union call once per component).  vertices: n_vertices x 3 float32 xyz, faces: n_faces x 3 int32, both on
 * the device (an array of no elements may be NULL).  The exact rule (snap to 1/64 cell, integer cover test per row, fp64 crossing position) is stated in DESIGN.md 34 and
 * tests/voxel_reference.py.  A face with an index outside [0, n_vertices), a NaN or Inf coordinate or a vertex farther than 2^14
 * cells from the origin is skipped and counted; nothing is read out of bounds for any input.  report (device int[2], may be NULL)
 * receives {open rows, bad faces}: a closed surface has no open row.  ws: fnx_voxelize_mesh_ws_bytes(g) bytes, 4-byte aligned --
 * (D*H*ceil((W+1)/32) + 2) * 4, whatever the face count; the call zeroes it on `stream` itself, so it can be captured into a graph
 * and replayed.  The toggles are integer XOR atomics: the result does not depend on their order. */
size_t fnx_voxelize_mesh_ws_bytes(const FnxGrid* g);   /* 0 (and fnx_last_error) for a grid the voxeliser refuses */
int fnx_voxelize_mesh(const FnxGrid* g, float* flags, const float* vertices, int n_vertices, const int* faces, int n_faces, int sample,
                      int* report, void* ws, size_t ws_bytes, void* stream);
/* getCentered, lib/fluid/grid.py:7-32: (B,2|3,D,H,W) MAC velocity -> (B,3,D,H,W) cell-centred velocity (the z channel
 * is 0 in 2D); what the drivers' field dumps plot (plume.py:243,336). */
int fnx_get_centered(const FnxGrid* g, const float* U, float* centered, void* stream);

/* One whole time step, lib/simulate.py:28-171 (the keys simulate() reads from mconf). */
typedef struct FnxStepParams {
  float dt;                   /* mconf['dt'] */
  float maccormack_strength;  /* mconf['maccormackStrength'] */
  int   sample_outside_fluid; /* mconf['sampleOutsideFluid'] */
  float buoyancy_scale;       /* mconf['buoyancyScale'] ; <= 0 skips addBuoyancy */
  float gravity_vec[3];       /* mconf['gravityVec'] x,y,z (scaled by -buoyancyScale inside, simulate.py:101-105) */
  float operating_density;    /* mconf['operatingDensity'] */
  float p_tol;                /* mconf['pTol'] */
  int   jacobi_iter;          /* mconf['jacobiIter'] */
  int   method;               /* 0 = 'jacobi', 1 = 'convnet', 2 = 'pcg' (ABI 20: fnx_pcg with pcg_tol / pcg_iter below; the wall BCs
                                 and periodic patches as for method 0).
                                 ABI 27: 3 = 'hybrid': the stages of method 2, but the solve is fnx_pcg_from started from the net's
                                 pressure of the staged U (st->net, precision_mode and normalize_threshold as for method 1: the
                                 un-normalised p that fnx_fluidnet_forward returns, written into st->p; the net updates no
                                 velocity; flags_stick is ignored as by methods 0 and 2); 4 = 'pcg' started from st->p as it
                                 stands on entry (the previous step's pressure; p = 0 gives the cold solve).  static_flags bits 0
                                 and 3 mean for 3 and 4 what they mean for 2.  The net's scratch and the solve's vectors overlap
                                 in the workspace tail -- the net has finished before the solve starts and the solve takes only
                                 st->p from it -- so fnx_workspace_bytes(FNX_OP_STEP) is what it was before ABI 27.
                                 ABI 35: the net of methods 1 and 3 is the ScaleNet, or the 2D bank net through fnx_simulate_step_net */
  float normalize_threshold;  /* mconf['normalizeInputThreshold'] (convnet) */
  int   precision_mode;       /* convnet: FNX_PRECISION_FP32 (0, the default), _FP32_DIRECT, _BF16X6 or _BF16X3, see fnx_multiscale_forward */
  int   static_flags;         /* promises about the previous fnx_simulate_step on this workspace (no reference key; every
                                 reference simulation keeps its flags and BC arrays fixed):
                                 bit 0: `flags` is unchanged -> the 3D Jacobi solver reuses the obstacle mask it left there;
                                 bit 1: UBC / UBCInvMask / densityBC / densityBCInvMask are unchanged -> the BC stages use a
                                        1-byte-per-cell class map kept in the workspace (see FnxState.bc_class);
                                 bit 2: that class map was already built by an earlier call with bit 1 set;
                                 bit 3 (method 2): the PCG multigrid hierarchy in this workspace was built by an earlier call for
                                        these flags AND this FnxGrid.ref_quirks (the hierarchy depends on both) -- reused only
                                        together with bit 0.
                                 ABI 33, 3D with bit 1 and a workspace of at least fnx_workspace_bytes(FNX_OP_STEP_STATIC) bytes:
                                 the stage before the projection and the pass after it (methods 0, 2, 3, 4) read one uint32 per cell,
                                 kept behind the step's layout, instead of seven `flags` values and seven class bytes: the flag
                                 codes and class bits of the cell and its six neighbours.  It is built in every call that does
                                 not set both bit 0 and bit 2 (it depends on the flags and on the BC arrays), and the results are
                                 bit for bit those of the smaller workspace.  The promises speak of the previous call with the
                                 same `ws` AND the same `ws_bytes`.
                                 The step workspace (fnx_workspace_bytes FNX_OP_STEP) holds that hierarchy for every method:
                                 ~2 bytes per cell + 16 bytes per coarse cell (~4.3 B per cell in 3D, ~2.7 in 2D), kept between
                                 steps; the PCG vectors (~26 B per cell) share the scratch tail with the advection and the CNN,
                                 whose needs are larger, so they add nothing there */
  /* Optional stages of lib/simulate.py (all off when zero; fnx_slab_step refuses them): */
  float viscosity;            /* mconf['viscosity'] > 0: the velocity advected is addViscosity(U.clone()), advected by U
                                 (simulate.py:66-69, :85-93).  2D only in this step: fnx_add_viscosity takes 3D grids since
                                 ABI 29, fnx_simulate_step still refuses a 3D grid with it (callers compose the 3D viscous step
                                 from the operators) */
  float gravity_scale;        /* mconf['gravityScale'] > 0: addGravity(gravityVec * -gravityScale) after the buoyancy, only with
                                 a density (simulate.py:107-114) */
  int   correct_scalar;       /* mconf['correctScalar']: density += dt/2 * density * div(U) on fluid cells after its
                                 advection (simulate.py:79-81, cpp/advection.py:9-12) */
  int   periodic;             /* bit 0: mconf has BOTH 'periodic-x' and 'periodic-y'; bit 1 / bit 2: their values.  Method 0
                                 only (simulate.py:121-128, :157-164): U[:,1,:,:,1] = U_temp[:,1,:,:,W-1],
                                 U[:,0,:,1] = U_temp[:,0,:,H-1] after each setWallBcs, U_temp the field before it */
  /* ABI 20, method 2 (mconf['pcgTol'], mconf['pcgIter']): */
  float pcg_tol;              /* (methods 2, 3, 4) relative residual ||b - A p|| / ||b|| to stop at; <= 0 runs exactly pcg_iter iterations, no host sync */
  int   pcg_iter;             /* at most that many CG iterations (>= 1) */
  /* ABI 22 (mconf['vorticityConfinementAmp']; off when <= 0; single domain only, fnx_slab_step refuses it): */
  float vorticity_confinement; /* fnx_add_vorticity_confinement with this amplitude after addGravity and before setWallBcs, for
                                 every method.  With it off the step launches what it launched before ABI 22. */
} FnxStepParams;

typedef struct FnxState {
  float* p;        /* (B,1,D,H,W) in/out */
  float* U;        /* (B,2|3,D,H,W) in/out */
  float* density;  /* (B,1,D,H,W) in/out, may be NULL (simulate.py:71-83: no 'density' key) */
  const float* flags;
  const float* UBC; const float* UBCInvMask;                 /* may be NULL */
  const float* densityBC; const float* densityBCInvMask;     /* may be NULL */
  const void*  net;  /* packed ScaleNet weights from fnx_scalenet_pack (methods 1 and 3), else NULL.  ABI 35, fnx_simulate_step_net: the
                        image of its net_kind -- fnx_banknet_pack's for FNX_NET_BANK */
  /* Optional (B,1,D,H,W) bytes from fnx_bc_classify, or NULL: bit 0 = setConstVals is x*1+0 for every velocity component
   * of the cell, bit 1 = the same for the density.  The BC stages then skip the 8 BC loads of such a cell (32 of its 64-68
   * bytes) and apply t = x*1, t + 0 directly: same bits.  Only valid while the four BC arrays do not change. */
  const unsigned char* bc_class;
  /* Optional (B,1,1,H,W) copy of flags with the no-slip cells set to 128 ('flags_stick' in batch_dict, cylinder.py:76), or
   * NULL.  Method 1 (convnet), 2D only in the step (fnx_set_wall_bcs_stick itself takes 3D grids since ABI 29): setWallBcsStick
   * before the second setConstVals and after the net (simulate.py:129-130, :165-166).  Method 0 ignores it, as the reference does. */
  const float* flags_stick;
  /* Optional promise to fnx_post_projection (0 = none): `density` already went through setConstVals with these BC arrays
   * since it was last written -- fnx_pre_projection leaves it that way.  On a cell of bc_class whose density BC is the
   * identity (x*1 + 0) a further setConstVals then changes no bit (the first one has already turned a -0 into +0), and the
   * pass neither reads nor writes the density there (8 of the ~41 bytes a cell of that pass moves).  Ignored without bc_class. */
  int density_bc_applied;
} FnxState;

/* Classifies every cell for FnxState.bc_class (reads the four BC arrays once; st->bc_class itself is ignored). */
int fnx_bc_classify(const FnxGrid* g, const FnxState* st, unsigned char* bc_class, void* stream);

int fnx_simulate_step(const FnxGrid* g, const FnxStepParams* prm, const FnxState* st,
                      void* ws, size_t ws_bytes, void* stream);

/* ABI 35: the step with the net of methods 1 and 3 named.  st->net is the image of that kind: fnx_scalenet_pack's (FNX_NET_SCALENET) or
 * fnx_banknet_pack's (FNX_NET_BANK: the 'FluidNet' bank model, 2D).  fnx_simulate_step(...) is
 * fnx_simulate_step_net(..., FNX_NET_SCALENET, ...); methods 0, 2 and 4 ignore net_kind as they ignore st->net.  With FNX_NET_BANK the
 * launches around the net are the ScaleNet step's (the per-sample scale, the fused input pass, the fused pass behind the net; with
 * flags_stick the unfused ones; method 3: the un-normalised pressure into st->p), only the net in the middle is fnx_banknet_forward's,
 * and the results are bit for bit those of the operators composed by hand around fnx_fluidnet_bank_forward.  The net's workspace (20 B a
 * cell, plus 12 B for its input and output) is carved from the step's scratch tail, which is sized for the ScaleNet's ~1 KB a cell:
 * fnx_workspace_bytes(FNX_OP_STEP) and FNX_OP_STEP_STATIC are what they were, and a grid whose tail were too small is FNX_EWORKSPACE.
 * Refused before the first launch, each text starting with "fnx_simulate_step_net:" (methods 1 and 3): an unknown net_kind; FNX_NET_BANK
 * on a 3D grid ("2D only"); H or W that is no positive multiple of 4; the bf16 modes ("fp32 arithmetic only"); a compute window or
 * z-slab view with FNX_NET_BANK; and FNX_NET_BANK3D, the kind of fnx_banknet3d_pack's image, which the step does not take yet ("not
 * built into the step": the Conv3d bank net runs through fnx_fluidnet_bank3d_forward, around the operators).  fnx_slab_step takes the
 * ScaleNet image only. */
enum { FNX_NET_SCALENET = 0, FNX_NET_BANK = 1, FNX_NET_BANK3D = 2 };
int fnx_simulate_step_net(const FnxGrid* g, const FnxStepParams* prm, const FnxState* st, int net_kind,
                          void* ws, size_t ws_bytes, void* stream);

/* The two fused stages of fnx_simulate_step, exposed for drivers that interleave their own work (halo exchange):
 *   pre : simulate.py:96-133 + :144  U_adv, rho_adv (advection outputs) -> st->U, st->density, div
 *         (setConstVals, addBuoyancy, addGravity [prm->gravity_scale > 0], setWallBcs + periodic patches [method 0 only],
 *         setConstVals [not with st->flags_stick in method 1: the caller runs setWallBcsStick first], velocityDivergence
 *         [div != NULL])
 *   post: simulate.py:154-168        velocityUpdate(st->p), setWallBcs, setConstVals, in place on st->U / st->density (no
 *         periodic patches: fnx_simulate_step wraps it with them)
 * With prm->vorticity_confinement > 0 the pre stage is cut in two around the confinement (stages up to addGravity -> st->U,
 * confinement st->U -> U_adv, the remaining stages U_adv -> st->U): U_adv is then OVERWRITTEN (it is scratch of the caller's
 * in every use the library makes of it), the density's second setConstVals is a pass of its own, and the grid must be whole (no
 * compute window, no z-slab view). */
int fnx_pre_projection(const FnxGrid* g, const FnxStepParams* prm, const FnxState* st, const float* U_adv,
                       const float* rho_adv, float* div, void* stream);
int fnx_post_projection(const FnxGrid* g, const FnxState* st, void* stream);

/* Adjoints of the linear stencil operators the training graph differentiates through (lib/model.py:190-227 and
 * fluid_net_train.py:366: velocityUpdate -> setWallBcs -> velocityDivergence; the reference gets them from autograd over
 * its ATen chains).  grad_* are (B,C,D,H,W) like the quantities they belong to; outputs are overwritten.
 *   velocityDivergence: grad_U = J^T grad_div
 *   velocityUpdate:     grad_U, grad_p from grad_U_out (the gradient w.r.t. the updated velocity); grad_U must not alias it
 *   setWallBcs:         zeroes a flag-dependent set of entries, so its adjoint is fnx_set_wall_bcs applied to the gradient */
int fnx_velocity_divergence_backward(const FnxGrid* g, const float* grad_div, const float* flags, float* grad_U, void* stream);
int fnx_velocity_update_backward(const FnxGrid* g, const float* grad_U_out, const float* flags, float* grad_U, float* grad_p,
                                 void* stream);

/* ---- z-slab decomposition of the 3D Jacobi step over the GPUs of one node (the reference is single
 * device, plume.py:131-135).  Rank r owns D_global / nranks planes and keeps `halo` ghost planes towards each
 * z-neighbour; its arrays hold local planes [0, owned + ghosts) = global planes [z_offset, ...).  One fnx_slab_step is
 * lib/simulate.py:28-171 (method 'jacobi', pTol 0) for the rank's owned planes, bit for bit what the single-domain
 * fnx_simulate_step computes there; ghost planes travel through an FnxSlabComm (neighbour exchange only, no collective on
 * the data path).  The driver enqueues on `stream` and on one internal communication stream joined back with events
 * (the whole step is capturable in a HIP graph); nothing synchronises except the optional CFL check. ---- */
typedef struct FnxSlabSeg {           /* one contiguous block of ghost planes of one field and channel */
  const void* send_lo; void* recv_lo;  /* to / from rank - 1 (NULL on rank 0) */
  const void* send_hi; void* recv_hi;  /* to / from rank + 1 (NULL on the last rank) */
  size_t bytes;
} FnxSlabSeg;
typedef struct FnxSlabComm {
  void* ctx;
  /* Stream-ordered exchange of all segments with both neighbours (RCCL: one ncclGroupStart/Send/Recv/GroupEnd). */
  int (*exchange)(void* ctx, const FnxSlabSeg* segs, int nsegs, void* stream);
  /* In-place max / sum over all ranks of n DEVICE floats (CFL guard, pTol residual; control path only). */
  int (*allreduce_max)(void* ctx, float* x, int n, void* stream);
  int (*allreduce_sum)(void* ctx, float* x, int n, void* stream);
  void (*destroy)(void* ctx);
  /* Optional (may be NULL): called by fnx_slab_step on the rank whose step FAILED, so that its neighbours -- which may already
   * be waiting for it inside exchange() -- return FNX_ECOMM instead of hanging (RCCL: ncclCommAbort; loopback: a group flag). */
  void (*abort)(void* ctx);
  /* Optional pair (both NULL or both set): DIRECT sends.  direct_begin(ctx, bytes, nsegs, dst, select, seg_stride, start_clock, stream)
   * names where the producing kernel may store the NEXT exchange's outgoing planes itself: towards rank - 1 (d = 0) / rank + 1 (d = 1;
   * NULL at the ends of the chain) into dst[d][q], q = (*select[d] + 1) & 1 read on the device (FnxPlaneMirror.slot_select; select[d]
   * NULL: q = 0), segment i of `bytes` bytes at + i * *seg_stride bytes; FNX_EINVAL when that exchange does not fit (the driver then
   * sends it the ordinary way).  direct_exchange(ctx, segs, nsegs, stream), enqueued behind the producing kernel, is exchange() for
   * segments whose send sides are already in place: it publishes them and receives.  *start_clock (may come back NULL): a device word
   * the producing kernel is asked to store its start time in (FnxPlaneMirror.start_clock).  The peer-store communicator hands out its
   * neighbours' mailbox slots (two per side, told apart by its device-side chunk counter: nothing in a captured step depends on how
   * many exchanges came before); the link model buffers of its own, and times the transfer from that clock. */
  int (*direct_begin)(void* ctx, size_t bytes, int nsegs, void* dst[2][2], const unsigned* select[2], size_t* seg_stride,
                      void** start_clock, void* stream);
  int (*direct_exchange)(void* ctx, const FnxSlabSeg* segs, int nsegs, void* stream);
} FnxSlabComm;
/* Ordering contract of a communicator: fnx_slab_step issues exchange() on its internal communication stream (the sweep blocks of
 * FNX_SLAB_DEEP_BESIDE: on its internal edge stream -- a communicator must take the stream it is given) and the
 * control-path all-reduces (CFL guard, pTol residual) on the caller's stream; every rank issues the same calls in the same
 * order (the step is deterministic).  An all-reduce is only issued when no exchange is pending (the caller's stream has
 * been made to wait for the last one) and is followed by a host synchronisation before the next exchange is posted, so the
 * two streams never have work of one communicator in flight at the same time. */
/* RCCL communicator (librccl is loaded on first use; no link-time dependency).  unique_id: the 128 bytes of
 * fnx_slab_rccl_unique_id() from rank 0, distributed by the caller (MPI, torch.distributed, a file ...). */
int fnx_slab_rccl_unique_id(void* out128);
int fnx_slab_comm_rccl(FnxSlabComm* out, int rank, int nranks, const void* unique_id128);
/* In-process communicator for `nranks` slabs driven by `nranks` host threads of one process (one device, or several
 * with peer access: each side of a pair records only its own event on its own stream): device-to-device copies ordered by
 * events.  A rank whose peer does not arrive within the group's timeout (120 s unless set) returns FNX_ECOMM from that call
 * and the group stays usable for DIRECT users of the communicator (a slow peer is not a dead one; an all-reduce round in which a
 * rank timed out is abandoned as a whole -- every rank of it fails, a retry starts a fresh round).  fnx_slab_step cannot resume a
 * step half-way: it calls abort() on ANY failure, a timeout included, so through the driver a timeout poisons the group like any
 * other error.  A rank whose group was aborted (FnxSlabComm.abort: some rank's step failed) returns FNX_ECOMM until
 * fnx_slab_loopback_group_reset, which the caller may issue once no rank is inside a call of the group.  Create the group
 * once, then one comm per rank. */
int fnx_slab_loopback_group(void** group, int nranks);
int fnx_slab_loopback_group_set_timeout(void* group, double seconds);
int fnx_slab_loopback_group_reset(void* group);
int fnx_slab_comm_loopback(FnxSlabComm* out, void* group, int rank);
void fnx_slab_loopback_group_free(void* group);
/* Link-model communicator (a rehearsal aid, not a transport): lets ONE process run the step of a middle rank (rank r of n with
 * 0 < r < n - 1) on one GPU.  An exchange is one launch that fills the ghost planes from the slab's own edge planes and occupies its
 * stream for latency_us + bytes per direction / gbytes_per_s (0 GB/s: no transfer time beyond the copy), so launch sequence, message
 * sizes and stream ordering are those of a real run and the time a schedule leaves exposed for an assumed link can be measured; the
 * field values are those of a periodic stack of this slab.  All-reduces return the rank's own value.  latency_us is the transport's:
 * ~20 us for a grouped RCCL send/recv, ~9 us for the peer-store launch (tools/peer_probe.py). */
int fnx_slab_comm_link_model(FnxSlabComm* out, double latency_us, double gbytes_per_s);
/* Peer-store communicator (no RCCL on the data path; the reference is single device, plume.py:131-135: no counterpart).  Every rank
 * owns a REGION of uncached device memory -- flag words and a mailbox of 2 x 2 slots of `mailbox_bytes` -- that its two z-neighbours
 * map (hipIpcOpenMemHandle between processes; ranks driven by threads of one process use the address as it is).  An exchange is ONE
 * short launch on the stream it is given: its first workgroups store this rank's planes straight into the neighbours' mailboxes over
 * xGMI and raise a flag there, its last workgroups wait -- on the device -- for the neighbours' flags and move the planes that arrived
 * into place; exchanges larger than a slot are cut into chunks (two may be in flight per direction).  No proxy thread, no host
 * synchronisation, 64 workgroups of the device while it runs.  The all-reduces of the control path (CFL guard, pTol residual, the CNN
 * projection's sums) travel along the chain of ranks through the same regions, driven by the host, added in RANK ORDER: the same bits on
 * every rank.  A wait that outlasts the timeout (30 s unless set) or sees an abort gives up and the communicator's next call
 * returns FNX_ECOMM.
 *   1. every rank: fnx_slab_peer_create -> its handle (FNX_PEER_HANDLE_BYTES bytes), to be carried to both neighbours by the caller
 *      (MPI, torch.distributed, a file ... like the RCCL unique id)
 *   2. every rank: fnx_slab_comm_peer with the handles of rank - 1 and rank + 1 (NULL at the ends of the chain)
 * The peer object must outlive the communicator (fnx_slab_comm_free, then fnx_slab_peer_free); all ranks use the same mailbox_bytes. */
#define FNX_PEER_HANDLE_BYTES 128
int fnx_slab_peer_create(void** peer, int rank, int nranks, size_t mailbox_bytes, void* handle_out);
int fnx_slab_peer_set_timeout(void* peer, double seconds);
/* FNX_ECOMM once a device-side wait of this rank's exchanges has timed out or the group was aborted (ABI 19).  The exchanges are
 * enqueued, not waited for, so a step or a replayed graph that met a dead neighbour still returns FNX_OK: ask after synchronising the
 * stream, before trusting the step's ghost planes.  (Every later communicator call fails with FNX_ECOMM by itself.) */
int fnx_slab_peer_failed(void* peer);
int fnx_slab_comm_peer(FnxSlabComm* out, void* peer, const void* handle_lo, const void* handle_hi);
void fnx_slab_peer_free(void* peer);
void fnx_slab_comm_free(FnxSlabComm* comm);

#define FNX_SLAB_MAX_HALO 64
/* How a block of sweeps_per_exchange Jacobi sweeps is ordered around its ghost exchange (all three give the same bits):
 *   DEEP_FIRST  every pass is cut a few planes inside each internal face; the deep parts of all passes run first -- they read
 *               no ghost plane, so the previous block's exchange (first block: the exchange of div) is still in flight --,
 *               then the edge parts (short launches), whose last one produces the planes the neighbours need next
 *   EDGE_FIRST  the edge parts of all passes first (shrinking plane ranges), their exchange posted, the interior parts behind it
 *   LAST_PASS   whole passes; only the last pass of a block is split into edge and interior
 *   DEEP_BESIDE the parts of DEEP_FIRST, the edge chain of a block on a second stream BESIDE its deep chain (edge part k waits
 *               for deep part k-1 only).  The exchanges of the sweep blocks are enqueued on that stream itself -- exchange(ctx, ...,
 *               stream) is called with the edge stream, behind the block's edge chain and ahead of the next block's -- so the chain
 *               exchange -> edge chain -> exchange crosses no stream; a block takes max(deep chain, exchange + edge chain) instead
 *               of their sum.  Pays with links of >= 150 GB/s per direction; a tie with DEEP_FIRST at 75 GB/s
 * Slabs thinner than 4 sweep blocks, solves of at most one block and pTol > 0 always run LAST_PASS. */
enum { FNX_SLAB_DEEP_FIRST = 0, FNX_SLAB_EDGE_FIRST = 1, FNX_SLAB_LAST_PASS = 2, FNX_SLAB_DEEP_BESIDE = 3 };
typedef struct FnxSlabConfig {
  int B, H, W, D_global;    /* the whole domain */
  int rank, nranks;         /* D_global % nranks == 0 */
  int halo;                 /* ghost planes per internal face (5 .. FNX_SLAB_MAX_HALO; the pressure solve uses all of them) */
  int sweeps_per_exchange;  /* Jacobi sweeps per ghost exchange of p (temporal blocking in z), clipped to halo */
  int static_flags;         /* 1: flags and BC arrays never change between steps (solver mask and BC class map are kept) */
  int cfl_check_every;      /* every that many steps the step begins with max |U| dt over all ranks (one host sync);
                               > 1 cell returns FNX_ECFL on every rank.  0 = never */
  int schedule;             /* FNX_SLAB_DEEP_FIRST (0, the default) / FNX_SLAB_EDGE_FIRST / FNX_SLAB_LAST_PASS / FNX_SLAB_DEEP_BESIDE */
  int method;               /* 0: Jacobi projection; 1: the driver is also sized for the CNN projection (prm->method 1 in
                               fnx_slab_step): needs halo >= FNX_SLAB_NET_MARGIN + 1, halo % 4 == 0, D_global / nranks % 4 == 0
                               when nranks > 1, and a workspace that holds the net's activations for owned + 2 x 48 planes (sized for the
                               untrimmed window; the towers run on nested crops of it, see FNX_SLAB_NET_MARGIN_FULL) */
  int direct_sends;         /* where the communicator offers direct sends (FnxSlabComm.direct_begin), the last edge part of a sweep block
                               can store the planes the neighbours need next straight into their windows (fnx_jacobi_pass_mirror) and the
                               exchange is then posted as direct_exchange.  0 (default): in DEEP_BESIDE, whose cycle exchange -> edge chain
                               the transport's launch and that part's run time then leave (middle rank modelled at 75 GB/s: 74 -> 78 % of a
                               ghost-free slab); not in DEEP_FIRST, which hides the exchange behind the deep chain anyway and only pays the
                               mirrored stores.  1: never.  2: in both.  Same bits in every case */
} FnxSlabConfig;
/* ghost planes of the MultiScaleNet's input a rank evaluates beyond its owned planes: the net's receptive field (< 48 cells at
 * full resolution), a multiple of 4 so that the rank's quarter- and half-resolution grids coincide with the global ones */
#define FNX_SLAB_NET_MARGIN 48
/* ... of which the towers need less: the full-resolution tower's receptive radius is 8 planes (5^3, four 3^3, 5^3), the
 * half-resolution tower's 14 (+ 2 for the resampling above it, + the 8), the quarter-resolution tower's 16 (+ 4, + the 24 = 44).  A
 * rank therefore runs each tower only on owned +- its own margin (nested crops, fnx_multiscale_forward_crop): 1.3 x the FLOPs of
 * its owned planes at 64 planes per rank instead of 2.5 x.  The pressure is then exact on the owned planes; the one plane below them
 * that velocityUpdate reads comes from the neighbour (a one-plane exchange of p). */
#define FNX_SLAB_NET_MARGIN_FULL 8
#define FNX_SLAB_NET_MARGIN_HALF 24
typedef struct FnxSlab FnxSlab;
/* Local geometry of a rank (what to allocate): planes it owns, ghosts below / above, global plane of local plane 0. */
int fnx_slab_layout(const FnxSlabConfig* cfg, int* owned, int* ghost_lo, int* ghost_hi, int* z_offset);
size_t fnx_slab_workspace_bytes(const FnxSlabConfig* cfg);
/* comm is borrowed (must outlive the slab).  nranks == 1 needs no communicator (comm may be NULL). */
int fnx_slab_create(FnxSlab** out, const FnxSlabConfig* cfg, const FnxSlabComm* comm);
void fnx_slab_destroy(FnxSlab* s);
/* One time step.  st: the rank's local arrays (with ghost planes), st->density required.  prm->method 0: the Jacobi projection
 * (st->net unused).  prm->method 1 (cfg.method 1, st->net = the packed weights): the CNN projection, lib/model.py:118-227 on
 * z-slabs -- _ScaleNet's std over the whole domain from per-rank fp64 (sum, sumsq) gathered and added in RANK ORDER (the same
 * bits on every rank; one host synchronisation), FNX_SLAB_NET_MARGIN + 1 ghost planes of U exchanged once, the net evaluated on
 * owned +- FNX_SLAB_NET_MARGIN planes, velocityUpdate / un-normalise / setWallBcs / setConstVals on the owned planes: p and U
 * within the CNN tolerance (1e-5 |ref|max) of the single-domain step, density bit for bit.
 * prm->method 2, 3, 4 (PCG, cold or warm-started) are refused with FNX_EINVAL: its dot products would need an all-reduce per iteration
 * (single domain only).
 * Jacobi:  prm->p_tol > 0 runs the reference's convergence test (fluids_init.cpp:961-979): one sweep per ghost exchange,
 * the squared differences over the owned planes all-reduced over the ranks, one host sync per sweep (as in fnx_jacobi);
 * every rank's part reproducible (fnx_residual).  The bit-for-bit statement above holds for p_tol == 0; with p_tol > 0 every
 * sweep still has the single-domain bits, but the residual is summed per rank and then over the ranks (fp32 all-reduce), so a
 * tolerance within rounding (~1e-7 relative) of a sweep's residual can stop one sweep earlier or later than fnx_jacobi does.
 * prm->static_flags is ignored (FnxSlabConfig.static_flags).  ws: fnx_slab_workspace_bytes, kept between steps.
 * On failure (other than FNX_ECFL, which every rank reports together) the communicator's abort() is called -- also when the
 * failure is a peer timeout of the loopback communicator -- and the caller's stream is made to wait for whatever the failed step
 * had already forked onto the driver's internal streams. */
int fnx_slab_step(FnxSlab* s, const FnxStepParams* prm, const FnxState* st, void* ws, size_t ws_bytes, void* stream);

/* Communication statistics of a rank (off by default: the event pairs they need cannot be recorded inside a graph capture).
 * enable(1) clears them; read() synchronises the recorded events, adds them up and clears the event list. */
typedef struct FnxSlabStats {
  double bytes_per_neighbour;  /* bytes posted towards EACH neighbour (and received from it) since enable() */
  double wait_ms;              /* time the compute stream stood in front of posted exchanges (HIP events around each wait) */
  long long exchanges;         /* ghost exchanges posted */
} FnxSlabStats;
int fnx_slab_stats_enable(FnxSlab* s, int on);
int fnx_slab_stats_read(FnxSlab* s, FnxSlabStats* out);
/* One-off probe of a communicator: `reps` exchanges of `bytes` bytes with each neighbour, back to back on `stream`, after
 * one untimed exchange; *ms_per_exchange = average duration (HIP events; synchronises).  scratch: 4 * bytes of device
 * memory.  Every rank of the communicator must call it with the same arguments. */
int fnx_slab_comm_probe(const FnxSlabComm* comm, void* scratch, size_t bytes, int reps, float* ms_per_exchange, void* stream);

/* MultiScaleNet / FluidNet.forward, lib/multi_scale_net.py:118-127 and lib/model.py:76-227 (ScaleNet variant).
 * weights_blob: 17 convs in the order convN_4[0..3], convN_2[0..5], convN_1[0..5], final; for each conv the
 * torch-layout weight (Cout,Cin,[kd,]kh,kw) then bias (Cout); fp32, DEVICE pointer.
 * fnx_scalenet_pack repacks it for the MFMA kernels into `packed` (size fnx_scalenet_packed_bytes). */
size_t fnx_scalenet_weight_floats(int is3D);
size_t fnx_scalenet_packed_bytes(int is3D);
int fnx_scalenet_pack(int is3D, const float* weights_blob, void* packed, void* stream);
/* precision_mode of the CNN entry points (and FnxStepParams.precision_mode).  The first two are exact-fp32 arithmetic on
 * v_mfma_f32_*_f32; the last two are opt-in and carry their own labels in every report (bench.py never puts them in the headline):
 *   FNX_PRECISION_FP32         the default: 3x3(x3) layers of launches that fill the chip run in the Winograd domain -- F(2x2,3x3)
 *                              (2.25x fewer multiplies) and, since round 6, F(4x4,3x3) in (y, x) (4x fewer) for the 64- and
 *                              128-output-channel layers; not the summation order of a direct convolution; within 1e-5 |ref|max of the
 *                              torch reference (tests/test_parity_gpu.py)
 *   FNX_PRECISION_FP32_DIRECT  every convolution as a direct sum over its taps (implicit GEMM), no Winograd
 *   FNX_PRECISION_BF16X6       FNX_PRECISION_FP32 with the Winograd-domain GEMMs of the 64- and 128-output-channel 3x3(x3) layers on
 *                              the bf16 matrix cores: every fp32 operand cut EXACTLY into three bf16 pieces (8 + 8 + 8 significand
 *                              bits), a product evaluated as six bf16 x bf16 MFMAs with fp32 accumulation (the three dropped
 *                              cross terms are below 2^-23 of the product: the size of one fp32 rounding).  Same tolerance as the
 *                              other modes in the tests (1e-5 |ref|max against oracle and goldens); every other layer as in
 *                              FNX_PRECISION_FP32
 *   FNX_PRECISION_BF16X3       FNX_PRECISION_BF16X6 with only the three products that involve no low piece (ah*bh + ah*bm + am*bh): half
 *                              the bf16 MFMAs and two thirds of the operand traffic; what is dropped is below 2^-15 of a product.  Its own
 *                              label and its own tolerance: 1e-4 |ref|max against oracle and goldens in the tests (measured 2-3e-5 on
 *                              the bias-dominated benchmark weights, 8-9.2e-5 on weights whose every layer reaches the output:
 *                              tests/test_cnn_fp64_gpu.py).  SURVEY.md section 7's "accurate bf16" mode; the reference's own convolutions run on
 *                              torch.nn.Conv2d, whose CUDA default admits TF32 (lib/multi_scale_net.py:21-127)
 *   FNX_PRECISION_FP32_F4      (round 6) the 64- and 128-output-channel 3x3(x3) layers in the Winograd F(4x4,3x3) domain (conv3_wino4_kernel: 36
 *                              multiplies per 16 outputs instead of F(2x2)'s 64; 3D: in (y, x), the z taps as stages): exact-fp32 MFMAs,
 *                              the transforms round more (multipliers 4, 5, 8, 1/6, 1/24) -- measured 2-3x F(2x2)'s error: up to 4.8e-6
 *                              |ref|max (3D) against a float64 model when every layer reaches the output (tests/test_cnn_fp64_gpu.py),
 *                              within the tests' 1e-5.  What FNX_PRECISION_FP32 runs since round 6 (256^3 CNN step 92.2 -> 81.0 ms,
 *                              1024^2 2.29 -> 2.14 ms)
 *   FNX_PRECISION_FP32_F2      F(2x2,3x3) for every Winograd layer: the default of rounds 2-5 (kept for A/B timing) */
enum { FNX_PRECISION_FP32 = 0, FNX_PRECISION_FP32_DIRECT = 1, FNX_PRECISION_BF16X6 = 2, FNX_PRECISION_BF16X3 = 3, FNX_PRECISION_FP32_F4 = 4,
       FNX_PRECISION_FP32_F2 = 5 };
/* x: (B,2,D,H,W) [div/s, occupancy] -> p (B,1,D,H,W) */
int fnx_multiscale_forward(const FnxGrid* g, const void* packed, const float* x, float* p, int precision_mode,
                           void* ws, size_t ws_bytes, void* stream);
/* The same pass on NESTED z-crops (what the z-slab driver's CNN projection runs on a rank's window, fnx_slab_step): x covers D
 * planes; the quarter-resolution tower runs on all of them, the half-resolution tower on planes [trim[2], D - trim[3]) and the
 * full-resolution tower on [trim[0], D - trim[1]) -- full-resolution plane counts, multiples of 4 (D too), trim[2] <= trim[0],
 * trim[3] <= trim[1].  p: (B,1,D - trim[0] - trim[1],H,W), the planes [trim[0], D - trim[1]).  Where a window ends at an artificial
 * face the tower's output is only meaningful beyond its receptive radius from that face (8 / 14 / 16 full-resolution planes for the
 * full / half / quarter tower, + 2 / 4 for the resampling between them): the caller sizes the windows (FNX_SLAB_NET_MARGIN and
 * FNX_SLAB_NET_MARGIN_FULL / _HALF above).  trim = {0,0,0,0} is fnx_multiscale_forward.  Workspace: as fnx_multiscale_forward for D planes. */
int fnx_multiscale_forward_crop(const FnxGrid* g, const void* packed, const float* x, float* p, int precision_mode,
                                const int trim[4], void* ws, size_t ws_bytes, void* stream);
/* input: (B,5|6,D,H,W) = [p, U, flags, density] -> p_out (B,1,..), U_out (B,2|3,..) */
int fnx_fluidnet_forward(const FnxGrid* g, const void* packed, const float* input, float normalize_threshold,
                         float* p_out, float* U_out, int precision_mode, void* ws, size_t ws_bytes, void* stream);

/* The reference's 16-channel "bank" net (ABI 30): lib/model.py:177-209, what mconf['model'] = 'FluidNet' selects -- 2D; its training entry points
 * (ABI 31) follow those of the 2D ScaleNet below.
 *   a = relu(conv1(x)); t = (bank(a) + up2(bank(avgpool2(a)))) + up4(bank(avgpool4(a))); bank = relu(block.2(relu(block.0(.)))), one set
 *   of weights for the three levels, zero padding at each level's own border, nearest upsampling;
 *   p = convOut(relu(conv3(relu(conv2(relu(conv2(t)))))))                       (conv2 is applied twice, model.py:204-205)
 * weights_blob: fnx_banknet_weight_floats() = 5361 floats, DEVICE pointer: conv1, convBank.block.0, convBank.block.2, conv2, conv3,
 * convOut, for each the torch-layout weight (Cout,Cin,kh,kw) then bias.  fnx_banknet_pack repacks it into `packed`
 * (fnx_banknet_packed_bytes()) in the operand order of v_mfma_f32_16x16x4_f32.
 * Every entry point refuses, before it touches the device and each with its own fnx_last_error text: null arguments; a 3D grid (the
 * reference asserts 2D); an unknown precision mode; the bf16 modes (every fp32 mode runs the one exact-fp32 kernel family); H or W that
 * is no multiple of 4 (the reference's sum of the three levels raises there); a short workspace (FNX_EWORKSPACE).
 * Three launches, no atomics, no host synchronisation (capturable); a sample's result does not depend on the rest of the batch.
 * Workspace: fnx_banknet_ws_bytes(g, 0) for the net alone -- the two coarser banks' results, 20 bytes per full-resolution cell --
 * and fnx_banknet_ws_bytes(g, 1) for the whole forward (0 for a grid without a workspace size). */
size_t fnx_banknet_weight_floats(void);
size_t fnx_banknet_packed_bytes(void);
int fnx_banknet_pack(const float* weights_blob, void* packed, void* stream);
size_t fnx_banknet_ws_bytes(const FnxGrid* g, int whole_forward);
/* x: (B,2,H,W) [div/s, occupancy] -> p (B,1,H,W) */
int fnx_banknet_forward(const FnxGrid* g, const void* packed, const float* x, float* p, int precision_mode, void* ws, size_t ws_bytes,
                        void* stream);
/* fnx_fluidnet_forward's contract with the bank net in the middle: input (B,5,1,H,W) = [p, U, flags, density] -> p_out (B,1,1,H,W),
 * U_out (B,2,1,H,W); the launches around the net are fnx_fluidnet_forward's.  fnx_simulate_step and fnx_slab_step take the ScaleNet
 * image only; fnx_simulate_step_net (ABI 35) takes this net's as FNX_NET_BANK. */
int fnx_fluidnet_bank_forward(const FnxGrid* g, const void* packed, const float* input, float normalize_threshold, float* p_out,
                              float* U_out, int precision_mode, void* ws, size_t ws_bytes, void* stream);

/* The Conv3d counterpart of the bank net (ABI 32): mconf['model'] = 'FluidNet3D', this project's own definition (the reference's net is 2D
 * only) -- every module of the net above replaced by its 3D sibling: Conv3d 3x3x3 with zero padding 1 at each level's own border (z
 * included), avgpool3d by 2 and 4, nearest upsampling in z, y and x, the same order of additions, the 1x1x1 tail with conv2 applied twice.
 * weights_blob: fnx_banknet3d_weight_floats() = 15153 floats, DEVICE pointer, the six layers in the order above, for each the torch-layout
 * weight (Cout,Cin,kd,kh,kw) then bias.  fnx_banknet3d_pack repacks it into `packed` (fnx_banknet3d_packed_bytes()).
 * Every entry point refuses, before it touches the device and each with its own fnx_last_error text that starts with the function's
 * name: null arguments; a grid that is not 3D (is3D == 0 or D < 4: "3D only"); an unknown precision mode; the bf16 modes ("fp32 arithmetic
 * only"; every fp32 mode runs the one exact-fp32 kernel family); D, H or W that is no positive multiple of 4 (the axis and its value are
 * named); a short workspace (FNX_EWORKSPACE).  'FluidNet' with a 3D grid stays refused by the 2D entry points above.
 * Six launches (conv1 with both poolings; block.0 and block.2 on the quarter and the half level; block.0 at full resolution; block.2 at
 * full resolution with the sum of the levels and the tail), no atomics, no host synchronisation (capturable); a sample's result depends
 * neither on the rest of the batch nor on how the launch plan splits z.
 * Workspace: fnx_banknet3d_ws_bytes(g, 0) for the net alone -- relu(conv1) and block.0's output at full resolution and three 16-channel
 * tensors at each coarser level, 64 + 64 + 3 * 8 + 3 * 1 = 155 bytes per full-resolution cell -- and fnx_banknet3d_ws_bytes(g, 1) for
 * the whole forward (0 for a grid without a workspace size).
 * fnx_banknet3d_launch_plan: how the 16 -> 16 convolution kernel is launched at level 1, 2 or 4 of the grid, a function of (B, D, H, W)
 * alone: plan = {x tiles, y tiles, z chunks, planes per chunk, tile height, tile width}; tile (i, j) owns rows [i * height, ..) and
 * columns [j * width, ..), chunk c the planes [c * planes, min(d, (c + 1) * planes)) of the level. */
size_t fnx_banknet3d_weight_floats(void);
size_t fnx_banknet3d_packed_bytes(void);
int fnx_banknet3d_pack(const float* weights_blob, void* packed, void* stream);
size_t fnx_banknet3d_ws_bytes(const FnxGrid* g, int whole_forward);
int fnx_banknet3d_launch_plan(const FnxGrid* g, int level, int plan[6]);
/* x: (B,2,D,H,W) [div/s, occupancy] -> p (B,1,D,H,W) */
int fnx_banknet3d_forward(const FnxGrid* g, const void* packed, const float* x, float* p, int precision_mode, void* ws, size_t ws_bytes,
                          void* stream);
/* fnx_fluidnet_forward's contract with this net in the middle: input (B,6,D,H,W) = [p, U, flags, density] -> p_out (B,1,D,H,W),
 * U_out (B,3,D,H,W); the launches around the net are fnx_fluidnet_bank_forward's on three velocity components.  fnx_simulate_step
 * and fnx_slab_step take the ScaleNet image only, and fnx_simulate_step_net (ABI 35) refuses this net's kind, FNX_NET_BANK3D. */
int fnx_fluidnet_bank3d_forward(const FnxGrid* g, const void* packed, const float* input, float normalize_threshold, float* p_out,
                                float* U_out, int precision_mode, void* ws, size_t ws_bytes, void* stream);

/* Training of the 2D net (ABI 21): gradients of a scalar loss of p (or of FluidNet.forward's (p, U)) with respect to the 34 parameter
 * tensors, fp32 arithmetic only.  Every entry point checks, before it touches the device: a 2D grid (is3D = 0, D = 1) and a precision mode
 * among FNX_PRECISION_FP32, _FP32_F4, _FP32_F2 and _FP32_DIRECT (the bf16 modes and 3D are FNX_EINVAL with their own fnx_last_error text).
 * No gradient with respect to the input, no dropout, no compute window.  No atomics: two calls on the same inputs give the same bits.
 *
 * The training forward writes every layer's input into one caller-provided buffer, the tape: the three concatenated tower inputs
 * ("xq" (B,2,H/4,W/4), "in2" (B,3,H/2,W/2), "in1" (B,3,H,W)) and the output "y<l>" of each of the first 16 convolutions AFTER its ReLU,
 * including the 8-channel "y15" that the inference forward's fused tail never writes -- about 420 floats per full-resolution pixel.
 * The derivative of a ReLU layer is (saved output > 0), torch's rule.  fnx_multiscale_tape_layout returns the tape's size in floats
 * (0 on error) and, if `entries` is not NULL, fills fnx_multiscale_tape_entries() of them in tape order; the layout is a function
 * of (B, H, W) alone.  p of the training forward is bit-identical to fnx_multiscale_forward's in the same mode. */
typedef struct FnxTapeEntry {
  char name[8];
  size_t offset;     /* floats from the start of the tape; the tensor is a contiguous (B,C,H,W) */
  int C, H, W;
} FnxTapeEntry;
int fnx_multiscale_tape_entries(void);
size_t fnx_multiscale_tape_layout(const FnxGrid* g, FnxTapeEntry* entries);
/* packed_t: what the backward reads of the weights -- the blob itself and, for the 3x3 layers between 32, 64 and 128 channels, the
 * images of the transposed, tap-flipped weight with zero bias (ten layers), so that their input gradients run through the forward's own launchers
 * by the same mode rule.  Repack it with fnx_scalenet_pack whenever the weights change; both run on the device. */
size_t fnx_scalenet_packed_t_bytes(void);
int fnx_scalenet_pack_t(const float* weights_blob, void* packed_t, void* stream);
size_t fnx_multiscale_backward_ws_bytes(const FnxGrid* g);
/* x (B,2,1,H,W) -> p (B,1,1,H,W) and the tape (fnx_multiscale_tape_layout floats).  No workspace. */
int fnx_multiscale_forward_train(const FnxGrid* g, const void* packed, const float* x, float* p, float* tape, int precision_mode,
                                 void* stream);
/* grad_p (B,1,1,H,W) and the tape of the forward -> grad_blob (fnx_scalenet_weight_floats(0) floats) in the layout of weights_blob:
 * per conv the weight gradient (Cout,Cin,kh,kw) then the bias gradient.  grad_p and the tape are not modified.  The weight gradients of the
 * 3x3 layers between 32, 64 and 128 channels (95 % of the FLOPs) run on the matrix cores in exact fp32 (v_mfma_f32_32x32x2_f32, a GEMM
 * over K = B H W split across workgroups, partials added in a fixed order).  precision_mode picks the launcher of the input-gradient
 * convolutions. */
int fnx_multiscale_backward(const FnxGrid* g, const void* packed_t, const float* grad_p, const float* tape, float* grad_blob,
                            int precision_mode, void* ws, size_t ws_bytes, void* stream);
/* The same call with the plain weight-gradient kernel of the thin layers for every layer: a cross-check of the MFMA kernel for tests and
 * A/B timing (7x slower), not something a training loop calls. */
int fnx_multiscale_backward_plain(const FnxGrid* g, const void* packed_t, const float* grad_p, const float* tape, float* grad_blob,
                                  int precision_mode, void* ws, size_t ws_bytes, void* stream);
/* FluidNet.forward for training and its backward (one workspace size for both).  The forward is fnx_fluidnet_forward with the taped
 * net; it also returns the flags channel as a contiguous (B,1,1,H,W) tensor and the per-sample scale s (B floats), which the backward
 * takes back.  Behind the net the forward is velocityUpdate(p, UDiv / s), p s, UDiv s, setWallBcs (model.py:213-226), so the
 * gradient that reaches the net's output is   g_net = s grad_p + velocity_update_backward_p(s setWallBcs(grad_U)). */
size_t fnx_fluidnet_train_ws_bytes(const FnxGrid* g);
int fnx_fluidnet_forward_train(const FnxGrid* g, const void* packed, const float* input, float normalize_threshold, float* p_out,
                               float* U_out, float* flags_out, float* scale_out, float* tape, int precision_mode, void* ws, size_t ws_bytes,
                               void* stream);
int fnx_fluidnet_backward(const FnxGrid* g, const void* packed_t, const float* flags, const float* scale, const float* grad_p,
                          const float* grad_U, const float* tape, float* grad_blob, int precision_mode, void* ws, size_t ws_bytes,
                          void* stream);

/* Training of the bank net in 2D (ABI 31): gradients of a scalar loss of p (or of FluidNet.forward's (p, U)) with respect to the twelve
 * parameter tensors of the 'FluidNet' model, exact fp32.  Every entry point refuses, before it touches the device and each with its own
 * fnx_last_error text, what the inference entry points of ABI 30 refuse: null arguments; a 3D grid and an unknown precision mode (the text
 * starts with the function's name); the bf16 modes; H or W that is no positive multiple of 4; a short workspace (FNX_EWORKSPACE).  No
 * gradient with respect to the input, no dropout.  No atomics and no host synchronisation (capturable): every cross-workgroup sum goes
 * through per-workgroup partial sums -- min(work items, 512) workgroups per launch, a function of (B, H, W) alone -- which one kernel adds
 * in index order in fp64, so two calls on the same inputs give the same bits.  grad_p, x and the tape are not modified.
 *
 * The training forward computes fnx_banknet_forward's arithmetic (p is bit-identical to it in every fp32 mode) and writes every ReLU
 * output, after its ReLU, into one caller-provided buffer, the tape, as contiguous (B,C,h,w) tensors: "a" = relu(conv1(x)); "h1", "b1" the
 * outputs of convBank.block.0 / block.2 at full resolution, "h2", "b2" at half and "h4", "b4" at quarter resolution; "a2", "a4" the
 * average-pooled a those two levels start from; "t" the sum of the three levels; "c2a", "c2b" the outputs of the first and the second
 * conv2; "c3" (8 channels) of conv3; and "x" (2 channels), the net's input, which only fnx_fluidnet_bank_forward_train writes (it builds
 * x itself).  fnx_banknet_tape_layout returns the tape's size in floats (0 on error) and, if `entries` is not NULL, fills
 * fnx_banknet_tape_entries() of them in tape order; names and offsets are a function of (B, H, W) alone.
 *
 * packed_t (fnx_banknet_packed_t_bytes()): the transposed, tap-flipped bank weights in the A-operand order of v_mfma_f32_16x16x4_f32 and
 * the transposed 1x1 weights; fnx_banknet_pack_t runs on the device.  Repack it, as `packed`, whenever the weights change.
 *
 * Backward: grad_p (B,1,H,W), the tape and x (B,2,H,W) -> grad_blob (fnx_banknet_weight_floats() floats) in the layout of weights_blob:
 * per conv the weight gradient, then the bias gradient.  The derivative of a ReLU is (saved output > 0), torch's rule.  conv2's gradient
 * is the sum over its two applications, a bank tensor's the sum over the three levels; the gradient reaches level 2 (4) as the sum of its
 * 2x2 (4x4) children and comes back from the pooling as g_a1 + up2(g_a2) / 4 + up4(g_a4) / 16.  The input gradients of the 16 -> 16
 * convolutions and every 16 x 16 weight gradient run on v_mfma_f32_16x16x4_f32; conv1's 288 weight gradients and the bias gradients are
 * plain sums.  Workspace: fnx_banknet_backward_ws_bytes(g) (0 for a grid without a size). */
int fnx_banknet_tape_entries(void);
size_t fnx_banknet_tape_layout(const FnxGrid* g, FnxTapeEntry* entries);
size_t fnx_banknet_packed_t_bytes(void);
int fnx_banknet_pack_t(const float* weights_blob, void* packed_t, void* stream);
size_t fnx_banknet_backward_ws_bytes(const FnxGrid* g);
int fnx_banknet_forward_train(const FnxGrid* g, const void* packed, const float* x, float* p, float* tape, int precision_mode, void* stream);
int fnx_banknet_backward(const FnxGrid* g, const void* packed_t, const float* x, const float* grad_p, const float* tape, float* grad_blob,
                         int precision_mode, void* ws, size_t ws_bytes, void* stream);
/* fnx_fluidnet_forward_train / fnx_fluidnet_backward's contract with the bank net in the middle, and their launches around the net:
 * g_net = s grad_p + velocity_update_backward_p(s setWallBcs(grad_U)).  One workspace size for both. */
size_t fnx_fluidnet_bank_train_ws_bytes(const FnxGrid* g);
int fnx_fluidnet_bank_forward_train(const FnxGrid* g, const void* packed, const float* input, float normalize_threshold, float* p_out,
                                    float* U_out, float* flags_out, float* scale_out, float* tape, int precision_mode, void* ws,
                                    size_t ws_bytes, void* stream);
int fnx_fluidnet_bank_backward(const FnxGrid* g, const void* packed_t, const float* flags, const float* scale, const float* grad_p,
                               const float* grad_U, const float* tape, float* grad_blob, int precision_mode, void* ws, size_t ws_bytes,
                               void* stream);

/* Training of the 3D net (ABI 25): the same gradients for the Conv3d net, under names of their own next to the 2D entry points above,
 * which keep refusing 3D.  Every entry point checks, before it touches the device and each with its own fnx_last_error text: null
 * arguments; a 3D grid (is3D = 1, D >= 4: "3D only"); H and W of at least 4; a precision mode among FNX_PRECISION_FP32, _FP32_F4, _FP32_F2
 * and _FP32_DIRECT ("fp32 arithmetic only"); a whole domain (no compute window k_begin / k_end, no z-slab view z_offset / D_global); at most
 * 2^26 cells per sample and 65535 planes B * D; and the size of the weight image it is given -- `packed` is fnx_scalenet_pack(1, ..)'s
 * fnx_scalenet_packed_bytes(1) bytes, `packed3d_t` fnx_scalenet3d_pack_t's fnx_scalenet3d_packed_t_bytes() bytes; the two look alike, and
 * a swapped pair is told apart by its size.  No gradient with respect to the input, no dropout.  No atomics: two calls on the same inputs
 * give the same bits.
 *
 * The tape holds the 2D tape's entries as contiguous (B,C,D,H,W) tensors: "xq" at int(n * 0.25) per axis, "in2" at int(n * 0.5), "in1"
 * at full resolution and the outputs "y0" .. "y15" after their ReLU -- 331 floats per full-resolution voxel, 324 per half- and 131 per
 * quarter-resolution voxel (373.5 per full-resolution voxel in all, 1.49 KB).  fnx_multiscale3d_tape_layout returns its size in floats (0 on error) and fills
 * fnx_multiscale_tape_entries() entries; the layout is a function of (B, D, H, W) alone.  p of the training forward is bit-identical to
 * fnx_multiscale_forward's on the 3D grid in the same mode. */
typedef struct FnxTapeEntry3D {
  char name[8];
  size_t offset;     /* floats from the start of the tape; the tensor is a contiguous (B,C,D,H,W) */
  int C, D, H, W;
} FnxTapeEntry3D;
size_t fnx_multiscale3d_tape_layout(const FnxGrid* g, FnxTapeEntry3D* entries);

/* Training of the Conv3d bank net (ABI 34): the 3D siblings of the ABI-31 block above for the 'FluidNet3D' model, with the same contracts.
 * Gradients of a scalar loss of p (or of FluidNet.forward's (p, U)) with respect to the twelve parameter tensors, exact fp32.  Every entry
 * point refuses, before it touches the device and each with its own fnx_last_error text, what fnx_banknet3d_forward refuses: null
 * arguments; a 2D grid ("3D only"); the bf16 modes; an unknown precision mode; D, H or W that is no positive multiple of 4; a short
 * workspace (FNX_EWORKSPACE).  No gradient with respect to the input, no dropout.  No atomics and no host synchronisation (capturable):
 * every cross-workgroup sum goes through per-workgroup partial sums which one kernel adds in index order in fp64, so two calls on the
 * same inputs give the same bits.  grad_p, x and the tape are not modified.
 *
 * The tape holds the 2D bank tape's fourteen entries, in its order and under its names, as contiguous (B,C,d,h,w) tensors: "a", "h1",
 * "b1", "t", "c2a", "c2b" (16 channels) and "c3" (8) at full resolution, "a2", "h2", "b2" at D/2 H/2 W/2, "a4", "h4", "b4" at D/4 H/4 W/4, and
 * "x" (2 channels), which only fnx_fluidnet_bank3d_forward_train writes: 106 + 48 / 8 + 48 / 64 = 112.75 floats a full-resolution voxel
 * (451 bytes), offsets rounded to 64 floats.  fnx_banknet3d_tape_layout returns the tape's size in floats (0 on error) and, if `entries`
 * is not NULL, fills fnx_banknet3d_tape_entries() of them; names and offsets are a function of (B, D, H, W) alone.  p of the training
 * forward is bit-identical to fnx_banknet3d_forward's in every fp32 mode; the training forward needs no workspace.
 *
 * packed_t (fnx_banknet3d_packed_t_bytes()): the transposed, tap-flipped bank weights in the A-operand order of the forward's convolution
 * kernel, 16 zeros as their bias, and the transposed 1x1x1 weights; fnx_banknet3d_pack_t runs on the device.  Repack it, as `packed`,
 * whenever the weights change.
 *
 * Backward: grad_p (B,1,D,H,W), the tape and x (B,2,D,H,W) -> grad_blob (fnx_banknet3d_weight_floats() floats) in the layout of
 * weights_blob.  The derivative of a ReLU is (saved output > 0).  conv2's gradient is the sum over its two applications, a bank tensor's
 * the sum over the three levels (added in the order quarter, half, full); the gradient reaches level 2 (4) as the sum of its 2x2x2
 * (4x4x4) children and comes back from the pooling as g_a1 + up2(g_a2) / 8 + up4(g_a4) / 64.  The input gradients of the 16 -> 16
 * convolutions run through the forward's z-marching kernel body on packed_t; every 16 x 16 weight gradient runs on
 * v_mfma_f32_16x16x4_f32 with the cells as K; conv1's 864 weight gradients and the bias gradients are plain sums.  Workspace:
 * fnx_banknet3d_backward_ws_bytes(g) (0 for a grid without a size): 146 bytes a full-resolution voxel and the partial sums.
 *
 * fnx_banknet3d_backward_plan: the fnx_banknet3d_backward_launches() launches of the backward that leave partial sums, in launch order:
 * the tail, the two weight gradients (block.2, block.0) of the quarter, the half and the full level, and conv1.  A launch takes
 * min(items, cap) workgroups, with item i on workgroup i mod workgroups, and workgroup s writes partial_floats floats at
 * partial_offset + 4 * s * partial_floats bytes of the workspace.  dims: a weight gradient's items are (sample, y tile, x tile, z chunk)
 * = B x dims[1] x dims[0] x dims[2] of tiles WG 4 x 36 cells and dims[3] planes a chunk; the tail's and conv1's are units of dims[1]
 * flattened cells, dims[0] a sample.  A function of (B, D, H, W) alone. */
typedef struct FnxBankBwdLaunch {
  char name[16];
  int level;               /* 1, 2 or 4 */
  long long items;
  int workgroups, cap;
  int partial_floats;
  size_t partial_offset;   /* bytes from the start of the backward's workspace */
  int dims[4];
} FnxBankBwdLaunch;
int fnx_banknet3d_tape_entries(void);
size_t fnx_banknet3d_tape_layout(const FnxGrid* g, FnxTapeEntry3D* entries);
size_t fnx_banknet3d_packed_t_bytes(void);
int fnx_banknet3d_pack_t(const float* weights_blob, void* packed_t, void* stream);
size_t fnx_banknet3d_backward_ws_bytes(const FnxGrid* g);
int fnx_banknet3d_backward_launches(void);
int fnx_banknet3d_backward_plan(const FnxGrid* g, FnxBankBwdLaunch* launches);
int fnx_banknet3d_forward_train(const FnxGrid* g, const void* packed, const float* x, float* p, float* tape, int precision_mode, void* stream);
int fnx_banknet3d_backward(const FnxGrid* g, const void* packed_t, const float* x, const float* grad_p, const float* tape, float* grad_blob,
                           int precision_mode, void* ws, size_t ws_bytes, void* stream);
/* fnx_fluidnet_bank_forward_train / fnx_fluidnet_bank_backward's contract on a (B,6,D,H,W) input with the Conv3d bank net in the middle:
 * (p, U) have fnx_fluidnet_bank3d_forward's bits.  One workspace size for both. */
size_t fnx_fluidnet_bank3d_train_ws_bytes(const FnxGrid* g);
int fnx_fluidnet_bank3d_forward_train(const FnxGrid* g, const void* packed, const float* input, float normalize_threshold, float* p_out,
                                      float* U_out, float* flags_out, float* scale_out, float* tape, int precision_mode, void* ws,
                                      size_t ws_bytes, void* stream);
int fnx_fluidnet_bank3d_backward(const FnxGrid* g, const void* packed_t, const float* flags, const float* scale, const float* grad_p,
                                 const float* grad_U, const float* tape, float* grad_blob, int precision_mode, void* ws, size_t ws_bytes,
                                 void* stream);
/* The adjoint of the net's trilinear resampling (align_corners = False, sample positions in float32) of one channel on its own, as
 * the backward applies it at the two tower joints: grad_dst (B,1,Do,Ho,Wo) -> grad_src (B,1,Di,Hi,Wi), every source voxel the sum of
 * its destinations in a fixed x, y, z order.  Exposed so that a test can hold it against the transposed interpolation matrices. */
int fnx_trilinear_upsample_backward(int B, int Di, int Hi, int Wi, int Do, int Ho, int Wo, const float* grad_dst, float* grad_src,
                                    void* stream);
/* packed3d_t: the 3D blob itself and, for the ten 3x3x3 layers between 32, 64 and 128 channels, the images of the transposed, tap-flipped
 * weight with zero bias, packed on the device by the forward's own pack kernels.  weights_blob: fnx_scalenet_weight_floats(1) floats. */
size_t fnx_scalenet3d_packed_t_bytes(void);
int fnx_scalenet3d_pack_t(const float* weights_blob, void* packed_t, void* stream);
size_t fnx_multiscale3d_backward_ws_bytes(const FnxGrid* g);
/* x (B,2,D,H,W) -> p (B,1,D,H,W) and the tape (fnx_multiscale3d_tape_layout floats).  No workspace. */
int fnx_multiscale3d_forward_train(const FnxGrid* g, const void* packed, size_t packed_bytes, const float* x, float* p, float* tape,
                                   int precision_mode, void* stream);
/* grad_p (B,1,D,H,W) and the tape of the forward -> grad_blob (fnx_scalenet_weight_floats(1) floats) in the layout of weights_blob: per
 * conv the weight gradient (Cout,Cin,kd,kh,kw) then the bias gradient.  grad_p and the tape are not modified.  The weight gradients of
 * the 3x3x3 layers between 32, 64 and 128 channels run on the matrix cores in exact fp32 (v_mfma_f32_32x32x2_f32), one workgroup per
 * (32 x 32 channel block, z tap, split of the pixel tiles), partials added in a fixed order in fp64. */
int fnx_multiscale3d_backward(const FnxGrid* g, const void* packed_t, size_t packed_t_bytes, const float* grad_p, const float* tape,
                              float* grad_blob, int precision_mode, void* ws, size_t ws_bytes, void* stream);
/* The same call with the plain fp64 weight-gradient kernel of the thin layers for every layer: a cross-check for tests and A/B timing. */
int fnx_multiscale3d_backward_plain(const FnxGrid* g, const void* packed_t, size_t packed_t_bytes, const float* grad_p, const float* tape,
                                    float* grad_blob, int precision_mode, void* ws, size_t ws_bytes, void* stream);
/* FluidNet.forward for training on a 3D grid and its backward (one workspace size for both): fnx_fluidnet_forward with the taped net;
 * input (B,6,D,H,W) = [p, Ux, Uy, Uz, flags, density]; flags_out (B,1,D,H,W) and scale_out (B) go back into the backward, where
 * g_net = s grad_p + velocity_update_backward_p(s setWallBcs(grad_U)), grad_U (B,3,D,H,W). */
size_t fnx_fluidnet3d_train_ws_bytes(const FnxGrid* g);
int fnx_fluidnet3d_forward_train(const FnxGrid* g, const void* packed, size_t packed_bytes, const float* input, float normalize_threshold,
                                 float* p_out, float* U_out, float* flags_out, float* scale_out, float* tape, int precision_mode, void* ws,
                                 size_t ws_bytes, void* stream);
int fnx_fluidnet3d_backward(const FnxGrid* g, const void* packed_t, size_t packed_t_bytes, const float* flags, const float* scale,
                            const float* grad_p, const float* grad_U, const float* tape, float* grad_blob, int precision_mode, void* ws,
                            size_t ws_bytes, void* stream);

/* ---- Training scenes and the training loss (ABI 23; the reference trains on a pre-computed Mantaflow data set and composes its loss
 * from ATen operators, fluid_net_train.py:276-285).  2D only, like the training entry points above; every entry point checks before it
 * touches the device: null arguments, a 2D grid, H and W of at least 4 (and at most 32768, B at most 65535), and what is said per call.
 *
 * Randomness is counter based, without state or atomics: a 32-bit word is
 *   hash(seed, scene, stream, counter) = mix(mix(mix(mix(seed + 0x9e3779b9) ^ scene) ^ stream) ^ counter)
 *   mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16      (the "lowbias32" finaliser)
 * and a uniform float is (hash >> 8) * 2^-24.  The bits of a scene depend on (seed, scene id, H, W) and the parameters only: not on the
 * batch slot, the batch size or the launch geometry.  Arithmetic: integer operations, fp32 add / subtract / multiply / compare and
 * int <-> float conversion, uncontracted, in the order tests/scene_reference.py states in numpy -- the kernels are bit-identical to it. */
#define FNX_SCENE_MAX_PRIMITIVES 16   /* the cap on n_max */
#define FNX_SCENE_MAX_OCTAVES 8
typedef struct FnxSceneParams {
  unsigned seed;
  /* obstacles: n_min .. n_max primitives per scene (0 <= n_min <= n_max <= FNX_SCENE_MAX_PRIMITIVES), each a disc or an axis-aligned box
   * by one hash bit; the centre is the grid centre ((W - 1) / 2, (H - 1) / 2) + an offset drawn per axis in [centre_min, centre_max] *
   * min(H, W); the radius (disc) or the two half extents (box) are drawn in [size_min, size_max] * min(H, W).  A cell centre (i, j)
   * is inside on squared distances: dx^2 + dy^2 <= r^2, resp. dx^2 <= a^2 and dy^2 <= b^2. */
  int n_min, n_max;
  float centre_min, centre_max;
  float size_min, size_max;
  /* turbulence: psi(node) = amplitude * sum_{o < octaves} 2^-o noise_o(node / (wavelength 2^-o)); noise_o is value noise on the integer
   * lattice (values 2 uniform - 1 from stream 16 + o, blended with the smoothstep t t (3 - 2 t)); 1 <= octaves <= FNX_SCENE_MAX_OCTAVES,
   * wavelength (cells) >= 2^(octaves - 1).  density = clamp(density_scale * the same sum on the streams 32 + o at the cell, 0, 1). */
  int octaves;
  float wavelength, amplitude, density_scale;
} FnxSceneParams;
/* scene_ids: B DEVICE ints.  flags (B,1,1,H,W) = emptyDomain (border ring TypeObstacle, interior TypeFluid) united with the scene's
 * primitives.  Refuses n_max above the cap and inverted ranges. */
int fnx_scene_obstacles(const FnxGrid* g, const FnxSceneParams* prm, const int* scene_ids, float* flags, void* stream);
/* U (B,2,1,H,W) = the discrete curl of psi on the grid nodes: U0(i,j) = psi(i,j+1) - psi(i,j), U1(i,j) = -(psi(i+1,j) - psi(i,j)):
 * divergence-free up to the rounding of the four differences, before any boundary condition.  density (B,1,1,H,W) may be NULL. */
int fnx_scene_turbulence(const FnxGrid* g, const FnxSceneParams* prm, const int* scene_ids, float* U, float* density, void* stream);

/* The loss of fluid_net_train.py:276-285 and its gradient.  div = fnx_velocity_divergence(out_U, flags), bit for bit (0 on the border
 * ring and in obstacles), N = B H W:
 *   terms[0..3] = mean (out_p - target_p)^2, mean div^2, mean |out_p - target_p|, mean |div|      (nn.MSELoss / nn.L1Loss, unweighted)
 *   terms[4]    = lambdas . terms[0..3]                                   lambdas = (pL2, divL2, pL1, divL1), 4 HOST floats
 *   grad_p      = upstream (2 pL2 (out_p - target_p) + pL1 sign(out_p - target_p)) / N;  exactly 0 when both pressure lambdas are 0
 *   grad_U      = the stencil of fnx_velocity_divergence_backward on upstream (2 divL2 div + divL1 sign(div)) / N, formed per face from
 *                 the face's two cells (div is never stored); sign(0) = 0, torch's subgradient
 * upstream: 1 DEVICE float (the gradient of whatever the total feeds).  target_p may be NULL when both pressure lambdas are 0 (the two
 * pressure terms are then 0); with one of them set a NULL target is refused.  terms (5 DEVICE floats) may be NULL (gradients only: ws
 * unused), or grad_p, grad_U and upstream may all be NULL (terms only).  The sums are fp64 partials per workgroup in ws
 * (fnx_train_loss_ws_bytes) added in index order by a second, one-workgroup launch: two calls give the same bits. */
size_t fnx_train_loss_ws_bytes(const FnxGrid* g);
int fnx_train_loss(const FnxGrid* g, const float* out_p, const float* out_U, const float* flags, const float* target_p,
                   const float lambdas[4], const float* upstream, float* terms, float* grad_p, float* grad_U, void* ws, size_t ws_bytes,
                   void* stream);

/* ---- Training scenes and the training loss in 3D (ABI 26; the reference has no 3D training at all).  The counterparts of the four
 * entry points above under names of their own, as fnx_fluidnet3d_* stand next to fnx_fluidnet_*: the 2D names keep refusing a 3D grid.
 * Every entry point checks before it touches the device, each case with its own text: a null argument ("null argument"); a 2D grid,
 * is3D = 0 or D < 4, since the net's three scales need 4 planes ("3D only"); H or W below 4 ("at least 4 cells per axis"); an axis above
 * 32768, B * D above 65535 or D * H * W of 2^31 and more (the range is stated); the parameter caps and inverted ranges of the 2D calls.
 *
 * The hash is the one above.  A lattice value at the integer point (lx, ly, lz) of octave o of a noise with the stream base s0 is
 *   hash(seed, scene, stream = (lz << 8) | (s0 + o), counter = ly * 65536 + lx)
 * -- the plane goes into the stream word above its low byte -- which is injective for lx, ly < 65536 and lz < 2^24, and the accepted
 * grids stay inside that.  Stream bases: 80 = the obstacle primitives, 96 + o = psi_x, 112 + o = psi_y, 128 + o = psi_z, 144 + o = the
 * density (the 2D kernels use 0, 16 + o, 32 + o; the samplers 64 and 65).  A scene's bits depend on (seed, scene id, D, H, W) and the
 * parameters only.  Arithmetic as in 2D; tests/scene_reference_3d.py is the numpy statement and the kernels are bit-identical to it.
 *
 * Obstacles: flags (B,1,D,H,W) = a border shell one cell wide (TypeObstacle) united with n_min .. n_max primitives, each a ball or an
 * axis-aligned box by one hash bit.  Primitive t draws at the counters 16 t + d of stream 80: d = 0 ball / box (the top bit),
 * d = 1, 2, 3 the centre's offset along x, y, z in [centre_min, centre_max] * m from the grid centre ((W-1)/2, (H-1)/2, (D-1)/2),
 * d = 4, 5, 6 the radius (d = 4) resp. the half extents along x, y, z in [size_min, size_max] * m, with m = min(D, H, W); the number of
 * primitives is drawn at counter 0xffff0000.  Inside on squared distances: (dx^2 + dy^2) + dz^2 <= a^2, resp. dx^2 <= a^2 and
 * dy^2 <= b^2 and dz^2 <= c^2. */
int fnx_scene_obstacles3d(const FnxGrid* g, const FnxSceneParams* prm, const int* scene_ids, float* flags, void* stream);
/* U (B,3,D,H,W) = the discrete curl of a vector potential whose component psi_a sits on the cell edges along axis a; psi_a(i,j,k) =
 * amplitude * the 2D sum over octaves with a trilinear smoothstep blend (along x, then y, then z) at the integer point (i,j,k):
 *   U0(i,j,k) = (psi_z(i,j+1,k) - psi_z(i,j,k)) - (psi_y(i,j,k+1) - psi_y(i,j,k))
 *   U1(i,j,k) = (psi_x(i,j,k+1) - psi_x(i,j,k)) - (psi_z(i+1,j,k) - psi_z(i,j,k))
 *   U2(i,j,k) = (psi_y(i+1,j,k) - psi_y(i,j,k)) - (psi_x(i,j+1,k) - psi_x(i,j,k))
 * so the MAC divergence cancels term by term, up to the rounding of the differences, before any boundary condition.  density
 * (B,1,D,H,W), = clamp(density_scale * the same sum on the streams 144 + o at the cell, 0, 1), may be NULL. */
int fnx_scene_turbulence3d(const FnxGrid* g, const FnxSceneParams* prm, const int* scene_ids, float* U, float* density, void* stream);
/* fnx_train_loss for out_p (B,1,D,H,W) and out_U (B,3,D,H,W), N = B D H W: div has the bits of fnx_velocity_divergence on the 3D grid,
 * grad_U is the stencil of fnx_velocity_divergence_backward formed per face; everything else as said there (the workspace is one fp64
 * quadruple per workgroup of 64 x 4 cells of a plane; fnx_train_loss3d_ws_bytes gives 0 for a grid that is refused). */
size_t fnx_train_loss3d_ws_bytes(const FnxGrid* g);
int fnx_train_loss3d(const FnxGrid* g, const float* out_p, const float* out_U, const float* flags, const float* target_p,
                     const float lambdas[4], const float* upstream, float* terms, float* grad_p, float* grad_U, void* ws, size_t ws_bytes,
                     void* stream);

/* Optional timing of the dominant kernels with HIP events on the launch stream (used by bench.py for the roofline
 * figures).  While enabled, every launch of the tagged kernel class is bracketed by an event pair (up to 16384 pairs,
 * later launches are not recorded).  fnx_profile_read synchronises the recorded events and returns the summed
 * kernel time and the number of launches of that class; fnx_profile_enable(1) also clears earlier records.
 * fnx_profile_enable(2) (round 6): ONE pair around each RUN of consecutive launches of a class on a stream (the 50 passes of a
 * Jacobi-100 solve, the consecutive Winograd layers of a tower) -- the launches then run back to back as they do in a step; a pair
 * per launch holds each kernel until the one before it has drained and reads 3-10 % long (rocprofv3's per-kernel durations of a
 * replayed step agree with the run figure: profiles/r06/c_wino4_versions.txt, tools/debug/trace_step_span.sh). */
enum { FNX_PROF_JACOBI = 0, FNX_PROF_CONV_MFMA = 1, FNX_PROF_ADVECT = 2, FNX_PROF_STAGE = 3, FNX_PROF_CONV_DIRECT = 4,
       FNX_PROF_CONV_MFMA16 = 5, FNX_PROF_CONV_BF16 = 6 /* FNX_PRECISION_BF16X6 launches; work = bf16 MFMA FLOPs issued */, FNX_PROF_NTAGS = 7 };
int fnx_profile_enable(int on);
/* roctx ranges ("fnx:jacobi", "fnx:advect", "fnx:stage", "fnx:conv_*") around the enqueue of the same kernel classes, for
 * `rocprofv3 --marker-trace`.  The marker library (librocprofiler-sdk-roctx.so, else libroctx64.so) is loaded by this call,
 * not linked; off by default.  The reference has no tracing hooks. */
int fnx_roctx_enable(int on);
int fnx_profile_read(int tag, double* total_ms, int* launches);
/* What the recorded launches of a class ISSUED: for the conv classes the multiply-add FLOPs actually sent to the matrix
 * cores (a Winograd F(2x2,3x3) launch issues 16/36 of the direct convolution's), so that issued / time / peak is the
 * MFMA utilisation rather than a direct-convolution-equivalent rate.  0 for the other classes. */
int fnx_profile_read_work(int tag, double* work);

#ifdef __cplusplus
}
#endif
#endif /* FLUIDNET_HIP_H */
