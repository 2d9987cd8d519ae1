#include <memory>
#include <optional>
// torch cpp-extension `fluidnet_cpp` for MI355X: the reference's three pybind entry points
// (pytorch/lib/fluid/cpp/fluids_init.cpp:1009-1014) with identical names and positional signatures, bound
// to the C ABI of libfluidnet_hip.so, plus the operators the reference implements in Python
// (lib/fluid/*.py) as additional entry points in the same style.
//
// This file is host plumbing only: shape/contiguity checks mirroring the reference's asserts, output and
// workspace allocation from torch's caching allocator, the current HIP stream, status -> RuntimeError.
// There is no CPU path: tensors must live on a HIP device.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <c10/hip/HIPGuard.h>

#include "../../include/fluidnet_hip.h"

namespace {

using at::Tensor;

// Per-call geometry options (no reference counterpart; the reference is single-device and has one 3D behaviour).  The
// extension keeps NO mutable state: every 3D-capable entry point takes an optional `geom` and is re-entrant like the
// reference's (SURVEY.md 8b "no globals").
struct Geom {
  bool ref_quirks = false;          // 3D only: reproduce the reference's 3D defects bit-for-bit (FnxGrid.ref_quirks)
  int z_offset = 0, D_global = 0;   // z-slab view: the tensors hold planes [z_offset, z_offset + D) of a D_global-deep domain
  int k_begin = 0, k_end = 0;       // compute window: plane-parallel operators produce local planes [k_begin, k_end) only
  int jacobi_x = 0;                 // tiling of the 3D two-sweep Jacobi march: 0 the plan's choice, 60 / 64 forced (A/B timing, tests; same bits)
};

void check_status(int rc) {
  TORCH_CHECK(rc == FNX_OK, fnx_last_error());
}

void check_field(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on the GPU (libfluidnet_hip has no CPU path)");
  TORCH_CHECK(t.scalar_type() == at::kFloat, name, " must be float32");
  TORCH_CHECK(t.dim() == 5, "Dimension mismatch");
  TORCH_CHECK(t.is_contiguous(), "Input is not contiguous");
}

FnxGrid grid_of(const Tensor& flags, bool is3D, const Geom* geom) {
  static const Geom none;
  const Geom& go = geom ? *geom : none;
  check_field(flags, "flags");
  TORCH_CHECK(flags.size(1) == 1, "flags is not scalar");
  FnxGrid g{};
  g.B = (int)flags.size(0); g.D = (int)flags.size(2); g.H = (int)flags.size(3); g.W = (int)flags.size(4);
  g.is3D = is3D ? 1 : 0;
  g.ref_quirks = (go.ref_quirks ? 1 : 0) |
                 ((go.jacobi_x == 60 ? FNX_JACOBI3D_X_60 : go.jacobi_x == 64 ? FNX_JACOBI3D_X_64 : FNX_JACOBI3D_X_AUTO) << FNX_JACOBI3D_X_SHIFT);
  g.z_offset = is3D ? go.z_offset : 0; g.D_global = is3D ? go.D_global : 0;
  g.k_begin = is3D ? go.k_begin : 0; g.k_end = is3D ? go.k_end : 0;
  if (!is3D) TORCH_CHECK(g.D == 1, "2D velocity field but zdepth > 1");
  return g;
}

void check_vel(const Tensor& U, const FnxGrid& g, const char* name) {
  check_field(U, name);
  TORCH_CHECK(U.size(1) == (g.is3D ? 3 : 2), g.is3D ? "3D velocity field must have 3 channels" : "2D velocity field must have only 2 channels");
  TORCH_CHECK(U.size(0) == g.B && U.size(2) == g.D && U.size(3) == g.H && U.size(4) == g.W, "Size mismatch");
}

void check_scalar(const Tensor& s, const FnxGrid& g, const char* name) {
  check_field(s, name);
  TORCH_CHECK(s.size(1) == 1 && s.size(0) == g.B && s.size(2) == g.D && s.size(3) == g.H && s.size(4) == g.W, "Size mismatch");
}

struct Workspace {
  Tensor t; void* ptr; size_t bytes;
  Workspace(const FnxGrid& g, int op, const Tensor& like) {
    bytes = fnx_workspace_bytes(&g, op);
    t = at::empty({(int64_t)(bytes ? bytes : 1)}, like.options().dtype(at::kByte));
    ptr = t.data_ptr();
  }
};

// In-place entry points bump the written tensor's version counter like torch's own in-place operators do: autograd's
// saved-tensor checks and simulate()'s "have flags / the BC arrays changed since the last step?" test (_simulate.py) rely on it.
void wrote(const Tensor& t) {
  if (t.defined() && !t.is_inference()) t.unsafeGetTensorImpl()->bump_version();
}
void wrote(const c10::optional<Tensor>& t) { if (t.has_value()) wrote(*t); }

void* cur_stream(const Tensor& t) { return (void*)c10::hip::getCurrentHIPStream(t.get_device()).stream(); }

int method_of(const std::string& m) {
  // cpp/advect_type.cpp:5-16
  if (m == "eulerFluidNet") return FNX_ADVECT_EULER;
  if (m == "maccormackFluidNet") return FNX_ADVECT_MACCORMACK;
  TORCH_CHECK(false, "Advection method not supported: ", m);
  return -1;
}

// ---- the reference's three entry points -------------------------------------------------------------
// `out` (not in the reference): write into an existing tensor -- with a compute window (set_window) the z-slab driver
// fills one advected field from several calls.
int plan_of(const std::string& plan) {
  TORCH_CHECK(plan == "auto" || plan == "tiles" || plan == "cells" || plan == "tiles_split", "plan must be 'auto', 'tiles', 'cells' or 'tiles_split'");
  return plan == "tiles" ? FNX_ADVECT_PLAN_TILES : (plan == "cells" ? FNX_ADVECT_PLAN_CELLS : (plan == "tiles_split" ? FNX_ADVECT_PLAN_TILES_SPLIT : FNX_ADVECT_PLAN_AUTO));
}

Tensor out_or_like(const c10::optional<Tensor>& out, const Tensor& like) {
  return (out.has_value() && out->defined()) ? *out : at::empty_like(like);
}

Tensor advect_scalar(float dt, Tensor src, Tensor U, Tensor flags, const std::string method, int bnd,
                     const bool sample_outside_fluid, const float maccormack_strength, c10::optional<Tensor> out,
                     const Geom* geom, const std::string& plan) {
  check_field(U, "U");
  FnxGrid g = grid_of(flags, U.size(1) == 3, geom);
  check_vel(U, g, "U"); check_scalar(src, g, "src");
  c10::hip::HIPGuard guard(flags.get_device());
  Tensor dst = out_or_like(out, src);
  check_scalar(dst, g, "out");
  Workspace ws(g, FNX_OP_ADVECT_SCALAR, src);
  check_status(fnx_advect_scalar_plan(&g, dt, src.data_ptr<float>(), U.data_ptr<float>(), flags.data_ptr<float>(),
                                      dst.data_ptr<float>(), method_of(method), bnd, sample_outside_fluid,
                                      maccormack_strength, plan_of(plan), ws.ptr, ws.bytes, cur_stream(src)));
  return dst;
}

// passive scalars (fnx_advect_scalars): src (B, C, D, H, W), C >= 1, all channels through one pair of line traces; returns a new tensor.
// `workspace`: a uint8 tensor of at least advect_scalars_workspace_bytes, or None (then it comes from the caching allocator).
Tensor advect_scalars(float dt, Tensor src, Tensor U, Tensor flags, const std::string method, int bnd,
                      const bool sample_outside_fluid, const float maccormack_strength, c10::optional<Tensor> workspace,
                      const Geom* geom, c10::optional<Tensor> out) {
  check_field(U, "U");
  FnxGrid g = grid_of(flags, U.size(1) == 3, geom);
  check_vel(U, g, "U"); check_field(src, "src");
  TORCH_CHECK(src.size(1) >= 1, "src has no channel");
  TORCH_CHECK(src.size(0) == g.B && src.size(2) == g.D && src.size(3) == g.H && src.size(4) == g.W, "Size mismatch");
  const int C = (int)src.size(1);
  c10::hip::HIPGuard guard(flags.get_device());
  Tensor dst = out_or_like(out, src);
  check_field(dst, "out");
  TORCH_CHECK(dst.sizes() == src.sizes(), "Size mismatch");
  Tensor ws;
  if (workspace.has_value() && workspace->defined()) {
    ws = *workspace;
    TORCH_CHECK(ws.is_cuda() && ws.scalar_type() == at::kByte && ws.is_contiguous(), "workspace must be a contiguous uint8 GPU tensor");
  } else {
    const size_t bytes = fnx_advect_scalars_workspace_bytes(&g, C);
    ws = at::empty({(int64_t)(bytes ? bytes : 1)}, src.options().dtype(at::kByte));
  }
  check_status(fnx_advect_scalars(&g, dt, C, src.data_ptr<float>(), U.data_ptr<float>(), flags.data_ptr<float>(), dst.data_ptr<float>(),
                                  method_of(method), bnd, sample_outside_fluid, maccormack_strength, ws.data_ptr(), (size_t)ws.numel(),
                                  cur_stream(src)));
  return dst;
}

Tensor advect_vel(float dt, Tensor orig, Tensor U, Tensor flags, const std::string method, int bnd,
                  const float maccormack_strength, c10::optional<Tensor> out, const Geom* geom, const std::string& plan) {
  check_field(U, "U");
  FnxGrid g = grid_of(flags, U.size(1) == 3, geom);
  check_vel(U, g, "U"); check_vel(orig, g, "orig");
  c10::hip::HIPGuard guard(flags.get_device());
  Tensor dst = out_or_like(out, U);
  check_vel(dst, g, "out");
  Workspace ws(g, FNX_OP_ADVECT_VEL, U);
  check_status(fnx_advect_vel_plan(&g, dt, orig.data_ptr<float>(), U.data_ptr<float>(), flags.data_ptr<float>(),
                                   dst.data_ptr<float>(), method_of(method), bnd, maccormack_strength, plan_of(plan), ws.ptr,
                                   ws.bytes, cur_stream(U)));
  return dst;
}

// the two advections of one step fused (fnx_advect_step): returns {density_adv, U_adv}
std::vector<Tensor> advect_step(float dt, Tensor density, Tensor U, Tensor flags, const bool sample_outside_fluid,
                                const float maccormack_strength, c10::optional<Tensor> out_density,
                                c10::optional<Tensor> out_U, const Geom* geom, const std::string& plan) {
  check_field(U, "U");
  FnxGrid g = grid_of(flags, U.size(1) == 3, geom);
  check_vel(U, g, "U"); check_scalar(density, g, "density");
  const int pl = plan_of(plan);
  c10::hip::HIPGuard guard(flags.get_device());
  Tensor rd = out_or_like(out_density, density);
  Tensor ud = out_or_like(out_U, U);
  check_scalar(rd, g, "out_density"); check_vel(ud, g, "out_U");
  Workspace ws(g, FNX_OP_ADVECT_STEP, U);
  check_status(fnx_advect_step_plan(&g, dt, density.data_ptr<float>(), U.data_ptr<float>(), flags.data_ptr<float>(),
                                    rd.data_ptr<float>(), ud.data_ptr<float>(), sample_outside_fluid, maccormack_strength, pl,
                                    ws.ptr, ws.bytes, cur_stream(U)));
  return {rd, ud};
}

std::vector<Tensor> solve_linear_system(Tensor flags, Tensor div, const bool is3D, const float p_tol,
                                        const int max_iter, const bool verbose, const Geom* geom) {
  FnxGrid g = grid_of(flags, is3D, geom);
  check_scalar(div, g, "div");
  if (!is3D) TORCH_CHECK(g.D == 1, "d > 1 for a 2D domain");
  TORCH_CHECK(max_iter >= 1, "At least 1 iteration is needed (maxIter < 1)");
  c10::hip::HIPGuard guard(flags.get_device());
  Tensor p = at::empty_like(flags);
  Tensor residual = at::zeros({}, flags.options());
  Workspace ws(g, FNX_OP_JACOBI, flags);
  int iters = 0;
  // verbose: the reference prints the residual after every sweep (fluids_init.cpp:968-971), which needs every iterate on the
  // host -- one sweep per launch and a host sync per sweep, like pTol > 0
  check_status((verbose ? fnx_jacobi_verbose : fnx_jacobi)(&g, flags.data_ptr<float>(), div.data_ptr<float>(), p.data_ptr<float>(),
                                                           residual.data_ptr<float>(), p_tol, max_iter, &iters, ws.ptr, ws.bytes,
                                                           cur_stream(flags)));
  return {p, residual};
}

// ---- the converged solve (fnx_pcg, ABI 20; no reference counterpart) -------------------------------------
// returns (p, residual, iterations per sample); the count needs a host synchronisation, so it is only read where the solve synchronises
// anyway (p_tol > 0 or verbose) and is None otherwise: with p_tol <= 0 the call only enqueues (capturable in a HIP graph).
// p0 (ABI 27, fnx_pcg_from): a starting guess; with it max_iter may be 0 (the line-searched guess is returned)
std::tuple<Tensor, Tensor, std::optional<std::vector<int>>> solve_linear_system_pcg(Tensor flags, Tensor div, const bool is3D, const float p_tol,
                                                                      const int max_iter, const bool verbose, const Geom* geom,
                                                                      c10::optional<Tensor> p0) {
  FnxGrid g = grid_of(flags, is3D, geom);
  check_scalar(div, g, "div");
  const bool from = p0.has_value() && p0->defined();
  if (from) check_scalar(*p0, g, "p0");
  TORCH_CHECK(from ? max_iter >= 0 : max_iter >= 1, from ? "max_iter must not be negative (maxIter < 0)" : "At least 1 iteration is needed (maxIter < 1)");
  c10::hip::HIPGuard guard(flags.get_device());
  Tensor p = at::empty_like(flags);
  Tensor residual = at::zeros({}, flags.options());
  const size_t bytes = fnx_pcg_workspace_bytes(&g);
  TORCH_CHECK(bytes > 0, fnx_last_error());
  Tensor ws = at::empty({(int64_t)bytes}, flags.options().dtype(at::kByte));
  std::vector<int> iters(g.B, 0);
  const bool count = p_tol > 0.f || verbose;
  if (from)
    check_status((verbose ? fnx_pcg_from_verbose : fnx_pcg_from)(&g, flags.data_ptr<float>(), div.data_ptr<float>(), p0->data_ptr<float>(),
                                                                 p.data_ptr<float>(), residual.data_ptr<float>(), p_tol, max_iter,
                                                                 count ? iters.data() : nullptr, ws.data_ptr(), bytes, cur_stream(flags)));
  else
    check_status((verbose ? fnx_pcg_verbose : fnx_pcg)(&g, flags.data_ptr<float>(), div.data_ptr<float>(), p.data_ptr<float>(),
                                                       residual.data_ptr<float>(), p_tol, max_iter, count ? iters.data() : nullptr,
                                                       ws.data_ptr(), bytes, cur_stream(flags)));
  if (!count) return {p, residual, std::nullopt};
  return {p, residual, iters};
}

Tensor poisson_apply(Tensor flags, Tensor p, const bool is3D, const Geom* geom) {
  FnxGrid g = grid_of(flags, is3D, geom);
  check_scalar(p, g, "p");
  c10::hip::HIPGuard guard(flags.get_device());
  Tensor Ap = at::empty_like(p);
  check_status(fnx_poisson_apply(&g, flags.data_ptr<float>(), p.data_ptr<float>(), Ap.data_ptr<float>(), cur_stream(flags)));
  return Ap;
}

Tensor pcg_precondition(Tensor flags, Tensor r, const bool is3D, const Geom* geom) {
  FnxGrid g = grid_of(flags, is3D, geom);
  check_scalar(r, g, "r");
  c10::hip::HIPGuard guard(flags.get_device());
  Tensor z = at::empty_like(r);
  const size_t bytes = fnx_pcg_workspace_bytes(&g);
  TORCH_CHECK(bytes > 0, fnx_last_error());
  Tensor ws = at::empty({(int64_t)bytes}, flags.options().dtype(at::kByte));
  check_status(fnx_pcg_precondition(&g, flags.data_ptr<float>(), r.data_ptr<float>(), z.data_ptr<float>(), ws.data_ptr(), bytes,
                                    cur_stream(flags)));
  return z;
}

// ---- operators the reference writes in Python -------------------------------------------------------
Tensor velocity_divergence(Tensor U, Tensor flags, const Geom* geom) {
  check_field(U, "U");
  FnxGrid g = grid_of(flags, U.size(1) == 3, geom);
  check_vel(U, g, "U");
  c10::hip::HIPGuard guard(flags.get_device());
  Tensor div = at::empty_like(flags);
  check_status(fnx_velocity_divergence(&g, U.data_ptr<float>(), flags.data_ptr<float>(), div.data_ptr<float>(), cur_stream(U)));
  return div;
}

void velocity_update_(Tensor pressure, Tensor U, Tensor flags, const Geom* geom) {
  check_field(U, "U");
  FnxGrid g = grid_of(flags, U.size(1) == 3, geom);
  check_vel(U, g, "U"); check_scalar(pressure, g, "pressure");
  c10::hip::HIPGuard guard(flags.get_device());
  check_status(fnx_velocity_update(&g, pressure.data_ptr<float>(), U.data_ptr<float>(), flags.data_ptr<float>(), cur_stream(U)));
  wrote(U);
}

void add_buoyancy_(Tensor U, Tensor flags, Tensor density, std::vector<double> gravity, double rho_star, double dt,
                   const Geom* geom) {
  check_field(U, "U");
  FnxGrid g = grid_of(flags, U.size(1) == 3, geom);
  check_vel(U, g, "U"); check_scalar(density, g, "density");
  TORCH_CHECK(gravity.size() == 3, "Gravity must be a 3D vector (even in 2D)");
  const float gv[3] = {(float)gravity[0], (float)gravity[1], (float)gravity[2]};
  c10::hip::HIPGuard guard(flags.get_device());
  check_status(fnx_add_buoyancy(&g, U.data_ptr<float>(), flags.data_ptr<float>(), density.data_ptr<float>(), gv,
                                (float)rho_star, (float)dt, cur_stream(U)));
  wrote(U);
}

void add_gravity_(Tensor U, Tensor flags, std::vector<double> gravity, double dt, const Geom* geom) {
  check_field(U, "U");
  FnxGrid g = grid_of(flags, U.size(1) == 3, geom);
  check_vel(U, g, "U");
  TORCH_CHECK(gravity.size() == 3, "Gravity must be a 3D vector (even in 2D)");
  const float gv[3] = {(float)gravity[0], (float)gravity[1], (float)gravity[2]};
  c10::hip::HIPGuard guard(flags.get_device());
  check_status(fnx_add_gravity(&g, U.data_ptr<float>(), flags.data_ptr<float>(), gv, (float)dt, cur_stream(U)));
  wrote(U);
}

// vorticity confinement (fnx_add_vorticity_confinement), in place on U like addGravity: the operator itself is out of place
void add_vorticity_confinement_(Tensor U, Tensor flags, double strength, const Geom* geom) {
  check_field(U, "U");
  FnxGrid g = grid_of(flags, U.size(1) == 3, geom);
  check_vel(U, g, "U");
  TORCH_CHECK(g.k_begin == 0 && g.k_end == 0 && g.z_offset == 0 && g.D_global == 0,
              "addVorticityConfinement: no compute window or z-slab view (whole grids only)");
  c10::hip::HIPGuard guard(flags.get_device());
  Tensor old = U.clone();
  check_status(fnx_add_vorticity_confinement(&g, old.data_ptr<float>(), U.data_ptr<float>(), flags.data_ptr<float>(), (float)strength,
                                             cur_stream(U)));
  wrote(U);
}

// the same out of place, as the C ABI has it: U is left alone, the confined field is returned
Tensor add_vorticity_confinement(Tensor U, Tensor flags, double strength, const Geom* geom) {
  check_field(U, "U");
  FnxGrid g = grid_of(flags, U.size(1) == 3, geom);
  check_vel(U, g, "U");
  c10::hip::HIPGuard guard(flags.get_device());
  Tensor out = at::empty_like(U);
  check_status(fnx_add_vorticity_confinement(&g, U.data_ptr<float>(), out.data_ptr<float>(), flags.data_ptr<float>(), (float)strength,
                                             cur_stream(U)));
  return out;
}

// volume rendering (fnx_render_volume): density (B,1,D,H,W) + flags -> image (B,2,R,Cc); directions 0..5 = +x -x +y -y +z -z.
// 1 - ambient is formed here, once, in fp32 (the kernels and tests/render_reference.py take it as given)
Tensor render_volume(Tensor density, Tensor flags, int view_dir, int light_dir, double k_view, double k_light, double ambient,
                     double albedo_smoke, double albedo_obstacle, int bnd) {
  check_field(density, "density");
  FnxGrid g = grid_of(flags, flags.size(2) > 1, nullptr);
  check_scalar(density, g, "density");
  TORCH_CHECK(density.get_device() == flags.get_device(), "density and flags are on different devices");
  FnxRenderParams prm{};
  prm.view_dir = view_dir; prm.light_dir = light_dir;
  prm.k_view = (float)k_view; prm.k_light = (float)k_light;
  prm.ambient = (float)ambient; prm.one_minus_ambient = 1.f - prm.ambient;
  prm.albedo_smoke = (float)albedo_smoke; prm.albedo_obstacle = (float)albedo_obstacle;
  prm.bnd = bnd;
  TORCH_CHECK(view_dir >= 0 && view_dir <= 5 && light_dir >= 0 && light_dir <= 5, "renderVolume: direction outside 0..5");
  c10::hip::HIPGuard guard(flags.get_device());
  const int va = view_dir >> 1;
  const int64_t R = va == 2 ? g.H : g.D, Cc = va == 0 ? g.H : g.W;
  Tensor image = at::empty({(int64_t)g.B, 2, R, Cc}, density.options());
  const size_t bytes = fnx_render_volume_ws_bytes(&g, &prm);
  Tensor ws = at::empty({(int64_t)(bytes ? bytes : 1)}, density.options().dtype(at::kByte));
  check_status(fnx_render_volume(&g, density.data_ptr<float>(), flags.data_ptr<float>(), &prm, image.data_ptr<float>(),
                                 bytes ? ws.data_ptr() : nullptr, bytes, cur_stream(density)));
  return image;
}

// correctScalar (cpp/advection.py:9-12), in place on src
void correct_scalar_(double dt, Tensor src, Tensor div, Tensor flags) {
  check_field(src, "src"); check_field(flags, "flags");
  FnxGrid g = grid_of(flags, flags.size(2) > 1, nullptr);
  check_scalar(src, g, "src"); check_scalar(div, g, "div"); check_scalar(flags, g, "flags");
  c10::hip::HIPGuard guard(flags.get_device());
  check_status(fnx_correct_scalar(&g, (float)dt, src.data_ptr<float>(), div.data_ptr<float>(), flags.data_ptr<float>(), cur_stream(src)));
  wrote(src);
}

// The reference multiplies dt and viscosity as Python floats (doubles) and the product meets the float tensor rounded once
// (viscosity.py:64).  fnx_add_viscosity takes two floats and forms (float)((double)dt * viscosity): rounding either factor first moves
// the coefficient by an ulp for about a third of all pairs.  So the product is formed here and handed over as dt, with a viscosity of 1 (the C
// function's product is then exact).  A negative viscosity goes through as it is, for the C function's own refusal.
struct ViscousArgs { float dt, viscosity; };
static ViscousArgs viscous_args(double dt, double viscosity) {
  if (!(viscosity >= 0)) return {(float)dt, (float)viscosity};
  return {(float)(dt * viscosity), 1.f};
}

// viscosity.py:7-70, in place on U like the reference; 2D (B,2,1,H,W) or 3D (B,3,D,H,W), the 3D form in default semantics
void add_viscosity_(double dt, Tensor U, Tensor flags, double viscosity) {
  check_field(U, "U");
  FnxGrid g = grid_of(flags, U.size(1) == 3, nullptr);
  check_vel(U, g, "U");
  c10::hip::HIPGuard guard(flags.get_device());
  Tensor old = U.clone();
  const ViscousArgs a = viscous_args(dt, viscosity);
  check_status(fnx_add_viscosity(&g, a.dt, old.data_ptr<float>(), U.data_ptr<float>(), flags.data_ptr<float>(), a.viscosity,
                                 cur_stream(U)));
  wrote(U);
}

// set_wall_bcs_stick.py:5-157 (2D; in place on U like the reference).  This is the reference's entry point and keeps the reference's
// reach: a 3D field is refused here as before, and the 3D operator (no reference counterpart) is set_wall_bcs_stick_out below
void set_wall_bcs_stick_(Tensor U, Tensor flags, Tensor flags_stick) {
  check_field(U, "U");
  TORCH_CHECK(U.size(1) != 3, "set_wall_bcs_stick_: 2D only (the reference's 3D branch cannot run, set_wall_bcs_stick.py:85-86; the 3D "
                              "operator of this package is set_wall_bcs_stick_out)");
  FnxGrid g = grid_of(flags, U.size(1) == 3, nullptr);
  check_vel(U, g, "U");
  check_scalar(flags_stick, g, "flags_stick");
  c10::hip::HIPGuard guard(flags.get_device());
  Tensor old = U.clone();
  check_status(fnx_set_wall_bcs_stick(&g, old.data_ptr<float>(), U.data_ptr<float>(), flags.data_ptr<float>(),
                                      flags_stick.data_ptr<float>(), cur_stream(U)));
  wrote(U);
}

// The same two operators out of place, as the C ABI has them (no reference counterpart): U is only read and `out`, a tensor of U's
// shape, is written and returned -- what a caller that owns both buffers uses to spare the copy above.  `out` must not be U.
Tensor add_viscosity_out(double dt, Tensor U, Tensor flags, double viscosity, Tensor out) {
  check_field(U, "U");
  FnxGrid g = grid_of(flags, U.size(1) == 3, nullptr);
  check_vel(U, g, "U"); check_vel(out, g, "out");
  c10::hip::HIPGuard guard(flags.get_device());
  const ViscousArgs a = viscous_args(dt, viscosity);
  check_status(fnx_add_viscosity(&g, a.dt, U.data_ptr<float>(), out.data_ptr<float>(), flags.data_ptr<float>(), a.viscosity,
                                 cur_stream(U)));
  wrote(out);
  return out;
}

Tensor set_wall_bcs_stick_out(Tensor U, Tensor flags, Tensor flags_stick, Tensor out) {
  check_field(U, "U");
  FnxGrid g = grid_of(flags, U.size(1) == 3, nullptr);
  check_vel(U, g, "U"); check_vel(out, g, "out");
  check_scalar(flags_stick, g, "flags_stick");
  c10::hip::HIPGuard guard(flags.get_device());
  check_status(fnx_set_wall_bcs_stick(&g, U.data_ptr<float>(), out.data_ptr<float>(), flags.data_ptr<float>(),
                                      flags_stick.data_ptr<float>(), cur_stream(U)));
  wrote(out);
  return out;
}

void set_wall_bcs_(Tensor U, Tensor flags, const Geom* geom) {
  check_field(U, "U");
  FnxGrid g = grid_of(flags, U.size(1) == 3, geom);
  check_vel(U, g, "U");
  c10::hip::HIPGuard guard(flags.get_device());
  check_status(fnx_set_wall_bcs(&g, U.data_ptr<float>(), flags.data_ptr<float>(), cur_stream(U)));
  wrote(U);
}

void set_const_vals_(Tensor U, c10::optional<Tensor> UBC, c10::optional<Tensor> UBCInvMask, c10::optional<Tensor> density,
                     c10::optional<Tensor> densityBC, c10::optional<Tensor> densityBCInvMask) {
  check_field(U, "U");
  FnxGrid g{}; g.B = (int)U.size(0); g.D = (int)U.size(2); g.H = (int)U.size(3); g.W = (int)U.size(4);
  g.is3D = U.size(1) == 3; g.ref_quirks = 0; g.z_offset = 0; g.D_global = 0;
  auto ptr = [&](c10::optional<Tensor>& t, bool vel) -> float* {
    if (!t.has_value() || !t->defined()) return nullptr;
    if (vel) check_vel(*t, g, "UBC"); else check_scalar(*t, g, "densityBC");
    return t->data_ptr<float>();
  };
  c10::hip::HIPGuard guard(U.get_device());
  check_status(fnx_set_const_vals(&g, U.data_ptr<float>(), ptr(UBC, true), ptr(UBCInvMask, true), ptr(density, false),
                                  ptr(densityBC, false), ptr(densityBCInvMask, false), cur_stream(U)));
  wrote(U); wrote(density);
}

// max |x| of a 5-D field as a 0-dim device tensor (no host sync) -- CFL guard of the z-slab driver
Tensor max_abs(Tensor x) {
  check_field(x, "x");
  FnxGrid g{}; g.B = (int)x.size(0); g.D = (int)x.size(2); g.H = (int)x.size(3); g.W = (int)x.size(4); g.is3D = g.D > 1;
  c10::hip::HIPGuard guard(x.get_device());
  Tensor out = at::empty({}, x.options());
  check_status(fnx_max_abs(&g, x.data_ptr<float>(), (int)x.size(1), out.data_ptr<float>(), cur_stream(x)));
  return out;
}

Tensor flags_to_occupancy(Tensor flags) {
  FnxGrid g = grid_of(flags, flags.size(2) > 1, nullptr);
  c10::hip::HIPGuard guard(flags.get_device());
  Tensor occ = at::empty_like(flags);
  check_status(fnx_flags_to_occupancy(&g, flags.data_ptr<float>(), occ.data_ptr<float>(), cur_stream(flags)));
  return occ;
}

void empty_domain_(Tensor flags, int boundary_width, const Geom* geom) {
  FnxGrid g = grid_of(flags, flags.size(2) > 1, geom);
  c10::hip::HIPGuard guard(flags.get_device());
  check_status(fnx_empty_domain(&g, flags.data_ptr<float>(), boundary_width, cur_stream(flags)));
  wrote(flags);
}

// adjoints of the linear stencil operators (fnx_velocity_divergence_backward, fnx_velocity_update_backward)
Tensor velocity_divergence_backward(Tensor grad_div, Tensor flags, bool is3D, const Geom* geom) {
  FnxGrid g = grid_of(flags, is3D, geom);
  check_scalar(grad_div, g, "grad_div");
  c10::hip::HIPGuard guard(flags.get_device());
  Tensor gU = at::empty({flags.size(0), is3D ? 3 : 2, flags.size(2), flags.size(3), flags.size(4)}, flags.options());
  check_status(fnx_velocity_divergence_backward(&g, grad_div.data_ptr<float>(), flags.data_ptr<float>(), gU.data_ptr<float>(), cur_stream(flags)));
  return gU;
}
std::vector<Tensor> velocity_update_backward(Tensor grad_U_out, Tensor flags, const Geom* geom) {
  check_field(grad_U_out, "grad_U_out");
  FnxGrid g = grid_of(flags, grad_U_out.size(1) == 3, geom);
  check_vel(grad_U_out, g, "grad_U_out");
  c10::hip::HIPGuard guard(flags.get_device());
  Tensor gU = at::empty_like(grad_U_out), gp = at::empty_like(flags);
  check_status(fnx_velocity_update_backward(&g, grad_U_out.data_ptr<float>(), flags.data_ptr<float>(), gU.data_ptr<float>(),
                                            gp.data_ptr<float>(), cur_stream(flags)));
  return {gU, gp};
}

// geometry written into flags (all z planes), lib/fluid/geometry_utils.py:4-63
void create_cylinder_(Tensor flags, double center_x, double center_y, double radius) {
  FnxGrid g = grid_of(flags, flags.size(2) > 1, nullptr);
  c10::hip::HIPGuard guard(flags.get_device());
  check_status(fnx_create_cylinder(&g, flags.data_ptr<float>(), center_x, center_y, radius, cur_stream(flags)));
  wrote(flags);
}

void create_box2d_(Tensor flags, double x0, double x1, double y0, double y1) {
  FnxGrid g = grid_of(flags, flags.size(2) > 1, nullptr);
  c10::hip::HIPGuard guard(flags.get_device());
  check_status(fnx_create_box2d(&g, flags.data_ptr<float>(), (float)x0, (float)x1, (float)y0, (float)y1, cur_stream(flags)));
  wrote(flags);
}

// 3D obstacles from geometry (no reference counterpart): any batch, sample -1 = every sample
void create_sphere_(Tensor flags, double center_x, double center_y, double center_z, double radius, int64_t sample) {
  FnxGrid g = grid_of(flags, flags.size(2) > 1, nullptr);
  c10::hip::HIPGuard guard(flags.get_device());
  check_status(fnx_create_sphere(&g, flags.data_ptr<float>(), center_x, center_y, center_z, radius, (int)sample, cur_stream(flags)));
  wrote(flags);
}

void create_box3d_(Tensor flags, double x0, double x1, double y0, double y1, double z0, double z1, int64_t sample) {
  FnxGrid g = grid_of(flags, flags.size(2) > 1, nullptr);
  c10::hip::HIPGuard guard(flags.get_device());
  check_status(fnx_create_box3d(&g, flags.data_ptr<float>(), (float)x0, (float)x1, (float)y0, (float)y1, (float)z0, (float)z1, (int)sample,
                                cur_stream(flags)));
  wrote(flags);
}

int64_t voxelize_mesh_ws_bytes(Tensor flags) {
  FnxGrid g = grid_of(flags, flags.size(2) > 1, nullptr);
  const size_t bytes = fnx_voxelize_mesh_ws_bytes(&g);
  TORCH_CHECK(bytes > 0, fnx_last_error());
  return (int64_t)bytes;
}

// returns the report {open rows, bad faces} as a device int32[2]; never synchronises.  workspace (optional): a device byte tensor of at
// least voxelize_mesh_ws_bytes(flags) bytes to use instead of one from the caching allocator
Tensor voxelize_mesh_(Tensor flags, Tensor vertices, Tensor faces, int64_t sample, c10::optional<Tensor> workspace) {
  FnxGrid g = grid_of(flags, flags.size(2) > 1, nullptr);
  TORCH_CHECK(vertices.is_cuda() && faces.is_cuda() && vertices.get_device() == flags.get_device() && faces.get_device() == flags.get_device(),
              "vertices and faces must be on the device of flags");
  TORCH_CHECK(vertices.scalar_type() == at::kFloat && vertices.dim() == 2 && vertices.size(1) == 3 && vertices.is_contiguous(),
              "vertices must be a contiguous (V,3) float32 tensor");
  TORCH_CHECK(faces.scalar_type() == at::kInt && faces.dim() == 2 && faces.size(1) == 3 && faces.is_contiguous(),
              "faces must be a contiguous (F,3) int32 tensor");
  TORCH_CHECK(vertices.size(0) < (1ll << 31) && faces.size(0) < (1ll << 31), "more than 2^31 vertices or faces");
  c10::hip::HIPGuard guard(flags.get_device());
  const size_t need = fnx_voxelize_mesh_ws_bytes(&g);
  TORCH_CHECK(need > 0, fnx_last_error());
  Tensor ws;
  if (workspace.has_value() && workspace->defined()) {
    ws = *workspace;
    TORCH_CHECK(ws.is_cuda() && ws.get_device() == flags.get_device() && ws.scalar_type() == at::kByte && ws.is_contiguous(),
                "workspace must be a contiguous uint8 tensor on the device of flags");
  } else {
    ws = at::empty({(int64_t)need}, flags.options().dtype(at::kByte));
  }
  Tensor report = at::empty({2}, flags.options().dtype(at::kInt));
  check_status(fnx_voxelize_mesh(&g, flags.data_ptr<float>(), vertices.data_ptr<float>(), (int)vertices.size(0), faces.data_ptr<int>(),
                                 (int)faces.size(0), (int)sample, report.data_ptr<int>(), ws.data_ptr(), (size_t)ws.numel(), cur_stream(flags)));
  wrote(flags);
  return report;
}

// lib/fluid/grid.py:7-32
Tensor get_centered(Tensor U) {
  check_field(U, "U");
  TORCH_CHECK(U.size(1) == 2 || U.size(1) == 3, "velocity field must have 2 or 3 channels");
  FnxGrid g{}; g.B = (int)U.size(0); g.D = (int)U.size(2); g.H = (int)U.size(3); g.W = (int)U.size(4); g.is3D = U.size(1) == 3;
  TORCH_CHECK(g.is3D || g.D == 1, "2D velocity field but zdepth > 1");
  c10::hip::HIPGuard guard(U.get_device());
  Tensor out = at::empty({U.size(0), 3, U.size(2), U.size(3), U.size(4)}, U.options());
  check_status(fnx_get_centered(&g, U.data_ptr<float>(), out.data_ptr<float>(), cur_stream(U)));
  return out;
}

// ---- CNN pressure projection --------------------------------------------------------------------------
Tensor scalenet_pack(Tensor blob, bool is3D) {
  TORCH_CHECK(blob.is_cuda() && blob.scalar_type() == at::kFloat && blob.is_contiguous(), "weights blob must be a contiguous float32 GPU tensor");
  TORCH_CHECK((size_t)blob.numel() == fnx_scalenet_weight_floats(is3D), "weights blob has ", blob.numel(), " floats, expected ",
              fnx_scalenet_weight_floats(is3D));
  c10::hip::HIPGuard guard(blob.get_device());
  Tensor packed = at::zeros({(int64_t)fnx_scalenet_packed_bytes(is3D)}, blob.options().dtype(at::kByte));
  check_status(fnx_scalenet_pack(is3D, blob.data_ptr<float>(), packed.data_ptr(), cur_stream(blob)));
  return packed;
}

// precision_mode: "fp32" (default: Winograd where the launch fills the chip), "fp32_direct", "bf16x6" or "bf16x3" (FNX_PRECISION_*)
static int precision_of(const std::string& m) {
  TORCH_CHECK(m == "fp32" || m == "fp32_direct" || m == "bf16x6" || m == "bf16x3" || m == "fp32_f4" || m == "fp32_f2",
              "precision_mode must be 'fp32', 'fp32_direct', 'fp32_f4', 'fp32_f2', 'bf16x6' or 'bf16x3', got '", m, "'");
  if (m == "fp32_f4") return FNX_PRECISION_FP32_F4;
  if (m == "fp32_f2") return FNX_PRECISION_FP32_F2;
  if (m == "bf16x6") return FNX_PRECISION_BF16X6;
  if (m == "bf16x3") return FNX_PRECISION_BF16X3;
  return m == "fp32_direct" ? FNX_PRECISION_FP32_DIRECT : FNX_PRECISION_FP32;
}

Tensor multiscale_forward(Tensor packed, Tensor x, const std::string& precision_mode, std::vector<int64_t> trim) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.is_contiguous(), "x must be a contiguous float32 GPU tensor");
  TORCH_CHECK((x.dim() == 4 || x.dim() == 5) && x.size(1) == 2, "x must be (B,2,H,W) or (B,2,D,H,W)");
  TORCH_CHECK(trim.empty() || trim.size() == 4, "trim: {full-tower low, high, half-tower low, high} full-resolution planes");
  const bool is3D = x.dim() == 5 && x.size(2) > 1;
  FnxGrid g{}; g.B = (int)x.size(0); g.is3D = is3D; g.ref_quirks = 0; g.z_offset = 0; g.D_global = 0;
  g.D = x.dim() == 5 ? (int)x.size(2) : 1; g.H = (int)x.size(x.dim() - 2); g.W = (int)x.size(x.dim() - 1);
  c10::hip::HIPGuard guard(x.get_device());
  int tr[4] = {0, 0, 0, 0};
  for (size_t a = 0; a < trim.size(); ++a) tr[a] = (int)trim[a];
  std::vector<int64_t> osz = x.sizes().vec(); osz[1] = 1;
  if (x.dim() == 5) osz[2] -= tr[0] + tr[1];
  TORCH_CHECK(x.dim() == 5 || !(tr[0] | tr[1] | tr[2] | tr[3]), "trim needs a (B,2,D,H,W) input");
  TORCH_CHECK(x.dim() != 5 || osz[2] > 0, "trim leaves no planes");
  Tensor p = at::empty(osz, x.options());
  const size_t bytes = fnx_workspace_bytes(&g, FNX_OP_FLUIDNET);
  Tensor ws = at::empty({(int64_t)bytes}, x.options().dtype(at::kByte));
  check_status(fnx_multiscale_forward_crop(&g, packed.data_ptr(), x.data_ptr<float>(), p.data_ptr<float>(), precision_of(precision_mode),
                                           tr, ws.data_ptr(), bytes, cur_stream(x)));
  return p;
}

// ---- the four pressure nets: the ScaleNet (fnx_cnn.hip, fnx_cnn_train.hip) and the 16-channel bank net, mconf['model'] = 'FluidNet' /
// 'FluidNet3D' (fnx_banknet*.hip), each in 2D and 3D.  One table row per net holds its C entry points under one signature per operation,
// and every operation is one body over a row; the module registers it under the row's names.  A body builds the grid it is given, of
// either dimension, and a grid the net's C ABI refuses (the other dimension, a size it does not take, a bf16 mode in training) gets a
// token tape and workspace, so that the C ABI's text is what is raised.
struct NetApi {
  bool bank;                       // the bank family: its backward takes x, its grids are 3D by their depth and not by the name called
  int ndim;
  const char *net_name, *whole_name;                   // "<net_name>_forward_train", "<whole_name>_backward", ...
  const char* pack_name;
  size_t (*weight_floats)(void);
  size_t (*packed_bytes)(void);
  // inference of the bank nets (the ScaleNet's has one name for both dimensions: scalenet_pack, multiscale_forward, fluidnet_forward)
  int (*pack)(const float*, void*, void*);
  size_t (*ws_bytes)(const FnxGrid*, int);
  int (*forward)(const FnxGrid*, const void*, const float*, float*, int, void*, size_t, void*);
  int (*whole_forward)(const FnxGrid*, const void*, const float*, float, float*, float*, int, void*, size_t, void*);
  // training.  image_sized: the binding checks an image's size (the 3D ScaleNet's entry points take it and refuse a wrong one themselves)
  const char *pack_t_name, *packed_t_what, *blob_note;
  bool image_sized;
  size_t (*packed_t_bytes)(void);
  int (*pack_t)(const float*, void*, void*);
  size_t (*tape_floats)(const FnxGrid*);
  size_t (*backward_ws_bytes)(const FnxGrid*);
  int (*forward_train)(const FnxGrid*, const void*, size_t, const float*, float*, float*, int, void*);
  int (*backward)(const FnxGrid*, const void*, size_t, const float*, const float*, const float*, float*, int, void*, size_t, void*);
  int (*backward_plain)(const FnxGrid*, const void*, size_t, const float*, const float*, const float*, float*, int, void*, size_t, void*);
  size_t (*train_ws_bytes)(const FnxGrid*);
  int (*whole_forward_train)(const FnxGrid*, const void*, size_t, const float*, float, float*, float*, float*, float*, float*, int, void*,
                             size_t, void*);
  int (*whole_backward)(const FnxGrid*, const void*, size_t, const float*, const float*, const float*, const float*, const float*, float*, int,
                        void*, size_t, void*);
};
// A C entry point under the table's signature (g, image, image bytes, [x,] ...): one that takes no image size, no x, or neither
template <auto F, class... A> static int no_size(const FnxGrid* g, const void* image, size_t, A... a) { return F(g, image, a...); }
template <auto F, class... A> static int no_x(const FnxGrid* g, const void* image, size_t n, const float*, A... a) { return F(g, image, n, a...); }
template <auto F, class... A> static int no_size_x(const FnxGrid* g, const void* image, size_t, const float*, A... a) { return F(g, image, a...); }
template <auto F> static size_t floats_of(const FnxGrid* g) { return F(g, nullptr); }      // a tape layout's size query: 0 for a refused grid
template <int IS3D> static size_t scalenet_floats(void) { return fnx_scalenet_weight_floats(IS3D); }
template <int IS3D> static size_t scalenet_bytes(void) { return fnx_scalenet_packed_bytes(IS3D); }
// The rows are positional, one numbered line per group of fields in the struct's order:
//   1: bank, ndim, net_name, whole_name
//   2: pack_name, weight_floats, packed_bytes
//   3: pack, ws_bytes, forward, whole_forward
//   4: pack_t_name, packed_t_what, blob_note, image_sized
//   5: packed_t_bytes, pack_t, tape_floats, backward_ws_bytes
//   6: forward_train, backward, backward_plain
//   7: train_ws_bytes, whole_forward_train, whole_backward
static const NetApi SCALE2D = {
    /* 1 */ false, 2, "multiscale", "fluidnet",
    /* 2 */ "scalenet_pack", scalenet_floats<0>, scalenet_bytes<0>,
    /* 3 */ nullptr, nullptr, nullptr, nullptr,
    /* 4 */ "scalenet_pack_t", "packed_t", "", true,
    /* 5 */ fnx_scalenet_packed_t_bytes, fnx_scalenet_pack_t, floats_of<fnx_multiscale_tape_layout>, fnx_multiscale_backward_ws_bytes,
    /* 6 */ no_size<fnx_multiscale_forward_train>, no_size_x<fnx_multiscale_backward>, no_size_x<fnx_multiscale_backward_plain>,
    /* 7 */ fnx_fluidnet_train_ws_bytes, no_size<fnx_fluidnet_forward_train>, no_size<fnx_fluidnet_backward>};
static const NetApi SCALE3D = {
    /* 1 */ false, 3, "multiscale3d", "fluidnet3d",
    /* 2 */ "scalenet_pack", scalenet_floats<1>, scalenet_bytes<1>,
    /* 3 */ nullptr, nullptr, nullptr, nullptr,
    /* 4 */ "scalenet3d_pack_t", "packed3d_t", " (the 3D net)", false,
    /* 5 */ fnx_scalenet3d_packed_t_bytes, fnx_scalenet3d_pack_t, floats_of<fnx_multiscale3d_tape_layout>, fnx_multiscale3d_backward_ws_bytes,
    /* 6 */ fnx_multiscale3d_forward_train, no_x<fnx_multiscale3d_backward>, no_x<fnx_multiscale3d_backward_plain>,
    /* 7 */ fnx_fluidnet3d_train_ws_bytes, fnx_fluidnet3d_forward_train, fnx_fluidnet3d_backward};
static const NetApi BANK2D = {
    /* 1 */ true, 2, "banknet", "fluidnet_bank",
    /* 2 */ "banknet_pack", fnx_banknet_weight_floats, fnx_banknet_packed_bytes,
    /* 3 */ fnx_banknet_pack, fnx_banknet_ws_bytes, fnx_banknet_forward, fnx_fluidnet_bank_forward,
    /* 4 */ "banknet_pack_t", "packed_t", "", true,
    /* 5 */ fnx_banknet_packed_t_bytes, fnx_banknet_pack_t, floats_of<fnx_banknet_tape_layout>, fnx_banknet_backward_ws_bytes,
    /* 6 */ no_size<fnx_banknet_forward_train>, no_size<fnx_banknet_backward>, nullptr,
    /* 7 */ fnx_fluidnet_bank_train_ws_bytes, no_size<fnx_fluidnet_bank_forward_train>, no_size<fnx_fluidnet_bank_backward>};
static const NetApi BANK3D = {
    /* 1 */ true, 3, "banknet3d", "fluidnet_bank3d",
    /* 2 */ "banknet3d_pack", fnx_banknet3d_weight_floats, fnx_banknet3d_packed_bytes,
    /* 3 */ fnx_banknet3d_pack, fnx_banknet3d_ws_bytes, fnx_banknet3d_forward, fnx_fluidnet_bank3d_forward,
    /* 4 */ "banknet3d_pack_t", "packed_t", "", true,
    /* 5 */ fnx_banknet3d_packed_t_bytes, fnx_banknet3d_pack_t, floats_of<fnx_banknet3d_tape_layout>, fnx_banknet3d_backward_ws_bytes,
    /* 6 */ no_size<fnx_banknet3d_forward_train>, no_size<fnx_banknet3d_backward>, nullptr,
    /* 7 */ fnx_fluidnet_bank3d_train_ws_bytes, no_size<fnx_fluidnet_bank3d_forward_train>, no_size<fnx_fluidnet_bank3d_backward>};
static const NetApi* const NETS[4] = {&SCALE2D, &SCALE3D, &BANK2D, &BANK3D};

// pack (transposed = false; the bank nets') or pack_t
static Tensor net_pack(const NetApi* net, bool transposed, Tensor blob) {
  TORCH_CHECK(blob.is_cuda() && blob.scalar_type() == at::kFloat && blob.is_contiguous(), "weights blob must be a contiguous float32 GPU tensor");
  TORCH_CHECK((size_t)blob.numel() == net->weight_floats(), "weights blob has ", blob.numel(), " floats, expected ", net->weight_floats(),
              transposed ? net->blob_note : "");
  c10::hip::HIPGuard guard(blob.get_device());
  Tensor packed = at::zeros({(int64_t)(transposed ? net->packed_t_bytes : net->packed_bytes)()}, blob.options().dtype(at::kByte));
  check_status((transposed ? net->pack_t : net->pack)(blob.data_ptr<float>(), packed.data_ptr(), cur_stream(blob)));
  return packed;
}

// the forward image of a net's kind, by its size (the packers' images differ in it): inference of the bank nets, and the step's `net`
static void check_forward_image(const NetApi* net, const Tensor& packed, const char* what) {
  TORCH_CHECK(packed.is_cuda() && packed.is_contiguous() && (size_t)packed.nbytes() == net->packed_bytes(),
              what, " must be the ", net->packed_bytes(), "-byte image from ", net->pack_name, " (got ", packed.nbytes(), " bytes)");
}
// In training the forward's weight image and the backward's look alike and differ in size: a swapped pair must not reach the device.  The
// ScaleNet's images are held to the input's device first, in words of their own; the bank nets' forward image is not held to it.
static void check_train_image(const NetApi* net, const Tensor& t, bool transposed, const Tensor& like) {
  // the bank nets' packed: the inference check, size and all, and no word about the device
  if (!transposed && net->bank) return check_forward_image(net, t, "packed");
  const char* what = transposed ? net->packed_t_what : "packed";
  const bool placed = t.is_cuda() && t.is_contiguous() && t.get_device() == like.get_device();
  // the ScaleNet's packed and packed_t, either dimension: the placement first, in words of its own
  if (!net->bank) TORCH_CHECK(placed, what, " must be a contiguous weight image on the input's device");
  // the 3D ScaleNet's two images: their size is the C ABI's to refuse
  if (!net->image_sized) return;
  // the size -- the 2D ScaleNet's two images (placed already) and the bank nets' packed_t, which says placement and size in one text
  const size_t bytes = transposed ? net->packed_t_bytes() : net->packed_bytes();
  TORCH_CHECK(placed && (size_t)t.nbytes() == bytes, what, " must be the ", bytes, "-byte image from ", transposed ? net->pack_t_name : net->pack_name,
              net->bank ? " on the input's device" : "", " (got ", t.nbytes(), " bytes)");
}

static Tensor bank_forward(const NetApi* net, Tensor packed, Tensor x, const std::string& precision_mode) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.is_contiguous(), "x must be a contiguous float32 GPU tensor");
  TORCH_CHECK((x.dim() == 4 || x.dim() == 5) && x.size(1) == 2, "x must be (B,2,H,W) or (B,2,D,H,W)");
  check_forward_image(net, packed, "packed");
  FnxGrid g{}; g.B = (int)x.size(0); g.D = x.dim() == 5 ? (int)x.size(2) : 1; g.H = (int)x.size(x.dim() - 2); g.W = (int)x.size(x.dim() - 1);
  g.is3D = g.D > 1;
  c10::hip::HIPGuard guard(x.get_device());
  std::vector<int64_t> osz = x.sizes().vec(); osz[1] = 1;
  Tensor p = at::empty(osz, x.options());
  const size_t bytes = std::max<size_t>(net->ws_bytes(&g, 0), 256);
  Tensor ws = at::empty({(int64_t)bytes}, x.options().dtype(at::kByte));
  check_status(net->forward(&g, packed.data_ptr(), x.data_ptr<float>(), p.data_ptr<float>(), precision_of(precision_mode), ws.data_ptr(), bytes,
                           cur_stream(x)));
  return p;
}

// FluidNet.forward of any model.  net == nullptr: the ScaleNet of either dimension, whose image has no size of its own to check
static std::vector<Tensor> whole_forward(const NetApi* net, Tensor packed, Tensor input, double normalize_threshold,
                                         const std::string& precision_mode) {
  check_field(input, "input");
  TORCH_CHECK(input.size(1) == 5 || input.size(1) == 6, "input must have 5 (2D) or 6 (3D) channels [p, U, flags, density]");
  if (net) check_forward_image(net, packed, "packed");
  const bool is3D = input.size(1) == 6;
  FnxGrid g{}; g.B = (int)input.size(0); g.D = (int)input.size(2); g.H = (int)input.size(3); g.W = (int)input.size(4);
  g.is3D = is3D;
  c10::hip::HIPGuard guard(input.get_device());
  Tensor p = at::empty({g.B, 1, g.D, g.H, g.W}, input.options());
  Tensor U = at::empty({g.B, is3D ? 3 : 2, g.D, g.H, g.W}, input.options());
  const size_t bytes = net ? std::max<size_t>(net->ws_bytes(&g, 1), 256) : fnx_workspace_bytes(&g, FNX_OP_FLUIDNET);
  Tensor ws = at::empty({(int64_t)bytes}, input.options().dtype(at::kByte));
  check_status((net ? net->whole_forward : fnx_fluidnet_forward)(&g, packed.data_ptr(), input.data_ptr<float>(), (float)normalize_threshold,
                                                                 p.data_ptr<float>(), U.data_ptr<float>(), precision_of(precision_mode),
                                                                 ws.data_ptr(), bytes, cur_stream(input)));
  return {p, U};
}

// ---- training: the nets' backward passes, the scenes and the loss (fnx_scenes.hip) ---------------------------------------------------
static FnxGrid make_grid(int64_t B, int64_t D, int64_t H, int64_t W, bool is3D) {
  FnxGrid g{}; g.B = (int)B; g.D = (int)D; g.H = (int)H; g.W = (int)W; g.is3D = is3D;
  return g;
}
// a (B,C,H,W) or (B,C,D,H,W) tensor of the net: 3D if it has more than one plane
static FnxGrid grid_of_net_tensor(const Tensor& x, const char* what) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.is_contiguous(), what, " must be a contiguous float32 GPU tensor");
  TORCH_CHECK(x.dim() == 4 || x.dim() == 5, what, " must be (B,C,H,W) or (B,C,D,H,W)");
  const int64_t D = x.dim() == 5 ? x.size(2) : 1;
  return make_grid(x.size(0), D, x.size(x.dim() - 2), x.size(x.dim() - 1), D > 1);
}
static void check_tape(const Tensor& tape, size_t floats) {
  TORCH_CHECK(tape.is_cuda() && tape.scalar_type() == at::kFloat && tape.is_contiguous(), "tape must be a contiguous float32 GPU tensor");
  TORCH_CHECK(!floats || (size_t)tape.numel() == floats, "tape has ", tape.numel(), " floats, not the layout of this grid");
}
// a byte workspace of the net's size query for a grid whose tape has `floats` floats; a refused grid's token one is never read
static Tensor train_ws(size_t floats, size_t (*bytes_of)(const FnxGrid*), const FnxGrid& g, const Tensor& like) {
  return at::empty({(int64_t)std::max<size_t>(floats ? bytes_of(&g) : 0, 256)}, like.options().dtype(at::kByte));
}

// A tape layout of the C ABI -> (name, offset, C, H, W) per tape entry for FnxTapeEntry, (name, offset, C, D, H, W) for FnxTapeEntry3D
template <typename Entry>
static std::vector<py::tuple> tape_tuples(const FnxGrid& g, int n, size_t (*layout)(const FnxGrid*, Entry*)) {
  std::vector<Entry> e(n);
  if (layout(&g, e.data()) == 0) check_status(FNX_EINVAL);
  std::vector<py::tuple> out;
  for (const Entry& t : e) {
    if constexpr (std::is_same_v<Entry, FnxTapeEntry3D>) out.push_back(py::make_tuple(std::string(t.name), (int64_t)t.offset, t.C, t.D, t.H, t.W));
    else out.push_back(py::make_tuple(std::string(t.name), (int64_t)t.offset, t.C, t.H, t.W));
  }
  return out;
}

// gd (B,1,Do,Ho,Wo) -> gs (B,1,Di,Hi,Wi): fnx_trilinear_upsample_backward
Tensor trilinear_upsample_backward(Tensor gd, std::vector<int64_t> size) {
  TORCH_CHECK(gd.is_cuda() && gd.scalar_type() == at::kFloat && gd.is_contiguous() && gd.dim() == 5 && gd.size(1) == 1,
              "grad_dst must be a contiguous float32 GPU tensor (B,1,Do,Ho,Wo)");
  TORCH_CHECK(size.size() == 3 && size[0] >= 1 && size[1] >= 1 && size[2] >= 1, "size: the source's (Di,Hi,Wi)");
  c10::hip::HIPGuard guard(gd.get_device());
  Tensor gs = at::empty({gd.size(0), 1, size[0], size[1], size[2]}, gd.options());
  check_status(fnx_trilinear_upsample_backward((int)gd.size(0), (int)size[0], (int)size[1], (int)size[2], (int)gd.size(2), (int)gd.size(3),
                                               (int)gd.size(4), gd.data_ptr<float>(), gs.data_ptr<float>(), cur_stream(gd)));
  return gs;
}

// x (B,2,[D,]H,W) -> p, tape
static std::vector<Tensor> net_forward_train(const NetApi* net, Tensor packed, Tensor x, const std::string& precision_mode) {
  const FnxGrid g = grid_of_net_tensor(x, "x");
  TORCH_CHECK(x.size(1) == 2, "x must have 2 channels");
  check_train_image(net, packed, false, x);
  c10::hip::HIPGuard guard(x.get_device());
  std::vector<int64_t> osz = x.sizes().vec(); osz[1] = 1;
  Tensor p = at::empty(osz, x.options());
  const size_t floats = net->tape_floats(&g);
  Tensor tape = at::empty({(int64_t)(floats ? floats : 1)}, x.options());
  check_status(net->forward_train(&g, packed.data_ptr(), (size_t)packed.nbytes(), x.data_ptr<float>(), p.data_ptr<float>(),
                                  tape.data_ptr<float>(), precision_of(precision_mode), cur_stream(x)));
  return {p, tape};
}

// grad_p (B,1,[D,]H,W), the forward's tape and, for the bank nets, its x -> the gradient in the blob's layout.  plain: the ScaleNet's plain
// weight-gradient kernel for every layer (fnx_multiscale*_backward_plain), a cross-check and not a training path
static Tensor net_backward(const NetApi* net, bool plain, Tensor packed_t, const Tensor* x, Tensor grad_p, Tensor tape,
                           const std::string& precision_mode) {
  const FnxGrid g = grid_of_net_tensor(grad_p, "grad_p");
  if (x) {
    grid_of_net_tensor(*x, "x");
    TORCH_CHECK(grad_p.size(1) == 1 && x->size(1) == 2 && x->dim() == grad_p.dim() && x->size(0) == grad_p.size(0) &&
                x->numel() == 2 * grad_p.numel() && x->size(x->dim() - 2) == grad_p.size(x->dim() - 2) &&
                x->size(x->dim() - 1) == grad_p.size(x->dim() - 1),
                "grad_p (1 channel) and x (2 channels) must share their grid");
  }
  check_train_image(net, packed_t, true, grad_p);
  if (!x) TORCH_CHECK(grad_p.size(1) == 1, "grad_p must have 1 channel");
  const size_t floats = net->tape_floats(&g);
  check_tape(tape, floats);
  c10::hip::HIPGuard guard(grad_p.get_device());
  Tensor grad = at::empty({(int64_t)net->weight_floats()}, grad_p.options());
  Tensor ws = train_ws(floats, net->backward_ws_bytes, g, grad_p);
  check_status((plain ? net->backward_plain : net->backward)(&g, packed_t.data_ptr(), (size_t)packed_t.nbytes(), x ? x->data_ptr<float>() : nullptr,
                                                             grad_p.data_ptr<float>(), tape.data_ptr<float>(), grad.data_ptr<float>(),
                                                             precision_of(precision_mode), ws.data_ptr(), (size_t)ws.nbytes(),
                                                             cur_stream(grad_p)));
  return grad;
}
static Tensor scalenet_backward(const NetApi* net, Tensor packed_t, Tensor grad_p, Tensor tape, const std::string& precision_mode) {
  return net_backward(net, false, packed_t, nullptr, grad_p, tape, precision_mode);
}
static Tensor scalenet_backward_plain(const NetApi* net, Tensor packed_t, Tensor grad_p, Tensor tape, const std::string& precision_mode) {
  return net_backward(net, true, packed_t, nullptr, grad_p, tape, precision_mode);
}
static Tensor bank_backward(const NetApi* net, Tensor packed_t, Tensor x, Tensor grad_p, Tensor tape, const std::string& precision_mode) {
  return net_backward(net, false, packed_t, &x, grad_p, tape, precision_mode);
}

// input (B,5|6,D,H,W) = [p, U, flags, density] -> p, U, tape, s (B), flags (B,1,D,H,W)
static std::vector<Tensor> whole_forward_train(const NetApi* net, Tensor packed, Tensor input, double normalize_threshold,
                                               const std::string& precision_mode) {
  check_field(input, "input");
  TORCH_CHECK(input.size(1) == 5 || input.size(1) == 6, "input must have 5 (2D) or 6 (3D) channels [p, U, flags, density]");
  const FnxGrid g = make_grid(input.size(0), input.size(2), input.size(3), input.size(4), input.size(1) == 6);
  check_train_image(net, packed, false, input);
  c10::hip::HIPGuard guard(input.get_device());
  Tensor p = at::empty({g.B, 1, g.D, g.H, g.W}, input.options());
  Tensor U = at::empty({g.B, g.is3D ? 3 : 2, g.D, g.H, g.W}, input.options());
  Tensor flags = at::empty({g.B, 1, g.D, g.H, g.W}, input.options());
  Tensor scale = at::empty({g.B}, input.options());
  const size_t floats = net->tape_floats(&g);
  Tensor tape = at::empty({(int64_t)(floats ? floats : 1)}, input.options());
  Tensor ws = train_ws(floats, net->train_ws_bytes, g, input);
  check_status(net->whole_forward_train(&g, packed.data_ptr(), (size_t)packed.nbytes(), input.data_ptr<float>(), (float)normalize_threshold,
                                        p.data_ptr<float>(), U.data_ptr<float>(), flags.data_ptr<float>(), scale.data_ptr<float>(),
                                        tape.data_ptr<float>(), precision_of(precision_mode), ws.data_ptr(), (size_t)ws.nbytes(),
                                        cur_stream(input)));
  return {p, U, tape, scale, flags};
}

// grad_p (B,1,D,H,W), grad_U (B,2|3,D,H,W), flags (B,1,D,H,W) and scale (B) of the forward -> the gradient in the blob's layout
static Tensor whole_backward(const NetApi* net, Tensor packed_t, Tensor flags, Tensor scale, Tensor grad_p, Tensor grad_U, Tensor tape,
                             const std::string& precision_mode) {
  check_field(grad_p, "grad_p"); check_field(grad_U, "grad_U"); check_field(flags, "flags");
  const int64_t nc = net->ndim;
  TORCH_CHECK(grad_p.size(1) == 1 && grad_U.size(1) == nc && flags.size(1) == 1, "grad_p and flags must have 1 channel, grad_U ", nc);
  TORCH_CHECK(grad_U.size(0) == grad_p.size(0) && grad_U.size(2) == grad_p.size(2) && grad_U.size(3) == grad_p.size(3) &&
              grad_U.size(4) == grad_p.size(4) && flags.sizes() == grad_p.sizes(), "grad_p, grad_U and flags must share their grid");
  const FnxGrid g = make_grid(grad_p.size(0), grad_p.size(2), grad_p.size(3), grad_p.size(4), net->bank ? grad_p.size(2) > 1 : nc == 3);
  check_train_image(net, packed_t, true, grad_p);
  TORCH_CHECK(scale.is_cuda() && scale.scalar_type() == at::kFloat && scale.is_contiguous() && scale.numel() == g.B, "scale must hold B floats on the GPU");
  const size_t floats = net->tape_floats(&g);
  check_tape(tape, floats);
  c10::hip::HIPGuard guard(grad_p.get_device());
  Tensor grad = at::empty({(int64_t)net->weight_floats()}, grad_p.options());
  Tensor ws = train_ws(floats, net->train_ws_bytes, g, grad_p);
  check_status(net->whole_backward(&g, packed_t.data_ptr(), (size_t)packed_t.nbytes(), flags.data_ptr<float>(), scale.data_ptr<float>(),
                                   grad_p.data_ptr<float>(), grad_U.data_ptr<float>(), tape.data_ptr<float>(), grad.data_ptr<float>(),
                                   precision_of(precision_mode), ws.data_ptr(), (size_t)ws.nbytes(), cur_stream(grad_p)));
  return grad;
}

// the grid of B scenes: 3D if it has more than one plane, whichever name was called
static FnxGrid scene_grid(const Tensor& ids, int64_t D, int64_t H, int64_t W) {
  TORCH_CHECK(ids.is_cuda() && ids.scalar_type() == at::kInt && ids.dim() == 1 && ids.is_contiguous() && ids.numel() >= 1,
              "scene_ids must be a contiguous int32 GPU tensor (B)");
  TORCH_CHECK(D >= 1 && H >= 1 && W >= 1, "the scenes' depth, H and W must be positive");
  return make_grid(ids.numel(), D, H, W, D > 1);
}
// -> flags (B,1,D,H,W)
Tensor scene_obstacles(bool is3d, Tensor scene_ids, int64_t D, int64_t H, int64_t W, int64_t seed, int n_min, int n_max, double centre_min,
                       double centre_max, double size_min, double size_max) {
  const FnxGrid g = scene_grid(scene_ids, D, H, W);
  FnxSceneParams prm{};
  prm.seed = (unsigned)seed; prm.n_min = n_min; prm.n_max = n_max;
  prm.centre_min = (float)centre_min; prm.centre_max = (float)centre_max; prm.size_min = (float)size_min; prm.size_max = (float)size_max;
  c10::hip::HIPGuard guard(scene_ids.get_device());
  Tensor flags = at::empty({g.B, 1, D, H, W}, scene_ids.options().dtype(at::kFloat));
  check_status((is3d ? fnx_scene_obstacles3d : fnx_scene_obstacles)(&g, &prm, scene_ids.data_ptr<int>(), flags.data_ptr<float>(), cur_stream(scene_ids)));
  return flags;
}
// -> U (B,2|3,D,H,W), density (B,1,D,H,W) or None
std::vector<Tensor> scene_turbulence(bool is3d, Tensor scene_ids, int64_t D, int64_t H, int64_t W, int64_t seed, int octaves, double wavelength,
                                     double amplitude, double density_scale, bool with_density) {
  const FnxGrid g = scene_grid(scene_ids, D, H, W);
  FnxSceneParams prm{};
  prm.seed = (unsigned)seed; prm.octaves = octaves; prm.wavelength = (float)wavelength; prm.amplitude = (float)amplitude;
  prm.density_scale = (float)density_scale;
  c10::hip::HIPGuard guard(scene_ids.get_device());
  Tensor U = at::empty({g.B, is3d ? 3 : 2, D, H, W}, scene_ids.options().dtype(at::kFloat));
  Tensor rho = with_density ? at::empty({g.B, 1, D, H, W}, U.options()) : Tensor();
  check_status((is3d ? fnx_scene_turbulence3d : fnx_scene_turbulence)(&g, &prm, scene_ids.data_ptr<int>(), U.data_ptr<float>(),
                                                                     with_density ? rho.data_ptr<float>() : nullptr, cur_stream(scene_ids)));
  return {U, rho};
}
// fluid_net_train.py:276-285 for out_p (B,1,D,H,W), out_U (B,2|3,D,H,W) -> [terms (5: pL2, divL2, pL1, divL1 unweighted, total) or None,
// grad_p or None, grad_U or None]; upstream: a one-element GPU tensor (the gradient of what the total feeds) or None for the terms alone
std::vector<Tensor> train_loss(bool is3d, Tensor out_p, Tensor out_U, Tensor flags, c10::optional<Tensor> target_p, std::vector<double> lambdas,
                               c10::optional<Tensor> upstream, bool terms) {
  check_field(out_U, "out_U");
  TORCH_CHECK(lambdas.size() == 4, "lambdas must be (pL2, divL2, pL1, divL1)");
  TORCH_CHECK(out_U.size(1) == 2 || out_U.size(1) == 3, "out_U must have 2 or 3 channels");
  FnxGrid g = grid_of(flags, out_U.size(1) == 3, nullptr);
  check_scalar(out_p, g, "out_p");
  TORCH_CHECK(out_U.size(0) == g.B && out_U.size(2) == g.D && out_U.size(3) == g.H && out_U.size(4) == g.W, "Size mismatch");
  const bool has_t = target_p.has_value() && target_p->defined();
  if (has_t) check_scalar(*target_p, g, "target_p");
  const bool grads = upstream.has_value() && upstream->defined();
  if (grads)
    TORCH_CHECK(upstream->is_cuda() && upstream->scalar_type() == at::kFloat && upstream->numel() == 1 && upstream->get_device() == out_p.get_device(),
                "upstream must be one float32 on the GPU");
  c10::hip::HIPGuard guard(out_p.get_device());
  const float lam[4] = {(float)lambdas[0], (float)lambdas[1], (float)lambdas[2], (float)lambdas[3]};
  Tensor t, gp, gU, ws;
  size_t bytes = 0;
  if (terms) {
    t = at::empty({5}, out_p.options());
    bytes = (is3d ? fnx_train_loss3d_ws_bytes : fnx_train_loss_ws_bytes)(&g);       // 0 for a grid the call below refuses
    ws = at::empty({(int64_t)(bytes ? bytes : 1)}, out_p.options().dtype(at::kByte));
  }
  if (grads) { gp = at::empty_like(out_p); gU = at::empty_like(out_U); }
  check_status((is3d ? fnx_train_loss3d : fnx_train_loss)(
      &g, out_p.data_ptr<float>(), out_U.data_ptr<float>(), flags.data_ptr<float>(), has_t ? target_p->data_ptr<float>() : nullptr, lam,
      grads ? upstream->data_ptr<float>() : nullptr, terms ? t.data_ptr<float>() : nullptr, grads ? gp.data_ptr<float>() : nullptr,
      grads ? gU.data_ptr<float>() : nullptr, terms ? ws.data_ptr() : nullptr, bytes, cur_stream(out_p)));
  return {t, gp, gU};
}

// an optional field of a step's state: its device pointer, or nullptr for None
static float* opt_field(const FnxGrid& g, c10::optional<Tensor>& t, bool vel, const char* name) {
  if (!t.has_value() || !t->defined()) return nullptr;
  if (vel) check_vel(*t, g, name); else check_scalar(*t, g, name);
  return t->data_ptr<float>();
}

// the fields every state has; the net, the class map and flags_stick are the caller's to add
static FnxState make_state(const FnxGrid& g, Tensor& p, Tensor& U, Tensor& flags, c10::optional<Tensor>& density,
                           c10::optional<Tensor>& UBC, c10::optional<Tensor>& UBCInvMask,
                           c10::optional<Tensor>& densityBC, c10::optional<Tensor>& densityBCInvMask) {
  FnxState st{};
  st.p = p.data_ptr<float>(); st.U = U.data_ptr<float>(); st.flags = flags.data_ptr<float>();
  st.density = opt_field(g, density, false, "density");
  st.UBC = opt_field(g, UBC, true, "UBC"); st.UBCInvMask = opt_field(g, UBCInvMask, true, "UBCInvMask");
  st.densityBC = opt_field(g, densityBC, false, "densityBC"); st.densityBCInvMask = opt_field(g, densityBCInvMask, false, "densityBCInvMask");
  return st;
}

// the parameters every caller of a step or of its stage sets (gravity_vec: x, y, z, checked by the caller); the rest start at zero
static FnxStepParams step_params(double dt, double buoyancy_scale, const std::vector<double>& gravity_vec, double operating_density) {
  FnxStepParams prm{};
  prm.dt = (float)dt; prm.buoyancy_scale = (float)buoyancy_scale;
  for (int a = 0; a < 3; ++a) prm.gravity_vec[a] = (float)gravity_vec[a];
  prm.operating_density = (float)operating_density;
  return prm;
}

// one whole step of lib/simulate.py:28-171, in place on p, U, density
void simulate_step_(Tensor p, Tensor U, Tensor flags, c10::optional<Tensor> density, c10::optional<Tensor> UBC,
                    c10::optional<Tensor> UBCInvMask, c10::optional<Tensor> densityBC,
                    c10::optional<Tensor> densityBCInvMask, c10::optional<Tensor> net, double dt,
                    double maccormack_strength, bool sample_outside_fluid, double buoyancy_scale,
                    std::vector<double> gravity_vec, double operating_density, double p_tol, int jacobi_iter,
                    const std::string method, double normalize_threshold, c10::optional<Tensor> workspace,
                    int static_flags, const Geom* geom, const std::string& precision_mode, double viscosity,
                    double gravity_scale, bool correct_scalar, int periodic, c10::optional<Tensor> flags_stick, double pcg_tol,
                    int pcg_iter, double vorticity_confinement, bool pcg_warm, const std::string& net_kind) {
  check_field(U, "U");
  FnxGrid g = grid_of(flags, U.size(1) == 3, geom);
  check_vel(U, g, "U"); check_scalar(p, g, "p");
  TORCH_CHECK(viscosity >= 0, "Viscosity must be positive");
  TORCH_CHECK(method == "jacobi" || method == "convnet" || method == "pcg" || method == "hybrid",
              "Simulation method not supported. Choose convnet, jacobi, pcg or hybrid.");
  TORCH_CHECK(gravity_vec.size() == 3, "gravityVec needs x, y, z");
  FnxStepParams prm = step_params(dt, buoyancy_scale, gravity_vec, operating_density);
  prm.maccormack_strength = (float)maccormack_strength; prm.sample_outside_fluid = sample_outside_fluid;
  prm.p_tol = (float)p_tol; prm.jacobi_iter = jacobi_iter;
  // 'hybrid': the solve started from the net's pressure; 'pcg' with pcg_warm: from p as it stands (the previous step's)
  prm.method = method == "convnet" ? 1 : (method == "hybrid" ? 3 : (method == "pcg" ? (pcg_warm ? 4 : 2) : 0)); prm.normalize_threshold = (float)normalize_threshold;
  prm.pcg_tol = (float)pcg_tol; prm.pcg_iter = pcg_iter;
  prm.precision_mode = precision_of(precision_mode);
  prm.viscosity = (float)viscosity; prm.gravity_scale = (float)gravity_scale; prm.correct_scalar = correct_scalar ? 1 : 0;
  prm.periodic = periodic;
  prm.vorticity_confinement = (float)vorticity_confinement;
  FnxState st = make_state(g, p, U, flags, density, UBC, UBCInvMask, densityBC, densityBCInvMask);
  st.net = (net.has_value() && net->defined()) ? net->data_ptr() : nullptr;
  // the image against its kind, by size (the three packers' images differ in it), as bank_forward checks its own (the nets' table)
  TORCH_CHECK(net_kind == "scalenet" || net_kind == "bank" || net_kind == "bank3d", "net_kind: 'scalenet', 'bank' or 'bank3d' (got '", net_kind, "')");
  const int kind = net_kind == "bank" ? FNX_NET_BANK : (net_kind == "bank3d" ? FNX_NET_BANK3D : FNX_NET_SCALENET);   // (bank3d: refused by the C ABI)
  if (st.net && (prm.method == 1 || prm.method == 3)) {
    if (kind == FNX_NET_SCALENET) check_forward_image(g.is3D ? &SCALE3D : &SCALE2D, *net, "net");
    else check_forward_image(kind == FNX_NET_BANK ? &BANK2D : &BANK3D, *net, "packed");
  }
  st.flags_stick = opt_field(g, flags_stick, false, "flags_stick");
  c10::hip::HIPGuard guard(flags.get_device());
  const size_t bytes = fnx_workspace_bytes(&g, FNX_OP_STEP);
  Tensor ws;
  const bool given = workspace.has_value() && workspace->defined() && (size_t)workspace->numel() * workspace->element_size() >= bytes;
  if (given) ws = *workspace;
  else ws = at::empty({(int64_t)bytes}, flags.options().dtype(at::kByte));
  // the mask lives in the workspace: only a caller-owned workspace carries it from one step to the next
  prm.static_flags = given ? static_flags : 0;      // (promises about the previous step need a caller-owned workspace)
  check_status(fnx_simulate_step_net(&g, &prm, &st, kind, ws.data_ptr(), (size_t)ws.numel() * ws.element_size(), cur_stream(U)));
  wrote(p); wrote(U); wrote(density);
}

// ---- native z-slab driver (fnx_slab_*): communicators and the per-rank driver object ---------------------------
struct PyLoopbackGroup {
  void* g = nullptr; int nranks;
  explicit PyLoopbackGroup(int n) : nranks(n) { check_status(fnx_slab_loopback_group(&g, n)); }
  ~PyLoopbackGroup() { fnx_slab_loopback_group_free(g); }
};
struct PyPeer {                                // a rank's peer-store region (fnx_slab_peer_create)
  void* p = nullptr;
  std::string handle;
  PyPeer(int rank, int nranks, int64_t mailbox_bytes) {
    char h[FNX_PEER_HANDLE_BYTES];
    check_status(fnx_slab_peer_create(&p, rank, nranks, (size_t)mailbox_bytes, h));
    handle.assign(h, FNX_PEER_HANDLE_BYTES);
  }
  ~PyPeer() { fnx_slab_peer_free(p); }
};
struct PySlabComm {
  FnxSlabComm c{};
  std::shared_ptr<PyLoopbackGroup> keep;      // a loopback comm keeps its group alive
  std::shared_ptr<PyPeer> keep_peer;          // a peer-store comm its region
  ~PySlabComm() { fnx_slab_comm_free(&c); }
};
py::bytes slab_rccl_unique_id() {
  char id[128];
  check_status(fnx_slab_rccl_unique_id(id));
  return py::bytes(id, 128);
}
std::shared_ptr<PySlabComm> slab_comm_rccl(int rank, int nranks, const std::string& unique_id) {
  TORCH_CHECK(unique_id.size() == 128, "the RCCL unique id has 128 bytes");
  auto c = std::make_shared<PySlabComm>();
  py::gil_scoped_release nogil;               // ncclCommInitRank blocks until every rank has arrived
  check_status(fnx_slab_comm_rccl(&c->c, rank, nranks, unique_id.data()));
  return c;
}
std::shared_ptr<PySlabComm> slab_comm_loopback(std::shared_ptr<PyLoopbackGroup> group, int rank) {
  auto c = std::make_shared<PySlabComm>();
  check_status(fnx_slab_comm_loopback(&c->c, group->g, rank));
  c->keep = group;
  return c;
}
struct PySlab {
  FnxSlab* s = nullptr;
  FnxSlabConfig cfg{};
  std::shared_ptr<PySlabComm> comm;
  PySlab(int B, int H, int W, int D_global, int rank, int nranks, int halo, int sweeps_per_exchange, bool static_flags,
         int cfl_check_every, std::shared_ptr<PySlabComm> comm_, const std::string& schedule, const std::string& method, const std::string& direct_sends) : comm(comm_) {
    cfg.B = B; cfg.H = H; cfg.W = W; cfg.D_global = D_global; cfg.rank = rank; cfg.nranks = nranks; cfg.halo = halo;
    cfg.sweeps_per_exchange = sweeps_per_exchange; cfg.static_flags = static_flags ? 1 : 0; cfg.cfl_check_every = cfl_check_every;
    TORCH_CHECK(schedule == "deep_first" || schedule == "edge_first" || schedule == "last_pass" || schedule == "deep_beside",
                "unknown z-slab schedule '", schedule, "'");
    cfg.schedule = schedule == "deep_first" ? FNX_SLAB_DEEP_FIRST : (schedule == "edge_first" ? FNX_SLAB_EDGE_FIRST :
                   (schedule == "deep_beside" ? FNX_SLAB_DEEP_BESIDE : FNX_SLAB_LAST_PASS));
    TORCH_CHECK(method == "jacobi" || method == "convnet", "unknown z-slab method '", method, "'");
    cfg.method = method == "convnet" ? 1 : 0;
    TORCH_CHECK(direct_sends == "auto" || direct_sends == "never" || direct_sends == "always", "direct_sends: 'auto', 'never' or 'always'");
    cfg.direct_sends = direct_sends == "auto" ? 0 : (direct_sends == "never" ? 1 : 2);
    check_status(fnx_slab_create(&s, &cfg, comm ? &comm->c : nullptr));
  }
  ~PySlab() { fnx_slab_destroy(s); }
  std::vector<int> layout() const {
    int o, l, h, z;
    check_status(fnx_slab_layout(&cfg, &o, &l, &h, &z));
    return {o, l, h, z};
  }
  int64_t workspace_bytes() const { return (int64_t)fnx_slab_workspace_bytes(&cfg); }
  void stats_enable(bool on) { check_status(fnx_slab_stats_enable(s, on ? 1 : 0)); }
  py::dict stats_read() {
    FnxSlabStats t{};
    check_status(fnx_slab_stats_read(s, &t));
    py::dict d;
    d["bytes_per_neighbour"] = t.bytes_per_neighbour; d["wait_ms"] = t.wait_ms; d["exchanges"] = (int64_t)t.exchanges;
    return d;
  }
  void step(Tensor p, Tensor U, Tensor flags, Tensor density, c10::optional<Tensor> UBC, c10::optional<Tensor> UBCInvMask,
            c10::optional<Tensor> densityBC, c10::optional<Tensor> densityBCInvMask, double dt, double maccormack_strength,
            bool sample_outside_fluid, double buoyancy_scale, std::vector<double> gravity_vec, double operating_density,
            double p_tol, int jacobi_iter, Tensor workspace, c10::optional<Tensor> net, const std::string& precision_mode,
            double normalize_threshold, const std::string& method, double viscosity) {
    check_field(U, "U");
    Geom none;
    FnxGrid g = grid_of(flags, true, &none);
    check_vel(U, g, "U"); check_scalar(p, g, "p"); check_scalar(density, g, "density");
    const std::vector<int> l = layout();
    TORCH_CHECK(g.B == cfg.B && g.H == cfg.H && g.W == cfg.W && g.D == l[0] + l[1] + l[2], "the tensors are not this rank's slab (",
                cfg.B, " x ", l[0] + l[1] + l[2], " x ", cfg.H, " x ", cfg.W, " with ghost planes)");
    TORCH_CHECK(gravity_vec.size() == 3, "gravityVec needs x, y, z");
    TORCH_CHECK(workspace.is_cuda() && workspace.is_contiguous(), "workspace must be a contiguous GPU tensor");
    FnxStepParams prm = step_params(dt, buoyancy_scale, gravity_vec, operating_density);
    prm.maccormack_strength = (float)maccormack_strength; prm.sample_outside_fluid = sample_outside_fluid;
    prm.p_tol = (float)p_tol; prm.jacobi_iter = jacobi_iter; prm.method = 0;
    const bool cnn = net.has_value() && net->defined();
    if (cnn) {                                       // the CNN projection (a driver created with method = "convnet")
      TORCH_CHECK(net->is_cuda() && net->is_contiguous(), "net: the packed weights (scalenet_pack) on the GPU");
      prm.method = 1; prm.precision_mode = precision_of(precision_mode); prm.normalize_threshold = (float)normalize_threshold;
    }
    TORCH_CHECK(method == "auto" || method == "jacobi" || method == "convnet" || method == "pcg", "unknown z-slab step method '", method, "'");
    if (method == "pcg") prm.method = 2;           // refused by fnx_slab_step (single-domain only)
    prm.viscosity = (float)viscosity;              // mconf['viscosity'] > 0: refused by fnx_slab_step as well (single-domain only)
    c10::optional<Tensor> rho(density);
    FnxState st = make_state(g, p, U, flags, rho, UBC, UBCInvMask, densityBC, densityBCInvMask);
    if (cnn) st.net = net->data_ptr();
    c10::hip::HIPGuard guard(flags.get_device());
    check_status(fnx_slab_step(s, &prm, &st, workspace.data_ptr(), (size_t)workspace.numel() * workspace.element_size(), cur_stream(U)));
  }
};

// `nsweeps` more sweeps on an existing pressure field (in place) -- used by the z-slab driver
void jacobi_sweeps_(Tensor flags, Tensor div, Tensor p, bool is3D, int nsweeps, c10::optional<Tensor> workspace,
                    bool reuse_mask, const Geom* geom, bool from_zero) {
  FnxGrid g = grid_of(flags, is3D, geom);
  check_scalar(div, g, "div"); check_scalar(p, g, "p");
  c10::hip::HIPGuard guard(flags.get_device());
  const size_t bytes = fnx_workspace_bytes(&g, FNX_OP_JACOBI);
  Tensor ws;
  if (workspace.has_value() && workspace->defined() && (size_t)workspace->numel() * workspace->element_size() >= bytes) ws = *workspace;
  else { ws = at::empty({(int64_t)bytes}, flags.options().dtype(at::kByte)); reuse_mask = false; }
  check_status(fnx_jacobi_sweeps_ex(&g, flags.data_ptr<float>(), div.data_ptr<float>(), p.data_ptr<float>(), nsweeps,
                                    ws.data_ptr(), (size_t)ws.numel() * ws.element_size(), (reuse_mask ? 1 : 0) | (from_zero ? 2 : 0),
                                    cur_stream(flags)));
  wrote(p);
}

// one pass (1|2 sweeps) p_in -> p_out on the output planes [k_begin, k_end) -- z-slab driver (overlap with exchange)
void jacobi_pass_(Tensor flags, Tensor div, c10::optional<Tensor> p_in_opt, Tensor p_out, int nsweeps, int k_begin,
                  int k_end, Tensor workspace, bool reuse_mask, int k_begin2, const Geom* geom, int layout) {
  FnxGrid g = grid_of(flags, true, geom);
  const bool zero = !(p_in_opt.has_value() && p_in_opt->defined());     // None: p = 0 (first pass of a solve)
  Tensor p_in = zero ? p_out : *p_in_opt;
  check_scalar(div, g, "div"); check_scalar(p_in, g, "p_in"); check_scalar(p_out, g, "p_out");
  c10::hip::HIPGuard guard(flags.get_device());
  check_status(fnx_jacobi_pass_layout(&g, flags.data_ptr<float>(), div.data_ptr<float>(), zero ? nullptr : p_in.data_ptr<float>(),
                                      p_out.data_ptr<float>(), nsweeps, k_begin, k_end, k_begin2, layout, workspace.data_ptr(),
                                      (size_t)workspace.numel() * workspace.element_size(), reuse_mask ? 1 : 0, cur_stream(flags)));
  wrote(p_out);
}

// may two-sweep passes on this 3D grid hand each other the pressure in the row-quad layout (jacobi_pass_'s `layout`)?
bool jacobi_quad_ok(int B, int D, int H, int W) {
  FnxGrid g{B, D, H, W, 1, 0, 0, 0};
  return fnx_jacobi_quad_ok(&g) != 0;
}

// fnx_jacobi_pass_mirror: `mirror` / `mirror2` are flat fp32 tensors of B * planes * H * W floats (sample stride planes * H * W)
void jacobi_pass_mirror_(Tensor flags, Tensor div, Tensor p_in, Tensor p_out, int k_begin, int k_end, Tensor workspace, bool reuse_mask,
                         Tensor mirror, int k_first, int planes, int k_begin2, c10::optional<Tensor> mirror2, int k_first2, const Geom* geom,
                         int layout) {
  FnxGrid g = grid_of(flags, true, geom);
  check_scalar(div, g, "div"); check_scalar(p_in, g, "p_in"); check_scalar(p_out, g, "p_out");
  const int64_t need = (int64_t)g.B * planes * g.H * g.W;
  auto chk = [&](const Tensor& t) { TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == at::kFloat && t.numel() >= need, "mirror: a contiguous fp32 GPU tensor of B * planes * H * W floats"); };
  chk(mirror);
  FnxPlaneMirror m{};
  m.out[0][0] = mirror.data_ptr<float>(); m.k_first[0] = k_first; m.planes = planes; m.sample_stride = (size_t)planes * g.H * g.W;
  if (mirror2.has_value() && mirror2->defined()) { chk(*mirror2); m.out[1][0] = mirror2->data_ptr<float>(); m.k_first[1] = k_first2; }
  c10::hip::HIPGuard guard(flags.get_device());
  check_status(fnx_jacobi_pass_mirror(&g, flags.data_ptr<float>(), div.data_ptr<float>(), p_in.data_ptr<float>(), p_out.data_ptr<float>(),
                                      k_begin, k_end, k_begin2, layout, &m, workspace.data_ptr(),
                                      (size_t)workspace.numel() * workspace.element_size(), reuse_mask ? 1 : 0, cur_stream(flags)));
  wrote(p_out); wrote(mirror); wrote(mirror2);
}

int64_t jacobi_workspace_bytes(int B, int D, int H, int W, bool is3D) {
  FnxGrid g{B, D, H, W, is3D ? 1 : 0, 0, 0, 0};
  return (int64_t)fnx_workspace_bytes(&g, FNX_OP_JACOBI);
}

static const unsigned char* bc_class_ptr(c10::optional<Tensor>& t, const Tensor& flags) {
  if (!t.has_value() || !t->defined()) return nullptr;
  TORCH_CHECK(t->scalar_type() == at::kByte && t->is_contiguous() && t->numel() == flags.numel() && t->device() == flags.device(),
              "bc_class: expected the uint8 tensor bc_classify returned for this grid");
  return t->data_ptr<unsigned char>();
}

// class map of the (static) BC arrays for pre_projection_ / post_projection_ (FnxState.bc_class)
Tensor bc_classify(Tensor flags, bool is3D, c10::optional<Tensor> UBC, c10::optional<Tensor> UBCInvMask,
                   c10::optional<Tensor> densityBC, c10::optional<Tensor> densityBCInvMask) {
  FnxGrid g = grid_of(flags, is3D, nullptr);
  Tensor dummy;
  c10::optional<Tensor> none;
  FnxState st{};
  st.UBC = opt_field(g, UBC, true, "UBC"); st.UBCInvMask = opt_field(g, UBCInvMask, true, "UBCInvMask");
  st.densityBC = opt_field(g, densityBC, false, "densityBC"); st.densityBCInvMask = opt_field(g, densityBCInvMask, false, "densityBCInvMask");
  c10::hip::HIPGuard guard(flags.get_device());
  Tensor cls = at::empty(flags.sizes(), flags.options().dtype(at::kByte));
  check_status(fnx_bc_classify(&g, &st, cls.data_ptr<unsigned char>(), cur_stream(flags)));
  return cls;
}

// simulate.py:96-133 (+ divergence): U_adv/rho_adv -> U, density (written), returns div
Tensor pre_projection_(Tensor U_adv, c10::optional<Tensor> rho_adv, Tensor p, Tensor U, Tensor flags,
                       c10::optional<Tensor> density, c10::optional<Tensor> UBC, c10::optional<Tensor> UBCInvMask,
                       c10::optional<Tensor> densityBC, c10::optional<Tensor> densityBCInvMask, double dt,
                       double buoyancy_scale, std::vector<double> gravity_vec, double operating_density,
                       bool jacobi_method, c10::optional<Tensor> bc_class, const Geom* geom) {
  check_field(U, "U");
  FnxGrid g = grid_of(flags, U.size(1) == 3, geom);
  check_vel(U, g, "U"); check_vel(U_adv, g, "U_adv"); check_scalar(p, g, "p");
  FnxStepParams prm = step_params(dt, buoyancy_scale, gravity_vec, operating_density);
  prm.method = jacobi_method ? 0 : 1;
  FnxState st = make_state(g, p, U, flags, density, UBC, UBCInvMask, densityBC, densityBCInvMask);
  const float* ra = nullptr;
  if (rho_adv.has_value() && rho_adv->defined()) { check_scalar(*rho_adv, g, "rho_adv"); ra = rho_adv->data_ptr<float>(); }
  st.bc_class = bc_class_ptr(bc_class, flags);
  c10::hip::HIPGuard guard(flags.get_device());
  Tensor div = at::empty_like(flags);
  check_status(fnx_pre_projection(&g, &prm, &st, U_adv.data_ptr<float>(), ra, div.data_ptr<float>(), cur_stream(U)));
  return div;
}

void post_projection_(Tensor p, Tensor U, Tensor flags, c10::optional<Tensor> density, c10::optional<Tensor> UBC,
                      c10::optional<Tensor> UBCInvMask, c10::optional<Tensor> densityBC,
                      c10::optional<Tensor> densityBCInvMask, c10::optional<Tensor> bc_class, const Geom* geom,
                      bool density_bc_applied) {
  check_field(U, "U");
  FnxGrid g = grid_of(flags, U.size(1) == 3, geom);
  check_vel(U, g, "U"); check_scalar(p, g, "p");
  FnxState st = make_state(g, p, U, flags, density, UBC, UBCInvMask, densityBC, densityBCInvMask);
  st.bc_class = bc_class_ptr(bc_class, flags);
  st.density_bc_applied = density_bc_applied ? 1 : 0;
  c10::hip::HIPGuard guard(flags.get_device());
  check_status(fnx_post_projection(&g, &st, cur_stream(U)));
  wrote(U); wrote(density);
}

int64_t step_workspace_bytes(int B, int D, int H, int W, bool is3D) {
  FnxGrid g{B, D, H, W, is3D ? 1 : 0, 0, 0, 0};
  return (int64_t)fnx_workspace_bytes(&g, FNX_OP_STEP_STATIC);   // (3D: with room for the stage word map; FNX_OP_STEP's size is still accepted)
}

}  // namespace

// an operation's one body with its dimension (scenes, loss) or its net's table row bound: what the module registers under the operation's
// names
template <class T, class R, class... A>
static auto in_dim(T which, R (*body)(T, A...)) {
  return [=](A... a) { return body(which, std::forward<A>(a)...); };
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  // Every compute entry point releases the GIL while it checks, allocates and enqueues: arguments are
  // converted before the guard is taken and results after it is dropped; nothing inside touches Python objects.
  using NoGil = py::call_guard<py::gil_scoped_release>;
  const auto GEOM = py::arg("geom") = py::none();
  py::class_<Geom>(m, "Geom", "per-call 3D geometry options: ref_quirks, z-slab view (z_offset, D_global), compute window [k_begin, k_end)")
      .def(py::init([](bool ref_quirks, int z_offset, int D_global, int k_begin, int k_end, int jacobi_x) {
             Geom g; g.ref_quirks = ref_quirks; g.z_offset = z_offset; g.D_global = D_global; g.k_begin = k_begin; g.k_end = k_end;
             g.jacobi_x = jacobi_x;
             return g;
           }),
           py::arg("ref_quirks") = false, py::arg("z_offset") = 0, py::arg("D_global") = 0, py::arg("k_begin") = 0,
           py::arg("k_end") = 0, py::arg("jacobi_x") = 0)
      .def_readwrite("jacobi_x", &Geom::jacobi_x)
      .def_readwrite("ref_quirks", &Geom::ref_quirks)
      .def_readwrite("z_offset", &Geom::z_offset)
      .def_readwrite("D_global", &Geom::D_global)
      .def_readwrite("k_begin", &Geom::k_begin)
      .def_readwrite("k_end", &Geom::k_end);
  // reference entry points (fluids_init.cpp:1009-1014): same names, same positional arguments; `out` / `geom` are
  // optional trailing extras
  m.def("advect_scalar", &advect_scalar, "Advect Scalar", py::arg("dt"), py::arg("src"), py::arg("U"), py::arg("flags"),
        py::arg("method"), py::arg("boundary_width"), py::arg("sample_outside_fluid"), py::arg("maccormack_strength"),
        py::arg("out") = py::none(), GEOM, py::arg("plan") = "auto", NoGil());
  m.def("advect_scalars", &advect_scalars, "Advect C passive scalars through one pair of line traces", py::arg("dt"), py::arg("src"),
        py::arg("U"), py::arg("flags"), py::arg("method"), py::arg("boundary_width"), py::arg("sample_outside_fluid"),
        py::arg("maccormack_strength"), py::arg("workspace") = py::none(), GEOM, py::arg("out") = py::none(), NoGil());
  m.def("advect_scalars_workspace_bytes", [](int B, int D, int H, int W, bool is3D, int channels) {
          FnxGrid g{}; g.B = B; g.D = D; g.H = H; g.W = W; g.is3D = is3D ? 1 : 0;
          return fnx_advect_scalars_workspace_bytes(&g, channels);
        }, py::arg("B"), py::arg("D"), py::arg("H"), py::arg("W"), py::arg("is3D"), py::arg("channels"));
  m.def("advect_step", &advect_step, py::arg("dt"), py::arg("density"), py::arg("U"), py::arg("flags"),
        py::arg("sample_outside_fluid"), py::arg("maccormack_strength"), py::arg("out_density") = py::none(),
        py::arg("out_U") = py::none(), GEOM, py::arg("plan") = "auto", NoGil());
  m.def("advect_vel", &advect_vel, "Advect Velocity", py::arg("dt"), py::arg("orig"), py::arg("U"), py::arg("flags"),
        py::arg("method"), py::arg("boundary_width"), py::arg("maccormack_strength"), py::arg("out") = py::none(), GEOM,
        py::arg("plan") = "auto", NoGil());
  m.def("solve_linear_system", &solve_linear_system, "Solve Linear System using Jacobi's method", py::arg("flags"),
        py::arg("div"), py::arg("is3D"), py::arg("p_tol"), py::arg("max_iter"), py::arg("verbose"), GEOM, NoGil());
  m.def("solve_linear_system_pcg", &solve_linear_system_pcg, "Converged pressure solve: multigrid-preconditioned CG (fnx_pcg); "
        "returns (p, residual, iterations per sample or None when p_tol <= 0).  p0: a starting guess (fnx_pcg_from; max_iter may then be 0)",
        py::arg("flags"), py::arg("div"), py::arg("is3D"), py::arg("p_tol") = 1e-5,
        py::arg("max_iter") = 50, py::arg("verbose") = false, GEOM, py::arg("p0") = py::none(), NoGil());
  m.def("poisson_apply", &poisson_apply, "A p, the operator of the pressure solve (fnx_poisson_apply)", py::arg("flags"), py::arg("p"),
        py::arg("is3D"), GEOM, NoGil());
  m.def("pcg_precondition", &pcg_precondition, "z = M^-1 r, one V-cycle of the PCG preconditioner (fnx_pcg_precondition)", py::arg("flags"),
        py::arg("r"), py::arg("is3D"), GEOM, NoGil());
  // operators the reference implements in Python
  m.def("velocity_divergence", &velocity_divergence, py::arg("U"), py::arg("flags"), GEOM, NoGil());
  m.def("velocity_update_", &velocity_update_, py::arg("pressure"), py::arg("U"), py::arg("flags"), GEOM, NoGil());
  m.def("add_buoyancy_", &add_buoyancy_, py::arg("U"), py::arg("flags"), py::arg("density"), py::arg("gravity"),
        py::arg("rho_star"), py::arg("dt"), GEOM, NoGil());
  m.def("correct_scalar_", &correct_scalar_, py::arg("dt"), py::arg("src"), py::arg("div"), py::arg("flags"), NoGil());
  m.def("add_gravity_", &add_gravity_, py::arg("U"), py::arg("flags"), py::arg("gravity"), py::arg("dt"), GEOM, NoGil());
  m.def("add_viscosity_", &add_viscosity_, NoGil());
  m.def("add_vorticity_confinement", &add_vorticity_confinement, py::arg("U"), py::arg("flags"), py::arg("strength"), GEOM, NoGil());
  m.def("add_vorticity_confinement_", &add_vorticity_confinement_, py::arg("U"), py::arg("flags"), py::arg("strength"), GEOM, NoGil());
  m.def("render_volume", &render_volume, "density + flags -> (B,2,R,Cc) radiance / transmittance image (fnx_render_volume)", py::arg("density"),
        py::arg("flags"), py::arg("view_dir"), py::arg("light_dir"), py::arg("k_view"), py::arg("k_light"), py::arg("ambient") = 0.25,
        py::arg("albedo_smoke") = 1.0, py::arg("albedo_obstacle") = 0.5, py::arg("bnd") = 1, NoGil());
  m.def("set_wall_bcs_", &set_wall_bcs_, py::arg("U"), py::arg("flags"), GEOM, NoGil());
  m.def("set_wall_bcs_stick_", &set_wall_bcs_stick_, NoGil());
  m.def("add_viscosity_out", &add_viscosity_out, "addViscosity of U into `out` (not U), returned (fnx_add_viscosity)", py::arg("dt"), py::arg("U"),
        py::arg("flags"), py::arg("viscosity"), py::arg("out"), NoGil());
  m.def("set_wall_bcs_stick_out", &set_wall_bcs_stick_out, "setWallBcsStick of U into `out` (not U), returned (fnx_set_wall_bcs_stick)",
        py::arg("U"), py::arg("flags"), py::arg("flags_stick"), py::arg("out"), NoGil());
  m.def("set_const_vals_", &set_const_vals_, NoGil());
  m.def("flags_to_occupancy", &flags_to_occupancy, NoGil());
  m.def("max_abs", &max_abs, NoGil());
  m.def("empty_domain_", &empty_domain_, py::arg("flags"), py::arg("boundary_width"), GEOM, NoGil());
  m.def("velocity_divergence_backward", &velocity_divergence_backward, py::arg("grad_div"), py::arg("flags"), py::arg("is3D"), GEOM, NoGil());
  m.def("velocity_update_backward", &velocity_update_backward, py::arg("grad_U_out"), py::arg("flags"), GEOM, NoGil());
  m.def("create_cylinder_", &create_cylinder_, NoGil());
  m.def("create_box2d_", &create_box2d_, NoGil());
  m.def("create_sphere_", &create_sphere_, py::arg("flags"), py::arg("center_x"), py::arg("center_y"), py::arg("center_z"), py::arg("radius"),
        py::arg("sample") = -1, NoGil());
  m.def("create_box3d_", &create_box3d_, py::arg("flags"), py::arg("x0"), py::arg("x1"), py::arg("y0"), py::arg("y1"), py::arg("z0"),
        py::arg("z1"), py::arg("sample") = -1, NoGil());
  m.def("voxelize_mesh_ws_bytes", &voxelize_mesh_ws_bytes, NoGil());
  m.def("voxelize_mesh_", &voxelize_mesh_, "mesh -> obstacle cells of flags; returns the device report {open rows, bad faces} (fnx_voxelize_mesh)",
        py::arg("flags"), py::arg("vertices"), py::arg("faces"), py::arg("sample") = -1, py::arg("workspace") = py::none(), NoGil());
  m.def("get_centered", &get_centered, NoGil());
  m.def("scalenet_pack", &scalenet_pack, NoGil());
  m.def("multiscale_forward", &multiscale_forward, py::arg("packed"), py::arg("x"), py::arg("precision_mode") = "fp32",
        py::arg("trim") = std::vector<int64_t>(), NoGil());
  m.def("fluidnet_forward", in_dim((const NetApi*)nullptr, &whole_forward), py::arg("packed"), py::arg("input"),
        py::arg("normalize_threshold"), py::arg("precision_mode") = "fp32", NoGil());
  m.def("multiscale_tape_layout", [](int64_t B, int64_t H, int64_t W) {
    return tape_tuples(make_grid(B, 1, H, W, false), fnx_multiscale_tape_entries(), fnx_multiscale_tape_layout); }, py::arg("B"), py::arg("H"), py::arg("W"));
  m.def("multiscale3d_tape_layout", [](int64_t B, int64_t D, int64_t H, int64_t W) {
    return tape_tuples(make_grid(B, D, H, W, true), fnx_multiscale_tape_entries(), fnx_multiscale3d_tape_layout); }, py::arg("B"), py::arg("D"), py::arg("H"), py::arg("W"));
  m.def("banknet_tape_layout", [](int64_t B, int64_t H, int64_t W) {
    return tape_tuples(make_grid(B, 1, H, W, false), fnx_banknet_tape_entries(), fnx_banknet_tape_layout); }, py::arg("B"), py::arg("H"), py::arg("W"));
  m.def("banknet3d_tape_layout", [](int64_t B, int64_t D, int64_t H, int64_t W) {
    return tape_tuples(make_grid(B, D, H, W, true), fnx_banknet3d_tape_entries(), fnx_banknet3d_tape_layout); }, py::arg("B"), py::arg("D"), py::arg("H"), py::arg("W"));
  // the four nets' operations, under the row's names; what one family alone has: the bank nets' inference names and their backward's x,
  // the ScaleNet's backward_plain
  for (const NetApi* net : NETS) {
    const std::string n = net->net_name, w = net->whole_name;
    m.def(net->pack_t_name, [net](Tensor blob) { return net_pack(net, true, blob); }, py::arg("blob"), NoGil());
    m.def((n + "_forward_train").c_str(), in_dim(net, &net_forward_train), py::arg("packed"), py::arg("x"), py::arg("precision_mode") = "fp32",
          NoGil());
    if (net->bank) {
      m.def(net->pack_name, [net](Tensor blob) { return net_pack(net, false, blob); }, py::arg("blob"), NoGil());
      m.def((n + "_forward").c_str(), in_dim(net, &bank_forward), py::arg("packed"), py::arg("x"), py::arg("precision_mode") = "fp32", NoGil());
      m.def((w + "_forward").c_str(), in_dim(net, &whole_forward), py::arg("packed"), py::arg("input"), py::arg("normalize_threshold"),
            py::arg("precision_mode") = "fp32", NoGil());
      m.def((n + "_backward").c_str(), in_dim(net, &bank_backward), py::arg("packed_t"), py::arg("x"), py::arg("grad_p"), py::arg("tape"),
            py::arg("precision_mode") = "fp32", NoGil());
    } else {
      m.def((n + "_backward").c_str(), in_dim(net, &scalenet_backward), py::arg("packed_t"), py::arg("grad_p"), py::arg("tape"),
            py::arg("precision_mode") = "fp32", NoGil());
      m.def((n + "_backward_plain").c_str(), in_dim(net, &scalenet_backward_plain), py::arg("packed_t"), py::arg("grad_p"), py::arg("tape"),
            py::arg("precision_mode") = "fp32", NoGil());
    }
    m.def((w + "_forward_train").c_str(), in_dim(net, &whole_forward_train), py::arg("packed"), py::arg("input"), py::arg("normalize_threshold"),
          py::arg("precision_mode") = "fp32", NoGil());
    m.def((w + "_backward").c_str(), in_dim(net, &whole_backward), py::arg("packed_t"), py::arg("flags"), py::arg("scale"), py::arg("grad_p"),
          py::arg("grad_U"), py::arg("tape"), py::arg("precision_mode") = "fp32", NoGil());
  }
  m.def("simulate_step_", &simulate_step_, py::arg("p"), py::arg("U"), py::arg("flags"), py::arg("density"), py::arg("UBC"),
        py::arg("UBCInvMask"), py::arg("densityBC"), py::arg("densityBCInvMask"), py::arg("net"), py::arg("dt"),
        py::arg("maccormack_strength"), py::arg("sample_outside_fluid"), py::arg("buoyancy_scale"), py::arg("gravity_vec"),
        py::arg("operating_density"), py::arg("p_tol"), py::arg("jacobi_iter"), py::arg("method"),
        py::arg("normalize_threshold"), py::arg("workspace") = py::none(), py::arg("static_flags") = 0, GEOM,
        py::arg("precision_mode") = "fp32", py::arg("viscosity") = 0.0, py::arg("gravity_scale") = 0.0,
        py::arg("correct_scalar") = false, py::arg("periodic") = 0, py::arg("flags_stick") = py::none(), py::arg("pcg_tol") = 1e-5,
        py::arg("pcg_iter") = 50, py::arg("vorticity_confinement") = 0.0, py::arg("pcg_warm") = false, py::arg("net_kind") = "scalenet",
        NoGil());
  m.def("step_workspace_bytes", &step_workspace_bytes);
  m.def("jacobi_sweeps_", &jacobi_sweeps_, py::arg("flags"), py::arg("div"), py::arg("p"), py::arg("is3D"), py::arg("nsweeps"),
        py::arg("workspace") = py::none(), py::arg("reuse_mask") = false, GEOM, py::arg("from_zero") = false, NoGil());
  m.def("jacobi_workspace_bytes", &jacobi_workspace_bytes);
  m.def("jacobi_pass_", &jacobi_pass_, py::arg("flags"), py::arg("div"), py::arg("p_in"), py::arg("p_out"), py::arg("nsweeps"),
        py::arg("k_begin"), py::arg("k_end"), py::arg("workspace"), py::arg("reuse_mask"), py::arg("k_begin2") = -1, GEOM,
        py::arg("layout") = 0, NoGil());
  m.def("jacobi_pass_mirror_", &jacobi_pass_mirror_, py::arg("flags"), py::arg("div"), py::arg("p_in"), py::arg("p_out"), py::arg("k_begin"),
        py::arg("k_end"), py::arg("workspace"), py::arg("reuse_mask"), py::arg("mirror"), py::arg("k_first"), py::arg("planes"),
        py::arg("k_begin2") = -1, py::arg("mirror2") = py::none(), py::arg("k_first2") = 0, GEOM, py::arg("layout") = 0, NoGil(),
        "two sweeps on planes [k_begin, k_end) (+ a second range) whose output planes [k_first, k_first + planes) also go to `mirror` (fnx_jacobi_pass_mirror)");
  m.def("jacobi_pass_mirror_ok", [](int B, int D, int H, int W, int planes_per_range, bool two_ranges, int layout) {
    FnxGrid g{}; g.B = B; g.D = D; g.H = H; g.W = W; g.is3D = 1;
    return fnx_jacobi_pass_mirror_ok(&g, planes_per_range, two_ranges ? 1 : 0, layout) != 0;
  });
  m.def("jacobi_quad_ok", &jacobi_quad_ok);
  m.def("pre_projection_", &pre_projection_, py::arg("U_adv"), py::arg("rho_adv"), py::arg("p"), py::arg("U"), py::arg("flags"),
        py::arg("density"), py::arg("UBC"), py::arg("UBCInvMask"), py::arg("densityBC"), py::arg("densityBCInvMask"),
        py::arg("dt"), py::arg("buoyancy_scale"), py::arg("gravity_vec"), py::arg("operating_density"),
        py::arg("jacobi_method"), py::arg("bc_class") = py::none(), GEOM, NoGil());
  m.def("post_projection_", &post_projection_, py::arg("p"), py::arg("U"), py::arg("flags"), py::arg("density"), py::arg("UBC"),
        py::arg("UBCInvMask"), py::arg("densityBC"), py::arg("densityBCInvMask"), py::arg("bc_class") = py::none(), GEOM,
        py::arg("density_bc_applied") = false, NoGil());
  m.def("bc_classify", &bc_classify, "uint8 class map of static BC arrays (FnxState.bc_class)", NoGil());
  py::class_<PyLoopbackGroup, std::shared_ptr<PyLoopbackGroup>>(m, "SlabLoopbackGroup", "in-process communicator group: n slabs driven by n host threads")
      .def(py::init<int>(), py::arg("nranks"))
      .def("set_timeout", [](PyLoopbackGroup& g, double seconds) { check_status(fnx_slab_loopback_group_set_timeout(g.g, seconds)); }, py::arg("seconds"),
           "how long a rank waits for a peer before its call fails (the group stays usable); default 120 s")
      .def("reset", [](PyLoopbackGroup& g) { check_status(fnx_slab_loopback_group_reset(g.g)); },
           "clear an abort (no rank may be inside a call of the group)");
  py::class_<PySlabComm, std::shared_ptr<PySlabComm>>(m, "SlabComm", "ghost-plane communicator of the native z-slab driver (FnxSlabComm)")
      .def("failed", [](PySlabComm& c) { return c.keep_peer ? fnx_slab_peer_failed(c.keep_peer->p) != FNX_OK : false; },
           "peer-store: an exchange of this rank timed out / the group was aborted (ask after synchronising; other transports report through their calls)")
      // the control-path collectives of the table, callable on their own (every rank of the communicator must call them)
      .def("allreduce_sum_", [](PySlabComm& c, Tensor x) {
             TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.scalar_type() == at::kFloat, "allreduce: a contiguous fp32 GPU tensor");
             c10::hip::HIPGuard guard(x.get_device());
             py::gil_scoped_release nogil;
             check_status(c.c.allreduce_sum(c.c.ctx, x.data_ptr<float>(), (int)x.numel(), cur_stream(x)));
           }, py::arg("x"))
      .def("allreduce_max_", [](PySlabComm& c, Tensor x) {
             TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.scalar_type() == at::kFloat, "allreduce: a contiguous fp32 GPU tensor");
             c10::hip::HIPGuard guard(x.get_device());
             py::gil_scoped_release nogil;
             check_status(c.c.allreduce_max(c.c.ctx, x.data_ptr<float>(), (int)x.numel(), cur_stream(x)));
           }, py::arg("x"));
  m.def("slab_rccl_unique_id", &slab_rccl_unique_id);
  m.def("slab_comm_rccl", &slab_comm_rccl, py::arg("rank"), py::arg("nranks"), py::arg("unique_id"));
  m.def("slab_comm_loopback", &slab_comm_loopback, py::arg("group"), py::arg("rank"));
  py::class_<PyPeer, std::shared_ptr<PyPeer>>(m, "SlabPeer", "a rank's peer-store region: flags + mailbox its z-neighbours map (fnx_slab_peer_create)")
      .def(py::init<int, int, int64_t>(), py::arg("rank"), py::arg("nranks"), py::arg("mailbox_bytes"))
      .def_property_readonly("handle", [](PyPeer& p) { return py::bytes(p.handle); }, "the bytes both neighbours need (FNX_PEER_HANDLE_BYTES)")
      .def("set_timeout", [](PyPeer& p, double seconds) { check_status(fnx_slab_peer_set_timeout(p.p, seconds)); }, py::arg("seconds"))
      .def("failed", [](PyPeer& p) { return fnx_slab_peer_failed(p.p) != FNX_OK; },
           "a device-side wait of this rank's exchanges has timed out, or the group was aborted (ask after synchronising the stream)");
  m.def("slab_comm_peer", [](std::shared_ptr<PyPeer> peer, py::object handle_lo, py::object handle_hi) {
    std::string lo = handle_lo.is_none() ? std::string() : handle_lo.cast<std::string>();
    std::string hi = handle_hi.is_none() ? std::string() : handle_hi.cast<std::string>();
    TORCH_CHECK((lo.empty() || lo.size() == FNX_PEER_HANDLE_BYTES) && (hi.empty() || hi.size() == FNX_PEER_HANDLE_BYTES), "a peer handle has ",
                FNX_PEER_HANDLE_BYTES, " bytes");
    auto c = std::make_shared<PySlabComm>();
    check_status(fnx_slab_comm_peer(&c->c, peer->p, lo.empty() ? nullptr : lo.data(), hi.empty() ? nullptr : hi.data()));
    c->keep_peer = peer;
    return c;
  }, py::arg("peer"), py::arg("handle_lo"), py::arg("handle_hi"), "peer-store communicator: device stores into the neighbours' mapped mailboxes + flags");
  m.def("slab_comm_link_model", [](double latency_us, double gbps) {
    auto c = std::make_shared<PySlabComm>();
    check_status(fnx_slab_comm_link_model(&c->c, latency_us, gbps));
    return c;
  }, py::arg("latency_us"), py::arg("gbytes_per_s"), "rehearsal communicator: one process runs a middle rank's step against an assumed link");
  m.def("slab_comm_probe", [](std::shared_ptr<PySlabComm> comm, int64_t bytes, int reps, Tensor scratch) {
    TORCH_CHECK(scratch.is_cuda() && scratch.is_contiguous() && (int64_t)scratch.numel() * scratch.element_size() >= 4 * bytes,
                "slab_comm_probe: scratch must be a contiguous GPU tensor of at least 4 * bytes");
    c10::hip::HIPGuard guard(scratch.get_device());
    float ms = 0.f;
    { py::gil_scoped_release nogil;
      check_status(fnx_slab_comm_probe(&comm->c, scratch.data_ptr(), (size_t)bytes, reps, &ms, cur_stream(scratch))); }
    return (double)ms;
  }, py::arg("comm"), py::arg("bytes"), py::arg("reps"), py::arg("scratch"),
        "average ms of one ghost exchange of `bytes` bytes with each neighbour (every rank must call it)");
  py::class_<PySlab>(m, "SlabDriver", "native z-slab driver of the 3D Jacobi step (fnx_slab_create / fnx_slab_step)")
      .def(py::init<int, int, int, int, int, int, int, int, bool, int, std::shared_ptr<PySlabComm>, const std::string&, const std::string&, const std::string&>(), py::arg("B"), py::arg("H"),
           py::arg("W"), py::arg("D_global"), py::arg("rank"), py::arg("nranks"), py::arg("halo"), py::arg("sweeps_per_exchange"),
           py::arg("static_flags") = false, py::arg("cfl_check_every") = 0, py::arg("comm") = nullptr, py::arg("schedule") = "deep_first",
           py::arg("method") = "jacobi", py::arg("direct_sends") = "auto")
      .def("stats_enable", &PySlab::stats_enable, py::arg("on"))
      .def("stats_read", &PySlab::stats_read, "dict(bytes_per_neighbour, wait_ms, exchanges) since stats_enable(True); synchronises")
      .def("layout", &PySlab::layout, "(owned planes, ghost planes below, above, global plane of local plane 0)")
      .def("workspace_bytes", &PySlab::workspace_bytes)
      .def("step", &PySlab::step, py::arg("p"), py::arg("U"), py::arg("flags"), py::arg("density"), py::arg("UBC"), py::arg("UBCInvMask"),
           py::arg("densityBC"), py::arg("densityBCInvMask"), py::arg("dt"), py::arg("maccormack_strength"),
           py::arg("sample_outside_fluid"), py::arg("buoyancy_scale"), py::arg("gravity_vec"), py::arg("operating_density"),
           py::arg("p_tol"), py::arg("jacobi_iter"), py::arg("workspace"), py::arg("net") = py::none(), py::arg("precision_mode") = "fp32",
           py::arg("normalize_threshold") = 1e-5, py::arg("method") = "auto", py::arg("viscosity") = 0.0, NoGil());
  m.def("device_name", []() { const char* n = fnx_device_name(); return std::string(n ? n : ""); });
  m.def("trilinear_upsample_backward", &trilinear_upsample_backward, py::arg("grad_dst"), py::arg("size"), NoGil());
  m.def("scene_obstacles",
        [](Tensor ids, int64_t H, int64_t W, int64_t seed, int n_min, int n_max, double centre_min, double centre_max, double size_min,
           double size_max, int64_t depth) {
          return scene_obstacles(false, ids, depth, H, W, seed, n_min, n_max, centre_min, centre_max, size_min, size_max);
        },
        py::arg("scene_ids"), py::arg("H"), py::arg("W"), py::arg("seed"), py::arg("n_min"), py::arg("n_max"), py::arg("centre_min"),
        py::arg("centre_max"), py::arg("size_min"), py::arg("size_max"), py::arg("depth") = 1, NoGil());
  m.def("scene_obstacles3d", in_dim(true, &scene_obstacles), py::arg("scene_ids"), py::arg("D"), py::arg("H"), py::arg("W"), py::arg("seed"),
        py::arg("n_min"), py::arg("n_max"), py::arg("centre_min"), py::arg("centre_max"), py::arg("size_min"), py::arg("size_max"), NoGil());
  m.def("scene_turbulence",
        [](Tensor ids, int64_t H, int64_t W, int64_t seed, int octaves, double wavelength, double amplitude, double density_scale,
           bool with_density, int64_t depth) {
          return scene_turbulence(false, ids, depth, H, W, seed, octaves, wavelength, amplitude, density_scale, with_density);
        },
        py::arg("scene_ids"), py::arg("H"), py::arg("W"), py::arg("seed"), py::arg("octaves"), py::arg("wavelength"), py::arg("amplitude"),
        py::arg("density_scale"), py::arg("with_density") = true, py::arg("depth") = 1, NoGil());
  m.def("scene_turbulence3d", in_dim(true, &scene_turbulence), py::arg("scene_ids"), py::arg("D"), py::arg("H"), py::arg("W"), py::arg("seed"),
        py::arg("octaves"), py::arg("wavelength"), py::arg("amplitude"), py::arg("density_scale"), py::arg("with_density") = true, NoGil());
  for (const bool is3d : {false, true})
    m.def(is3d ? "train_loss3d" : "train_loss", in_dim(is3d, &train_loss), py::arg("out_p"), py::arg("out_U"), py::arg("flags"),
          py::arg("target_p"), py::arg("lambdas"), py::arg("upstream") = py::none(), py::arg("terms") = true, NoGil());
  m.def("abi_version", &fnx_abi_version);
  m.def("profile_enable", [](bool on, bool runs) { fnx_profile_enable(on ? (runs ? 2 : 1) : 0); }, py::arg("on"), py::arg("runs") = false);
  m.def("roctx_enable", [](bool on) { check_status(fnx_roctx_enable(on ? 1 : 0)); });
  m.def("profile_read_work", [](int tag) { double w = 0; fnx_profile_read_work(tag, &w); return w; });
  m.def("profile_read", [](int tag) { double ms = 0; int n = 0; fnx_profile_read(tag, &ms, &n); return std::make_pair(ms, n); });
}
