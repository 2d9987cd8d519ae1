// What fnx_simulate_step and fnx_pre_projection decide before they launch anything, as pure functions: the layout of the step's
// workspace and, from the parameters and from which optional arrays the state has, which launches the step is made of.  No HIP call;
// a host-only program can include this file alone (it needs FnxStepParams of include/fluidnet_hip.h and nothing else).  fnx_api.hip
// sizes and carves by step_layout and issues the sequence that step_plan names.
#pragma once
#include <stddef.h>

#include "../../include/fluidnet_hip.h"

namespace fnx {

// ---- the workspace of a step ----------------------------------------------------------------------------------------------------------
// In this order, each region rounded up to 256 bytes: the advected density and velocity, the divergence, the 3D Jacobi neighbour mask,
// the BC class map and the PCG hierarchy (these three are kept between steps), in 2D the viscous velocity that is advected
// (FnxStepParams.viscosity), then the tail that the advection, the solve, the net and the periodic patches use one after the other.
// (Behind all of it, where the caller's workspace has FNX_OP_STEP_STATIC's size: the 3D stage word map, see stage_word_plan below.)
struct StepLayout {
  float *rho2, *U2, *div;
  unsigned char *mask, *cls;      // mask: 3D only
  void* pcg_kept;
  float* orig;                    // 2D only
  void* tail;
  size_t tail_bytes, bytes;
};
// cells: B*D*H*W; nc: velocity channels; tail_need: the most any user of the tail takes.  base == nullptr: the size only.
inline StepLayout step_layout(size_t cells, size_t nc, bool is3d, size_t mask_bytes, size_t pcg_kept_bytes, size_t tail_need, void* base) {
  size_t off = 0;
  auto take = [&](size_t bytes) { void* r = base ? (char*)base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return r; };
  StepLayout L{};
  L.rho2 = (float*)take(cells * 4);
  L.U2 = (float*)take(cells * 4 * nc);
  L.div = (float*)take(cells * 4);
  if (is3d) L.mask = (unsigned char*)take(mask_bytes);
  L.cls = (unsigned char*)take(cells);
  L.pcg_kept = take(pcg_kept_bytes);
  if (!is3d) L.orig = (float*)take(cells * 4 * nc);
  L.tail = take(0);
  L.tail_bytes = tail_need;
  L.bytes = off + tail_need;
  return L;
}

// ---- the stage between the advection and the projection (simulate.py:96-133, + :144) -------------------------------------------------
struct StagePlan {
  bool buoy; float s[3];          // addBuoyancy, strengths gravity_vec * -buoyancy_scale * dt
  float rho_star;                 // its operating density
  bool grav; float g[3];          // addGravity, forces (gravity_vec * -gravity_scale) * dt
  bool wall;                      // setWallBcs: every method but the convnet's (simulate.py:119-120)
  bool periodic, px, py;          // the periodic patches after setWallBcs (simulate.py:121-128): with wall only
  bool second_bcs;                // the setConstVals of simulate.py:133; not with flags_stick before the net: the caller runs
                                  // setWallBcsStick between the two
  bool confine; float amp;        // vorticity confinement after addGravity and before setWallBcs
};
// has_rho: an advected density goes through the stage; has_stick: the state has flags_stick
inline StagePlan stage_plan(const FnxStepParams* prm, bool has_rho, bool has_stick) {
  StagePlan p{};
  p.buoy = has_rho && prm->buoyancy_scale > 0.f;
  p.rho_star = prm->operating_density;
  if (p.buoy) {
    const float ns = -prm->buoyancy_scale;                       // gravity.mul_(-buoyancyScale), simulate.py:101-105
    const float gx = prm->gravity_vec[0] * ns, gy = prm->gravity_vec[1] * ns, gz = prm->gravity_vec[2] * ns;
    p.s[0] = gx * prm->dt; p.s[1] = gy * prm->dt; p.s[2] = gz * prm->dt;       // strength = gravity * dt, source_terms.py:45
  }
  // simulate.py:107-114: addGravity(gravityVec * -gravityScale) after the buoyancy, inside the density branch
  p.grav = has_rho && prm->gravity_scale > 0.f;
  if (p.grav) {
    const float ns = -prm->gravity_scale;
    for (int a = 0; a < 3; ++a) p.g[a] = (prm->gravity_vec[a] * ns) * prm->dt;  // force = gravity * dt, source_terms.py
  }
  p.wall = prm->method != 1;
  p.periodic = p.wall && (prm->periodic & 1);
  p.px = (prm->periodic & 2) != 0;
  p.py = (prm->periodic & 4) != 0;
  p.second_bcs = !(prm->method == 1 && has_stick);
  p.confine = prm->vorticity_confinement > 0.f;
  p.amp = prm->vorticity_confinement;
  return p;
}

// ---- one whole step (simulate.py:28-171) ----------------------------------------------------------------------------------------------
// PAIR: density and velocity in one pair of launches; RHO_THEN_VEL: the density, then the velocity (the viscous one is advected, which
// the pair cannot do); VEL_ONLY: no density in the state
enum class StepAdvect { PAIR, RHO_THEN_VEL, VEL_ONLY };
enum class StepClassMap { NONE, BUILD, REUSE };             // the BC class map kept in the workspace (static_flags bits 1 and 2)
// the solves take the divergence the stage wrote; the nets project st->U themselves.  PCG_FROM_NET: the net's pressure goes into st->p
// first; NET_FUSED: the net's last pass is also the step's tail; NET_STICK: setWallBcsStick before the second setConstVals and the net
enum class StepProjection { JACOBI, PCG_COLD, PCG_FROM_NET, PCG_FROM_P, NET_FUSED, NET_STICK };
// POST: velocityUpdate, setWallBcs, setConstVals in one pass; POST_PERIODIC: that pass between the save and the restore of the periodic
// patches' source row and column; STICK_BCS: setWallBcsStick, then the last setConstVals; NONE: the net's last pass was the tail
enum class StepTail { POST, POST_PERIODIC, STICK_BCS, NONE };
struct StepPlan {
  bool viscous;                   // addViscosity of U is what the velocity advection advects (2D)
  StepAdvect advect;
  bool correct_scalar;            // by the divergence of the old U
  StepClassMap class_map;
  StagePlan stage;
  StepProjection projection;
  bool solve;                     // the projection is a linear solve: the stage writes its right-hand side
  bool pcg_rebuild;               // the hierarchy is trusted only when the caller says both that flags are unchanged (bit 0) and that this
                                  // workspace holds the hierarchy of these flags (bit 3)
  bool reuse_mask;                // 3D Jacobi: the neighbour mask the last step left in the workspace is current (bit 0)
  StepTail tail;
};
// has_rho / has_stick: the state has a density / flags_stick; has_bc: it has UBC or densityBC
inline StepPlan step_plan(const FnxStepParams* prm, bool has_rho, bool has_stick, bool has_bc) {
  StepPlan p{};
  p.viscous = prm->viscosity > 0.f;
  p.advect = !has_rho ? StepAdvect::VEL_ONLY : p.viscous ? StepAdvect::RHO_THEN_VEL : StepAdvect::PAIR;
  p.correct_scalar = has_rho && prm->correct_scalar;
  p.class_map = !((prm->static_flags & 2) && has_bc) ? StepClassMap::NONE : (prm->static_flags & 4) ? StepClassMap::REUSE : StepClassMap::BUILD;
  p.stage = stage_plan(prm, has_rho, has_stick);
  switch (prm->method) {
    case 0: p.projection = StepProjection::JACOBI; break;
    case 1: p.projection = has_stick ? StepProjection::NET_STICK : StepProjection::NET_FUSED; break;   // simulate.py:129-130, :165-166
    case 2: p.projection = StepProjection::PCG_COLD; break;
    case 3: p.projection = StepProjection::PCG_FROM_NET; break;
    default: p.projection = StepProjection::PCG_FROM_P; break;
  }
  p.solve = prm->method != 1;
  p.pcg_rebuild = (prm->static_flags & 9) != 9;
  p.reuse_mask = (prm->static_flags & 1) != 0;
  p.tail = p.projection == StepProjection::NET_FUSED ? StepTail::NONE
         : p.projection == StepProjection::NET_STICK ? StepTail::STICK_BCS
         : p.stage.periodic ? StepTail::POST_PERIODIC : StepTail::POST;
  return p;
}

// ---- the 3D stage word map (fnx_stage_word.h) -----------------------------------------------------------------------------------------
// One uint32 per cell behind the layout's last byte, for callers whose workspace has FNX_OP_STEP_STATIC's size: 3D steps that go by the
// class map then stage and finish on the word.  It depends on `flags` as well as on the BC arrays, so it is trusted only when the caller
// says both that the flags are unchanged (bit 0) and that the class map -- with which it is built -- was there already (bit 2).
enum class StepStageWord { NONE, BUILD, REUSE };
inline size_t stage_word_offset(const StepLayout& L) { return (L.bytes + 255) & ~(size_t)255; }
inline size_t stage_word_bytes(size_t cells, bool is3d) { return is3d ? cells * 4 : 0; }
// ws_bytes: what the caller's workspace holds
inline StepStageWord stage_word_plan(const FnxStepParams* prm, bool is3d, StepClassMap class_map, const StepLayout& L, size_t cells,
                                     size_t ws_bytes) {
  if (!is3d || class_map == StepClassMap::NONE || ws_bytes < stage_word_offset(L) + stage_word_bytes(cells, true)) return StepStageWord::NONE;
  return (prm->static_flags & 5) == 5 ? StepStageWord::REUSE : StepStageWord::BUILD;
}

}  // namespace fnx
