// brax_launch.hpp -- host-side rules of the Brax entry points, shared by their translation units (carl_brax.hip: reset /
// step / open-loop rollout; the closed-loop units through brax_policy_host.hpp): the batch / model / io checks, the kernel
// class of a model, the lanes-per-env rule, the launch shape (workgroups, wavefronts per workgroup, dynamic LDS) and the
// kernels' Prepared argument.  A kernel table is whatever array of entries with a class `c` and a width `k` the unit
// instantiates; the rules are templates over it, so that each unit instantiates its own kernels only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/carl_amd.h"
#include "brax_kernels.hip.h"
#include "host_common.hpp"

namespace carl_host {
namespace brax {

inline int validate_brax(const carl_batch_t* b, const carl_brax_sys_t* sd, const carl_brax_sys_t* sh, const char* who) {
  if (b == nullptr || sd == nullptr || sh == nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: batch / sys pointer is NULL", who);
  if (b->n_lanes < 0) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_lanes %d < 0", who, b->n_lanes);
  if (b->n_contexts <= 0 || b->ctx_stride < b->n_contexts)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_contexts %d / ctx_stride %d invalid", who, b->n_contexts,
                b->ctx_stride);
  if (!b->state || !b->elapsed || !b->ctx_idx || !b->episode || !b->n_calls || !b->ep_return || !b->ctx_table)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: a required batch pointer is NULL", who);
  if (sh->n_links < 1 || sh->n_links > CARL_BRAX_MAX_LINKS || sh->n_dof > CARL_BRAX_MAX_DOF ||
      sh->n_q > CARL_BRAX_MAX_Q || sh->n_act > CARL_BRAX_MAX_ACT || sh->n_coll > CARL_BRAX_MAX_COLL ||
      sh->n_frames < 1 || sh->obs_dim < 1)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: model table out of range", who);
  for (int i = 0; i < sh->n_links; ++i) {
    const bool free_root = sh->parent[i] < 0 && sh->n_link_dof[i] == 6;
    const int n_rot = sh->n_link_dof[i] - sh->n_slide[i];
    const bool hinge = sh->n_slide[i] >= 0 && sh->n_slide[i] <= 2 && n_rot >= 0 && n_rot <= 3 && sh->n_link_dof[i] >= 1;
    if (sh->parent[i] >= i || !(free_root || hinge))
      return fail(CARL_ERR_UNSUPPORTED,
                  "%s: link %d: supported joints are a free root, or 0-2 prismatic dofs + 0-3 stacked hinges", who, i);
    if (!free_root && n_rot == 3 && sh->dof_sign3[i] != 1.0f && sh->dof_sign3[i] != -1.0f)
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: link %d: dof_sign3 must be +1 or -1", who, i);
  }
  if (sh->obs_trig_from < 0 || sh->obs_trig_from >= sh->n_q ||
      (sh->obs_trig_from > 0 && sh->obs_trig_from < sh->exclude_current_positions))
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: obs_trig_from %d out of range", who, sh->obs_trig_from);
  if (sh->tip_link < 0 || sh->tip_link >= sh->n_links)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: tip_link %d out of range", who, sh->tip_link);
  if (sh->tip_link > 0 && sh->target_link == 0 && sh->push_link == 0)
    for (int k = 0; k < 2; ++k)
      if (sh->tip_vel_dof[k] < 0 || sh->tip_vel_dof[k] >= sh->n_dof)
        return fail(CARL_ERR_INVALID_ARGUMENT, "%s: tip_vel_dof[%d] = %d out of range", who, k, sh->tip_vel_dof[k]);
  for (int k = 0; k < sh->n_act; ++k) {
    if (sh->act_dof[k] < 0 || sh->act_dof[k] >= sh->n_dof)
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: actuator %d drives dof %d (of %d)", who, k, sh->act_dof[k], sh->n_dof);
    for (int j = 0; j < k; ++j)
      if (sh->act_dof[j] == sh->act_dof[k])  // the kernel adds actuator torques to their dofs in parallel
        return fail(CARL_ERR_UNSUPPORTED, "%s: actuators %d and %d drive the same dof", who, j, k);
  }
  if (sh->healthy_q_index >= 0 &&
      (sh->healthy_q_index < sh->exclude_current_positions || sh->healthy_q_index >= sh->n_q))
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: healthy_q_index %d must be an observed coordinate", who,
                sh->healthy_q_index);
  if (sh->push_link != 0) {  // push task (see carl_brax_sys_t::push_link)
    const int t = sh->push_link;
    if (t != sh->n_links - 1 || t < 1 || sh->parent[t] != -1 || sh->n_slide[t] != 2 || sh->n_link_dof[t] != 2)
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: push_link must be the last link, on two slides against the world", who);
    if (sh->target_link != 0 || sh->tip_link < 1 || sh->tip_link >= t || sh->exclude_current_positions != 0 ||
        sh->obs_trig_from != 0 || sh->obs_extended || sh->goal_mode || !sh->reset_vel_uniform)
      return fail(CARL_ERR_INVALID_ARGUMENT,
                  "%s: the push task needs an end-effector link, the plain q ++ qd observation and uniform reset rates", who);
    if (sh->q_start[t] != sh->dof_start[t])
      return fail(CARL_ERR_UNSUPPORTED, "%s: push task: the arm must be hinges only", who);
    if (sh->n_pair < 0 || sh->n_pair > CARL_BRAX_MAX_PAIR || (sh->n_pair > 0 && (sh->pair_link < 0 || sh->pair_link >= t)))
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: pair contact table out of range", who);
  } else if (sh->n_pair != 0) {
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: pair contacts belong to the push task", who);
  }
  if (sh->target_link != 0) {  // reach task (see carl_brax_sys_t::target_link)
    const int t = sh->target_link;
    if (t != sh->n_links - 1 || t < 1 || sh->parent[t] != -1 || sh->n_slide[t] != 2 || sh->n_link_dof[t] != 2)
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: target_link must be the last link, on two slides against the world", who);
    if (sh->tip_link < 1 || sh->tip_link >= t || sh->exclude_current_positions != 0 || sh->obs_trig_from != 0 ||
        sh->obs_extended || sh->goal_mode || !sh->reset_vel_uniform)
      return fail(CARL_ERR_INVALID_ARGUMENT,
                  "%s: the reach task needs a tip link, the plain q ++ qd observation and uniform reset rates", who);
    if (sh->n_q + sh->dof_start[t] > 12 * sh->n_links)
      return fail(CARL_ERR_UNSUPPORTED, "%s: reach task: %d coordinates do not fit the staging rows", who, sh->n_q);
  }
  {
    const int base = sh->n_q - sh->exclude_current_positions + sh->n_dof +
                     (sh->obs_trig_from > 0 ? sh->n_q - sh->obs_trig_from : 0);
    int want = sh->obs_extended ? base + 16 * sh->n_links + sh->n_dof : base;
    if (sh->target_link > 0) want = sh->q_start[sh->target_link] + sh->n_q + sh->dof_start[sh->target_link] + 3;
    if (sh->push_link > 0) want = 2 * sh->q_start[sh->push_link] + 9;
    if (sh->obs_dim != want)
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: obs_dim %d does not match the model (%d)", who, sh->obs_dim, want);
  }
  if (b->fin_count != nullptr && (b->fin_capacity <= 0 || !b->fin_lane || !b->fin_return || !b->fin_length))
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: finished-episode log is incomplete", who);
  if ((b->flags & CARL_FLAG_AUTORESET_FIRST_STATE) && b->first_state == nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: CARL_FLAG_AUTORESET_FIRST_STATE needs carl_batch_t::first_state", who);
  return 0;
}

// The GENERAL kernels (template parameter TASK of brax_kernel): the reach / push task models -- and every model with a link
// whose principal moments of inertia differ.  Every shipped locomotion model has isotropic effective inertia
// (spring_inertia_scale = 1), so the rotated-inertia code R diag(1 / I) R^T lives in the general kernels only: the lean and
// multi-hinge kernels compile isotropy in (brax_kernels.hip.h: substep, all_iso) and carry neither its instructions nor its
// registers through the substep loop.  A general kernel runs a non-task model unchanged (its task epilogues are guarded by
// the model's own target_link / push_link / n_pair).
inline bool brax_is_task(const carl_brax_sys_t* sh) {
  if (sh->target_link > 0 || sh->push_link > 0) return true;
  for (int i = 0; i < sh->n_links; ++i)
    if (!(sh->inv_inertia[i][0] == sh->inv_inertia[i][1] && sh->inv_inertia[i][1] == sh->inv_inertia[i][2])) return true;
  return false;
}
inline bool brax_is_planar(const carl_brax_sys_t* sh);
// The general kernels (MULTI): any link with 0, 2 or 3 hinges (Euler-angle path), a link frame that is rotated against
// its parent's (link_rot != identity: the relative rotation of the joint frames then needs the full 4 x 4 map,
// brax_kernels.hip.h: LinkRec), or prismatic dofs outside the planar kernels (whose root slides are their own code) --
// of the shipped models Humanoid / HumanoidStandup (stacked hinges, rotated frames), the inverted pendulums (the cart).
// The lean kernels (MULTI = false) are "a free root and single hinges": Ant.
inline bool brax_is_multi(const carl_brax_sys_t* sh) {
  bool multi = false, slides = false;
  for (int i = 0; i < sh->n_links; ++i) {
    const bool free_root = sh->parent[i] < 0 && sh->n_link_dof[i] == 6;
    multi |= !free_root && sh->n_link_dof[i] - sh->n_slide[i] != 1;
    multi |= !free_root && !(sh->link_rot[i][0] == 1.0f && sh->link_rot[i][1] == 0.0f && sh->link_rot[i][2] == 0.0f &&
                             sh->link_rot[i][3] == 0.0f);
    slides |= !free_root && sh->n_slide[i] > 0;
  }
  return multi || (slides && !brax_is_planar(sh));
}
// Planar single-hinge model (Halfcheetah, Hopper, Walker2d as this package builds them): the root hangs on the world by
// two slides along x and z and a hinge about y, every other link by one hinge about +-y; link frames are unrotated, the
// joint frame is "x -> +-y", and anchors, centres of mass and spheres all lie in the y = 0 plane.  Then a state produced
// by reset never leaves that plane and brax_kernels.hip.h's substep_planar computes the same substep without the
// zero components.  Anything else -- and any batch with CARL_FLAG_BRAX_GENERIC -- takes the general substep.
inline bool brax_is_planar(const carl_brax_sys_t* sh) {
  if (brax_is_task(sh) || sh->n_links < 1 || sh->n_pair > 0) return false;  // (the per-link checks below cover the rest)
  const float r = 0.70710678f;
  auto near = [](float a, float b) { return a - b < 1e-6f && b - a < 1e-6f; };
  for (int i = 0; i < sh->n_links; ++i) {
    const bool root = i == 0;
    if (root ? sh->parent[i] >= 0 : (sh->parent[i] < 0 || sh->parent[i] >= i)) return false;
    if (sh->n_slide[i] != (root ? 2 : 0) || sh->n_link_dof[i] != (root ? 3 : 1)) return false;
    if (!(sh->link_rot[i][0] == 1.0f && sh->link_rot[i][1] == 0.0f && sh->link_rot[i][2] == 0.0f && sh->link_rot[i][3] == 0.0f))
      return false;
    if (!(near(sh->joint_rot[i][0], r) && sh->joint_rot[i][1] == 0.0f && sh->joint_rot[i][2] == 0.0f &&
          (near(sh->joint_rot[i][3], r) || near(sh->joint_rot[i][3], -r))))  // x -> +y or x -> -y
      return false;
    if (sh->link_pos[i][1] != 0.0f || sh->joint_pos[i][1] != 0.0f || sh->com[i][1] != 0.0f) return false;
    if (!(sh->inv_inertia[i][0] == sh->inv_inertia[i][1] && sh->inv_inertia[i][1] == sh->inv_inertia[i][2])) return false;
    if (root && !(sh->slide_axis[i][0][0] == 1.0f && sh->slide_axis[i][0][1] == 0.0f && sh->slide_axis[i][0][2] == 0.0f &&
                  sh->slide_axis[i][1][0] == 0.0f && sh->slide_axis[i][1][1] == 0.0f && sh->slide_axis[i][1][2] == 1.0f))
      return false;
  }
  for (int k = 0; k < sh->n_coll; ++k)
    if (sh->coll_pos[k][1] != 0.0f) return false;
  return true;
}

// The kernel class a launch of this model takes: reset (MODE 0) never takes the planar substep or float32 pose algebra.
struct BraxClass {
  bool multi, task, planar, f32;
};
inline BraxClass brax_class(const carl_brax_sys_t* sh, uint32_t flags, bool step) {
  const bool task = brax_is_task(sh), planar_model = brax_is_planar(sh);
  const bool planar = step && !(flags & CARL_FLAG_BRAX_GENERIC) && planar_model;
  // task models run the multi-hinge general kernels; a planar model stepped by the general substep
  // (CARL_FLAG_BRAX_GENERIC): its root's slides need the multi-hinge kernels
  const bool multi = task || brax_is_multi(sh) || (step && planar_model && !planar);
  return {multi, task, planar, step && (flags & CARL_FLAG_BRAX_FP32) != 0};
}

inline bool same_class(const BraxClass& a, const BraxClass& b) {
  return a.multi == b.multi && a.task == b.task && a.planar == b.planar && a.f32 == b.f32;
}

// the narrowest instantiated width >= w of the class in kernel table `tab`; 0 if there is none
template <class Entry, size_t N>
int brax_width_from(const Entry (&tab)[N], const BraxClass& c, int w) {
  int k = 0;
  for (const Entry& e : tab)
    if (same_class(e.c, c) && e.k >= w && (k == 0 || e.k < k)) k = e.k;
  return k;
}

// Lanes per env (the kernels' kSub).  The Brax kernel is bound by the instruction stream a
// wavefront issues (~4.3 cycles per wavefront instruction with two resident waves per SIMD,
// profiles/r01g), so a joint or body round with one busy lane per env costs as much as a full one:
// the width is the number of links (every phase = one round), rounded up to an instantiated
// width of the class, and widened for small batches so that the launch has at least two
// wavefronts per SIMD.  carl_brax_sys_t::lanes_per_env pins it (autotune, tests).
template <class Entry, size_t N>
int brax_lanes_per_env(const Entry (&tab)[N], int n_links, const BraxClass& c, int n_lanes, int hint) {
  int want = n_links;
  bool pinned = false;
  if (hint > 0) {  // sys.lanes_per_env (autotuned by the caller); never narrower than one lane per link (the kernels'
                   // mapping since round 5: a lane keeps its link's body in registers through the substeps)
    want = hint > n_links ? hint : n_links;
    pinned = true;
  }
  int k = brax_width_from(tab, c, want);
  if (k == 0) k = 16;
  if (!pinned)
    while (k < 16 && ((long long)n_lanes + 64 / k - 1) / (64 / k) < 2048) {
      const int next = brax_width_from(tab, c, k + 1);
      k = next == 0 ? 16 : next;
    }
  return k;
}

// The shape of a launch: lanes per env, workgroups, wavefronts per workgroup, dynamic LDS.
struct BraxShape {
  int K, W, grid;
  size_t wave_bytes, lds_bytes;  // dynamic LDS per wavefront / per workgroup
};

// `step`: a step / rollout launch (the kernels' MODE >= 1; false: reset).  `policy`: the closed-loop rollout (MODE 2),
// whose wavefront slice is policy_layout_of's -- the kernel's own choice between the two layouts (run()).
template <class Entry, size_t N>
int brax_launch_shape(const Entry (&tab)[N], const carl_batch_t* b, const carl_brax_sys_t* sh, const BraxClass& c,
                      bool step, int n_steps, bool policy, const char* who, BraxShape* out) {
  const int K = brax_lanes_per_env(tab, sh->n_links, c, b->n_lanes, sh->lanes_per_env);
  const int envs = carl::brax::kLanes / K;  // one wavefront = envs x K lanes; LDS rows are `envs` floats wide
  const carl::brax::Layout lay = policy ? carl::brax::policy_layout_of(*sh) : carl::brax::layout_of(*sh);
  // independent wavefronts per workgroup, sharing the LDS copy of the static tables: as many (<= kMaxWavesPerWg) as fit
  // (the kernel's static LDS: model table, prepared topology / records, the fragment hand-over flags)
  const size_t static_lds = sizeof(carl_brax_sys_t) + sizeof(carl::brax::Prepared) +
                            (size_t)carl::brax::kLinkRecBytes * CARL_BRAX_MAX_LINKS + 16 * CARL_BRAX_MAX_DOF +
                            (size_t)carl::brax::kSphRecBytes * (CARL_BRAX_MAX_COLL + 1) +
                            sizeof(int) * carl::brax::kMaxWavesPerWg3;
  const size_t wave_bytes = lay.bytes(envs);
  if (wave_bytes + static_lds > carl::kCuLdsBytes)
    return fail(CARL_ERR_UNSUPPORTED, "%s: model needs %zu B of LDS per wavefront", who, wave_bytes);
  // Registers allow 2 (multi-hinge / task models) or 3 wavefronts per SIMD = 8 / 12 per CU (brax_kernels.hip.h:
  // CARL_BRAX_WAVES_PER_EU): take the SMALLEST
  // workgroup that gets there LDS-wise (or as close as LDS allows) -- small workgroups retire independently, larger
  // ones cost the launch's tail (Ant, 4 wavefronts per workgroup: 2.97e8 -> 2.57e8 env-steps/s)
  // A step / rollout launch with more groups (a group = one wavefront's `envs` envs) than the chip holds at once:
  // launch exactly the resident number of workgroups; each deals its share of the groups to its wavefronts in
  // equal (group, step-range) pieces (brax_kernels.hip.h: run(), "fragments").  Then fewer, larger workgroups
  // lose less to the rounding of groups per workgroup: take the size with the smallest ceil(groups per
  // workgroup) / wavefronts.
  int n_cu = 256;  // (asked of the current device at every launch: no process-wide cache to go stale in a multi-device process)
  {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
      n_cu = v;
  }
  const int max_w = carl::brax::max_waves_per_wg(c.task);
  const int n_groups = (b->n_lanes + envs - 1) / envs;
  int per_cu_of[16] = {0};
  int W = 1, best = 0;
  for (int w = 1; w <= max_w; ++w) {
    const size_t wg = (size_t)w * wave_bytes + static_lds;
    if (wg > carl::kCuLdsBytes) break;
    if (w > 1 && (long long)(w - 1) * envs >= b->n_lanes) break;  // a small batch: no empty wavefronts
    int per_cu = (int)(carl::kCuLdsBytes / wg) * w;                    // resident wavefronts per CU, LDS-wise
    const int waves_per_eu = c.f32 ? CARL_BRAX_WAVES_PER_EU_F32(c.task) : CARL_BRAX_WAVES_PER_EU(c.task);
    if (per_cu > 4 * waves_per_eu) per_cu = 4 * waves_per_eu;
    per_cu -= per_cu % w;  // whole workgroups
    per_cu_of[w] = per_cu;
    if (per_cu > best) {
      best = per_cu;
      W = w;
    }
  }
  int grid = (n_groups + W - 1) / W;
  // (launches of fewer than 4 env steps keep one wavefront per group, dispatched as slots free up: a fragment
  // boundary costs about one env step, which such a launch cannot amortise -- measured, tools/brax_per_call.py:
  // Ant x 32 768, 2-step launches 205 us as groups vs 226 us as fragments; 5-step launches 452 vs 411 us)
  if (step && n_steps >= 4 && (long long)n_groups > (long long)n_cu * best) {  // more than one "round": the balanced schedule
    double best_cost = 1e30;
    for (int w = 1; w <= max_w; ++w) {
      if (per_cu_of[w] != best) continue;
      const int n_wg = n_cu * (best / w);
      const double cost = (double)((n_groups + n_wg - 1) / n_wg) / (double)w;
      if (cost < best_cost - 1e-9) {
        best_cost = cost;
        W = w;
        grid = n_wg;
      }
    }
  }
  *out = BraxShape{K, W, grid, wave_bytes, (size_t)W * wave_bytes};
  return 0;
}

// What every Brax kernel takes by value beside the model: its topology and derived per-link constants, built on the host
// at every launch (microseconds).
inline carl::brax::Prepared make_prepared(const carl_brax_sys_t* sh) {
  carl::brax::Prepared prep{};
  carl::brax::build_topo_host(*sh, prep.topo);
  carl::brax::build_packed_host(*sh, prep.topo, prep.packed);
  return prep;
}

inline int validate_brax_io(const carl_step_io_t* io, const char* who) {
  if (io == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: io is NULL", who);
  if (!io->action || !io->obs || !io->reward || !io->terminated || !io->truncated)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: a required io pointer is NULL", who);
  if (io->action_dtype != CARL_ACTION_F32)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: Brax families take float32 actions", who);
  if (io->row_pitch != 0)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: Brax families take dense rows (io.row_pitch = 0)", who);
  return 0;
}

}  // namespace brax
}  // namespace carl_host
