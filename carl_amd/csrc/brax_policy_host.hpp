// brax_policy_host.hpp -- the host side of the closed-loop entry points of the Brax families, shared by their five
// translation units (carl_brax_policy.hip: carl_brax_rollout_policy; carl_brax_episodes.hip: carl_brax_evaluate_policy;
// carl_brax_policy_stats.hip: carl_brax_evaluate_policy_stats; carl_brax_policy_sample.hip:
// carl_brax_rollout_policy_sampled; carl_brax_policy_value.hip: carl_brax_rollout_policy_valued): the packed size of a
// policy's shape, the kernel class of a closed-loop launch, the policy's validation against the batch and the model, the list of kernel instances and the entry
// type of a unit's table of them, the kernels' policy argument, the launch shape and the launch.  Host code only; the
// kernels are each unit's own: every table is one expansion of the list with the unit's kernel template.
#pragma once

#include <cstdint>

#include "../../include/carl_amd.h"
#include "brax_launch.hpp"
#include "host_common.hpp"
#include "policy_host.hpp"

namespace carl_host {
namespace brax {

inline int brax_policy_floats(const carl_policy_t* p) {
  if (p->n_in < 1 || p->n_in > CARL_POLICY_MAX_IN || p->n_out < 1 || p->n_out > CARL_BRAX_MAX_ACT || p->n_hidden < 0 ||
      p->n_hidden > CARL_POLICY_MAX_HIDDEN)
    return -1;
  for (int l = 0; l < p->n_hidden; ++l)
    if (p->width[l] < 1 || p->width[l] > CARL_POLICY_MAX_WIDTH) return -1;
  const int64_t total = (int64_t)carl_host::policy_transform_offset(p) + 2 * (int64_t)p->n_in + 1;
  return (int)((total + 3) / 4 * 4);
}

// the class of a closed-loop launch, or the refusal of CARL_FLAG_BRAX_FP32
inline int policy_class(const char* who, const carl_batch_t* b, const carl_brax_sys_t* sh, BraxClass* c) {
  if (b->flags & CARL_FLAG_BRAX_FP32)
    return fail(CARL_ERR_UNSUPPORTED, "%s: CARL_FLAG_BRAX_FP32 is not built for the closed-loop rollout (the float64 "
                "kernel classes only)", who);
  *c = brax_class(sh, b->flags, true);
  return 0;
}

inline int validate_policy(const char* who, const carl_batch_t* b, const carl_brax_sys_t* sh, const carl_policy_t* p) {
  if (int e = carl_host::check_hidden_layers(who, p)) return e;
  if (p->n_ctx < 0 || p->n_ctx > CARL_POLICY_MAX_IN)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_ctx %d outside [0, %d]", who, p->n_ctx, CARL_POLICY_MAX_IN);
  if (p->n_ctx + sh->obs_dim > CARL_POLICY_MAX_IN)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: %d context inputs + %d observations are more than CARL_POLICY_MAX_IN = %d "
                "policy inputs (Humanoid-size observations are out of scope)", who, p->n_ctx, sh->obs_dim, CARL_POLICY_MAX_IN);
  // a Brax batch does not say how many rows its context table has: a policy sees the rows the batch makes visible
  for (int k = 0; k < p->n_ctx; ++k) {
    bool visible = false;
    for (int j = 0; j < b->n_ctx_obs && j < CARL_MAX_CTX_OBS; ++j) visible |= b->ctx_obs_feat[j] == p->ctx_rows[k];
    if (p->ctx_rows[k] < 0 || !visible)
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: ctx_rows[%d] = %d is not one of the batch's observed context rows "
                  "(ctx_obs_feat)", who, k, p->ctx_rows[k]);
  }
  if (p->n_in != p->n_ctx + sh->obs_dim)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_in %d != n_ctx %d + obs_dim %d", who, p->n_in, p->n_ctx, sh->obs_dim);
  if (p->n_out != sh->n_act)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: head width %d, the model has %d actuators", who, p->n_out, sh->n_act);
  if (p->head != CARL_POLICY_HEAD_BOX)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: head kind %d: the Brax families take Box actions (CARL_POLICY_HEAD_BOX)", who,
                p->head);
  if (int e = carl_host::check_activation(who, p)) return e;
  if (p->n_sets < 1) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_sets %d < 1", who, p->n_sets);
  const int q = carl_policy_lane_quantum();
  if (p->lanes_per_set < q || p->lanes_per_set % q != 0)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: lanes_per_set %d is not a positive multiple of %d (carl_policy_lane_quantum)",
                who, p->lanes_per_set, q);
  if ((int64_t)p->n_sets * p->lanes_per_set < b->n_lanes)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: %d sets x %d lanes do not cover %d lanes", who, p->n_sets, p->lanes_per_set,
                b->n_lanes);
  if (int e = carl_host::check_params(who, p)) return e;
  if (reinterpret_cast<uintptr_t>(p->params) % 16 != 0)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: params must start on a 16-byte boundary (weight rows are read 16 bytes at a time)",
                who);
  return 0;
}

// What every entry point checks first, in this order: the batch and the model, policy / obs non-NULL, the kernel class
// (CARL_FLAG_BRAX_FP32 is refused), the policy.
inline int validate_closed_loop(const char* who, const carl_batch_t* batch, const carl_brax_sys_t* sys_dev,
                                const carl_brax_sys_t* sys_host, const float* obs, const carl_policy_t* policy_host,
                                BraxClass* c) {
  if (int e = validate_brax(batch, sys_dev, sys_host, who)) return e;
  if (policy_host == nullptr || obs == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: policy / obs is NULL", who);
  if (int e = policy_class(who, batch, sys_host, c)) return e;
  return validate_policy(who, batch, sys_host, policy_host);
}

// What the rollout entry points (carl_brax_rollout_policy, carl_brax_rollout_policy_sampled,
// carl_brax_rollout_policy_valued) check after that, in this order: the step count, io (NULL: summary mode) and the summary.
inline bool summary_complete(const carl_policy_summary_t* s) { return s->episodes && s->return_sum && s->length_sum; }
inline int validate_rollout(const char* who, const carl_batch_t* batch, const carl_step_io_t* io, int32_t n_steps,
                            const carl_policy_summary_t* summary_out) {
  if (n_steps < 0) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_steps %d < 0", who, n_steps);
  if (io == nullptr) {
    if (summary_out == nullptr || !summary_complete(summary_out))
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: summary mode (io NULL) needs all three summary arrays", who);
  } else {
    if (int e = validate_brax_io(io, who)) return e;
    if (summary_out != nullptr && !summary_complete(summary_out))
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: a summary needs all three arrays", who);
  }
  if (summary_out != nullptr && !(batch->flags & CARL_FLAG_AUTORESET))
    return fail(CARL_ERR_UNSUPPORTED, "%s: a summary needs CARL_FLAG_AUTORESET (without auto-reset a finished lane "
                "reports done on every later step, and its episode would be counted on each of them)", who);
  return 0;
}

// What the sampled entry points (carl_brax_rollout_policy_sampled, carl_brax_rollout_policy_valued) check after that, in
// this order.  block << 28 | elapsed under the draws' 0x40000000 tag: two bits of block (eight actuators), 28 of elapsed.
constexpr int kMaxSampledAct = 8;
constexpr int64_t kMaxSampledEpisodeSteps = (int64_t)1 << 28;
inline int validate_sampling(const char* who, const carl_batch_t* batch, const carl_brax_sys_t* sys_host,
                             const carl_step_io_t* io, const carl_policy_sampling_t* sampling) {
  if (sampling == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: sampling is NULL", who);
  if (sampling->log_std == nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: sampling->log_std is NULL (one value per weight set and actuator)", who);
  if (io == nullptr && sampling->log_prob != nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: log_prob in summary mode (io NULL): a summary stores nothing per step", who);
  if (sys_host->n_act > kMaxSampledAct)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: %d actuators: the draws' counter holds the Philox block in two bits (at most "
                "%d actuators)", who, sys_host->n_act, kMaxSampledAct);
  if (batch->max_episode_steps <= 0 || (int64_t)batch->max_episode_steps > kMaxSampledEpisodeSteps)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: max_episode_steps %lld outside [1, 2^28]: the draws' counter holds the step "
                "count of an episode in 28 bits", who, (long long)batch->max_episode_steps);
  return 0;
}

// What the episodes entry points (carl_brax_evaluate_policy, carl_brax_evaluate_policy_stats) check after that, in this order.
inline int validate_episodes(const char* who, const carl_batch_t* batch, int32_t n_episodes, int32_t max_steps,
                             const carl_policy_episodes_t* out) {
  if (out == nullptr || !out->episodes || !out->steps || !out->ret || !out->length || !out->context_id || !out->terminated)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: out and its six arrays must not be NULL", who);
  if (n_episodes < 1) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_episodes %d < 1", who, n_episodes);
  if (max_steps < 0) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: max_steps %d < 0", who, max_steps);
  if ((int64_t)n_episodes * batch->n_lanes >= (int64_t)1 << 31)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: %d episodes x %d lanes: more than 2^31 - 1 records", who, n_episodes,
                batch->n_lanes);
  if (!(batch->flags & CARL_FLAG_AUTORESET))
    return fail(CARL_ERR_UNSUPPORTED, "%s: needs CARL_FLAG_AUTORESET (without auto-reset a finished lane reports done on "
                "every later step, and its episode would be counted on each of them)", who);
  return 0;
}

// Every instantiated closed-loop kernel<MULTI, K, TASK, PLANAR>, of each of the five variants: the non-F32 step classes
// of carl_brax.hip's kBraxKernels, at the widths it has for them (tests/test_brax_policy_abi.py holds the list against
// that table).  A unit's table is `#define X(M, K, T, P) {{M, T, P, false}, K, its_kernel<M, K, T, P>},` around one
// expansion.
#define CARL_BRAX_CLOSED_LOOP_INSTANCES(X)                                                                      \
  /* lean */                                                                                                    \
  X(false, 4, false, false) X(false, 7, false, false) X(false, 8, false, false) X(false, 9, false, false)       \
  X(false, 16, false, false)                                                                                    \
  /* multi-hinge */                                                                                             \
  X(true, 2, false, false) X(true, 11, false, false) X(true, 16, false, false)                                  \
  /* general: reach / push task models and anisotropic inertia */                                               \
  X(true, 4, true, false) X(true, 8, true, false) X(true, 16, true, false)                                      \
  /* planar */                                                                                                  \
  X(false, 4, false, true) X(false, 7, false, true) X(false, 8, false, true) X(false, 9, false, true)           \
  X(false, 16, false, true)

// An entry of a unit's table; Pol: the kernels' policy argument (carl::brax::BraxPolicy or a variant of it).
template <class Pol>
struct ClosedLoopKernel {
  static_assert(sizeof(carl_batch_t) + sizeof(carl::brax::Prepared) + sizeof(carl_step_io_t) + sizeof(Pol) + 64 <= 4096,
                "the closed-loop kernel's arguments do not fit the 4 KiB kernel-argument segment");
  BraxClass c;
  int k;
  void (*kern)(carl_batch_t, const carl_brax_sys_t*, carl::brax::Prepared, carl_step_io_t, Pol, int);
};

// The kernels' policy argument, level by level.  BraxPolicy's fields, of it or a variant `Pol` of it: no summary.
template <class Pol>
Pol make_policy(const carl_policy_t* policy_host, float* obs) {
  Pol pol{};
  pol.p = *policy_host;
  pol.set_floats = brax_policy_floats(policy_host);
  pol.sum = carl_policy_summary_t{nullptr, nullptr, nullptr};
  pol.cur_obs = obs;
  return pol;
}
// BraxEpisodesPolicy's on top of them.
template <class Pol>
Pol make_episodes_policy(const carl_policy_t* policy_host, float* obs, const carl_policy_episodes_t* out, int32_t n_episodes) {
  Pol pol = make_policy<Pol>(policy_host, obs);
  pol.ep = *out;
  pol.n_episodes = n_episodes;
  return pol;
}

// The shape of a closed-loop launch of n_steps (episodes mode: max_steps) steps, and its kernel out of the unit's table
// `tab`: one rule for every entry point, whose tables hold the same (class, width) instances, so
// carl_brax_policy_launch_shape answers for all of them.
template <class Entry, size_t N>
int policy_launch(const Entry (&tab)[N], const carl_batch_t* batch, const carl_brax_sys_t* sys_host, const BraxClass& c,
                  int n_steps, const char* who, BraxShape* shape, decltype(Entry::kern)* kern) {
  if (int e = brax_launch_shape(tab, batch, sys_host, c, true, n_steps, true, who, shape)) return e;
  if (kern == nullptr) return 0;  // (the shape alone)
  *kern = nullptr;
  for (const Entry& e : tab)
    if (same_class(e.c, c) && e.k == shape->K) *kern = e.kern;
  if (*kern == nullptr) return fail(CARL_ERR_UNSUPPORTED, "%s: no kernel for %d lanes per env", who, shape->K);
  if (shape->lds_bytes > 48 * 1024) {
    if (int e = carl_host::ensure_dynamic_lds(reinterpret_cast<const void*>(*kern), shape->lds_bytes, who)) return e;
  }
  return 0;
}

// The launch of every closed-loop entry point: n_steps (episodes mode: max_steps) > 0 steps of a batch with lanes.
// io_v all NULL: no per-step record (run()'s summary mode).
template <class Pol, size_t N>
int launch_closed_loop(const ClosedLoopKernel<Pol> (&tab)[N], const carl_batch_t* batch, const carl_brax_sys_t* sys_dev,
                       const carl_brax_sys_t* sys_host, const BraxClass& c, int n_steps, const carl_step_io_t& io_v,
                       const Pol& pol, void* stream, const char* who) {
  BraxShape shape;
  decltype(ClosedLoopKernel<Pol>::kern) kern = nullptr;
  if (int e = policy_launch(tab, batch, sys_host, c, n_steps, who, &shape, &kern)) return e;
  const carl::brax::Prepared prep = make_prepared(sys_host);
  hipLaunchKernelGGL(kern, dim3(shape.grid), dim3(carl::brax::kLanes * shape.W), shape.lds_bytes, (hipStream_t)stream, *batch,
                     sys_dev, prep, io_v, pol, n_steps);
  return check_launch(who);
}

}  // namespace brax
}  // namespace carl_host
