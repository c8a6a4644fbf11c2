// ppo_host_checks.hpp -- the shape and grid rules and the checks, with their messages, of the PPO update on the device: what
// ppo_host.hpp's launch path (carl_ppo.hip, carl_brax_ppo.hip) and a population's unit (carl_ppo_sets.hip) share.  Each rule
// is written once.  Host code only: including this file instantiates no kernel (ppo_host.hpp's launch_ppo_net does).
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/carl_amd.h"
#include "host_common.hpp"
#include "policy_host.hpp"
#include "ppo_device.hip.h"

namespace carl_host {

// set_floats: the unit's packed size of a network (policy_set_floats / carl_brax_policy_set_floats)
inline carl::PpoShape ppo_shape_of(const carl_policy_t* p, int (*set_floats)(const carl_policy_t*)) {
  carl::PpoShape s{};
  s.n_in = p->n_in, s.n_out = p->n_out, s.n_hidden = p->n_hidden, s.act = p->activation;
  s.w0 = p->n_hidden > 0 ? p->width[0] : 0;
  s.w1 = p->n_hidden > 1 ? p->width[1] : 0;
  s.weight_floats = policy_transform_offset(p);
  s.set_floats = set_floats(p);
  return s;
}

// carl_ppo_grad_workgroups / carl_brax_ppo_grad_workgroups
inline int ppo_workgroups(int32_t n_samples) {
  if (n_samples < 1) return 0;
  const int tiles = (n_samples + carl::kPpoTile - 1) / carl::kPpoTile;
  return tiles < carl::kPpoMaxWorkgroups ? tiles : carl::kPpoMaxWorkgroups;
}

inline bool ppo_bad_coef(float v) { return !std::isfinite(v) || v < 0.0f; }

// What carl_ppo_grad and carl_ppo_grad_sets check of a classic-control buffer first: the family (*fi receives its info), the
// lane and step counts, the pitch and the observation width
inline int check_ppo_classic_buffer(const char* who, const carl_ppo_batch_t* ppo, carl_family_info_t* fi) {
  if (ppo->family >= CARL_N_FAMILIES)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: family %d is a Brax family -- the PPO update covers the classic-control "
                "families only", who, ppo->family);
  if (int e = carl_family_info(ppo->family, fi)) return e;
  if (ppo->n_lanes < 1 || ppo->n_steps < 1)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_lanes %d / n_steps %d < 1", who, ppo->n_lanes, ppo->n_steps);
  if (ppo->row_pitch != 0 && ppo->row_pitch < ppo->n_lanes)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: row_pitch %d < n_lanes %d", who, ppo->row_pitch, ppo->n_lanes);
  if (ppo->obs_dim != fi->obs_dim)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: obs_dim %d, the family's is %d", who, ppo->obs_dim, fi->obs_dim);
  return 0;
}

// the action column's dtype against the family's head
inline int check_ppo_classic_action(const char* who, const carl_ppo_batch_t* ppo, const carl_family_info_t& fi) {
  if (ppo->action_dtype != (fi.action_is_discrete ? CARL_ACTION_I32 : CARL_ACTION_F32))
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: the action column is %s for this family", who,
                fi.action_is_discrete ? "int32 (CARL_ACTION_I32)" : "float32 (CARL_ACTION_F32)");
  return 0;
}

// What carl_rollout_policy_valued checks of a classic-control network's shape, without a batch (carl_ppo_grad,
// carl_ppo_grad_sets): `fi` the family's info, `head_out` the head width the family needs of this network.  The weight
// sets and params are the entry point's to check.
inline int check_ppo_classic_network(const char* who, const carl_policy_t* p, const carl_family_info_t& fi, int head_out,
                                     const char* kind) {
  if (int e = check_hidden_layers(who, p)) return e;
  if (p->n_ctx < 0 || p->n_ctx > fi.n_features)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_ctx %d outside [0, F = %d]", who, p->n_ctx, fi.n_features);
  for (int k = 0; k < p->n_ctx; ++k)
    if (p->ctx_rows[k] < 0 || p->ctx_rows[k] >= fi.n_features)
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: ctx_rows[%d] = %d is not a context-table row (F = %d)", who, k,
                  p->ctx_rows[k], fi.n_features);
  if (p->n_in != p->n_ctx + fi.obs_dim)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_in %d != n_ctx %d + obs_dim %d", who, p->n_in, p->n_ctx, fi.obs_dim);
  if (p->n_out != head_out)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: head width %d, the family needs %d (%s)", who, p->n_out, head_out, kind);
  return check_activation(who, p);
}

// `cwho`: "<entry point>: critic"
inline int check_ppo_critic_inputs(const char* cwho, const carl_policy_t* critic, const carl_policy_t* actor) {
  if (critic->n_ctx != actor->n_ctx)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_ctx %d, the actor has %d (the critic reads the actor's inputs)", cwho,
                critic->n_ctx, actor->n_ctx);
  for (int k = 0; k < actor->n_ctx; ++k)
    if (critic->ctx_rows[k] != actor->ctx_rows[k])
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: ctx_rows[%d] = %d, the actor's is %d", cwho, k, critic->ctx_rows[k],
                  actor->ctx_rows[k]);
  return 0;
}

// What both entry points check of the batch and the outputs after their own checks, in this order; pitch: the unit's
// resolved row pitch (never 0)
inline int check_ppo_batch(const char* who, const carl_ppo_batch_t* ppo, int pitch, const carl_ppo_out_t* out) {
  if (ppo->n_contexts < 1 || ppo->ctx_stride < ppo->n_contexts)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_contexts %d / ctx_stride %d invalid", who, ppo->n_contexts,
                ppo->ctx_stride);
  const int64_t all = (int64_t)ppo->n_steps * ppo->n_lanes;
  if ((int64_t)ppo->n_steps * pitch >= ((int64_t)1 << 31))
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: %d steps x %d lanes per row: flat indices do not fit 2^31 - 1", who,
                ppo->n_steps, pitch);
  if (ppo->n_samples < 1) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_samples %d < 1", who, ppo->n_samples);
  if (ppo->n_samples > all)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_samples %d > n_steps %d x n_lanes %d", who, ppo->n_samples, ppo->n_steps,
                ppo->n_lanes);
  if (ppo->idx == nullptr && ppo->n_samples != all)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: idx is NULL (every sample) but n_samples %d != n_steps %d x n_lanes %d", who,
                ppo->n_samples, ppo->n_steps, ppo->n_lanes);
  if (ppo_bad_coef(ppo->clip_range)) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: clip_range %g is not finite and >= 0", who, (double)ppo->clip_range);
  if (ppo_bad_coef(ppo->vf_coef)) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: vf_coef %g is not finite and >= 0", who, (double)ppo->vf_coef);
  if (ppo_bad_coef(ppo->ent_coef)) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: ent_coef %g is not finite and >= 0", who, (double)ppo->ent_coef);
  if (!ppo->obs0 || !ppo->obs || !ppo->context_id || !ppo->ctx_table || !ppo->action || !ppo->log_prob || !ppo->advantage ||
      !ppo->ret)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: a required pointer of ppo is NULL (all but idx and adv_norm)", who);
  if (!out->grad_actor || !out->grad_critic || !out->stats)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: out->grad_actor, out->grad_critic and out->stats are required", who);
  return 0;
}

// need: the unit's workspace size for this call; size_fn: the name of the function that returns it, for the message
inline int check_ppo_workspace(const char* who, const carl_ppo_out_t* out, int64_t need, const char* size_fn) {
  if (out->workspace == nullptr || (reinterpret_cast<uintptr_t>(out->workspace) & 15) != 0)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: out->workspace is NULL or not on a 16-byte boundary", who);
  if (out->workspace_floats < need)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: workspace of %lld floats, %lld needed (%s)", who,
                (long long)out->workspace_floats, (long long)need, size_fn);
  return 0;
}

}  // namespace carl_host
