// carl_brax_ppo.hip -- C-ABI entry points of the PPO update of the Brax families (include/carl_amd.h:
// carl_brax_policy_context_trace, carl_brax_ppo_grad) and their launches.  A translation unit of its own, so that every
// other unit's kernels compile exactly as they did.  The actor's kernel and the reduction are brax_ppo_kernels.hip.h's;
// the critic is this unit's instances of ppo_net_kernel<H> through ppo_host.hpp's launch_ppo_net, the trace carl_ppo.hip's
// context_trace_kernel through launch_context_trace.  The host path the two units share is ppo_host.hpp's; the packed
// size of a Brax network is carl_brax_policy_set_floats(), the shape checks policy_host.hpp's.
#include "classic_control.hip.h"
#include "ppo_host.hpp"
#include "brax_ppo_kernels.hip.h"

namespace {

using carl_host::fail;
// floats per packed weight set under the Brax packing rule (carl_brax_policy.hip), -1 for an invalid shape
int brax_policy_floats(const carl_policy_t* p) { return carl_brax_policy_set_floats(p); }

bool classic_family(int32_t family) { return family >= 0 && family < CARL_N_FAMILIES; }

// what carl_brax_rollout_policy_valued checks of a network, without a batch (a carl_ppo_batch_t does not say which
// context rows its producer made visible: a row index is checked for its sign alone); head_out: the head width needed
int check_network(const char* who, const carl_policy_t* p, const carl_brax_sys_t* sh, int head_out, const char* kind) {
  if (int e = carl_host::check_hidden_layers(who, p)) return e;
  if (p->n_ctx < 0 || p->n_ctx > CARL_POLICY_MAX_IN)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_ctx %d outside [0, %d]", who, p->n_ctx, CARL_POLICY_MAX_IN);
  if (p->n_ctx + sh->obs_dim > CARL_POLICY_MAX_IN)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: %d context inputs + %d observations are more than CARL_POLICY_MAX_IN = %d "
                "policy inputs (Humanoid-size observations are out of scope)", who, p->n_ctx, sh->obs_dim, CARL_POLICY_MAX_IN);
  for (int k = 0; k < p->n_ctx; ++k)
    if (p->ctx_rows[k] < 0)
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: ctx_rows[%d] = %d is not a context-table row", who, k, p->ctx_rows[k]);
  if (p->n_in != p->n_ctx + sh->obs_dim)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_in %d != n_ctx %d + obs_dim %d", who, p->n_in, p->n_ctx, sh->obs_dim);
  if (p->n_out != head_out)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: head width %d, the model needs %d (%s)", who, p->n_out, head_out, kind);
  if (p->head != CARL_POLICY_HEAD_BOX)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: head kind %d: the Brax families take Box actions (CARL_POLICY_HEAD_BOX)", who,
                p->head);
  if (int e = carl_host::check_activation(who, p)) return e;
  if (p->n_sets != 1)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_sets %d, a gradient step has one weight set (several are evolution "
                "strategies' territory)", who, p->n_sets);
  return carl_host::check_params(who, p);
}

int launch_actor(const char* who, int H, const carl::PpoNetArgs& a, int grid, hipStream_t s) {
  return carl_host::with_padded_hidden(H, [&](auto h) {
    constexpr int kH = decltype(h)::value;
    static_assert(carl::brax_ppo_lds_bytes(kH) <= carl::kCuLdsBytes, "the Brax PPO actor launch's LDS does not fit a compute unit");
    return carl_host::launch_ppo_kernel(who, carl::brax_ppo_actor_kernel<kH>, carl::brax_ppo_lds_bytes(kH), a, grid, s);
  });
}

}  // namespace

extern "C" {

int32_t carl_brax_ppo_tile(void) { return carl::kPpoTile; }

int32_t carl_brax_ppo_grad_workgroups(int32_t n_samples) { return carl_host::ppo_workgroups(n_samples); }

int64_t carl_brax_ppo_workspace_floats(const carl_policy_t* policy_host, const carl_policy_t* critic_host, int32_t n_samples) {
  if (policy_host == nullptr || critic_host == nullptr || n_samples < 1) return -1;
  if (brax_policy_floats(policy_host) < 0 || brax_policy_floats(critic_host) < 0) return -1;
  if (policy_host->n_out > carl::kBraxPpoOut || critic_host->n_out != 1) return -1;
  return (int64_t)carl_host::ppo_workgroups(n_samples) *
         (carl::brax_ppo_slab_floats(carl_host::policy_padded_hidden(policy_host)) +
          carl::ppo_slab_floats(carl_host::policy_padded_hidden(critic_host)));
}

int carl_brax_policy_context_trace(const carl_batch_t* batch, const int32_t* ctx_idx0, const uint32_t* episode0,
                                   const uint8_t* terminated, const uint8_t* truncated, int32_t n_steps,
                                   int32_t* context_id, void* stream) {
  const char* who = "carl_brax_policy_context_trace";
  if (batch == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: batch is NULL", who);
  if (classic_family(batch->family))
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: family %d is a classic-control family -- its trace is "
                "carl_policy_context_trace", who, batch->family);
  if (batch->n_lanes < 0 || n_steps < 0)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_lanes %d / n_steps %d < 0", who, batch->n_lanes, n_steps);
  if (batch->n_contexts < 1) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_contexts %d < 1", who, batch->n_contexts);
  if (batch->selector < CARL_SEL_STATIC || batch->selector > CARL_SEL_HOST)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: unknown selector %d", who, batch->selector);
  if (!ctx_idx0 || !episode0 || !terminated || !truncated || !context_id)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: a required pointer is NULL", who);
  if (batch->n_lanes == 0 || n_steps == 0) return 0;
  // The first-state auto-reset keeps a done env's context and episode counter (brax_kernels.hip.h: the auto-reset branch
  // of Group<K>::run): for the walk that is a batch without auto-reset.
  carl_batch_t b = *batch;
  if ((b.flags & CARL_FLAG_AUTORESET_FIRST_STATE) && b.first_state != nullptr) b.flags &= ~(uint32_t)CARL_FLAG_AUTORESET;
  return carl_host::launch_context_trace(who, b, ctx_idx0, episode0, terminated, truncated, n_steps, b.n_lanes, context_id,
                                         (hipStream_t)stream);
}

int carl_brax_ppo_grad(const carl_ppo_batch_t* ppo, const carl_brax_sys_t* sys_host, const carl_policy_t* policy_host,
                       const carl_policy_t* critic_host, const float* log_std, const carl_ppo_out_t* out, void* stream) {
  const char* who = "carl_brax_ppo_grad";
  if (ppo == nullptr || sys_host == nullptr || policy_host == nullptr || critic_host == nullptr || out == nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: ppo / sys / policy / critic / out is NULL", who);
  if (classic_family(ppo->family))
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: family %d is a classic-control family -- its update is carl_ppo_grad", who,
                ppo->family);
  if (ppo->n_lanes < 1 || ppo->n_steps < 1)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_lanes %d / n_steps %d < 1", who, ppo->n_lanes, ppo->n_steps);
  if (ppo->row_pitch != 0 && ppo->row_pitch != ppo->n_lanes)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: row_pitch %d: Brax families take dense rows (0 or n_lanes = %d)", who,
                ppo->row_pitch, ppo->n_lanes);
  if (sys_host->obs_dim < 1 || sys_host->n_act < 1 || sys_host->n_act > CARL_BRAX_MAX_ACT)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: model table out of range", who);
  if (ppo->obs_dim != sys_host->obs_dim)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: obs_dim %d, the model's is %d", who, ppo->obs_dim, sys_host->obs_dim);
  if (sys_host->n_act > carl::kBraxPpoOut)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: %d actuators: the sampled closed loop and its update hold at most %d", who,
                sys_host->n_act, carl::kBraxPpoOut);
  if (int e = check_network(who, policy_host, sys_host, sys_host->n_act, "one output per actuator")) return e;
  const char* cwho = "carl_brax_ppo_grad: critic";
  if (int e = check_network(cwho, critic_host, sys_host, 1, "a value network has 1")) return e;
  if (int e = carl_host::check_ppo_critic_inputs(cwho, critic_host, policy_host)) return e;
  if (ppo->action_dtype != CARL_ACTION_F32)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: the action column is float32 (CARL_ACTION_F32) for the Brax families", who);
  const int pitch = ppo->n_lanes;  // (dense rows)
  if (int e = carl_host::check_ppo_batch(who, ppo, pitch, out)) return e;
  if (log_std == nullptr || out->grad_log_std == nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: log_std and out->grad_log_std are required ([n_act] on the device)", who);
  const int64_t need = carl_brax_ppo_workspace_floats(policy_host, critic_host, ppo->n_samples);
  if (int e = carl_host::check_ppo_workspace(who, out, need, "carl_brax_ppo_workspace_floats")) return e;

  const hipStream_t s = (hipStream_t)stream;
  const carl_host::PpoUnit unit{brax_policy_floats, carl::brax_ppo_slab_floats, carl::brax_ppo_reduce_kernel,
                                6 + carl::kBraxPpoOut};
  return carl_host::launch_ppo_update(
      who, unit, ppo, pitch, carl::kPpoGaussian, policy_host, critic_host, log_std, out, s,
      [&](int H, const carl::PpoNetArgs& a, int grid) { return launch_actor(who, H, a, grid, s); });
}

}  // extern "C"
