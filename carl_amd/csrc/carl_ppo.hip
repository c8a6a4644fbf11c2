// carl_ppo.hip -- C-ABI entry points of the PPO update on the device (include/carl_amd.h: carl_policy_context_trace,
// carl_ppo_grad) and their launches.  A translation unit of its own, so that every other unit's kernels compile exactly
// as they did.  The kernels are ppo_kernels.hip.h's; this unit holds the library's one trace walk, which the Brax unit
// launches through launch_context_trace below.  The host path the two units share is ppo_host.hpp's, the network shape
// checks the closed-loop rollout shares are policy_host.hpp's.
#include "classic_control.hip.h"
#include "ppo_host.hpp"
#include "ppo_kernels.hip.h"

int carl_host::launch_context_trace(const char* who, const carl_batch_t& b, const int32_t* ctx_idx0, const uint32_t* episode0,
                                    const uint8_t* terminated, const uint8_t* truncated, int n_steps, int pitch,
                                    int32_t* context_id, hipStream_t s) {
  const int grid = (b.n_lanes + carl::kTraceThreads - 1) / carl::kTraceThreads;
  hipLaunchKernelGGL(carl::context_trace_kernel, dim3(grid), dim3(carl::kTraceThreads), 0, s, b, ctx_idx0, episode0,
                     terminated, truncated, n_steps, pitch, context_id);
  return check_launch(who);
}

namespace {

using carl_host::fail;

// ppo_host.hpp's check of a classic network's shape, then what is this entry point's: one weight set
int check_network(const char* who, const carl_policy_t* p, const carl_family_info_t& fi, int head_out, const char* kind) {
  if (int e = carl_host::check_ppo_classic_network(who, p, fi, head_out, kind)) return e;
  if (p->n_sets != 1)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_sets %d, a gradient step has one weight set (several are evolution "
                "strategies' territory)", who, p->n_sets);
  return carl_host::check_params(who, p);
}

}  // namespace

extern "C" {

int32_t carl_ppo_tile(void) { return carl::kPpoTile; }

int32_t carl_ppo_grad_workgroups(int32_t n_samples) { return carl_host::ppo_workgroups(n_samples); }

int64_t carl_ppo_workspace_floats(const carl_policy_t* policy_host, const carl_policy_t* critic_host, int32_t n_samples) {
  if (policy_host == nullptr || critic_host == nullptr || n_samples < 1) return -1;
  if (carl_host::policy_set_floats(policy_host) < 0 || carl_host::policy_set_floats(critic_host) < 0) return -1;
  return (int64_t)carl_host::ppo_workgroups(n_samples) *
         (carl::ppo_slab_floats(carl_host::policy_padded_hidden(policy_host)) +
          carl::ppo_slab_floats(carl_host::policy_padded_hidden(critic_host)));
}

int carl_policy_context_trace(const carl_batch_t* batch, const int32_t* ctx_idx0, const uint32_t* episode0,
                              const uint8_t* terminated, const uint8_t* truncated, int32_t n_steps, int32_t row_pitch,
                              int32_t* context_id, void* stream) {
  const char* who = "carl_policy_context_trace";
  if (batch == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: batch is NULL", who);
  if (batch->family >= CARL_N_FAMILIES)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: family %d is a Brax family -- the PPO update covers the classic-control "
                "families only", who, batch->family);
  if (batch->family < 0) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: unknown family %d", who, batch->family);
  if (batch->n_lanes < 0 || n_steps < 0)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_lanes %d / n_steps %d < 0", who, batch->n_lanes, n_steps);
  if (batch->n_contexts < 1) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_contexts %d < 1", who, batch->n_contexts);
  if (batch->selector < CARL_SEL_STATIC || batch->selector > CARL_SEL_HOST)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: unknown selector %d", who, batch->selector);
  if (row_pitch != 0 && row_pitch < batch->n_lanes)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: row_pitch %d < n_lanes %d", who, row_pitch, batch->n_lanes);
  if (!ctx_idx0 || !episode0 || !terminated || !truncated || !context_id)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: a required pointer is NULL", who);
  if (batch->n_lanes == 0 || n_steps == 0) return 0;
  return carl_host::launch_context_trace(who, *batch, ctx_idx0, episode0, terminated, truncated, n_steps,
                                         row_pitch > 0 ? row_pitch : batch->n_lanes, context_id, (hipStream_t)stream);
}

int carl_ppo_grad(const carl_ppo_batch_t* ppo, const carl_policy_t* policy_host, const carl_policy_t* critic_host,
                  const float* log_std, const carl_ppo_out_t* out, void* stream) {
  const char* who = "carl_ppo_grad";
  if (ppo == nullptr || policy_host == nullptr || critic_host == nullptr || out == nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: ppo / policy / critic / out is NULL", who);
  carl_family_info_t fi;
  if (int e = carl_host::check_ppo_classic_buffer(who, ppo, &fi)) return e;
  const int want_out = fi.action_is_discrete ? fi.n_actions : 1;
  if (int e = check_network(who, policy_host, fi, want_out, fi.action_is_discrete ? "n_actions" : "one Box value")) return e;
  if (policy_host->head != (fi.action_is_discrete ? CARL_POLICY_HEAD_ARGMAX : CARL_POLICY_HEAD_BOX))
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: head kind %d does not match the family's action space", who,
                policy_host->head);
  const char* cwho = "carl_ppo_grad: critic";
  if (int e = check_network(cwho, critic_host, fi, 1, "a value network has 1")) return e;
  if (int e = carl_host::check_ppo_critic_inputs(cwho, critic_host, policy_host)) return e;
  if (int e = carl_host::check_ppo_classic_action(who, ppo, fi)) return e;
  const int pitch = ppo->row_pitch > 0 ? ppo->row_pitch : ppo->n_lanes;
  if (int e = carl_host::check_ppo_batch(who, ppo, pitch, out)) return e;
  if (!fi.action_is_discrete && (log_std == nullptr || out->grad_log_std == nullptr))
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: a Box family needs log_std and out->grad_log_std ([1] on the device)", who);
  const int64_t need = carl_ppo_workspace_floats(policy_host, critic_host, ppo->n_samples);
  if (int e = carl_host::check_ppo_workspace(who, out, need, "carl_ppo_workspace_floats")) return e;

  const hipStream_t s = (hipStream_t)stream;
  const carl_host::PpoUnit unit{carl_host::policy_set_floats, carl::ppo_slab_floats, carl::ppo_reduce_kernel, 8};
  return carl_host::launch_ppo_update(
      who, unit, ppo, pitch, fi.action_is_discrete ? carl::kPpoCategorical : carl::kPpoGaussian, policy_host, critic_host,
      log_std, out, s, [&](int H, const carl::PpoNetArgs& a, int grid) { return carl_host::launch_ppo_net(who, H, a, grid, s); });
}

}  // extern "C"
