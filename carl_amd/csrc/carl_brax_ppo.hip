// carl_brax_ppo.hip -- C-ABI entry points of the PPO update of the Brax families (include/carl_amd.h:
// carl_brax_policy_context_trace, carl_brax_ppo_grad) and their launches.  A translation unit of its own, so that every
// other unit's kernels compile exactly as they did.  The actor's kernel and the reduction are brax_ppo_kernels.hip.h's;
// the critic's launch and the trace are instances of ppo_kernels.hip.h's kernels as they are; the packed size of a Brax
// network is carl_brax_policy_set_floats(), the shape checks policy_host.hpp's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/carl_amd.h"
#include "classic_control.hip.h"
#include "host_common.hpp"
#include "policy_host.hpp"
#include "brax_ppo_kernels.hip.h"

namespace {

using carl_host::check_launch;
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

carl::PpoShape shape_of(const carl_policy_t* p) {
  carl::PpoShape s{};
  s.n_in = p->n_in, s.n_out = p->n_out, s.n_hidden = p->n_hidden, s.act = p->activation;
  s.w0 = p->n_hidden > 0 ? p->width[0] : 0;
  s.w1 = p->n_hidden > 1 ? p->width[1] : 0;
  s.weight_floats = carl_host::policy_transform_offset(p);
  s.set_floats = brax_policy_floats(p);
  return s;
}

int workgroups(int32_t n_samples) {
  if (n_samples < 1) return 0;
  const int tiles = (n_samples + carl::kPpoTile - 1) / carl::kPpoTile;
  return tiles < carl::kPpoMaxWorkgroups ? tiles : carl::kPpoMaxWorkgroups;
}

template <int H>
int launch_actor(const char* who, const carl::PpoNetArgs& a, int grid, hipStream_t s) {
  static_assert(carl::brax_ppo_lds_bytes(H) <= carl::kCuLdsBytes, "the Brax PPO actor launch's LDS does not fit a compute unit");
  const auto fn = carl::brax_ppo_actor_kernel<H>;
  if (int e = carl_host::ensure_dynamic_lds(reinterpret_cast<const void*>(fn), carl::brax_ppo_lds_bytes(H), who)) return e;
  hipLaunchKernelGGL(fn, dim3(grid), dim3(carl::kPpoThreads), carl::brax_ppo_lds_bytes(H), s, a);
  return check_launch(who);
}

// the critic: ppo_net_kernel<H> (kPpoValue), instantiated here
template <int H>
int launch_critic(const char* who, const carl::PpoNetArgs& a, int grid, hipStream_t s) {
  static_assert(carl::ppo_lds_bytes(H) <= carl::kCuLdsBytes, "a PPO network launch's LDS does not fit a compute unit");
  const auto fn = carl::ppo_net_kernel<H>;
  if (int e = carl_host::ensure_dynamic_lds(reinterpret_cast<const void*>(fn), carl::ppo_lds_bytes(H), who)) return e;
  hipLaunchKernelGGL(fn, dim3(grid), dim3(carl::kPpoThreads), carl::ppo_lds_bytes(H), s, a);
  return check_launch(who);
}

bool bad_coef(float v) { return !std::isfinite(v) || v < 0.0f; }

}  // namespace

extern "C" {

int32_t carl_brax_ppo_tile(void) { return carl::kPpoTile; }

int32_t carl_brax_ppo_grad_workgroups(int32_t n_samples) { return workgroups(n_samples); }

int64_t carl_brax_ppo_workspace_floats(const carl_policy_t* policy_host, const carl_policy_t* critic_host, int32_t n_samples) {
  if (policy_host == nullptr || critic_host == nullptr || n_samples < 1) return -1;
  if (brax_policy_floats(policy_host) < 0 || brax_policy_floats(critic_host) < 0) return -1;
  if (policy_host->n_out > carl::kBraxPpoOut || critic_host->n_out != 1) return -1;
  return (int64_t)workgroups(n_samples) * (carl::brax_ppo_slab_floats(carl_host::policy_padded_hidden(policy_host)) +
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
  const int grid = (b.n_lanes + carl::kTraceThreads - 1) / carl::kTraceThreads;
  hipLaunchKernelGGL(carl::brax_unit_context_trace_kernel, dim3(grid), dim3(carl::kTraceThreads), 0, (hipStream_t)stream, b, ctx_idx0,
                     episode0, terminated, truncated, n_steps, b.n_lanes, context_id);
  return check_launch(who);
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
  if (critic_host->n_ctx != policy_host->n_ctx)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_ctx %d, the actor has %d (the critic reads the actor's inputs)", cwho,
                critic_host->n_ctx, policy_host->n_ctx);
  for (int k = 0; k < policy_host->n_ctx; ++k)
    if (critic_host->ctx_rows[k] != policy_host->ctx_rows[k])
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: ctx_rows[%d] = %d, the actor's is %d", cwho, k, critic_host->ctx_rows[k],
                  policy_host->ctx_rows[k]);
  if (ppo->action_dtype != CARL_ACTION_F32)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: the action column is float32 (CARL_ACTION_F32) for the Brax families", who);
  if (ppo->n_contexts < 1 || ppo->ctx_stride < ppo->n_contexts)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_contexts %d / ctx_stride %d invalid", who, ppo->n_contexts,
                ppo->ctx_stride);
  const int64_t all = (int64_t)ppo->n_steps * ppo->n_lanes;
  if (all >= ((int64_t)1 << 31))
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: %d steps x %d lanes per row: flat indices do not fit 2^31 - 1", who,
                ppo->n_steps, ppo->n_lanes);
  if (ppo->n_samples < 1) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_samples %d < 1", who, ppo->n_samples);
  if (ppo->n_samples > all)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_samples %d > n_steps %d x n_lanes %d", who, ppo->n_samples, ppo->n_steps,
                ppo->n_lanes);
  if (ppo->idx == nullptr && ppo->n_samples != all)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: idx is NULL (every sample) but n_samples %d != n_steps %d x n_lanes %d", who,
                ppo->n_samples, ppo->n_steps, ppo->n_lanes);
  if (bad_coef(ppo->clip_range)) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: clip_range %g is not finite and >= 0", who, (double)ppo->clip_range);
  if (bad_coef(ppo->vf_coef)) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: vf_coef %g is not finite and >= 0", who, (double)ppo->vf_coef);
  if (bad_coef(ppo->ent_coef)) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: ent_coef %g is not finite and >= 0", who, (double)ppo->ent_coef);
  if (!ppo->obs0 || !ppo->obs || !ppo->context_id || !ppo->ctx_table || !ppo->action || !ppo->log_prob || !ppo->advantage ||
      !ppo->ret)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: a required pointer of ppo is NULL (all but idx and adv_norm)", who);
  if (!out->grad_actor || !out->grad_critic || !out->stats)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: out->grad_actor, out->grad_critic and out->stats are required", who);
  if (log_std == nullptr || out->grad_log_std == nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: log_std and out->grad_log_std are required ([n_act] on the device)", who);
  const int64_t need = carl_brax_ppo_workspace_floats(policy_host, critic_host, ppo->n_samples);
  if (out->workspace == nullptr || (reinterpret_cast<uintptr_t>(out->workspace) & 15) != 0)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: out->workspace is NULL or not on a 16-byte boundary", who);
  if (out->workspace_floats < need)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: workspace of %lld floats, %lld needed (carl_brax_ppo_workspace_floats)", who,
                (long long)out->workspace_floats, (long long)need);

  const hipStream_t s = (hipStream_t)stream;
  const int grid = workgroups(ppo->n_samples);
  const int ha = carl_host::policy_padded_hidden(policy_host), hc = carl_host::policy_padded_hidden(critic_host);
  carl::PpoNetArgs a{};
  a.b = *ppo;
  a.b.row_pitch = ppo->n_lanes;
  a.n_ctx = policy_host->n_ctx;
  for (int k = 0; k < policy_host->n_ctx; ++k) a.ctx_rows[k] = policy_host->ctx_rows[k];
  a.xform = policy_host->params + carl_host::policy_transform_offset(policy_host);
  a.log_std = log_std;
  a.n_tiles = (ppo->n_samples + carl::kPpoTile - 1) / carl::kPpoTile;
  // the actor
  a.shape = shape_of(policy_host);
  a.kind = carl::kPpoGaussian;
  a.params = policy_host->params;
  a.slab = out->workspace;
  a.new_out = out->new_log_prob;
  if (int e = ha == 0 ? launch_actor<0>(who, a, grid, s) : ha == 32 ? launch_actor<32>(who, a, grid, s)
                                                                     : launch_actor<64>(who, a, grid, s))
    return e;
  // the critic, on the actor's transformed inputs
  carl::PpoNetArgs c = a;
  c.shape = shape_of(critic_host);
  c.kind = carl::kPpoValue;
  c.params = critic_host->params;
  c.slab = out->workspace + (size_t)grid * carl::brax_ppo_slab_floats(ha);
  c.new_out = out->new_value;
  if (int e = hc == 0 ? launch_critic<0>(who, c, grid, s) : hc == 32 ? launch_critic<32>(who, c, grid, s)
                                                                      : launch_critic<64>(who, c, grid, s))
    return e;
  // the slabs, in workgroup order
  carl::PpoReduceArgs r{};
  r.actor = a.shape, r.critic = c.shape;
  r.h_actor = ha, r.h_critic = hc;
  r.n_workgroups = grid;
  r.gaussian = 1;
  r.inv_m = 1.0 / (double)ppo->n_samples;
  r.n_samples = (float)ppo->n_samples;
  r.slab_actor = a.slab, r.slab_critic = c.slab;
  r.grad_actor = out->grad_actor, r.grad_critic = out->grad_critic, r.grad_log_std = out->grad_log_std;
  r.stats = out->stats;
  const int outputs = r.actor.set_floats + r.critic.set_floats + 6 + carl::kBraxPpoOut;
  hipLaunchKernelGGL(carl::brax_ppo_reduce_kernel, dim3((outputs + 255) / 256), dim3(256), 0, s, r);
  return check_launch(who);
}

}  // extern "C"
