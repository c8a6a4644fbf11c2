// carl_ppo.hip -- C-ABI entry points of the PPO update on the device (include/carl_amd.h: carl_policy_context_trace,
// carl_ppo_grad) and their launches.  A translation unit of its own, so that every other unit's kernels compile exactly
// as they did; the kernels are ppo_kernels.hip.h's, the network shape checks the closed-loop rollout shares are
// policy_host.hpp's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/carl_amd.h"
#include "classic_control.hip.h"
#include "host_common.hpp"
#include "policy_host.hpp"
#include "ppo_kernels.hip.h"

namespace {

using carl_host::check_launch;
using carl_host::fail;

// what carl_rollout_policy_valued checks of a network, without a batch: `fi` the family's info, `head_out` the head
// width the family needs of this network
int check_network(const char* who, const carl_policy_t* p, const carl_family_info_t& fi, int head_out, const char* kind) {
  if (int e = carl_host::check_hidden_layers(who, p)) return e;
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
  s.set_floats = carl_host::policy_set_floats(p);
  return s;
}

int workgroups(int32_t n_samples) {
  if (n_samples < 1) return 0;
  const int tiles = (n_samples + carl::kPpoTile - 1) / carl::kPpoTile;
  return tiles < carl::kPpoMaxWorkgroups ? tiles : carl::kPpoMaxWorkgroups;
}

template <int H>
int launch_net(const char* who, const carl::PpoNetArgs& a, int grid, hipStream_t s) {
  static_assert(carl::ppo_lds_bytes(H) <= carl::kCuLdsBytes, "a PPO network launch's LDS does not fit a compute unit");
  const auto fn = carl::ppo_net_kernel<H>;
  if (int e = carl_host::ensure_dynamic_lds(reinterpret_cast<const void*>(fn), carl::ppo_lds_bytes(H), who)) return e;
  hipLaunchKernelGGL(fn, dim3(grid), dim3(carl::kPpoThreads), carl::ppo_lds_bytes(H), s, a);
  return check_launch(who);
}

int launch_net_at(const char* who, int H, const carl::PpoNetArgs& a, int grid, hipStream_t s) {
  return H == 0 ? launch_net<0>(who, a, grid, s) : H == 32 ? launch_net<32>(who, a, grid, s) : launch_net<64>(who, a, grid, s);
}

bool bad_coef(float v) { return !std::isfinite(v) || v < 0.0f; }

}  // namespace

extern "C" {

int32_t carl_ppo_tile(void) { return carl::kPpoTile; }

int32_t carl_ppo_grad_workgroups(int32_t n_samples) { return workgroups(n_samples); }

int64_t carl_ppo_workspace_floats(const carl_policy_t* policy_host, const carl_policy_t* critic_host, int32_t n_samples) {
  if (policy_host == nullptr || critic_host == nullptr || n_samples < 1) return -1;
  if (carl_host::policy_set_floats(policy_host) < 0 || carl_host::policy_set_floats(critic_host) < 0) return -1;
  return (int64_t)workgroups(n_samples) * (carl::ppo_slab_floats(carl_host::policy_padded_hidden(policy_host)) +
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
  const int pitch = row_pitch > 0 ? row_pitch : batch->n_lanes;
  const int grid = (batch->n_lanes + carl::kTraceThreads - 1) / carl::kTraceThreads;
  hipLaunchKernelGGL(carl::context_trace_kernel, dim3(grid), dim3(carl::kTraceThreads), 0, (hipStream_t)stream, *batch,
                     ctx_idx0, episode0, terminated, truncated, n_steps, pitch, context_id);
  return check_launch(who);
}

int carl_ppo_grad(const carl_ppo_batch_t* ppo, const carl_policy_t* policy_host, const carl_policy_t* critic_host,
                  const float* log_std, const carl_ppo_out_t* out, void* stream) {
  const char* who = "carl_ppo_grad";
  if (ppo == nullptr || policy_host == nullptr || critic_host == nullptr || out == nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: ppo / policy / critic / out is NULL", who);
  if (ppo->family >= CARL_N_FAMILIES)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: family %d is a Brax family -- the PPO update covers the classic-control "
                "families only", who, ppo->family);
  carl_family_info_t fi;
  if (int e = carl_family_info(ppo->family, &fi)) return e;
  if (ppo->n_lanes < 1 || ppo->n_steps < 1)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_lanes %d / n_steps %d < 1", who, ppo->n_lanes, ppo->n_steps);
  if (ppo->row_pitch != 0 && ppo->row_pitch < ppo->n_lanes)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: row_pitch %d < n_lanes %d", who, ppo->row_pitch, ppo->n_lanes);
  if (ppo->obs_dim != fi.obs_dim)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: obs_dim %d, the family's is %d", who, ppo->obs_dim, fi.obs_dim);
  const int want_out = fi.action_is_discrete ? fi.n_actions : 1;
  if (int e = check_network(who, policy_host, fi, want_out, fi.action_is_discrete ? "n_actions" : "one Box value")) return e;
  if (policy_host->head != (fi.action_is_discrete ? CARL_POLICY_HEAD_ARGMAX : CARL_POLICY_HEAD_BOX))
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: head kind %d does not match the family's action space", who,
                policy_host->head);
  const char* cwho = "carl_ppo_grad: critic";
  if (int e = check_network(cwho, critic_host, fi, 1, "a value network has 1")) return e;
  if (critic_host->n_ctx != policy_host->n_ctx)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_ctx %d, the actor has %d (the critic reads the actor's inputs)", cwho,
                critic_host->n_ctx, policy_host->n_ctx);
  for (int k = 0; k < policy_host->n_ctx; ++k)
    if (critic_host->ctx_rows[k] != policy_host->ctx_rows[k])
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: ctx_rows[%d] = %d, the actor's is %d", cwho, k, critic_host->ctx_rows[k],
                  policy_host->ctx_rows[k]);
  if (ppo->action_dtype != (fi.action_is_discrete ? CARL_ACTION_I32 : CARL_ACTION_F32))
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: the action column is %s for this family", who,
                fi.action_is_discrete ? "int32 (CARL_ACTION_I32)" : "float32 (CARL_ACTION_F32)");
  if (ppo->n_contexts < 1 || ppo->ctx_stride < ppo->n_contexts)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_contexts %d / ctx_stride %d invalid", who, ppo->n_contexts,
                ppo->ctx_stride);
  const int64_t all = (int64_t)ppo->n_steps * ppo->n_lanes;
  const int pitch = ppo->row_pitch > 0 ? ppo->row_pitch : ppo->n_lanes;
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
  if (bad_coef(ppo->clip_range)) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: clip_range %g is not finite and >= 0", who, (double)ppo->clip_range);
  if (bad_coef(ppo->vf_coef)) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: vf_coef %g is not finite and >= 0", who, (double)ppo->vf_coef);
  if (bad_coef(ppo->ent_coef)) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: ent_coef %g is not finite and >= 0", who, (double)ppo->ent_coef);
  if (!ppo->obs0 || !ppo->obs || !ppo->context_id || !ppo->ctx_table || !ppo->action || !ppo->log_prob || !ppo->advantage ||
      !ppo->ret)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: a required pointer of ppo is NULL (all but idx and adv_norm)", who);
  if (!out->grad_actor || !out->grad_critic || !out->stats)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: out->grad_actor, out->grad_critic and out->stats are required", who);
  if (!fi.action_is_discrete && (log_std == nullptr || out->grad_log_std == nullptr))
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: a Box family needs log_std and out->grad_log_std ([1] on the device)", who);
  const int64_t need = carl_ppo_workspace_floats(policy_host, critic_host, ppo->n_samples);
  if (out->workspace == nullptr || (reinterpret_cast<uintptr_t>(out->workspace) & 15) != 0)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: out->workspace is NULL or not on a 16-byte boundary", who);
  if (out->workspace_floats < need)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: workspace of %lld floats, %lld needed (carl_ppo_workspace_floats)", who,
                (long long)out->workspace_floats, (long long)need);

  const hipStream_t s = (hipStream_t)stream;
  const int grid = workgroups(ppo->n_samples);
  const int ha = carl_host::policy_padded_hidden(policy_host), hc = carl_host::policy_padded_hidden(critic_host);
  carl::PpoNetArgs a{};
  a.b = *ppo;
  a.b.row_pitch = pitch;
  a.n_ctx = policy_host->n_ctx;
  for (int k = 0; k < policy_host->n_ctx; ++k) a.ctx_rows[k] = policy_host->ctx_rows[k];
  a.xform = policy_host->params + carl_host::policy_transform_offset(policy_host);
  a.log_std = log_std;
  a.n_tiles = (ppo->n_samples + carl::kPpoTile - 1) / carl::kPpoTile;
  // the actor
  a.shape = shape_of(policy_host);
  a.kind = fi.action_is_discrete ? carl::kPpoCategorical : carl::kPpoGaussian;
  a.params = policy_host->params;
  a.slab = out->workspace;
  a.new_out = out->new_log_prob;
  if (int e = launch_net_at(who, ha, a, grid, s)) return e;
  // the critic, on the actor's transformed inputs
  carl::PpoNetArgs c = a;
  c.shape = shape_of(critic_host);
  c.kind = carl::kPpoValue;
  c.params = critic_host->params;
  c.slab = out->workspace + (size_t)grid * carl::ppo_slab_floats(ha);
  c.new_out = out->new_value;
  if (int e = launch_net_at(who, hc, c, grid, s)) return e;
  // the slabs, in workgroup order
  carl::PpoReduceArgs r{};
  r.actor = a.shape, r.critic = c.shape;
  r.h_actor = ha, r.h_critic = hc;
  r.n_workgroups = grid;
  r.gaussian = fi.action_is_discrete ? 0 : 1;
  r.inv_m = 1.0 / (double)ppo->n_samples;
  r.n_samples = (float)ppo->n_samples;
  r.slab_actor = a.slab, r.slab_critic = c.slab;
  r.grad_actor = out->grad_actor, r.grad_critic = out->grad_critic, r.grad_log_std = out->grad_log_std;
  r.stats = out->stats;
  const int outputs = r.actor.set_floats + r.critic.set_floats + 8;
  hipLaunchKernelGGL(carl::ppo_reduce_kernel, dim3((outputs + 255) / 256), dim3(256), 0, s, r);
  return check_launch(who);
}

}  // extern "C"
