// carl_policy_value.hip -- C-ABI entry points of the closed-loop rollout with a critic (include/carl_amd.h:
// carl_rollout_policy_valued) and of the GAE kernel (carl_gae), and their kernel dispatch.  A translation unit of its
// own, so that the kernels of carl_policy.hip and carl_policy_sample.hip compile exactly as they did; the batch / policy /
// io validation, the sampling checks and the network shape checks the critic shares with the actor are policy_host.hpp's,
// the launch path policy_launch.hpp's, the kernels are policy_value_kernels.hip.h's.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/carl_amd.h"
#include "classic_control.hip.h"
#include "host_common.hpp"
#include "policy_host.hpp"
#include "policy_value_kernels.hip.h"
#include "policy_launch.hpp"

namespace {

using carl_host::check_launch;
using carl_host::fail;

// the critic against the actor (which check_rollout_policy has validated against the batch); cwho: "<who>: critic"
int check_critic(const char* who, const char* cwho, const carl_policy_t* p, const carl_policy_t* c) {
  if (c == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: critic is NULL", who);
  if (int e = carl_host::check_hidden_layers(cwho, c)) return e;
  if (c->n_out != 1) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: head width %d, a value network has 1", cwho, c->n_out);
  if (c->n_in != p->n_in || c->n_ctx != p->n_ctx)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_in %d / n_ctx %d, the actor has %d / %d (the critic reads the actor's "
                "inputs)", cwho, c->n_in, c->n_ctx, p->n_in, p->n_ctx);
  for (int k = 0; k < p->n_ctx; ++k)
    if (c->ctx_rows[k] != p->ctx_rows[k])
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: ctx_rows[%d] = %d, the actor's is %d", cwho, k, c->ctx_rows[k],
                  p->ctx_rows[k]);
  if (int e = carl_host::check_activation(cwho, c)) return e;
  if (c->n_sets != p->n_sets || c->lanes_per_set != p->lanes_per_set)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: %d sets x %d lanes, the actor has %d x %d", cwho, c->n_sets,
                c->lanes_per_set, p->n_sets, p->lanes_per_set);
  return carl_host::check_params(cwho, c);
}

int check_value_out(const char* who, const carl_batch_t* b, const carl_policy_value_t* out) {
  if (out == nullptr || out->value == nullptr || out->last_value == nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: out, out->value and out->last_value are required", who);
  if (((reinterpret_cast<uintptr_t>(out->value) | reinterpret_cast<uintptr_t>(out->boot_value)) & 15) != 0)
    return fail(CARL_ERR_UNSUPPORTED, "%s: out->value / out->boot_value is not on a 16-byte boundary", who);
  if (out->boot_value != nullptr && !(b->flags & CARL_FLAG_AUTORESET))
    return fail(CARL_ERR_UNSUPPORTED, "%s: out->boot_value needs CARL_FLAG_AUTORESET (without auto-reset no terminal "
                "observation is kept apart from the next one)", who);
  return 0;
}

template <class Fam>
int launch_valued(const carl_batch_t* b, const carl_policy_t* p, const carl_policy_t* c, const carl_policy_sampling_t* smp,
                  const carl_step_io_t* io, int n_steps, const carl_policy_summary_t* sum, const carl_policy_value_t* out,
                  hipStream_t s) {
  const int ha = carl_host::policy_padded_hidden(p), hc = carl_host::policy_padded_hidden(c);
  const bool sampled = smp != nullptr;
  // the chunk of 4 must fit whatever valued_chunk decides (records, four columns, both weight regions at H = 64, the
  // terminal-observation slots, the family's static tables)
  static_assert(carl::valued_lds_bytes_at<Fam, 64, true>(4) + carl::static_lds_bytes<Fam>() <= carl::kCuLdsBytes,
                "the valued rollout's LDS at a chunk of 4 steps does not fit a compute unit");
  static_assert(carl::valued_lds_bytes<Fam, 64, true>() + carl::static_lds_bytes<Fam>() <= carl::kCuLdsBytes &&
                    carl::valued_lds_bytes<Fam, 64, false>() + carl::static_lds_bytes<Fam>() <= carl::kCuLdsBytes,
                "the valued rollout's LDS does not fit a compute unit");
  const auto k = carl_host::with_padded_hidden(ha > hc ? ha : hc, [&](auto h) {
    constexpr int H = decltype(h)::value;
    if (sampled)
      return carl_host::PolicyKernel{carl::policy_rollout_valued_kernel<Fam, H, true>, carl::valued_lds_bytes<Fam, H, true>()};
    return carl_host::PolicyKernel{carl::policy_rollout_valued_kernel<Fam, H, false>, carl::valued_lds_bytes<Fam, H, false>()};
  });
  return carl_host::launch_policy_kernel("carl_rollout_policy_valued", k, b->n_lanes, carl::kPolicyThreadsTransitions, s, *b,
                                         carl_host::launch_io(b, io), *p, carl_host::policy_set_floats(p), *c,
                                         carl_host::policy_set_floats(c), carl_host::launch_summary(sum), n_steps,
                                         carl_host::launch_sampling(smp), *out);
}

}  // namespace

extern "C" {

int carl_rollout_policy_valued(const carl_batch_t* batch, const carl_policy_t* policy_host,
                               const carl_policy_t* critic_host, const carl_policy_sampling_t* sampling,
                               const carl_step_io_t* io, int32_t n_steps, const carl_policy_summary_t* summary_out,
                               const carl_policy_value_t* out, void* stream) {
  const char* who = "carl_rollout_policy_valued";
  carl_family_info_t fi;
  if (io == nullptr && batch != nullptr && policy_host != nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: io is NULL -- transitions mode only (a summary has no use for values)", who);
  if (int e = carl_host::check_rollout_policy(who, batch, policy_host, io, n_steps, summary_out, &fi)) return e;
  if (sampling != nullptr)
    if (int e = carl_host::check_sampling(who, sampling, fi, carl_host::LogProb::kRequired)) return e;
  if (int e = check_critic(who, "carl_rollout_policy_valued: critic", policy_host, critic_host)) return e;
  if (int e = check_value_out(who, batch, out)) return e;
  if (batch->n_lanes == 0 || n_steps == 0) return carl_host::policy_rollout_without_steps(who, batch, summary_out, stream);
  return carl_host::with_classic_family(batch, [&](auto fam) {
    return launch_valued<decltype(fam)>(batch, policy_host, critic_host, sampling, io, n_steps, summary_out, out,
                                        (hipStream_t)stream);
  });
}

int carl_gae(const carl_gae_t* g, void* stream) {
  const char* who = "carl_gae";
  if (g == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: gae is NULL", who);
  if (g->n_lanes < 0 || g->n_steps < 0)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_lanes %d / n_steps %d < 0", who, g->n_lanes, g->n_steps);
  if (g->row_pitch != 0 && g->row_pitch < g->n_lanes)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: row_pitch %d < n_lanes %d", who, g->row_pitch, g->n_lanes);
  if (!g->reward || !g->value || !g->last_value || !g->terminated || !g->truncated || !g->advantage || !g->ret)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: a required pointer is NULL (all but boot_value)", who);
  if (g->n_lanes == 0 || g->n_steps == 0) return 0;
  carl_gae_t r = *g;
  r.row_pitch = g->row_pitch > 0 ? g->row_pitch : g->n_lanes;
  volatile float gamma = g->gamma, lambda = g->lambda;  // (volatile: the product is rounded to fp32 here, once)
  volatile float gl = gamma * lambda;
  const int grid = (g->n_lanes + carl::kGaeThreads - 1) / carl::kGaeThreads;
  if (g->boot_value != nullptr)
    hipLaunchKernelGGL(carl::gae_kernel<true>, dim3(grid), dim3(carl::kGaeThreads), 0, (hipStream_t)stream, r, (float)gl);
  else
    hipLaunchKernelGGL(carl::gae_kernel<false>, dim3(grid), dim3(carl::kGaeThreads), 0, (hipStream_t)stream, r, (float)gl);
  return check_launch(who);
}

}  // extern "C"
