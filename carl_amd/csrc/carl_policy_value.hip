// carl_policy_value.hip -- C-ABI entry points of the closed-loop rollout with a critic (include/carl_amd.h:
// carl_rollout_policy_valued) and of the GAE kernel (carl_gae), and their kernel dispatch.  A translation unit of its
// own, so that the kernels of carl_policy.hip and carl_policy_sample.hip compile exactly as they did; the batch / policy /
// io validation is carl_policy.hip's (policy_host.hpp), the kernels are policy_value_kernels.hip.h's.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/carl_amd.h"
#include "classic_control.hip.h"
#include "host_common.hpp"
#include "policy_host.hpp"
#include "policy_value_kernels.hip.h"

namespace {

using carl_host::check_launch;
using carl_host::fail;

// the sampling checks of carl_rollout_policy_sampled's transitions mode, and the log_prob column a valued launch needs
int check_valued_sampling(const char* who, const carl_policy_sampling_t* smp, const carl_family_info_t& fi) {
  if (!fi.action_is_discrete && smp->log_std == nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: a Box family needs sampling->log_std ([n_sets] on the device)", who);
  if (smp->log_prob == nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: a sampled launch with a critic stores the log-probabilities: "
                "sampling->log_prob is NULL", who);
  if ((reinterpret_cast<uintptr_t>(smp->log_prob) & 15) != 0)
    return fail(CARL_ERR_UNSUPPORTED, "%s: sampling->log_prob is not on a 16-byte boundary", who);
  return 0;
}

// the critic against the actor (which check_rollout_policy has validated against the batch)
int check_critic(const char* who, const carl_policy_t* p, const carl_policy_t* c) {
  if (c == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: critic is NULL", who);
  if (c->n_hidden < 0 || c->n_hidden > CARL_POLICY_MAX_HIDDEN)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: critic: n_hidden %d outside [0, %d]", who, c->n_hidden, CARL_POLICY_MAX_HIDDEN);
  for (int l = 0; l < c->n_hidden; ++l)
    if (c->width[l] < 1 || c->width[l] > CARL_POLICY_MAX_WIDTH)
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: critic: hidden width[%d] = %d outside [1, %d]", who, l, c->width[l],
                  CARL_POLICY_MAX_WIDTH);
  if (c->n_out != 1) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: critic: head width %d, a value network has 1", who, c->n_out);
  if (c->n_in != p->n_in || c->n_ctx != p->n_ctx)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: critic: n_in %d / n_ctx %d, the actor has %d / %d (the critic reads the "
                "actor's inputs)", who, c->n_in, c->n_ctx, p->n_in, p->n_ctx);
  for (int k = 0; k < p->n_ctx; ++k)
    if (c->ctx_rows[k] != p->ctx_rows[k])
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: critic: ctx_rows[%d] = %d, the actor's is %d", who, k, c->ctx_rows[k],
                  p->ctx_rows[k]);
  if (c->activation < CARL_POLICY_IDENTITY || c->activation > CARL_POLICY_RELU)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: critic: unknown activation %d", who, c->activation);
  if (c->n_sets != p->n_sets || c->lanes_per_set != p->lanes_per_set)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: critic: %d sets x %d lanes, the actor has %d x %d", who, c->n_sets,
                c->lanes_per_set, p->n_sets, p->lanes_per_set);
  if (c->params == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: critic: params is NULL", who);
  return 0;
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

// a policy_rollout_valued_kernel instance and the dynamic LDS it takes
struct ValuedKernel {
  void (*fn)(carl_batch_t, carl_step_io_t, carl_policy_t, int, carl_policy_t, int, carl_policy_summary_t, int,
             carl_policy_sampling_t, carl_policy_value_t);
  size_t lds;
};

template <class Fam, int H>
ValuedKernel valued_kernel(bool sampled) {
  if (sampled) return {carl::policy_rollout_valued_kernel<Fam, H, true>, carl::valued_lds_bytes<Fam, H, true>()};
  return {carl::policy_rollout_valued_kernel<Fam, H, false>, carl::valued_lds_bytes<Fam, H, false>()};
}

template <class Fam>
int launch_valued(const carl_batch_t* b, const carl_policy_t* p, const carl_policy_t* c, const carl_policy_sampling_t* smp,
                  const carl_step_io_t* io, int n_steps, const carl_policy_summary_t* sum, const carl_policy_value_t* out,
                  hipStream_t s) {
  const char* who = "carl_rollout_policy_valued";
  const int ha = carl_host::policy_padded_hidden(p), hc = carl_host::policy_padded_hidden(c);
  const int H = ha > hc ? ha : hc;
  const bool sampled = smp != nullptr;
  const ValuedKernel k = H == 0 ? valued_kernel<Fam, 0>(sampled) : H == 32 ? valued_kernel<Fam, 32>(sampled)
                                                                  : valued_kernel<Fam, 64>(sampled);
  // the chunk of 4 must fit whatever valued_chunk decides (records, four columns, both weight regions at H = 64, the
  // terminal-observation slots, the family's static tables)
  static_assert(carl::valued_lds_bytes_at<Fam, 64, true>(4) + carl::static_lds_bytes<Fam>() <= carl::kCuLdsBytes,
                "the valued rollout's LDS at a chunk of 4 steps does not fit a compute unit");
  static_assert(carl::valued_lds_bytes<Fam, 64, true>() + carl::static_lds_bytes<Fam>() <= carl::kCuLdsBytes &&
                    carl::valued_lds_bytes<Fam, 64, false>() + carl::static_lds_bytes<Fam>() <= carl::kCuLdsBytes,
                "the valued rollout's LDS does not fit a compute unit");
  if (int e = carl_host::ensure_dynamic_lds(reinterpret_cast<const void*>(k.fn), k.lds, who)) return e;
  carl_step_io_t io_r = *io;
  io_r.row_pitch = io->row_pitch > 0 ? io->row_pitch : b->n_lanes;  // the kernel reads the pitch as given: never 0
  const carl_policy_summary_t sum_r = sum != nullptr ? *sum : carl_policy_summary_t{nullptr, nullptr, nullptr};
  const carl_policy_sampling_t smp_r = sampled ? *smp : carl_policy_sampling_t{0, nullptr, nullptr};
  const int grid = (b->n_lanes + carl::kPolicyLanes - 1) / carl::kPolicyLanes;
  hipLaunchKernelGGL(k.fn, dim3(grid), dim3(carl::kPolicyThreadsTransitions), k.lds, s, *b, io_r, *p,
                     carl_host::policy_set_floats(p), *c, carl_host::policy_set_floats(c), sum_r, n_steps, smp_r, *out);
  return check_launch(who);
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
    if (int e = check_valued_sampling(who, sampling, fi)) return e;
  if (int e = check_critic(who, policy_host, critic_host)) return e;
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
