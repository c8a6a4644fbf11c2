// carl_policy_sample.hip -- C-ABI entry points of the closed-loop rollout with sampled actions (include/carl_amd.h:
// carl_rollout_policy_sampled, carl_evaluate_policy_sampled) and their kernel dispatch.  A translation unit of its own,
// so that the deterministic kernels of carl_policy.hip compile exactly as they did; the validation is carl_policy.hip's
// (policy_host.hpp), the launch path policy_launch.hpp's, the kernels are the same bodies with SampledPick choosing the
// action (policy_kernels.hip.h).  The sampling checks of every unit (policy_host.hpp: check_sampling) live here.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/carl_amd.h"
#include "classic_control.hip.h"
#include "host_common.hpp"
#include "policy_host.hpp"
#include "policy_kernels.hip.h"
#include "policy_launch.hpp"

namespace carl_host {

int check_sampling(const char* who, const carl_policy_sampling_t* smp, const carl_family_info_t& fi, LogProb log_prob) {
  if (smp == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: sampling is NULL", who);
  if (!fi.action_is_discrete && smp->log_std == nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: a Box family needs sampling->log_std ([n_sets] on the device)", who);
  if (log_prob == LogProb::kRefused && smp->log_prob != nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: sampling->log_prob is a transitions-mode output (io != NULL); this mode "
                "stores nothing per step", who);
  if (log_prob == LogProb::kRequired && smp->log_prob == nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: a sampled launch with a critic stores the log-probabilities: "
                "sampling->log_prob is NULL", who);
  if ((reinterpret_cast<uintptr_t>(smp->log_prob) & 15) != 0)  // (drained in 16-byte pieces, as io->action)
    return fail(CARL_ERR_UNSUPPORTED, "%s: sampling->log_prob is not on a 16-byte boundary", who);
  return 0;
}

}  // namespace carl_host

namespace {

using carl_host::check_sampling;
using carl_host::launch_policy_kernel;
using carl_host::LogProb;
using carl_host::PolicyKernel;
using carl_host::with_padded_hidden;

template <class Fam>
int launch_sampled(const carl_batch_t* b, const carl_policy_t* p, const carl_policy_sampling_t* smp,
                   const carl_step_io_t* io, int n_steps, const carl_policy_summary_t* sum, hipStream_t s) {
  const bool summary = io == nullptr, logp = smp->log_prob != nullptr;
  static_assert(carl::policy_lds_bytes<Fam, 64, false, true>() + carl::static_lds_bytes<Fam>() <= carl::kCuLdsBytes,
                "the sampled rollout's LDS (the log_prob column included) does not fit a compute unit");
  const auto k = with_padded_hidden(carl_host::policy_padded_hidden(p), [&](auto h) {
    constexpr int H = decltype(h)::value;
    using carl::policy_lds_bytes;
    if (summary) return PolicyKernel{carl::policy_rollout_sampled_kernel<Fam, H, true, false>, policy_lds_bytes<Fam, H, true>()};
    if (logp)
      return PolicyKernel{carl::policy_rollout_sampled_kernel<Fam, H, false, true>, policy_lds_bytes<Fam, H, false, true>()};
    return PolicyKernel{carl::policy_rollout_sampled_kernel<Fam, H, false, false>, policy_lds_bytes<Fam, H, false>()};
  });
  const int threads = summary ? carl::kPolicyThreadsSummary : carl::kPolicyThreadsTransitions;
  return launch_policy_kernel("carl_rollout_policy_sampled", k, b->n_lanes, threads, s, *b, carl_host::launch_io(b, io), *p,
                              carl_host::policy_set_floats(p), carl_host::launch_summary(sum), n_steps, *smp);
}

template <class Fam>
int launch_sampled_episodes(const carl_batch_t* b, const carl_policy_t* p, const carl_policy_sampling_t* smp,
                            int n_episodes, int max_steps, const carl_policy_episodes_t* out, hipStream_t s) {
  // the LDS: the weight set alone
  const auto k = with_padded_hidden(carl_host::policy_padded_hidden(p), [](auto h) {
    constexpr int H = decltype(h)::value;
    return PolicyKernel{carl::policy_episodes_sampled_kernel<Fam, H>, carl::policy_lds_bytes<Fam, H, true>()};
  });
  return launch_policy_kernel("carl_evaluate_policy_sampled", k, b->n_lanes, carl::kPolicyThreadsSummary, s, *b, *p,
                              carl_host::policy_set_floats(p), *out, n_episodes, max_steps, *smp);
}

}  // namespace

extern "C" {

int carl_rollout_policy_sampled(const carl_batch_t* batch, const carl_policy_t* policy_host,
                                const carl_policy_sampling_t* sampling, const carl_step_io_t* io, int32_t n_steps,
                                const carl_policy_summary_t* summary_out, void* stream) {
  const char* who = "carl_rollout_policy_sampled";
  carl_family_info_t fi;
  if (int e = carl_host::check_rollout_policy(who, batch, policy_host, io, n_steps, summary_out, &fi)) return e;
  if (int e = check_sampling(who, sampling, fi, io != nullptr ? LogProb::kOptional : LogProb::kRefused)) return e;
  if (batch->n_lanes == 0 || n_steps == 0) return carl_host::policy_rollout_without_steps(who, batch, summary_out, stream);
  return carl_host::with_classic_family(batch, [&](auto fam) {
    return launch_sampled<decltype(fam)>(batch, policy_host, sampling, io, n_steps, summary_out, (hipStream_t)stream);
  });
}

int carl_evaluate_policy_sampled(const carl_batch_t* batch, const carl_policy_t* policy_host,
                                 const carl_policy_sampling_t* sampling, int32_t n_episodes, int32_t max_steps,
                                 const carl_policy_episodes_t* out, void* stream) {
  const char* who = "carl_evaluate_policy_sampled";
  carl_family_info_t fi;
  if (int e = carl_host::check_evaluate_policy(who, batch, policy_host, n_episodes, max_steps, out, &fi)) return e;
  if (int e = check_sampling(who, sampling, fi, LogProb::kRefused)) return e;
  if (batch->n_lanes == 0) return 0;
  return carl_host::with_classic_family(batch, [&](auto fam) {
    return launch_sampled_episodes<decltype(fam)>(batch, policy_host, sampling, n_episodes, max_steps, out,
                                                  (hipStream_t)stream);
  });
}

}  // extern "C"
