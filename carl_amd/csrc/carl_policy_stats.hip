// carl_policy_stats.hip -- C-ABI entry points of the input statistics of the closed-loop rollout (include/carl_amd.h:
// carl_evaluate_policy_stats, carl_policy_stats_merge, carl_brax_policy_stats_merge) and their kernel dispatch.  A translation unit of its own, so that
// every other unit's kernels compile exactly as they did; the validation is carl_policy.hip's and
// carl_policy_sample.hip's (policy_host.hpp), the launch path policy_launch.hpp's, the kernels are
// policy_stats_kernels.hip.h's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/carl_amd.h"
#include "classic_control.hip.h"
#include "host_common.hpp"
#include "policy_host.hpp"
#include "policy_stats_kernels.hip.h"
#include "policy_launch.hpp"

// (policy_host.hpp)
int carl_host::check_policy_stats(const char* who, const carl_policy_stats_t* stats, int n_slabs, const char* slabs) {
  if (stats == nullptr || stats->partial == nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: stats / stats->partial is NULL", who);
  if ((reinterpret_cast<uintptr_t>(stats->partial) & 15) != 0)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: stats->partial is not on a 16-byte boundary", who);
  if (stats->partial_capacity < n_slabs)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: stats->partial_capacity %d < %d %s", who, stats->partial_capacity, n_slabs, slabs);
  return 0;
}

namespace {

using carl_host::check_launch;
using carl_host::fail;

constexpr const char* kClassicSlabs = "workgroups (carl_policy_stats_workgroups)";

template <class Fam>
int launch_stats(const carl_batch_t* b, const carl_policy_t* p, const carl_policy_sampling_t* smp, int n_episodes,
                 int max_steps, const carl_policy_episodes_t* out, double* partial, hipStream_t s) {
  const bool sampled = smp != nullptr;
  const auto k = carl_host::with_padded_hidden(carl_host::policy_padded_hidden(p), [&](auto h) {
    constexpr int H = decltype(h)::value;
    // the weight set and the waves' float64 sums
    const size_t lds = carl::policy_lds_bytes<Fam, H, true>() + carl::policy_stats_lds_bytes<Fam, H>();
    if (sampled) return carl_host::PolicyKernel{carl::policy_episodes_stats_kernel<Fam, H, true>, lds};
    return carl_host::PolicyKernel{carl::policy_episodes_stats_kernel<Fam, H, false>, lds};
  });
  return carl_host::launch_policy_kernel("carl_evaluate_policy_stats", k, b->n_lanes, carl::kPolicyThreadsSummary, s, *b, *p,
                                         carl_host::policy_set_floats(p), *out, n_episodes, max_steps,
                                         carl_host::launch_sampling(smp), partial);
}

// carl_policy_stats_merge and carl_brax_policy_stats_merge: one validation list, one launch.  set_floats: the floats of a
// packed weight set by the caller's packing rule (< 0: the shape is outside its limits); the transform offset -- the floats
// of every W and b -- is the same function of the shape under both rules.
int merge_stats(const char* who, const char* slabs, const carl_policy_t* policy_host, int set_floats, const carl_policy_stats_t* stats,
                int32_t n_workgroups, const int32_t* steps, int32_t n_lanes, const carl_policy_running_stats_t* running, double eps,
                double min_std, float* params_out, int32_t n_write, void* stream) {
  if (policy_host == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: policy is NULL", who);
  if (set_floats < 0) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: the policy's shape is outside the limits", who);
  if (policy_host->params == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: params is NULL", who);
  if (n_workgroups < 0) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_workgroups %d < 0", who, n_workgroups);
  if (int e = carl_host::check_policy_stats(who, stats, n_workgroups, slabs)) return e;
  if (n_lanes < 0) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_lanes %d < 0", who, n_lanes);
  if (steps == nullptr && n_lanes > 0) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: steps is NULL", who);
  if (running == nullptr || !running->count || !running->mean || !running->m2)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: running and its three arrays are required", who);
  if (!std::isfinite(eps) || eps < 0.0) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: eps %g is not finite and >= 0", who, eps);
  if (!std::isfinite(min_std) || min_std < 0.0)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: min_std %g is not finite and >= 0", who, min_std);
  if (n_write < 0) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_write %d < 0", who, n_write);
  const int p_shift = carl_host::policy_transform_offset(policy_host);
  hipLaunchKernelGGL(carl::policy_stats_merge_kernel, dim3(1), dim3(carl::kStatsMergeThreads), 0, (hipStream_t)stream,
                     stats->partial, n_workgroups, steps, n_lanes, policy_host->n_in, policy_host->params + p_shift,
                     running->count, running->mean, running->m2, eps, min_std, params_out, n_write, set_floats, p_shift);
  return check_launch(who);
}

}  // namespace

extern "C" {

int32_t carl_policy_stats_workgroups(int32_t n_lanes) { return carl_host::policy_workgroups(n_lanes); }

int carl_evaluate_policy_stats(const carl_batch_t* batch, const carl_policy_t* policy_host,
                               const carl_policy_sampling_t* sampling, int32_t n_episodes, int32_t max_steps,
                               const carl_policy_episodes_t* episodes_out, const carl_policy_stats_t* stats, void* stream) {
  const char* who = "carl_evaluate_policy_stats";
  carl_family_info_t fi;
  if (int e = carl_host::check_evaluate_policy(who, batch, policy_host, n_episodes, max_steps, episodes_out, &fi)) return e;
  if (sampling != nullptr)
    if (int e = carl_host::check_sampling(who, sampling, fi, carl_host::LogProb::kRefused)) return e;
  if (int e = carl_host::check_policy_stats(who, stats, carl_host::policy_workgroups(batch->n_lanes), kClassicSlabs)) return e;
  if (batch->n_lanes == 0) return 0;
  return carl_host::with_classic_family(batch, [&](auto fam) {
    return launch_stats<decltype(fam)>(batch, policy_host, sampling, n_episodes, max_steps, episodes_out, stats->partial,
                                       (hipStream_t)stream);
  });
}

int carl_policy_stats_merge(const carl_policy_t* policy_host, const carl_policy_stats_t* stats, int32_t n_workgroups,
                            const int32_t* steps, int32_t n_lanes, const carl_policy_running_stats_t* running, double eps,
                            double min_std, float* params_out, int32_t n_write, void* stream) {
  return merge_stats("carl_policy_stats_merge", kClassicSlabs, policy_host, policy_host ? carl_host::policy_set_floats(policy_host) : -1, stats,
                     n_workgroups, steps, n_lanes, running, eps, min_std, params_out, n_write, stream);
}

// The same merge for a policy packed by the Brax rule (n_out up to CARL_BRAX_MAX_ACT: carl_brax_policy_set_floats, which the
// call above refuses through carl_policy_set_floats); n_slabs: the wavefront slabs of carl_brax_evaluate_policy_stats.
int carl_brax_policy_stats_merge(const carl_policy_t* policy_host, const carl_policy_stats_t* stats, int32_t n_slabs,
                                 const int32_t* steps, int32_t n_lanes, const carl_policy_running_stats_t* running, double eps,
                                 double min_std, float* params_out, int32_t n_write, void* stream) {
  return merge_stats("carl_brax_policy_stats_merge", "slabs (carl_brax_policy_stats_slabs)", policy_host, carl_brax_policy_set_floats(policy_host), stats, n_slabs, steps,
                     n_lanes, running, eps, min_std, params_out, n_write, stream);
}

}  // extern "C"
