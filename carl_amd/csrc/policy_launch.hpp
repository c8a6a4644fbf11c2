// policy_launch.hpp -- the one host-side launch path of the closed-loop rollout, included by its four translation units
// (carl_policy.hip, carl_policy_sample.hip, carl_policy_value.hip, carl_policy_stats.hip): the dispatch on the padded
// hidden width, a kernel instance with its LDS, the grid rule and the launch, and the by-value kernel arguments made
// from the entry points' optional structs.  Host code only; a unit adds its kernel instances and its own checks.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>

#include "../../include/carl_amd.h"
#include "host_common.hpp"
#include "policy_kernels.hip.h"

namespace carl_host {

// fn(std::integral_constant<int, H>{}) for a padded hidden width H (policy_padded_hidden: 0, 32 or 64)
template <class Fn>
auto with_padded_hidden(int H, Fn&& fn) {
  return H == 0    ? fn(std::integral_constant<int, 0>{})
         : H == 32 ? fn(std::integral_constant<int, 32>{})
                   : fn(std::integral_constant<int, 64>{});
}

// a kernel instance and the dynamic LDS it takes
template <class... P>
struct PolicyKernel {
  void (*fn)(P...);
  size_t lds;
};
template <class... P>
PolicyKernel(void (*)(P...), size_t) -> PolicyKernel<P...>;

// workgroups of a launch over n_lanes lanes (carl_policy_stats_workgroups): kPolicyLanes lanes each
inline int policy_workgroups(int32_t n_lanes) {
  return n_lanes <= 0 ? 0 : (n_lanes + carl::kPolicyLanes - 1) / carl::kPolicyLanes;
}

template <class... P>
int launch_policy_kernel(const char* who, PolicyKernel<P...> k, int32_t n_lanes, int threads, hipStream_t s,
                         const P&... args) {
  if (int e = ensure_dynamic_lds(reinterpret_cast<const void*>(k.fn), k.lds, who)) return e;
  hipLaunchKernelGGL(k.fn, dim3(policy_workgroups(n_lanes)), dim3(threads), k.lds, s, args...);
  return check_launch(who);
}

// `io` as a kernel takes it: zeroed in summary mode (io NULL); the kernel reads the pitch as given: never 0
inline carl_step_io_t launch_io(const carl_batch_t* b, const carl_step_io_t* io) {
  carl_step_io_t r{};
  if (io != nullptr) {
    r = *io;
    r.row_pitch = io->row_pitch > 0 ? io->row_pitch : b->n_lanes;
  }
  return r;
}

inline carl_policy_summary_t launch_summary(const carl_policy_summary_t* sum) {
  return sum != nullptr ? *sum : carl_policy_summary_t{nullptr, nullptr, nullptr};
}

inline carl_policy_sampling_t launch_sampling(const carl_policy_sampling_t* smp) {
  return smp != nullptr ? *smp : carl_policy_sampling_t{0, nullptr, nullptr};
}

}  // namespace carl_host
