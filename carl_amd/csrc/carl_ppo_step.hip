// carl_ppo_step.hip -- C-ABI entry points of PPO's minibatch step (include/carl_amd.h: carl_ppo_adv_stats, carl_adam_step)
// and their launches.  A translation unit of its own, so that every other unit's kernels compile exactly as they did.  The
// kernels are ppo_step_kernels.hip.h's; the checks are ppo_step_host.hpp's, which a population's entry points
// (carl_ppo_sets.hip) share.  Neither call knows a family: both serve the classic and the Brax engines.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/carl_amd.h"
#include "host_common.hpp"
#include "ppo_step_host.hpp"
#include "ppo_step_kernels.hip.h"

namespace {

using carl_host::check_launch;

}  // namespace

extern "C" {

int32_t carl_ppo_adv_stats_rows(int32_t n_total, int32_t batch_size) { return carl_host::adv_rows(n_total, batch_size); }

int carl_ppo_adv_stats(const carl_ppo_adv_stats_t* as, void* stream) {
  const char* who = "carl_ppo_adv_stats";
  if (int e = carl_host::check_adv_stats(who, as)) return e;
  const carl::PpoAdvStatsArgs a = carl_host::adv_stats_args(as);
  hipLaunchKernelGGL(carl::ppo_adv_stats_kernel, dim3(carl_host::adv_rows(as->n_total, as->batch_size)),
                     dim3(carl::kAdvThreads), 0, (hipStream_t)stream, a);
  return check_launch(who);
}

int64_t carl_adam_step_max_floats(void) { return carl::kAdamMaxFloats; }

int carl_adam_step(const carl_adam_t* ad, void* stream) {
  const char* who = "carl_adam_step";
  int64_t total = 0;
  if (int e = carl_host::check_adam(who, ad, true, &total)) return e;
  if (total == 0) return 0;
  const carl::AdamArgs a = carl_host::adam_args(ad);
  hipLaunchKernelGGL(carl::adam_step_kernel, dim3(1), dim3(carl::kAdamThreads), 0, (hipStream_t)stream, a);
  return check_launch(who);
}

}  // extern "C"
