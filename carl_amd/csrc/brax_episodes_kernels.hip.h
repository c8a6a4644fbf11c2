// brax_episodes_kernels.hip.h -- the episodes mode of the Brax closed-loop rollout (include/carl_amd.h:
// carl_brax_evaluate_policy): the policy type that selects it in Group<K>::run's MODE 2 (brax_kernels.hip.h: Pol::kEpisodes)
// and the kernel around it.  The network, its arithmetic and where it runs are BraxPolicy's (brax_policy_kernels.hip.h),
// inherited, not restated; the step, observe, reward, done and auto-reset text is run()'s, shared with every other mode.
// What the variant adds is there, beside the MODE == 2 blocks: an env is live while it has episodes left to finish, its
// global writes stop when it freezes, and the wavefront leaves the step loop under a ballot once no env is live.
#pragma once

#include "brax_policy_kernels.hip.h"

namespace carl {
namespace brax {

struct BraxEpisodesPolicy : BraxPolicy {
  static constexpr bool kEpisodes = true;
  carl_policy_episodes_t ep;  // the records; every slot is written (validated by the host: carl_brax_episodes.hip)
  int n_episodes;             // an env stops after this many (the kernel's n_steps is max_steps)
};

// brax_policy_kernel's episodes twin, one instance per instance of it.
template <bool MULTI, int K, bool TASK = false, bool PLANAR = false>
__global__ void __launch_bounds__(kLanes * max_waves_per_wg(TASK)) __attribute__((amdgpu_waves_per_eu(CARL_BRAX_WAVES_PER_EU(TASK))))
brax_episodes_kernel(const carl_batch_t b, const carl_brax_sys_t* __restrict__ sys_dev, const Prepared prep,
                     const carl_step_io_t io, const BraxEpisodesPolicy pol, const int max_steps) {
  Group<K>::template run<2, MULTI, TASK, PLANAR, false, BraxEpisodesPolicy>(b, sys_dev, prep, io, nullptr, nullptr, max_steps, pol);
}

}  // namespace brax
}  // namespace carl
