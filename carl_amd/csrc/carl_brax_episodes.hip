// carl_brax_episodes.hip -- C-ABI entry point of the episodes mode of the Brax closed-loop rollout (include/carl_amd.h:
// carl_brax_evaluate_policy) and its kernel table.  A translation unit of its own, as carl_brax_policy.hip is: the
// kernels are the Pol::kEpisodes variant of MODE 2 of brax_kernels.hip.h's run(), instantiated here and nowhere else, so
// that every other unit -- carl_brax_policy.hip included -- compiles exactly as it did without them
// (profiles/brax_episodes_isa_identity.txt).  The checks, the list of instances and the launch are the three closed-loop
// units' (brax_launch.hpp, brax_policy_host.hpp).  Same flags as carl_brax_policy.hip (carl_amd/build.py).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/carl_amd.h"
#include "brax_episodes_kernels.hip.h"
#include "brax_launch.hpp"
#include "brax_policy_host.hpp"
#include "host_common.hpp"

namespace carl {
namespace brax {

// max_steps == 0: nothing is stepped and no episode finishes, but every output is still written.  (Defined in this unit,
// not in the kernels' header: carl_brax_policy_stats.hip includes that header and calls the entry point below instead.)
__global__ void __launch_bounds__(256) brax_episodes_empty_kernel(const carl_policy_episodes_t ep, const int n_lanes,
                                                                  const int n_episodes) {
  const int env = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (env >= n_lanes) return;
  ep.episodes[env] = 0;
  ep.steps[env] = 0;
  for (int k = 0; k < n_episodes; ++k) {
    const size_t at = (size_t)k * (size_t)n_lanes + (size_t)env;
    ep.ret[at] = __builtin_nanf("");
    ep.length[at] = 0;
    ep.context_id[at] = -1;
    ep.terminated[at] = 0;
  }
}

}  // namespace brax
}  // namespace carl

namespace {

using carl_host::check_launch;
using carl_host::brax::BraxClass;

// Every instantiated brax_episodes_kernel<MULTI, K, TASK, PLANAR>.
#define X(M, K, T, P) {{M, T, P, false}, K, carl::brax::brax_episodes_kernel<M, K, T, P>},
const carl_host::brax::ClosedLoopKernel<carl::brax::BraxEpisodesPolicy> kBraxEpisodesKernels[] = {
    CARL_BRAX_CLOSED_LOOP_INSTANCES(X)};
#undef X

}  // namespace

extern "C" {

int carl_brax_evaluate_policy(const carl_batch_t* batch, const carl_brax_sys_t* sys_dev, const carl_brax_sys_t* sys_host,
                              float* obs, const carl_policy_t* policy_host, int32_t n_episodes, int32_t max_steps,
                              const carl_policy_episodes_t* out, void* stream) {
  const char* who = "carl_brax_evaluate_policy";
  BraxClass c;
  if (int e = carl_host::brax::validate_closed_loop(who, batch, sys_dev, sys_host, obs, policy_host, &c)) return e;
  if (int e = carl_host::brax::validate_episodes(who, batch, n_episodes, max_steps, out)) return e;
  if (batch->n_lanes == 0) return 0;
  if (max_steps == 0) {
    hipLaunchKernelGGL(carl::brax::brax_episodes_empty_kernel, dim3((batch->n_lanes + 255) / 256), dim3(256), 0,
                       (hipStream_t)stream, *out, (int)batch->n_lanes, (int)n_episodes);
    return check_launch(who);
  }

  const carl::brax::BraxEpisodesPolicy pol =
      carl_host::brax::make_episodes_policy<carl::brax::BraxEpisodesPolicy>(policy_host, obs, out, n_episodes);
  return carl_host::brax::launch_closed_loop(kBraxEpisodesKernels, batch, sys_dev, sys_host, c, max_steps, carl_step_io_t{}, pol,
                                             stream, who);
}

}  // extern "C"
