// carl_brax_episodes.hip -- C-ABI entry point of the episodes mode of the Brax closed-loop rollout (include/carl_amd.h:
// carl_brax_evaluate_policy) and its kernel dispatch.  A translation unit of its own, as carl_brax_policy.hip is: the
// kernels are the Pol::kEpisodes variant of MODE 2 of brax_kernels.hip.h's run(), instantiated here and nowhere else, so
// that every other unit -- carl_brax_policy.hip included -- compiles exactly as it did without them
// (profiles/brax_episodes_isa_identity.txt).  The batch, model and policy checks and the launch rule are the closed-loop
// rollout's (brax_launch.hpp, brax_policy_host.hpp).  Same flags as carl_brax_policy.hip (carl_amd/build.py).
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
using carl_host::fail;
using carl_host::brax::BraxClass;
using carl_host::brax::BraxShape;

// Every instantiated brax_episodes_kernel<MULTI, K, TASK, PLANAR>: carl_brax_policy.hip's kBraxPolicyKernels, entry for
// entry (tests/test_brax_episodes_abi.py holds the two tables together; carl_brax_policy_launch_shape answers for both).
using brax_episodes_kern_t = void (*)(carl_batch_t, const carl_brax_sys_t*, carl::brax::Prepared, carl_step_io_t,
                                      carl::brax::BraxEpisodesPolicy, int);
struct BraxEpisodesKernel {
  BraxClass c;
  int k;
  brax_episodes_kern_t kern;
};
#define CARL_BRAX_EPISODES(MULTI, K, TASK, PLANAR) \
  {{MULTI, TASK, PLANAR, false}, K, carl::brax::brax_episodes_kernel<MULTI, K, TASK, PLANAR>}
const BraxEpisodesKernel kBraxEpisodesKernels[] = {
    // lean
    CARL_BRAX_EPISODES(false, 4, false, false), CARL_BRAX_EPISODES(false, 7, false, false),
    CARL_BRAX_EPISODES(false, 8, false, false), CARL_BRAX_EPISODES(false, 9, false, false),
    CARL_BRAX_EPISODES(false, 16, false, false),
    // multi-hinge
    CARL_BRAX_EPISODES(true, 2, false, false), CARL_BRAX_EPISODES(true, 11, false, false),
    CARL_BRAX_EPISODES(true, 16, false, false),
    // general: reach / push task models and anisotropic inertia
    CARL_BRAX_EPISODES(true, 4, true, false), CARL_BRAX_EPISODES(true, 8, true, false), CARL_BRAX_EPISODES(true, 16, true, false),
    // planar
    CARL_BRAX_EPISODES(false, 4, false, true), CARL_BRAX_EPISODES(false, 7, false, true),
    CARL_BRAX_EPISODES(false, 8, false, true), CARL_BRAX_EPISODES(false, 9, false, true),
    CARL_BRAX_EPISODES(false, 16, false, true),
};
#undef CARL_BRAX_EPISODES

static_assert(sizeof(carl_batch_t) + sizeof(carl::brax::Prepared) + sizeof(carl_step_io_t) + sizeof(carl::brax::BraxEpisodesPolicy) + 64 <= 4096,
              "the episodes kernel's arguments do not fit the 4 KiB kernel-argument segment");

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

  BraxShape shape;
  brax_episodes_kern_t kern = nullptr;
  if (int e = carl_host::brax::policy_launch(kBraxEpisodesKernels, batch, sys_host, c, max_steps, who, &shape, &kern)) return e;
  carl::brax::BraxEpisodesPolicy pol{};
  pol.p = *policy_host;
  pol.set_floats = carl_host::brax::brax_policy_floats(policy_host);
  pol.sum = carl_policy_summary_t{nullptr, nullptr, nullptr};
  pol.cur_obs = obs;
  pol.ep = *out;
  pol.n_episodes = n_episodes;
  carl::brax::Prepared prep{};
  carl::brax::build_topo_host(*sys_host, prep.topo);
  carl::brax::build_packed_host(*sys_host, prep.topo, prep.packed);
  // (no per-step record: the all-NULL io is run()'s summary mode)
  hipLaunchKernelGGL(kern, dim3(shape.grid), dim3(carl::brax::kLanes * shape.W), shape.lds_bytes, (hipStream_t)stream, *batch,
                     sys_dev, prep, carl_step_io_t{}, pol, (int)max_steps);
  return check_launch(who);
}

}  // extern "C"
