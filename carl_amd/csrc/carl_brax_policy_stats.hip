// carl_brax_policy_stats.hip -- C-ABI entry points of the input statistics of the Brax closed-loop rollout
// (include/carl_amd.h: carl_brax_evaluate_policy_stats, carl_brax_policy_stats_slabs) and their kernel table.  A
// translation unit of its own, as carl_brax_episodes.hip is: the kernels are the Pol::kStats variant of the episodes mode
// of brax_kernels.hip.h's run(), instantiated here and nowhere else, so that every other unit -- carl_brax_episodes.hip
// included -- compiles exactly as it did without them (profiles/brax_stats_isa_identity.txt).  The checks, the list of
// instances and the launch are the three closed-loop units' (brax_launch.hpp, brax_policy_host.hpp), the check of the
// statistics output is carl_evaluate_policy_stats' (policy_host.hpp); the merge, carl_brax_policy_stats_merge, sits beside
// the kernel it calls in carl_policy_stats.hip.  Same flags as carl_brax_episodes.hip (carl_amd/build.py).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/carl_amd.h"
#include "brax_launch.hpp"
#include "brax_policy_host.hpp"
#include "brax_stats_kernels.hip.h"
#include "host_common.hpp"

namespace {

using carl_host::check_launch;
using carl_host::brax::BraxClass;
using carl_host::brax::BraxShape;

// Every instantiated brax_episodes_stats_kernel<MULTI, K, TASK, PLANAR>.
#define X(M, K, T, P) {{M, T, P, false}, K, carl::brax::brax_episodes_stats_kernel<M, K, T, P>},
const carl_host::brax::ClosedLoopKernel<carl::brax::BraxStatsPolicy> kBraxStatsKernels[] = {CARL_BRAX_CLOSED_LOOP_INSTANCES(X)};
#undef X

// the launch shape of max_steps steps; a launch of no step has the slabs of a launch of one
int stats_shape(const char* who, const carl_batch_t* batch, const carl_brax_sys_t* sys_host, const BraxClass& c, int max_steps,
                BraxShape* shape) {
  return carl_host::brax::policy_launch(kBraxStatsKernels, batch, sys_host, c, max_steps > 0 ? max_steps : 1, who, shape, nullptr);
}

}  // namespace

extern "C" {

int32_t carl_brax_policy_stats_slabs(const carl_batch_t* batch, const carl_brax_sys_t* sys_host, const carl_policy_t* policy_host,
                                     int32_t max_steps) {
  if (batch == nullptr || sys_host == nullptr || policy_host == nullptr || max_steps < 0 || sys_host->n_links < 1 ||
      sys_host->n_links > CARL_BRAX_MAX_LINKS || (batch->flags & CARL_FLAG_BRAX_FP32))
    return -1;
  if (batch->n_lanes <= 0) return 0;
  BraxShape shape;
  if (stats_shape("carl_brax_policy_stats_slabs", batch, sys_host, carl_host::brax::brax_class(sys_host, batch->flags, true),
                  max_steps, &shape))
    return -1;
  return shape.grid * shape.W;
}

int carl_brax_evaluate_policy_stats(const carl_batch_t* batch, const carl_brax_sys_t* sys_dev, const carl_brax_sys_t* sys_host,
                                    float* obs, const carl_policy_t* policy_host, int32_t n_episodes, int32_t max_steps,
                                    const carl_policy_episodes_t* out, const carl_policy_stats_t* stats, void* stream) {
  const char* who = "carl_brax_evaluate_policy_stats";
  BraxClass c;
  if (int e = carl_host::brax::validate_closed_loop(who, batch, sys_dev, sys_host, obs, policy_host, &c)) return e;
  if (int e = carl_host::brax::validate_episodes(who, batch, n_episodes, max_steps, out)) return e;
  // (the shape alone first: the refusals below come before anything touches the device, the kernel's LDS limit included)
  BraxShape shape{};
  if (batch->n_lanes > 0)
    if (int e = stats_shape(who, batch, sys_host, c, max_steps, &shape)) return e;
  const int n_slabs = shape.grid * shape.W;
  if (int e = carl_host::check_policy_stats(who, stats, n_slabs, "slabs (carl_brax_policy_stats_slabs)")) return e;
  if (batch->n_lanes == 0) return 0;
  if (max_steps == 0) {
    // (the records of a launch of no step: the episodes entry point's own, every check of it passed above)
    if (int e = carl_brax_evaluate_policy(batch, sys_dev, sys_host, obs, policy_host, n_episodes, 0, out, stream)) return e;
    const size_t n = (size_t)n_slabs * 2 * CARL_POLICY_MAX_IN;
    hipLaunchKernelGGL(carl::brax::brax_stats_zero_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       stats->partial, n);
    return check_launch(who);
  }

  carl::brax::BraxStatsPolicy pol =
      carl_host::brax::make_episodes_policy<carl::brax::BraxStatsPolicy>(policy_host, obs, out, n_episodes);
  pol.partial = stats->partial;
  return carl_host::brax::launch_closed_loop(kBraxStatsKernels, batch, sys_dev, sys_host, c, max_steps, carl_step_io_t{}, pol,
                                             stream, who);
}

}  // extern "C"
