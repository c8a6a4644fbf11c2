// carl_brax_policy_stats.hip -- C-ABI entry points of the input statistics of the Brax closed-loop rollout
// (include/carl_amd.h: carl_brax_evaluate_policy_stats, carl_brax_policy_stats_slabs) and their kernel dispatch.  A
// translation unit of its own, as carl_brax_episodes.hip is: the kernels are the Pol::kStats variant of the episodes mode
// of brax_kernels.hip.h's run(), instantiated here and nowhere else, so that every other unit -- carl_brax_episodes.hip
// included -- compiles exactly as it did without them (profiles/brax_stats_isa_identity.txt).  The checks and the launch
// rule are the episodes entry point's (brax_launch.hpp, brax_policy_host.hpp), the check of the statistics output is
// carl_evaluate_policy_stats' (policy_host.hpp); the merge, carl_brax_policy_stats_merge, sits beside the kernel it calls
// in carl_policy_stats.hip.  Same flags as carl_brax_episodes.hip (carl_amd/build.py).
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

// Every instantiated brax_episodes_stats_kernel<MULTI, K, TASK, PLANAR>: carl_brax_episodes.hip's kBraxEpisodesKernels,
// entry for entry (tests/test_brax_stats_abi.py holds the tables together).
using brax_stats_kern_t = void (*)(carl_batch_t, const carl_brax_sys_t*, carl::brax::Prepared, carl_step_io_t,
                                   carl::brax::BraxStatsPolicy, int);
struct BraxStatsKernel {
  BraxClass c;
  int k;
  brax_stats_kern_t kern;
};
#define CARL_BRAX_STATS(MULTI, K, TASK, PLANAR) \
  {{MULTI, TASK, PLANAR, false}, K, carl::brax::brax_episodes_stats_kernel<MULTI, K, TASK, PLANAR>}
const BraxStatsKernel kBraxStatsKernels[] = {
    // lean
    CARL_BRAX_STATS(false, 4, false, false), CARL_BRAX_STATS(false, 7, false, false),
    CARL_BRAX_STATS(false, 8, false, false), CARL_BRAX_STATS(false, 9, false, false),
    CARL_BRAX_STATS(false, 16, false, false),
    // multi-hinge
    CARL_BRAX_STATS(true, 2, false, false), CARL_BRAX_STATS(true, 11, false, false),
    CARL_BRAX_STATS(true, 16, false, false),
    // general: reach / push task models and anisotropic inertia
    CARL_BRAX_STATS(true, 4, true, false), CARL_BRAX_STATS(true, 8, true, false), CARL_BRAX_STATS(true, 16, true, false),
    // planar
    CARL_BRAX_STATS(false, 4, false, true), CARL_BRAX_STATS(false, 7, false, true),
    CARL_BRAX_STATS(false, 8, false, true), CARL_BRAX_STATS(false, 9, false, true),
    CARL_BRAX_STATS(false, 16, false, true),
};
#undef CARL_BRAX_STATS

static_assert(sizeof(carl_batch_t) + sizeof(carl::brax::Prepared) + sizeof(carl_step_io_t) + sizeof(carl::brax::BraxStatsPolicy) + 64 <= 4096,
              "the statistics kernel's arguments do not fit the 4 KiB kernel-argument segment");

// the launch shape of max_steps steps; a launch of no step has the slabs of a launch of one
int stats_shape(const char* who, const carl_batch_t* batch, const carl_brax_sys_t* sys_host, const BraxClass& c, int max_steps,
                BraxShape* shape, brax_stats_kern_t* kern) {
  return carl_host::brax::policy_launch(kBraxStatsKernels, batch, sys_host, c, max_steps > 0 ? max_steps : 1, who, shape, kern);
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
                  max_steps, &shape, nullptr))
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
    if (int e = stats_shape(who, batch, sys_host, c, max_steps, &shape, nullptr)) return e;
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

  brax_stats_kern_t kern = nullptr;
  if (int e = stats_shape(who, batch, sys_host, c, max_steps, &shape, &kern)) return e;
  carl::brax::BraxStatsPolicy pol{};
  pol.p = *policy_host;
  pol.set_floats = carl_host::brax::brax_policy_floats(policy_host);
  pol.sum = carl_policy_summary_t{nullptr, nullptr, nullptr};
  pol.cur_obs = obs;
  pol.ep = *out;
  pol.n_episodes = n_episodes;
  pol.partial = stats->partial;
  carl::brax::Prepared prep{};
  carl::brax::build_topo_host(*sys_host, prep.topo);
  carl::brax::build_packed_host(*sys_host, prep.topo, prep.packed);
  // (no per-step record: the all-NULL io is run()'s summary mode)
  hipLaunchKernelGGL(kern, dim3(shape.grid), dim3(carl::brax::kLanes * shape.W), shape.lds_bytes, (hipStream_t)stream, *batch,
                     sys_dev, prep, carl_step_io_t{}, pol, (int)max_steps);
  return check_launch(who);
}

}  // extern "C"
