// carl_brax_policy.hip -- C-ABI entry points of the closed-loop rollout of the Brax families (include/carl_amd.h:
// carl_brax_rollout_policy) and their kernel table.  A translation unit of its own: the kernels are MODE 2 of
// brax_kernels.hip.h's run(), instantiated here and nowhere else, so that the reset / step / rollout kernels of
// carl_brax.hip compile exactly as they did without them (profiles/brax_policy_isa_identity.txt).  The batch, model and io
// checks and the launch-shape rule are carl_brax.hip's (brax_launch.hpp); the network's shape rules are the classic
// closed-loop rollout's (policy_host.hpp); the policy's and the rollout's checks, the list of instances and the launch are
// the closed-loop units' (brax_policy_host.hpp).  The tables of all of them hold the same instances under one launch
// rule, so carl_brax_policy_launch_shape answers for carl_brax_rollout_policy_sampled too.  Same flags as carl_brax.hip (carl_amd/build.py).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/carl_amd.h"
#include "brax_launch.hpp"
#include "brax_policy_kernels.hip.h"
#include "brax_policy_host.hpp"
#include "host_common.hpp"
#include "policy_host.hpp"

namespace {

using carl_host::fail;
using carl_host::brax::BraxClass;
using carl_host::brax::BraxShape;
using carl_host::brax::brax_policy_floats;
using carl_host::brax::policy_class;

// Every instantiated brax_policy_kernel<MULTI, K, TASK, PLANAR>.
#define X(M, K, T, P) {{M, T, P, false}, K, carl::brax::brax_policy_kernel<M, K, T, P>},
const carl_host::brax::ClosedLoopKernel<carl::brax::BraxPolicy> kBraxPolicyKernels[] = {CARL_BRAX_CLOSED_LOOP_INSTANCES(X)};
#undef X

}  // namespace

extern "C" {

int32_t carl_brax_policy_set_floats(const carl_policy_t* policy_host) {
  if (policy_host == nullptr) return -1;
  return brax_policy_floats(policy_host);
}

int carl_brax_policy_launch_shape(const carl_batch_t* batch, const carl_brax_sys_t* sys_host, const carl_policy_t* policy_host,
                                  int32_t n_steps, carl_brax_launch_shape_t* out) {
  const char* who = "carl_brax_policy_launch_shape";
  if (batch == nullptr || sys_host == nullptr || policy_host == nullptr || out == nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: NULL argument", who);
  if (batch->n_lanes < 1 || n_steps < 1 || sys_host->n_links < 1 || sys_host->n_links > CARL_BRAX_MAX_LINKS)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_lanes %d / n_steps %d / n_links %d out of range", who, batch->n_lanes, n_steps,
                sys_host->n_links);
  BraxClass c;
  if (int e = policy_class(who, batch, sys_host, &c)) return e;
  BraxShape shape;
  if (int e = carl_host::brax::policy_launch(kBraxPolicyKernels, batch, sys_host, c, n_steps, who, &shape, nullptr)) return e;
  *out = carl_brax_launch_shape_t{shape.grid, shape.W, shape.K, 0, (int64_t)shape.lds_bytes};
  return 0;
}

int carl_brax_rollout_policy(const carl_batch_t* batch, const carl_brax_sys_t* sys_dev, const carl_brax_sys_t* sys_host,
                             float* obs, const carl_policy_t* policy_host, const carl_step_io_t* io, int32_t n_steps,
                             const carl_policy_summary_t* summary_out, void* stream) {
  const char* who = "carl_brax_rollout_policy";
  BraxClass c;
  if (int e = carl_host::brax::validate_closed_loop(who, batch, sys_dev, sys_host, obs, policy_host, &c)) return e;
  if (int e = carl_host::brax::validate_rollout(who, batch, io, n_steps, summary_out)) return e;
  if (batch->n_lanes == 0 || n_steps == 0) return carl_host::policy_rollout_without_steps(who, batch, summary_out, stream);

  carl_step_io_t io_v{};
  if (io != nullptr) io_v = *io;
  carl::brax::BraxPolicy pol = carl_host::brax::make_policy<carl::brax::BraxPolicy>(policy_host, obs);
  if (summary_out != nullptr) pol.sum = *summary_out;
  return carl_host::brax::launch_closed_loop(kBraxPolicyKernels, batch, sys_dev, sys_host, c, n_steps, io_v, pol, stream, who);
}

}  // extern "C"
