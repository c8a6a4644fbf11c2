// carl_brax_policy_sample.hip -- C-ABI entry point of the sampled closed-loop rollout of the Brax families
// (include/carl_amd.h: carl_brax_rollout_policy_sampled) and its kernel table.  A translation unit of its own, as
// carl_brax_episodes.hip is: the kernels are the Pol::kSampled variant of MODE 2 of brax_kernels.hip.h's run(),
// instantiated here and nowhere else, so that every other unit -- carl_brax_policy.hip included -- compiles exactly as it
// did without them (profiles/brax_policy_sample_isa_identity.txt).  The checks, the list of instances and the launch are
// the closed-loop units' (brax_launch.hpp, brax_policy_host.hpp); the launch shape is carl_brax_policy_launch_shape's.
// Same flags as carl_brax_policy.hip (carl_amd/build.py).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/carl_amd.h"
#include "brax_launch.hpp"
#include "brax_policy_host.hpp"
#include "brax_sample_kernels.hip.h"
#include "host_common.hpp"
#include "policy_host.hpp"

namespace {

using carl_host::fail;
using carl_host::brax::BraxClass;

// Every instantiated brax_policy_sampled_kernel<MULTI, K, TASK, PLANAR>.
#define X(M, K, T, P) {{M, T, P, false}, K, carl::brax::brax_policy_sampled_kernel<M, K, T, P>},
const carl_host::brax::ClosedLoopKernel<carl::brax::BraxSampledPolicy> kBraxSampledKernels[] = {CARL_BRAX_CLOSED_LOOP_INSTANCES(X)};
#undef X

}  // namespace

extern "C" {

int carl_brax_rollout_policy_sampled(const carl_batch_t* batch, const carl_brax_sys_t* sys_dev, const carl_brax_sys_t* sys_host,
                                     float* obs, const carl_policy_t* policy_host, const carl_policy_sampling_t* sampling,
                                     const carl_step_io_t* io, int32_t n_steps, const carl_policy_summary_t* summary_out,
                                     void* stream) {
  const char* who = "carl_brax_rollout_policy_sampled";
  BraxClass c;
  if (int e = carl_host::brax::validate_closed_loop(who, batch, sys_dev, sys_host, obs, policy_host, &c)) return e;
  if (int e = carl_host::brax::validate_rollout(who, batch, io, n_steps, summary_out)) return e;
  if (int e = carl_host::brax::validate_sampling(who, batch, sys_host, io, sampling)) return e;
  if (batch->n_lanes == 0 || n_steps == 0) return carl_host::policy_rollout_without_steps(who, batch, summary_out, stream);

  carl_step_io_t io_v{};
  if (io != nullptr) io_v = *io;
  carl::brax::BraxSampledPolicy pol = carl_host::brax::make_policy<carl::brax::BraxSampledPolicy>(policy_host, obs);
  if (summary_out != nullptr) pol.sum = *summary_out;
  pol.seed = sampling->seed;
  pol.log_std = sampling->log_std;
  pol.log_prob = sampling->log_prob;
  return carl_host::brax::launch_closed_loop(kBraxSampledKernels, batch, sys_dev, sys_host, c, n_steps, io_v, pol, stream, who);
}

}  // extern "C"
