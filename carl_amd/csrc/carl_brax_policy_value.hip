// carl_brax_policy_value.hip -- C-ABI entry point of the sampled closed-loop rollout of the Brax families with a critic
// (include/carl_amd.h: carl_brax_rollout_policy_valued) and its kernel table.  A translation unit of its own, as
// carl_brax_policy_sample.hip is: the kernels are the Pol::kValued variant of the sampled MODE 2 of brax_kernels.hip.h's
// run(), instantiated here and nowhere else, so that every other unit compiles exactly as it did without them
// (profiles/brax_policy_value_isa_identity.txt).  The checks, the list of instances and the launch are the closed-loop
// units' (brax_launch.hpp, brax_policy_host.hpp); the launch shape is carl_brax_policy_launch_shape's.
// Same flags as carl_brax_policy.hip (carl_amd/build.py).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/carl_amd.h"
#include "brax_launch.hpp"
#include "brax_policy_host.hpp"
#include "brax_value_kernels.hip.h"
#include "host_common.hpp"
#include "policy_host.hpp"

namespace {

using carl_host::fail;
using carl_host::brax::BraxClass;

// Every instantiated brax_policy_valued_kernel<MULTI, K, TASK, PLANAR>.
#define X(M, K, T, P) {{M, T, P, false}, K, carl::brax::brax_policy_valued_kernel<M, K, T, P>},
const carl_host::brax::ClosedLoopKernel<carl::brax::BraxValuedPolicy> kBraxValuedKernels[] = {CARL_BRAX_CLOSED_LOOP_INSTANCES(X)};
#undef X

// the critic against the actor, which validate_closed_loop has checked against the batch and the model
int check_critic(const char* who, const carl_policy_t* p, const carl_policy_t* c) {
  if (int e = carl_host::check_hidden_layers(who, c)) return e;
  if (c->n_out != 1) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: head width %d, a value network has 1", who, c->n_out);
  if (c->n_in != p->n_in || c->n_ctx != p->n_ctx)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_in %d / n_ctx %d, the actor has %d / %d (the critic reads the actor's "
                "inputs)", who, c->n_in, c->n_ctx, p->n_in, p->n_ctx);
  for (int k = 0; k < p->n_ctx; ++k)
    if (c->ctx_rows[k] != p->ctx_rows[k])
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: ctx_rows[%d] = %d, the actor's is %d", who, k, c->ctx_rows[k], p->ctx_rows[k]);
  if (int e = carl_host::check_activation(who, c)) return e;
  if (c->n_sets != p->n_sets || c->lanes_per_set != p->lanes_per_set)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: %d sets x %d lanes, the actor has %d x %d", who, c->n_sets, c->lanes_per_set,
                p->n_sets, p->lanes_per_set);
  if (int e = carl_host::check_params(who, c)) return e;
  if (reinterpret_cast<uintptr_t>(c->params) % 16 != 0)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: params must start on a 16-byte boundary (weight rows are read 16 bytes at a time)",
                who);
  return 0;
}

}  // namespace

extern "C" {

int carl_brax_rollout_policy_valued(const carl_batch_t* batch, const carl_brax_sys_t* sys_dev, const carl_brax_sys_t* sys_host,
                                    float* obs, const carl_policy_t* policy_host, const carl_policy_t* critic_host,
                                    const carl_policy_sampling_t* sampling, const carl_step_io_t* io, int32_t n_steps,
                                    const carl_policy_summary_t* summary_out, const carl_policy_value_t* out, void* stream) {
  const char* who = "carl_brax_rollout_policy_valued";
  BraxClass c;
  if (int e = carl_host::brax::validate_closed_loop(who, batch, sys_dev, sys_host, obs, policy_host, &c)) return e;
  if (int e = carl_host::brax::validate_rollout(who, batch, io, n_steps, summary_out)) return e;
  if (io == nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: io is NULL -- transitions mode only (a summary has no use for values)", who);
  if (int e = carl_host::brax::validate_sampling(who, batch, sys_host, io, sampling)) return e;
  if (sampling->log_prob == nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: sampling->log_prob is NULL (a valued launch always stores the "
                "log-probabilities)", who);
  if (critic_host == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: critic is NULL", who);
  if (int e = check_critic("carl_brax_rollout_policy_valued: critic", policy_host, critic_host)) return e;
  if (out == nullptr || out->value == nullptr || out->last_value == nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: out, out->value and out->last_value are required", who);
  if (out->boot_value != nullptr && !(batch->flags & CARL_FLAG_AUTORESET))
    return fail(CARL_ERR_UNSUPPORTED, "%s: out->boot_value needs CARL_FLAG_AUTORESET (without auto-reset no terminal "
                "observation is kept apart from the next one)", who);
  if (batch->n_lanes == 0 || n_steps == 0) return carl_host::policy_rollout_without_steps(who, batch, summary_out, stream);

  carl::brax::BraxValuedPolicy pol = carl_host::brax::make_policy<carl::brax::BraxValuedPolicy>(policy_host, obs);
  if (summary_out != nullptr) pol.sum = *summary_out;
  pol.seed = sampling->seed;
  pol.log_std = sampling->log_std;
  pol.log_prob = sampling->log_prob;
  pol.critic = *critic_host;
  pol.critic_set_floats = carl_host::brax::brax_policy_floats(critic_host);
  pol.xf_at = carl_host::policy_transform_offset(policy_host);
  pol.value = out->value;
  pol.last_value = out->last_value;
  pol.boot_value = out->boot_value;
  return carl_host::brax::launch_closed_loop(kBraxValuedKernels, batch, sys_dev, sys_host, c, n_steps, *io, pol, stream, who);
}

}  // extern "C"
