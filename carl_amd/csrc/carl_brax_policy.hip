// carl_brax_policy.hip -- C-ABI entry points of the closed-loop rollout of the Brax families (include/carl_amd.h:
// carl_brax_rollout_policy) and their kernel dispatch.  A translation unit of its own: the kernels are MODE 2 of
// brax_kernels.hip.h's run(), instantiated here and nowhere else, so that the reset / step / rollout kernels of
// carl_brax.hip compile exactly as they did without them (profiles/brax_policy_isa_identity.txt).  The batch, model and io
// checks and the launch-shape rule are carl_brax.hip's (brax_launch.hpp); the network's shape rules are the classic
// closed-loop rollout's (policy_host.hpp); the policy's checks and the launch rule are shared with the episodes mode's unit
// (brax_policy_host.hpp; carl_brax_episodes.hip).  Same flags as carl_brax.hip (carl_amd/build.py).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/carl_amd.h"
#include "brax_launch.hpp"
#include "brax_policy_kernels.hip.h"
#include "brax_policy_host.hpp"
#include "host_common.hpp"
#include "policy_host.hpp"

namespace {

using carl_host::check_launch;
using carl_host::fail;
using carl_host::brax::BraxClass;
using carl_host::brax::BraxShape;
using carl_host::brax::brax_policy_floats;
using carl_host::brax::policy_class;

// Every instantiated brax_policy_kernel<MULTI, K, TASK, PLANAR>: the non-F32 step classes of carl_brax.hip's kBraxKernels,
// at the widths it has for them (tests/test_brax_policy_abi.py holds the two tables together).
using brax_policy_kern_t = void (*)(carl_batch_t, const carl_brax_sys_t*, carl::brax::Prepared, carl_step_io_t,
                                    carl::brax::BraxPolicy, int);
struct BraxPolicyKernel {
  BraxClass c;
  int k;
  brax_policy_kern_t kern;
};
#define CARL_BRAX_POLICY(MULTI, K, TASK, PLANAR) \
  {{MULTI, TASK, PLANAR, false}, K, carl::brax::brax_policy_kernel<MULTI, K, TASK, PLANAR>}
const BraxPolicyKernel kBraxPolicyKernels[] = {
    // lean
    CARL_BRAX_POLICY(false, 4, false, false), CARL_BRAX_POLICY(false, 7, false, false),
    CARL_BRAX_POLICY(false, 8, false, false), CARL_BRAX_POLICY(false, 9, false, false),
    CARL_BRAX_POLICY(false, 16, false, false),
    // multi-hinge
    CARL_BRAX_POLICY(true, 2, false, false), CARL_BRAX_POLICY(true, 11, false, false),
    CARL_BRAX_POLICY(true, 16, false, false),
    // general: reach / push task models and anisotropic inertia
    CARL_BRAX_POLICY(true, 4, true, false), CARL_BRAX_POLICY(true, 8, true, false), CARL_BRAX_POLICY(true, 16, true, false),
    // planar
    CARL_BRAX_POLICY(false, 4, false, true), CARL_BRAX_POLICY(false, 7, false, true),
    CARL_BRAX_POLICY(false, 8, false, true), CARL_BRAX_POLICY(false, 9, false, true),
    CARL_BRAX_POLICY(false, 16, false, true),
};
#undef CARL_BRAX_POLICY

static_assert(sizeof(carl_batch_t) + sizeof(carl::brax::Prepared) + sizeof(carl_step_io_t) + sizeof(carl::brax::BraxPolicy) + 64 <= 4096,
              "the closed-loop kernel's arguments do not fit the 4 KiB kernel-argument segment");

bool summary_complete(const carl_policy_summary_t* s) { return s->episodes && s->return_sum && s->length_sum; }

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
  if (n_steps < 0) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_steps %d < 0", who, n_steps);
  if (io == nullptr) {
    if (summary_out == nullptr || !summary_complete(summary_out))
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: summary mode (io NULL) needs all three summary arrays", who);
  } else {
    if (int e = carl_host::brax::validate_brax_io(io, who)) return e;
    if (summary_out != nullptr && !summary_complete(summary_out))
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: a summary needs all three arrays", who);
  }
  if (summary_out != nullptr && !(batch->flags & CARL_FLAG_AUTORESET))
    return fail(CARL_ERR_UNSUPPORTED, "%s: a summary needs CARL_FLAG_AUTORESET (without auto-reset a finished lane "
                "reports done on every later step, and its episode would be counted on each of them)", who);
  if (batch->n_lanes == 0 || n_steps == 0) return carl_host::policy_rollout_without_steps(who, batch, summary_out, stream);

  BraxShape shape;
  brax_policy_kern_t kern = nullptr;
  if (int e = carl_host::brax::policy_launch(kBraxPolicyKernels, batch, sys_host, c, n_steps, who, &shape, &kern)) return e;
  carl_step_io_t io_v{};
  if (io != nullptr) io_v = *io;
  carl::brax::BraxPolicy pol{*policy_host, brax_policy_floats(policy_host), carl_policy_summary_t{nullptr, nullptr, nullptr}, obs};
  if (summary_out != nullptr) pol.sum = *summary_out;
  carl::brax::Prepared prep{};
  carl::brax::build_topo_host(*sys_host, prep.topo);
  carl::brax::build_packed_host(*sys_host, prep.topo, prep.packed);
  hipLaunchKernelGGL(kern, dim3(shape.grid), dim3(carl::brax::kLanes * shape.W), shape.lds_bytes, (hipStream_t)stream, *batch,
                     sys_dev, prep, io_v, pol, (int)n_steps);
  return check_launch(who);
}

}  // extern "C"
