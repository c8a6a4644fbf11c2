// carl_brax_policy.hip -- C-ABI entry points of the closed-loop rollout of the Brax families (include/carl_amd.h:
// carl_brax_rollout_policy) and their kernel dispatch.  A translation unit of its own: the kernels are MODE 2 of
// brax_kernels.hip.h's run(), instantiated here and nowhere else, so that the reset / step / rollout kernels of
// carl_brax.hip compile exactly as they did without them (profiles/brax_policy_isa_identity.txt).  The batch, model and io
// checks and the launch-shape rule are carl_brax.hip's (brax_launch.hpp); the network's shape rules are the classic
// closed-loop rollout's (policy_host.hpp).  Same flags as carl_brax.hip (carl_amd/build.py).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/carl_amd.h"
#include "brax_launch.hpp"
#include "brax_policy_kernels.hip.h"
#include "host_common.hpp"
#include "policy_host.hpp"

namespace {

using carl_host::check_launch;
using carl_host::fail;
using carl_host::brax::BraxClass;
using carl_host::brax::BraxShape;
using carl_host::brax::same_class;

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

int brax_policy_floats(const carl_policy_t* p) {
  if (p->n_in < 1 || p->n_in > CARL_POLICY_MAX_IN || p->n_out < 1 || p->n_out > CARL_BRAX_MAX_ACT || p->n_hidden < 0 ||
      p->n_hidden > CARL_POLICY_MAX_HIDDEN)
    return -1;
  for (int l = 0; l < p->n_hidden; ++l)
    if (p->width[l] < 1 || p->width[l] > CARL_POLICY_MAX_WIDTH) return -1;
  const int64_t total = (int64_t)carl_host::policy_transform_offset(p) + 2 * (int64_t)p->n_in + 1;
  return (int)((total + 3) / 4 * 4);
}

// the class of a closed-loop launch, or the refusal of CARL_FLAG_BRAX_FP32
int policy_class(const char* who, const carl_batch_t* b, const carl_brax_sys_t* sh, BraxClass* c) {
  if (b->flags & CARL_FLAG_BRAX_FP32)
    return fail(CARL_ERR_UNSUPPORTED, "%s: CARL_FLAG_BRAX_FP32 is not built for the closed-loop rollout (the float64 "
                "kernel classes only)", who);
  *c = carl_host::brax::brax_class(sh, b->flags, true);
  return 0;
}

int validate_policy(const char* who, const carl_batch_t* b, const carl_brax_sys_t* sh, const carl_policy_t* p) {
  if (int e = carl_host::check_hidden_layers(who, p)) return e;
  if (p->n_ctx < 0 || p->n_ctx > CARL_POLICY_MAX_IN)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_ctx %d outside [0, %d]", who, p->n_ctx, CARL_POLICY_MAX_IN);
  if (p->n_ctx + sh->obs_dim > CARL_POLICY_MAX_IN)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: %d context inputs + %d observations are more than CARL_POLICY_MAX_IN = %d "
                "policy inputs (Humanoid-size observations are out of scope)", who, p->n_ctx, sh->obs_dim, CARL_POLICY_MAX_IN);
  // a Brax batch does not say how many rows its context table has: a policy sees the rows the batch makes visible
  for (int k = 0; k < p->n_ctx; ++k) {
    bool visible = false;
    for (int j = 0; j < b->n_ctx_obs && j < CARL_MAX_CTX_OBS; ++j) visible |= b->ctx_obs_feat[j] == p->ctx_rows[k];
    if (p->ctx_rows[k] < 0 || !visible)
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: ctx_rows[%d] = %d is not one of the batch's observed context rows "
                  "(ctx_obs_feat)", who, k, p->ctx_rows[k]);
  }
  if (p->n_in != p->n_ctx + sh->obs_dim)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_in %d != n_ctx %d + obs_dim %d", who, p->n_in, p->n_ctx, sh->obs_dim);
  if (p->n_out != sh->n_act)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: head width %d, the model has %d actuators", who, p->n_out, sh->n_act);
  if (p->head != CARL_POLICY_HEAD_BOX)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: head kind %d: the Brax families take Box actions (CARL_POLICY_HEAD_BOX)", who,
                p->head);
  if (int e = carl_host::check_activation(who, p)) return e;
  if (p->n_sets < 1) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_sets %d < 1", who, p->n_sets);
  const int q = carl_policy_lane_quantum();
  if (p->lanes_per_set < q || p->lanes_per_set % q != 0)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: lanes_per_set %d is not a positive multiple of %d (carl_policy_lane_quantum)",
                who, p->lanes_per_set, q);
  if ((int64_t)p->n_sets * p->lanes_per_set < b->n_lanes)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: %d sets x %d lanes do not cover %d lanes", who, p->n_sets, p->lanes_per_set,
                b->n_lanes);
  if (int e = carl_host::check_params(who, p)) return e;
  if (reinterpret_cast<uintptr_t>(p->params) % 16 != 0)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: params must start on a 16-byte boundary (weight rows are read 16 bytes at a time)",
                who);
  return 0;
}

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
  if (int e = carl_host::brax::brax_launch_shape(kBraxPolicyKernels, batch, sys_host, c, true, n_steps, true, who,
                                                 &shape))
    return e;
  *out = carl_brax_launch_shape_t{shape.grid, shape.W, shape.K, 0, (int64_t)shape.lds_bytes};
  return 0;
}

int carl_brax_rollout_policy(const carl_batch_t* batch, const carl_brax_sys_t* sys_dev, const carl_brax_sys_t* sys_host,
                             float* obs, const carl_policy_t* policy_host, const carl_step_io_t* io, int32_t n_steps,
                             const carl_policy_summary_t* summary_out, void* stream) {
  const char* who = "carl_brax_rollout_policy";
  if (int e = carl_host::brax::validate_brax(batch, sys_dev, sys_host, who)) return e;
  if (policy_host == nullptr || obs == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: policy / obs is NULL", who);
  BraxClass c;
  if (int e = policy_class(who, batch, sys_host, &c)) return e;
  if (int e = validate_policy(who, batch, sys_host, policy_host)) return e;
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
  if (int e = carl_host::brax::brax_launch_shape(kBraxPolicyKernels, batch, sys_host, c, true, n_steps, true, who,
                                                 &shape))
    return e;
  brax_policy_kern_t kern = nullptr;
  for (const BraxPolicyKernel& e : kBraxPolicyKernels)
    if (same_class(e.c, c) && e.k == shape.K) kern = e.kern;
  if (kern == nullptr) return fail(CARL_ERR_UNSUPPORTED, "%s: no kernel for %d lanes per env", who, shape.K);
  if (shape.lds_bytes > 48 * 1024) {
    if (int e = carl_host::ensure_dynamic_lds(reinterpret_cast<const void*>(kern), shape.lds_bytes, who)) return e;
  }
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
