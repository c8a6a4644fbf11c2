// carl_policy.hip -- C-ABI entry points of the closed-loop rollout (include/carl_amd.h: carl_rollout_policy) and their
// kernel dispatch.  A translation unit of its own: the kernels (policy_kernels.hip.h) instantiate the engine's device
// templates anew, and the open-loop kernels of carl_amd.hip compile exactly as they did without them.  The host rules
// of policy_host.hpp live here too; the other units of the closed-loop rollout call them.  The launch itself is
// policy_launch.hpp's.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/carl_amd.h"
#include "classic_control.hip.h"
#include "host_common.hpp"
#include "policy_host.hpp"
#include "policy_kernels.hip.h"
#include "policy_launch.hpp"

namespace carl_host {

int policy_set_floats(const carl_policy_t* p) {
  if (p->n_in < 1 || p->n_in > CARL_POLICY_MAX_IN || p->n_out < 1 || p->n_out > 4 || p->n_hidden < 0 ||
      p->n_hidden > CARL_POLICY_MAX_HIDDEN)
    return -1;
  for (int l = 0; l < p->n_hidden; ++l)
    if (p->width[l] < 1 || p->width[l] > CARL_POLICY_MAX_WIDTH) return -1;
  const int64_t total = (int64_t)policy_transform_offset(p) + 2 * (int64_t)p->n_in + 1;
  return (int)((total + 3) / 4 * 4);
}

int policy_transform_offset(const carl_policy_t* p) {
  int total = 0, prev = p->n_in;  // (<= 32 x 64 + 64 x 64 + 4 x 64 + biases: far from 2^31)
  for (int l = 0; l <= p->n_hidden; ++l) {
    const int w = l < p->n_hidden ? p->width[l] : p->n_out;
    total += w * prev + w;
    prev = w;
  }
  return total;
}

int policy_padded_hidden(const carl_policy_t* p) {
  int wmax = 0;
  for (int l = 0; l < p->n_hidden; ++l) wmax = wmax > p->width[l] ? wmax : p->width[l];
  return p->n_hidden == 0 ? 0 : wmax <= 32 ? 32 : 64;
}

int check_hidden_layers(const char* who, const carl_policy_t* p) {
  if (p->n_hidden < 0 || p->n_hidden > CARL_POLICY_MAX_HIDDEN)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_hidden %d outside [0, %d]", who, p->n_hidden, CARL_POLICY_MAX_HIDDEN);
  for (int l = 0; l < p->n_hidden; ++l)
    if (p->width[l] < 1 || p->width[l] > CARL_POLICY_MAX_WIDTH)
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: hidden width[%d] = %d outside [1, %d]", who, l, p->width[l],
                  CARL_POLICY_MAX_WIDTH);
  return 0;
}

int check_activation(const char* who, const carl_policy_t* p) {
  if (p->activation < CARL_POLICY_IDENTITY || p->activation > CARL_POLICY_RELU)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: unknown activation %d", who, p->activation);
  return 0;
}

int check_params(const char* who, const carl_policy_t* p) {
  if (p->params == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: params is NULL", who);
  return 0;
}

namespace {

int validate_policy(const carl_batch_t* b, const carl_policy_t* p, const carl_family_info_t& fi, const char* who) {
  if (int e = check_hidden_layers(who, p)) return e;
  if (p->n_ctx < 0 || p->n_ctx > fi.n_features)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_ctx %d outside [0, F = %d]", who, p->n_ctx, fi.n_features);
  for (int k = 0; k < p->n_ctx; ++k)
    if (p->ctx_rows[k] < 0 || p->ctx_rows[k] >= fi.n_features)
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: ctx_rows[%d] = %d is not a context-table row (F = %d)", who, k,
                  p->ctx_rows[k], fi.n_features);
  if (p->n_in != p->n_ctx + fi.obs_dim)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_in %d != n_ctx %d + obs_dim %d", who, p->n_in, p->n_ctx, fi.obs_dim);
  const int want_out = fi.action_is_discrete ? fi.n_actions : 1;
  if (p->n_out != want_out)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: head width %d, the family needs %d (%s)", who, p->n_out, want_out,
                fi.action_is_discrete ? "n_actions" : "one Box value");
  if (p->head != (fi.action_is_discrete ? CARL_POLICY_HEAD_ARGMAX : CARL_POLICY_HEAD_BOX))
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: head kind %d does not match the family's action space", who, p->head);
  if (int e = check_activation(who, p)) return e;
  if (p->n_sets < 1) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_sets %d < 1", who, p->n_sets);
  if (p->lanes_per_set < carl::kPolicyLanes || p->lanes_per_set % carl::kPolicyLanes != 0)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: lanes_per_set %d is not a positive multiple of %d (carl_policy_lane_quantum)",
                who, p->lanes_per_set, carl::kPolicyLanes);
  if ((int64_t)p->n_sets * p->lanes_per_set < b->n_lanes)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: %d sets x %d lanes do not cover %d lanes", who, p->n_sets,
                p->lanes_per_set, b->n_lanes);
  return check_params(who, p);
}

// transitions mode: the staged layout of carl_rollout (see include/carl_amd.h: carl_step_io_t::row_pitch)
int validate_io(const carl_batch_t* b, const carl_step_io_t* io, const carl_family_info_t& fi, const char* who) {
  if (!io->action || !io->obs || !io->reward || !io->terminated || !io->truncated)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: a required io pointer is NULL", who);
  const int want = fi.action_is_discrete ? CARL_ACTION_I32 : CARL_ACTION_F32;
  if (io->action_dtype != want)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: the action column is %s for this family", who,
                fi.action_is_discrete ? "int32 (CARL_ACTION_I32)" : "float32 (CARL_ACTION_F32)");
  if (io->row_pitch != 0 && io->row_pitch < b->n_lanes)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: io.row_pitch %d < n_lanes %d", who, io->row_pitch, b->n_lanes);
  if (!carl_host::staged_rows(b, io, 15))
    return fail(CARL_ERR_UNSUPPORTED, "%s: rows of %d lanes for %d lanes: the closed-loop rollout writes the staged layout "
                "only (pitch %% 16 == 0 and n_lanes %% 16 == 0 or pitch == carl_rollout_pitch(n_lanes), arrays on 16-byte "
                "boundaries)", who, io->row_pitch > 0 ? io->row_pitch : b->n_lanes, b->n_lanes);
  return 0;
}

// what every closed-loop entry point checks first; `fi`: the batch family's info
int check_batch_and_policy(const char* who, const carl_batch_t* batch, const carl_policy_t* policy_host,
                           carl_family_info_t* fi) {
  if (batch == nullptr || policy_host == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: batch / policy is NULL", who);
  if (batch->family >= CARL_N_FAMILIES)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: family %d is a Brax family -- the closed-loop rollout covers the "
                "classic-control families only", who, batch->family);
  if (int e = validate_batch(batch, who)) return e;
  if (int e = carl_family_info(batch->family, fi)) return e;
  return validate_policy(batch, policy_host, *fi, who);
}

}  // namespace

int check_rollout_policy(const char* who, const carl_batch_t* batch, const carl_policy_t* policy_host,
                         const carl_step_io_t* io, int32_t n_steps, const carl_policy_summary_t* summary_out,
                         carl_family_info_t* fi) {
  if (int e = check_batch_and_policy(who, batch, policy_host, fi)) return e;
  if (n_steps < 0) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_steps %d < 0", who, n_steps);
  if (io == nullptr) {
    if (summary_out == nullptr || !summary_out->episodes || !summary_out->return_sum || !summary_out->length_sum)
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: summary mode (io NULL) needs all three summary arrays", who);
  } else {
    if (int e = validate_io(batch, io, *fi, who)) return e;
    if (summary_out != nullptr && (!summary_out->episodes || !summary_out->return_sum || !summary_out->length_sum))
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: a summary needs all three arrays", who);
  }
  // Without auto-reset a finished lane stays done and reports done again on every later step (its return and length
  // still growing): the per-lane totals would count one episode many times.  A summary needs CARL_FLAG_AUTORESET.
  if (summary_out != nullptr && !(batch->flags & CARL_FLAG_AUTORESET))
    return fail(CARL_ERR_UNSUPPORTED, "%s: a summary needs CARL_FLAG_AUTORESET (without auto-reset a finished lane "
                "reports done on every later step, and its episode would be counted on each of them)", who);
  return 0;
}

int policy_rollout_without_steps(const char* who, const carl_batch_t* batch, const carl_policy_summary_t* summary_out,
                                 void* stream) {
  if (summary_out == nullptr || batch->n_lanes == 0) return 0;
  // no step: every total is zero
  hipStream_t s = (hipStream_t)stream;
  const size_t bytes = (size_t)batch->n_lanes * 4;
  for (void* p : {(void*)summary_out->episodes, (void*)summary_out->return_sum, (void*)summary_out->length_sum})
    if (const hipError_t e = hipMemsetAsync(p, 0, bytes, s); e != hipSuccess)
      return fail((int)e, "%s: hipMemsetAsync: %s", who, hipGetErrorString(e));
  return 0;
}

int check_evaluate_policy(const char* who, const carl_batch_t* batch, const carl_policy_t* policy_host,
                          int32_t n_episodes, int32_t max_steps, const carl_policy_episodes_t* out,
                          carl_family_info_t* fi) {
  if (int e = check_batch_and_policy(who, batch, policy_host, fi)) return e;
  if (out == nullptr || !out->episodes || !out->steps || !out->ret || !out->length || !out->context_id ||
      !out->terminated)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: out and all six of its arrays are required", who);
  if (n_episodes < 1) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_episodes %d < 1", who, n_episodes);
  if (max_steps < 0) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: max_steps %d < 0", who, max_steps);
  if ((int64_t)n_episodes * batch->n_lanes >= ((int64_t)1 << 31))
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_episodes %d x %d lanes records do not fit 2^31 - 1", who, n_episodes,
                batch->n_lanes);
  // as a summary: without auto-reset a finished lane reports done on every later step
  if (!(batch->flags & CARL_FLAG_AUTORESET))
    return fail(CARL_ERR_UNSUPPORTED, "%s: needs CARL_FLAG_AUTORESET (without auto-reset a finished lane reports done on "
                "every later step, and its episode would be counted on each of them)", who);
  return 0;
}

}  // namespace carl_host

namespace {

using carl_host::launch_policy_kernel;
using carl_host::PolicyKernel;
using carl_host::with_padded_hidden;

template <class Fam>
int launch_policy(const carl_batch_t* b, const carl_policy_t* p, const carl_step_io_t* io, int n_steps,
                  const carl_policy_summary_t* sum, hipStream_t s) {
  const bool summary = io == nullptr;
  static_assert(carl::policy_lds_bytes<Fam, 64, false>() + carl::static_lds_bytes<Fam>() <= carl::kCuLdsBytes,
                "the closed-loop rollout's LDS does not fit a compute unit");
  const auto k = with_padded_hidden(carl_host::policy_padded_hidden(p), [&](auto h) {
    constexpr int H = decltype(h)::value;
    if (summary) return PolicyKernel{carl::policy_rollout_kernel<Fam, H, true>, carl::policy_lds_bytes<Fam, H, true>()};
    return PolicyKernel{carl::policy_rollout_kernel<Fam, H, false>, carl::policy_lds_bytes<Fam, H, false>()};
  });
  const int threads = summary ? carl::kPolicyThreadsSummary : carl::kPolicyThreadsTransitions;
  return launch_policy_kernel("carl_rollout_policy", k, b->n_lanes, threads, s, *b, carl_host::launch_io(b, io), *p,
                              carl_host::policy_set_floats(p), carl_host::launch_summary(sum), n_steps);
}

template <class Fam>
int launch_episodes(const carl_batch_t* b, const carl_policy_t* p, int n_episodes, int max_steps,
                    const carl_policy_episodes_t* out, hipStream_t s) {
  // summary mode's LDS: the weight set alone
  const auto k = with_padded_hidden(carl_host::policy_padded_hidden(p), [](auto h) {
    constexpr int H = decltype(h)::value;
    return PolicyKernel{carl::policy_episodes_kernel<Fam, H>, carl::policy_lds_bytes<Fam, H, true>()};
  });
  return launch_policy_kernel("carl_evaluate_policy", k, b->n_lanes, carl::kPolicyThreadsSummary, s, *b, *p,
                              carl_host::policy_set_floats(p), *out, n_episodes, max_steps);
}

}  // namespace

extern "C" {

int32_t carl_policy_lane_quantum(void) { return carl::kPolicyLanes; }

int32_t carl_policy_set_floats(const carl_policy_t* policy_host) {
  if (policy_host == nullptr) return -1;
  return carl_host::policy_set_floats(policy_host);
}

int carl_rollout_policy(const carl_batch_t* batch, const carl_policy_t* policy_host, const carl_step_io_t* io,
                        int32_t n_steps, const carl_policy_summary_t* summary_out, void* stream) {
  const char* who = "carl_rollout_policy";
  carl_family_info_t fi;
  if (int e = carl_host::check_rollout_policy(who, batch, policy_host, io, n_steps, summary_out, &fi)) return e;
  if (batch->n_lanes == 0 || n_steps == 0) return carl_host::policy_rollout_without_steps(who, batch, summary_out, stream);
  return carl_host::with_classic_family(batch, [&](auto fam) {
    return launch_policy<decltype(fam)>(batch, policy_host, io, n_steps, summary_out, (hipStream_t)stream);
  });
}

int carl_evaluate_policy(const carl_batch_t* batch, const carl_policy_t* policy_host, int32_t n_episodes,
                         int32_t max_steps, const carl_policy_episodes_t* out, void* stream) {
  carl_family_info_t fi;
  if (int e = carl_host::check_evaluate_policy("carl_evaluate_policy", batch, policy_host, n_episodes, max_steps, out, &fi))
    return e;
  if (batch->n_lanes == 0) return 0;
  return carl_host::with_classic_family(batch, [&](auto fam) {
    return launch_episodes<decltype(fam)>(batch, policy_host, n_episodes, max_steps, out, (hipStream_t)stream);
  });
}

}  // extern "C"
