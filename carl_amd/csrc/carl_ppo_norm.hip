// carl_ppo_norm.hip -- C-ABI entry points of PPO's running normalisation (include/carl_amd.h: carl_ppo_input_stats,
// carl_brax_ppo_input_stats, carl_ppo_return_stats, carl_ppo_return_merge) and their launches.  A translation unit of its
// own, so that every other unit's kernels compile exactly as they did.  The kernels are ppo_norm_kernels.hip.h's; the
// packed shapes and the statistics output's check are policy_host.hpp's.  The input sums go to the slabs the two existing
// merges read (carl_policy_stats_merge, carl_brax_policy_stats_merge): no merge for inputs is written here.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/carl_amd.h"
#include "classic_control.hip.h"
#include "host_common.hpp"
#include "policy_host.hpp"
#include "ppo_norm_kernels.hip.h"

namespace {

using carl_host::check_launch;
using carl_host::fail;

bool classic_family(int32_t family) { return family >= 0 && family < CARL_N_FAMILIES; }

int input_slabs(int64_t n_lanes, int64_t n_steps) {
  if (n_lanes < 1 || n_steps < 1) return 0;
  const int64_t tiles = (n_lanes * n_steps + carl::kPpoThreads - 1) / carl::kPpoThreads;
  return (int)(tiles < carl::kPpoMaxWorkgroups ? tiles : carl::kPpoMaxWorkgroups);
}

int return_slabs(int64_t n_lanes) {
  return n_lanes < 1 ? 0 : (int)((n_lanes + carl::kReturnThreads - 1) / carl::kReturnThreads);
}

// What both input-sums entry points check after their family rule, and the launch.  set_floats: the floats of a packed
// weight set by the caller's packing rule (< 0: the shape is outside its limits); n_features: the rows of the family's
// context table, or -1 where the buffer does not say (a Brax model: the sign of a row alone is checked).
int input_stats(const char* who, const carl_ppo_batch_t* ppo, const carl_policy_t* p, int set_floats, int n_features,
                const carl_policy_stats_t* stats, void* stream) {
  if (set_floats < 0) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: the policy's shape is outside the limits", who);
  if (p->params == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: params is NULL", who);
  if (p->n_ctx < 0 || p->n_ctx > p->n_in)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_ctx %d outside [0, n_in = %d]", who, p->n_ctx, p->n_in);
  for (int k = 0; k < p->n_ctx; ++k)
    if (p->ctx_rows[k] < 0 || (n_features >= 0 && p->ctx_rows[k] >= n_features))
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: ctx_rows[%d] = %d is not a context-table row", who, k, p->ctx_rows[k]);
  if (ppo->obs_dim < 1 || p->n_in != p->n_ctx + ppo->obs_dim)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_in %d != n_ctx %d + obs_dim %d", who, p->n_in, p->n_ctx, ppo->obs_dim);
  if (ppo->idx != nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: idx must be NULL (the sums run over every sample of the buffer)", who);
  if (ppo->n_steps < 1 || ppo->n_lanes < 0)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_steps %d < 1 or n_lanes %d < 0", who, ppo->n_steps, ppo->n_lanes);
  if (ppo->row_pitch != 0 && ppo->row_pitch < ppo->n_lanes)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: row_pitch %d < n_lanes %d", who, ppo->row_pitch, ppo->n_lanes);
  const int pitch = ppo->row_pitch > 0 ? ppo->row_pitch : ppo->n_lanes;
  if ((int64_t)ppo->n_steps * pitch >= ((int64_t)1 << 31))
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: %d steps x %d lanes per row: flat indices do not fit 2^31 - 1", who,
                ppo->n_steps, pitch);
  if (ppo->n_contexts < 1 || ppo->ctx_stride < ppo->n_contexts)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_contexts %d / ctx_stride %d invalid", who, ppo->n_contexts,
                ppo->ctx_stride);
  if (!ppo->obs0 || !ppo->obs || !ppo->context_id || !ppo->ctx_table)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: obs0, obs, context_id and ctx_table are required", who);
  const int slabs = input_slabs(ppo->n_lanes, ppo->n_steps);
  if (int e = carl_host::check_policy_stats(who, stats, slabs, "slabs (carl_ppo_input_stats_slabs)")) return e;
  if (ppo->n_lanes == 0) return 0;

  carl::PpoInputStatsArgs a{};
  a.b = *ppo;
  a.b.row_pitch = pitch;
  a.n_in = p->n_in, a.n_ctx = p->n_ctx;
  for (int k = 0; k < p->n_ctx; ++k) a.ctx_rows[k] = p->ctx_rows[k];
  a.shift = p->params + carl_host::policy_transform_offset(p);
  a.partial = stats->partial;
  a.n_samples = (long long)ppo->n_steps * ppo->n_lanes;
  hipLaunchKernelGGL(carl::ppo_input_stats_kernel, dim3(slabs), dim3(carl::kPpoThreads), 0, (hipStream_t)stream, a);
  return check_launch(who);
}

}  // namespace

extern "C" {

int32_t carl_ppo_input_stats_slabs(int32_t n_lanes, int32_t n_steps) { return input_slabs(n_lanes, n_steps); }

int carl_ppo_input_stats(const carl_ppo_batch_t* ppo, const carl_policy_t* policy_host, const carl_policy_stats_t* stats,
                         void* stream) {
  const char* who = "carl_ppo_input_stats";
  if (ppo == nullptr || policy_host == nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: ppo / policy is NULL", who);
  if (ppo->family >= CARL_N_FAMILIES)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: family %d is a Brax family -- its sums are carl_brax_ppo_input_stats", who,
                ppo->family);
  carl_family_info_t fi;
  if (int e = carl_family_info(ppo->family, &fi)) return e;
  if (ppo->obs_dim != fi.obs_dim)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: obs_dim %d, the family's is %d", who, ppo->obs_dim, fi.obs_dim);
  return input_stats(who, ppo, policy_host, carl_host::policy_set_floats(policy_host), fi.n_features, stats, stream);
}

int carl_brax_ppo_input_stats(const carl_ppo_batch_t* ppo, const carl_policy_t* policy_host,
                              const carl_policy_stats_t* stats, void* stream) {
  const char* who = "carl_brax_ppo_input_stats";
  if (ppo == nullptr || policy_host == nullptr)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: ppo / policy is NULL", who);
  if (classic_family(ppo->family))
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: family %d is a classic-control family -- its sums are carl_ppo_input_stats",
                who, ppo->family);
  if (ppo->row_pitch != 0 && ppo->row_pitch != ppo->n_lanes)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: row_pitch %d: Brax families take dense rows (0 or n_lanes = %d)", who,
                ppo->row_pitch, ppo->n_lanes);
  return input_stats(who, ppo, policy_host, carl_brax_policy_set_floats(policy_host), -1, stats, stream);
}

int32_t carl_ppo_return_stats_slabs(int32_t n_lanes) { return return_slabs(n_lanes); }

int carl_ppo_return_stats(const carl_ppo_return_stats_t* rs, void* stream) {
  const char* who = "carl_ppo_return_stats";
  if (rs == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: the argument struct is NULL", who);
  if (rs->n_steps < 1 || rs->n_lanes < 0)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_steps %d < 1 or n_lanes %d < 0", who, rs->n_steps, rs->n_lanes);
  if (rs->row_pitch != 0 && rs->row_pitch < rs->n_lanes)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: row_pitch %d < n_lanes %d", who, rs->row_pitch, rs->n_lanes);
  if (!std::isfinite(rs->gamma) || rs->gamma < 0.0f)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: gamma %g is not finite and >= 0", who, (double)rs->gamma);
  if (!rs->reward || !rs->terminated || !rs->truncated || !rs->ret)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: reward, terminated, truncated and ret are required", who);
  const int slabs = return_slabs(rs->n_lanes);
  if (rs->partial == nullptr || (reinterpret_cast<uintptr_t>(rs->partial) & 15) != 0)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: partial is NULL or not on a 16-byte boundary", who);
  if (rs->partial_capacity < slabs)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: partial_capacity %d < %d slabs (carl_ppo_return_stats_slabs)", who,
                rs->partial_capacity, slabs);
  if (rs->n_lanes == 0) return 0;
  carl::PpoReturnStatsArgs a{};
  a.n_lanes = rs->n_lanes, a.n_steps = rs->n_steps, a.pitch = rs->row_pitch > 0 ? rs->row_pitch : rs->n_lanes;
  a.gamma = rs->gamma;
  a.reward = rs->reward, a.terminated = rs->terminated, a.truncated = rs->truncated;
  a.ret = rs->ret, a.ret_rows = rs->ret_rows, a.partial = rs->partial;
  hipLaunchKernelGGL(carl::ppo_return_stats_kernel, dim3(slabs), dim3(carl::kReturnThreads), 0, (hipStream_t)stream, a);
  return check_launch(who);
}

int carl_ppo_return_merge(const double* partial, int32_t n_slabs, int64_t n_b, const carl_policy_running_stats_t* running,
                          double eps, float* scale, void* stream) {
  const char* who = "carl_ppo_return_merge";
  if (partial == nullptr || (reinterpret_cast<uintptr_t>(partial) & 15) != 0)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: partial is NULL or not on a 16-byte boundary", who);
  if (n_slabs < 0) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_slabs %d < 0", who, n_slabs);
  if (n_b < 0) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_b %lld < 0", who, (long long)n_b);
  if (running == nullptr || !running->count || !running->mean || !running->m2)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: running and its three arrays are required", who);
  if (!std::isfinite(eps) || eps < 0.0) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: eps %g is not finite and >= 0", who, eps);
  if (scale == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: scale is NULL", who);
  if (n_b == 0) return 0;
  hipLaunchKernelGGL(carl::ppo_return_merge_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, partial, (int)n_slabs,
                     (long long)n_b, running->count, running->mean, running->m2, eps, scale);
  return check_launch(who);
}

}  // extern "C"
