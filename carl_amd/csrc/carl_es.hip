// carl_es.hip -- C-ABI entry points of evolution strategies on the device (include/carl_amd.h: carl_es_perturb,
// carl_es_gradient) and their launches.  A translation unit of its own, so that every other unit's kernels compile
// exactly as they did; the kernels are es_kernels.hip.h's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/carl_amd.h"
#include "es_kernels.hip.h"
#include "host_common.hpp"

namespace {

using carl_host::check_launch;
using carl_host::fail;

// the struct's own rules, shared by both calls
int check_es(const char* who, const carl_es_t* es) {
  if (es == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: es is NULL", who);
  if (es->n_pairs < 1) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_pairs %d < 1", who, es->n_pairs);
  if (es->set_floats <= 0 || es->set_floats % 4 != 0)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: set_floats %d is not a positive multiple of 4 (carl_policy_set_floats)", who,
                es->set_floats);
  if (es->n_noisy < 1 || es->n_noisy > es->set_floats)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_noisy %d outside [1, set_floats = %d]", who, es->n_noisy, es->set_floats);
  if (!std::isfinite(es->sigma) || !(es->sigma > 0.0f))
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: sigma %g is not finite and positive", who, (double)es->sigma);
  if (2 * (int64_t)es->n_pairs * (int64_t)es->set_floats >= (int64_t)1 << 31)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: 2 x %d pairs x %d floats: more than 2^31 - 1 parameters", who, es->n_pairs,
                es->set_floats);
  return 0;
}

}  // namespace

extern "C" {

int32_t carl_es_slice_pairs(void) { return carl::kEsSlicePairs; }

int carl_es_perturb(const carl_es_t* es_host, const float* center, float* params, float* noise, void* stream) {
  const char* who = "carl_es_perturb";
  if (int e = check_es(who, es_host)) return e;
  if (center == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: center is NULL", who);
  if (params == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: params is NULL", who);
  if ((reinterpret_cast<uintptr_t>(params) & 15) != 0)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: params is not on a 16-byte boundary", who);
  const int threads = es_host->n_pairs * (es_host->set_floats / 2);  // (< 2^29 by check_es)
  const int grid = (threads + carl::kEsThreads - 1) / carl::kEsThreads;
  hipLaunchKernelGGL(carl::es_perturb_kernel, dim3(grid), dim3(carl::kEsThreads), 0, (hipStream_t)stream, *es_host, center,
                     params, noise);
  return check_launch(who);
}

int carl_es_gradient(const carl_es_t* es_host, const float* weight, float* grad, void* stream) {
  const char* who = "carl_es_gradient";
  if (int e = check_es(who, es_host)) return e;
  if (weight == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: weight is NULL", who);
  if (grad == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: grad is NULL", who);
  const int blocks = (es_host->n_noisy + 1) / 2;
  const int grid = (blocks + carl::kEsGradBlocks - 1) / carl::kEsGradBlocks;
  hipLaunchKernelGGL(carl::es_gradient_kernel, dim3(grid), dim3(carl::kEsThreads), 0, (hipStream_t)stream, *es_host, weight,
                     grad);
  return check_launch(who);
}

}  // extern "C"
