// ppo_step_host.hpp -- the host checks of PPO's minibatch step, shared by its one-set entry points (carl_ppo_step.hip:
// carl_ppo_adv_stats, carl_adam_step) and a population's (carl_ppo_sets.hip: carl_ppo_adv_stats_sets, carl_adam_step_sets).
// Each check and its message is written once.  Host code; no kernel is named here.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/carl_amd.h"
#include "host_common.hpp"
#include "ppo_step_device.hip.h"

namespace carl_host {

inline int adv_rows(int64_t n_total, int64_t batch_size) {
  if (n_total < 1 || batch_size < 1) return 0;
  return (int)((n_total + batch_size - 1) / batch_size);
}

// every check of carl_ppo_adv_stats, in its order
inline int check_adv_stats(const char* who, const carl_ppo_adv_stats_t* as) {
  if (as == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: the argument struct is NULL", who);
  if (!as->advantage || !as->idx || !as->adv_norm)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: advantage, idx and adv_norm are required", who);
  if (as->n_total < 1 || as->batch_size < 1)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_total %d < 1 or batch_size %d < 1", who, as->n_total, as->batch_size);
  if (as->storage_floats < 1)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: storage_floats %lld < 1", who, (long long)as->storage_floats);
  if (!std::isfinite(as->eps) || as->eps < 0.0)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: eps %g is not finite and >= 0", who, as->eps);
  return 0;
}

inline carl::PpoAdvStatsArgs adv_stats_args(const carl_ppo_adv_stats_t* as) {
  carl::PpoAdvStatsArgs a{};
  a.advantage = as->advantage, a.storage_floats = (long long)as->storage_floats, a.idx = as->idx;
  a.n_total = as->n_total, a.batch_size = as->batch_size, a.eps = as->eps, a.adv_norm = as->adv_norm;
  return a;
}

// Every check of carl_adam_step, in its order; own_hyper: lr and max_grad_norm are the struct's (a population reads them
// from the device).  *total: the elements of one learner
inline int check_adam(const char* who, const carl_adam_t* ad, bool own_hyper, int64_t* total_out) {
  if (ad == nullptr) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: the argument struct is NULL", who);
  if (ad->n_tensors < 1 || ad->n_tensors > CARL_ADAM_MAX_TENSORS)
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n_tensors %d outside [1, %d]", who, ad->n_tensors, CARL_ADAM_MAX_TENSORS);
  int64_t total = 0;
  for (int t = 0; t < ad->n_tensors; ++t) {
    if (ad->n[t] < 0) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: n[%d] = %lld < 0", who, t, (long long)ad->n[t]);
    if (ad->n[t] > carl::kAdamMaxFloats - total)
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: more than %lld elements in all (carl_adam_step_max_floats)", who,
                  carl::kAdamMaxFloats);
    total += ad->n[t];
    if (!ad->param[t] || !ad->grad[t] || !ad->m[t] || !ad->v[t])
      return fail(CARL_ERR_INVALID_ARGUMENT, "%s: param, grad, m and v of tensor %d are required", who, t);
  }
  if (!ad->step || !ad->beta_pow) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: step and beta_pow are required", who);
  if (own_hyper && (!std::isfinite(ad->lr) || ad->lr < 0.0))
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: lr %g is not finite and >= 0", who, ad->lr);
  if (!std::isfinite(ad->eps) || ad->eps <= 0.0) return fail(CARL_ERR_INVALID_ARGUMENT, "%s: eps %g is not finite and > 0", who, ad->eps);
  if (!(ad->beta1 >= 0.0 && ad->beta1 < 1.0) || !(ad->beta2 >= 0.0 && ad->beta2 < 1.0))
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: beta1 %g / beta2 %g outside [0, 1)", who, ad->beta1, ad->beta2);
  if (own_hyper && !(ad->max_grad_norm >= 0.0))
    return fail(CARL_ERR_INVALID_ARGUMENT, "%s: max_grad_norm %g is negative or NaN (+inf: no clip)", who, ad->max_grad_norm);
  *total_out = total;
  return 0;
}

inline carl::AdamArgs adam_args(const carl_adam_t* ad) {
  carl::AdamArgs a{};
  a.n_tensors = ad->n_tensors;
  for (int t = 0; t < ad->n_tensors; ++t)
    a.n[t] = (long long)ad->n[t], a.param[t] = ad->param[t], a.grad[t] = ad->grad[t], a.m[t] = ad->m[t], a.v[t] = ad->v[t];
  a.lr = ad->lr, a.beta1 = ad->beta1, a.beta2 = ad->beta2, a.eps = ad->eps, a.max_grad_norm = ad->max_grad_norm;
  a.step = ad->step, a.beta_pow = ad->beta_pow, a.norm_out = ad->norm_out;
  return a;
}

}  // namespace carl_host
