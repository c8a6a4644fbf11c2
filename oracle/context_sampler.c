/* context_sampler.c -- TEST INFRASTRUCTURE (oracle), not product code.
 *
 * CPU restatement of the device context sampler / verifier (include/carl_amd.h:
 * carl_sample_contexts, carl_verify_contexts), i.e. of what replaces
 * ContextSampler.sample_contexts (carl/context/sampler.py:45-61) + the default fill
 * (carl/envs/carl_env.py:135-137) and ContextSpace.verify_context
 * (carl/context/context_space.py:54-59) for dense context sets.
 *
 * The device sampler is a NEW random stream (Philox keyed by seed / context id / feature), not
 * the reference's NumPy MT19937 one: the reference's recorded sampler outputs pin the HOST
 * sampler (carl_amd/context/sampler.py, tests/golden/notebook_sampler_outputs.json); what can be
 * pinned here is the distribution family per feature type (tests/test_device_sampler.py) and the
 * device kernel against this file.  Uniform / integer / categorical / constant draws are the
 * same float32 expressions as the kernel (bit-exact); the normal draw is evaluated in double
 * and rounded once (the kernel's float32 log/sqrt/sincos differ in the last bits).
 *
 * oracle_scan_u / oracle_normal_trace serve tests/context_kernel_cases.py: the first finds the context ids whose
 * first draw is an extreme of u01 (0, 1 - 2^-24), the second lays a bounded normal's 32 attempts open.
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../include/carl_amd.h"

void oracle_lane_words(uint64_t seed, uint64_t glane, uint32_t episode, uint32_t sub, uint32_t out[4]);
float oracle_u01(uint32_t w);

#define SUB_SAMPLER 0x40000000u
#define NORMAL_TRIES 32

static float sample_feature(const carl_feature_spec_t* sp, uint64_t seed, uint64_t gctx, uint32_t f) {
  if (sp->kind == CARL_FEAT_CONSTANT) return sp->value;
  uint32_t w[4];
  oracle_lane_words(seed, gctx, f, SUB_SAMPLER, w);
  const float u = oracle_u01(w[0]);
  if (sp->kind == CARL_FEAT_UNIFORM_FLOAT) {
    if (sp->log_scale) {
      const double lo = log((double)sp->lower), hi = log((double)sp->upper);
      float v = (float)exp(lo + (hi - lo) * (double)u);
      if (v < sp->lower) v = sp->lower; /* the kernel's clamp; never taken in double */
      if (v > sp->upper) v = sp->upper;
      return v;
    }
    return fmaf(sp->upper - sp->lower, u, sp->lower);
  }
  if (sp->kind == CARL_FEAT_UNIFORM_INT) {
    const float span = sp->upper - sp->lower + 1.0f;
    float k = floorf(u * span);
    if (k > span - 1.0f) k = span - 1.0f;
    return sp->lower + k;
  }
  if (sp->kind == CARL_FEAT_CATEGORICAL) {
    int k = (int)(u * (float)sp->n_choices);
    if (k > sp->n_choices - 1) k = sp->n_choices - 1;
    return sp->choices[k];
  }
  float v = 0.0f;
  for (int attempt = 0; attempt < NORMAL_TRIES; ++attempt) {
    if (attempt > 0) oracle_lane_words(seed, gctx, f, SUB_SAMPLER | (uint32_t)attempt, w);
    const double u1 = (double)oracle_u01(w[0]), u2 = (double)oracle_u01(w[1]);
    const double z = sqrt(-2.0 * log(1.0 - u1)) * cos(6.28318530717958647692 * u2);
    v = (float)((double)sp->mu + (double)sp->sigma * z);
    if (v >= sp->lower && v <= sp->upper) return v;
  }
  if (v < sp->lower) v = sp->lower;
  if (v > sp->upper) v = sp->upper;
  return v;
}

void oracle_sample_contexts(const carl_feature_spec_t* specs, int n_features, int n_contexts, int ctx_stride,
                            int64_t context_offset, uint64_t seed, float* ctx_table) {
  for (int f = 0; f < n_features; ++f)
    for (int c = 0; c < n_contexts; ++c)
      ctx_table[(size_t)f * ctx_stride + c] = sample_feature(&specs[f], seed, (uint64_t)(context_offset + c), (uint32_t)f);
}

int oracle_verify_contexts(const carl_feature_spec_t* specs, int n_features, int n_contexts, int ctx_stride,
                           const float* ctx_table) {
  int bad = 0;
  for (int f = 0; f < n_features; ++f)
    for (int c = 0; c < n_contexts; ++c) {
      const float v = ctx_table[(size_t)f * ctx_stride + c];
      int ok;
      if (specs[f].kind == CARL_FEAT_CATEGORICAL) {
        ok = 0;
        for (int k = 0; k < specs[f].n_choices; ++k) ok |= (v == specs[f].choices[k]);
      } else {
        ok = (v >= specs[f].lower) && (v <= specs[f].upper);
      }
      bad += !ok;
    }
  return bad;
}

/* Context ids in [start, start + count) whose first word of (seed, id, feature, attempt 0) gives u = 0 (ids_zero) and
 * u = 1 - 2^-24 (ids_top): up to `cap` of each, the numbers found in n_found[0..1].  best[0] is the id with the
 * largest u otherwise (a NORMAL_FLOAT's u1: the largest |z| its first attempt can reach), best[1] its 24-bit draw. */
void oracle_scan_u(uint64_t seed, uint32_t feature, uint64_t start, uint64_t count, int cap, uint64_t* ids_zero,
                   uint64_t* ids_top, int* n_found, uint64_t* best) {
  uint32_t w[4];
  n_found[0] = n_found[1] = 0;
  best[0] = start;
  best[1] = 0;
  for (uint64_t i = 0; i < count; ++i) {
    oracle_lane_words(seed, start + i, feature, SUB_SAMPLER, w);
    const uint32_t m = w[0] >> 8;
    if (m == 0u && n_found[0] < cap) ids_zero[n_found[0]++] = start + i;
    if (m == 0xFFFFFFu && n_found[1] < cap) ids_top[n_found[1]++] = start + i;
    if (m >= best[1]) { best[1] = m; best[0] = start + i; }
  }
}

/* The 32 attempts of a NORMAL_FLOAT feature for contexts context_offset .. + n_contexts - 1, in double: per attempt
 * the two uniforms, z = sqrt(-2 log(1 - u1)) cos(2 pi u2) and the candidate mu + sigma z BEFORE its rounding to
 * float32 ([n_contexts][32] each); accepted[c] is the attempt whose rounded candidate lies in [lower, upper], 32 when
 * every attempt failed (the result is then the last candidate, clipped). */
void oracle_normal_trace(const carl_feature_spec_t* sp, uint64_t seed, int64_t context_offset, int n_contexts,
                         uint32_t f, float* u1_out, float* u2_out, double* z_out, double* cand_out, int32_t* accepted) {
  for (int c = 0; c < n_contexts; ++c) {
    accepted[c] = NORMAL_TRIES;
    for (int attempt = 0; attempt < NORMAL_TRIES; ++attempt) {
      uint32_t w[4];
      oracle_lane_words(seed, (uint64_t)(context_offset + c), f, SUB_SAMPLER | (uint32_t)attempt, w);
      const float u1 = oracle_u01(w[0]), u2 = oracle_u01(w[1]);
      const double z = sqrt(-2.0 * log(1.0 - (double)u1)) * cos(6.28318530717958647692 * (double)u2);
      const double cand = (double)sp->mu + (double)sp->sigma * z;
      const size_t k = (size_t)c * NORMAL_TRIES + attempt;
      u1_out[k] = u1; u2_out[k] = u2; z_out[k] = z; cand_out[k] = cand;
      const float v = (float)cand;
      if (accepted[c] == NORMAL_TRIES && v >= sp->lower && v <= sp->upper) accepted[c] = attempt;
    }
  }
}
