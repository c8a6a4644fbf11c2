// policy_stats_kernels.hip.h -- input statistics inside the episodes launch (include/carl_amd.h:
// carl_evaluate_policy_stats, carl_policy_stats_merge).
//
// policy_episodes_stats_kernel is the episodes-mode body (policy_episodes_body.inc, the one policy_episodes_kernel and
// policy_episodes_sampled_kernel include) with `InputStats` in the place of their `NoInputStats`: for every live
// lane-step and every policy input it gathers d = fp32(x_raw - shift) -- normalize_input's first operation, before the
// scale and the clip -- and d * d.  The step, the records and the engine state are those of the kernels without it.
//
//   per lane, fp32, registers   s1[D], s2[D] for the observation entries: s1 += d, s2 = fma(d, d, s2) at every live
//                               step; they span at most one chunk (policy_chunk<Fam>() <= 8 steps).  A context input's
//                               d does not change while the lane stays in its context, so the step only counts
//                               (cnt += 1): no per-step arithmetic for the context inputs.
//   per wave, float64, LDS      at the end of every chunk -- also the one a wave leaves early -- each observation
//                               entry's two partials are widened to float64 and summed across the wavefront by a
//                               butterfly of __shfl_xor (a fixed tree of lane pairs: the same bits in every lane,
//                               whatever the schedule), and lane 0 adds them into the wave's own [2][K] float64 region
//                               behind the weight set (slot order: context input k at k, observation entry d at F + d).
//                               The context inputs go the same way as cnt * d and cnt * d * d formed in float64 -- both
//                               exact: 3 + 24 and 3 + 48 bits -- there and whenever a lane of the wave changes its
//                               context (flush_context, under the wave-uniform branch that re-reads the context row
//                               anyway; the old context's value is read again from the table).  So a constant input's
//                               sums carry float64 rounding only, which is what lets carl_policy_stats_merge tell it
//                               from one that varies.  Only lane 0 of a wave ever touches its region inside the step
//                               loop: no barrier, and the wave-uniform early exit of the loop stays as it is.
//   per workgroup, float64      after the loop, one barrier; then 64 threads add the four regions in wave order and
//                               write the workgroup's slab partial[blockIdx.x][2][CARL_POLICY_MAX_IN] in input order,
//                               zeros at and beyond n_in.
// No floating-point atomics anywhere: the slab is a fixed function of the launch's inputs.
//
// Registers: 2 D + 1 more per lane (D <= 6) and the flush's temporaries; the H = 64 instances keep their 256 VGPRs and
// take the rest as AGPR copies, none uses scratch (profiles/policy_stats_kernel_resources.txt).  LDS: 4 x 2 K x 8 bytes
// <= 1 280 bytes.
#pragma once

#include <type_traits>

#include "policy_kernels.hip.h"

namespace carl {

// sum over the wavefront, the same bits in every lane: lane l adds lane l ^ m for m = 1, 2, .. 32
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) v += __shfl_xor(v, m, kWave);
  return v;
}

template <class Fam, int H>
__host__ __device__ constexpr size_t policy_stats_lds_bytes() {
  return (size_t)(kPolicyLanes / kWave) * 2 * PolicyLayout<Fam, H>::K * sizeof(double);
}

template <class Fam, int H>
struct InputStats {
  using L = PolicyLayout<Fam, H>;
  static constexpr bool kOn = true;
  double* partial;  // [n_workgroups][2][CARL_POLICY_MAX_IN]
  double* region;   // the wave's [2][K] float64 sums in LDS
  float s1[Fam::D], s2[Fam::D];  // the observation entries' fp32 partials of the running chunk
  int cnt;                       // live steps since the context inputs were last flushed

  // after the weights are staged; `after_weights`: the first LDS byte behind the weight set
  __device__ __forceinline__ void begin(float* after_weights) {
    region = reinterpret_cast<double*>(after_weights) + ((int)threadIdx.x / kWave) * 2 * L::K;
    if (lane_id() == 0) {
#pragma unroll
      for (int s = 0; s < 2 * L::K; ++s) region[s] = 0.0;
    }
#pragma unroll
    for (int d = 0; d < Fam::D; ++d) s1[d] = s2[d] = 0.0f;
    cnt = 0;
  }

  // v summed over the wavefront, added to entry `at` of the wave's region (every lane of the wave calls it)
  __device__ __forceinline__ void add_wave(int at, double v) {
    const double t = wave_sum_f64(v);
    if (lane_id() == 0) region[at] += t;
  }

  // the context inputs of the `cnt` steps the lanes ran in context `cidx` (every lane of the wave calls it)
  __device__ __forceinline__ void flush_context(const GlobalCtx& ctx, const carl_policy_t& pol, const float* wts, int n_ctx,
                                                int cidx) {
#pragma clang fp contract(off)
    const bool any = cnt > 0;  // (cidx is -1 before the first step: nothing counted yet, and a 0 * inf must not count)
    const double c = (double)cnt;
#pragma unroll
    for (int k = 0; k < Fam::F; ++k)
      if (k < n_ctx) {  // (wave-uniform)
        const float d = ctx.get(pol.ctx_rows[k], cidx < 0 ? 0 : cidx) - wts[L::kShift + k];
        const double a = any ? c * (double)d : 0.0;
        add_wave(k, a);
        add_wave(L::K + k, any ? a * (double)d : 0.0);
      }
    cnt = 0;
  }

  // one step's observation `o` (before the step), and the step itself
  __device__ __forceinline__ void add_step(bool live, const float (&o)[Fam::D], const float* wts) {
#pragma clang fp contract(off)
#pragma unroll
    for (int d = 0; d < Fam::D; ++d) {
      const float v = o[d] - wts[L::kShift + Fam::F + d];
      s1[d] = live ? s1[d] + v : s1[d];
      s2[d] = live ? __fmaf_rn(v, v, s2[d]) : s2[d];
    }
    cnt += live ? 1 : 0;
  }

  // the end of a chunk (every lane of the wave calls it): everything gathered since the last flush -> the wave's sums
  __device__ __forceinline__ void flush(const GlobalCtx& ctx, const carl_policy_t& pol, const float* wts, int n_ctx,
                                        int cidx) {
    flush_context(ctx, pol, wts, n_ctx, cidx);
#pragma unroll
    for (int d = 0; d < Fam::D; ++d) {
      add_wave(Fam::F + d, (double)s1[d]);
      add_wave(L::K + Fam::F + d, (double)s2[d]);
      s1[d] = s2[d] = 0.0f;
    }
  }

  // after the step loop (every thread of the workgroup calls it): the four waves' sums, in wave order, to the slab
  __device__ __forceinline__ void store(const float* after_weights, int n_ctx, int n_in) const {
    __syncthreads();
    const double* all = reinterpret_cast<const double*>(after_weights);
    for (int e = threadIdx.x; e < 2 * CARL_POLICY_MAX_IN; e += blockDim.x) {
      const int which = e / CARL_POLICY_MAX_IN, i = e % CARL_POLICY_MAX_IN;
      double t = 0.0;
      if (i < n_in) {
        const int slot = i < n_ctx ? i : Fam::F + (i - n_ctx);
        for (int w = 0; w < kPolicyLanes / kWave; ++w) t += all[(w * 2 + which) * L::K + slot];
      }
      partial[((size_t)blockIdx.x * 2 + which) * CARL_POLICY_MAX_IN + i] = t;
    }
  }
};

// carl_evaluate_policy_stats: policy_episodes_kernel (SAMPLED: policy_episodes_sampled_kernel) gathering InputStats.
// Preconditions as theirs; `partial` holds gridDim.x slabs; dynamic LDS: the weight set + policy_stats_lds_bytes.
template <class Fam, int H, bool SAMPLED>
__global__ void __launch_bounds__(kPolicyThreadsSummary)
    policy_episodes_stats_kernel(const carl_batch_t b, const carl_policy_t pol, const int set_floats,
                                 const carl_policy_episodes_t ep, const int n_episodes, const int max_steps,
                                 const carl_policy_sampling_t smp, double* const partial) {
  using Pick = std::conditional_t<SAMPLED, SampledPick<Fam, false>, ModePick<Fam>>;
  Pick pick{};
  if constexpr (SAMPLED) pick = Pick::of(smp, pol);
  using Stats = InputStats<Fam, H>;
  Stats istats;
  istats.partial = partial;
#include "policy_episodes_body.inc"
}

// carl_policy_stats_merge (include/carl_amd.h states the arithmetic): one workgroup; thread i < n_in owns input i.
constexpr int kStatsMergeThreads = 256;

__global__ __launch_bounds__(kStatsMergeThreads) void policy_stats_merge_kernel(
    const double* __restrict__ partial, const int n_workgroups, const int32_t* __restrict__ steps, const int n_lanes,
    const int n_in, const float* shift_in, int64_t* count, double* mean, double* m2, const double eps,
    const double min_std, float* params_out, const int n_write, const int set_floats, const int p_shift) {
#pragma clang fp contract(off)
  __shared__ long long part[kStatsMergeThreads];
  const int t = (int)threadIdx.x;
  long long c = 0;
  for (int l = t; l < n_lanes; l += kStatsMergeThreads) c += steps[l];
  part[t] = c;
  __syncthreads();
  for (int h = kStatsMergeThreads / 2; h > 0; h >>= 1) {
    if (t < h) part[t] += part[t + h];
    __syncthreads();
  }
  const long long n_b = part[0];
  if (n_b == 0) return;  // (workgroup-uniform) nothing was gathered: the running state and the blocks stay
  const long long n_a = *count;
  __syncthreads();  // every thread holds the old count before thread 0 replaces it
  if (t >= n_in) return;
  double sd = 0.0, sq = 0.0;
  for (int w = 0; w < n_workgroups; ++w) {
    sd += partial[((size_t)w * 2 + 0) * CARL_POLICY_MAX_IN + t];
    sq += partial[((size_t)w * 2 + 1) * CARL_POLICY_MAX_IN + t];
  }
  const double nb = (double)n_b, na = (double)n_a;
  const double mean_b = (double)shift_in[t] + sd / nb;
  double m2_b = sq - sd * sd / nb;
  m2_b = m2_b > 0.0 ? m2_b : 0.0;
  double mu = mean_b, ss = m2_b;
  const long long n = n_a + n_b;
  const double nn = (double)n;
  if (n_a > 0) {  // Chan et al.'s pairwise update
    const double delta = mean_b - mean[t];
    mu = mean[t] + delta * (nb / nn);
    ss = (m2[t] + m2_b) + delta * delta * (na * nb / nn);
  }
  mean[t] = mu;
  m2[t] = ss;
  if (t == 0) *count = n;
  if (params_out == nullptr) return;
  const double var = ss / nn;
  const double rel = 0x1p-18 * fabs(mu);
  const double floor2 = fmax(min_std * min_std, rel * rel);
  const double scale = var <= floor2 ? 0.0 : 1.0 / sqrt(var + eps);
  for (int k = 0; k < n_write; ++k) {
    float* blk = params_out + (size_t)k * set_floats + p_shift;
    blk[t] = (float)mu;
    blk[n_in + t] = (float)scale;
  }
}

}  // namespace carl
