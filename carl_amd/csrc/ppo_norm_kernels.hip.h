// ppo_norm_kernels.hip.h -- the kernels of PPO's running normalisation (include/carl_amd.h: carl_ppo_input_stats,
// carl_ppo_return_stats, carl_ppo_return_merge).  Included by carl_ppo_norm.hip only.  ppo_device.hip.h gives the buffer
// struct and the workgroup shape; no device function of another header is called, no existing kernel is instantiated.
//
// ppo_input_stats_kernel: the shifted sums of every policy input over a rollout buffer, float64 from the first sample.
// A thread owns ONE input slot i of a block of samples, so it carries one (S1, S2) pair whatever n_in is (a per-thread
// [2][32] array indexed by a run-time loop would live in scratch).  With spt = 256 / n_in samples per pass, thread
// tid < spt * n_in has i = tid % n_in and takes sample pass * spt + tid / n_in of every pass its workgroup runs:
// consecutive threads read consecutive floats of consecutive samples' observation rows (a wavefront's loads of a pass
// are one contiguous run of 256 bytes apart from the context slots), the context slots read the table through the
// sample's id.  The passes go round the grid (pass p to workgroup p % gridDim.x); a thread chains its samples in pass
// order, then thread i < 32 adds the spt partial pairs of its slot from LDS in slot order and writes the slab.  No
// atomics: the slabs are a fixed function of the buffer and the launch shape.
#pragma once

#include "ppo_device.hip.h"

namespace carl {

struct PpoInputStatsArgs {
  carl_ppo_batch_t b;    // row_pitch resolved (never 0); idx NULL; the action / log_prob / advantage / ret columns not read
  int n_in, n_ctx;
  int ctx_rows[CARL_POLICY_MAX_IN];
  const float* shift;    // [n_in] of the actor's weight set 0
  double* partial;       // [gridDim.x][2][CARL_POLICY_MAX_IN]
  long long n_samples;   // n_steps * n_lanes
};

constexpr int kInputAhead = 8;       // passes of a thread whose loads are in flight together

// Preconditions (host, carl_ppo_norm.hip): 1 <= n_in <= 32, n_samples >= 1, gridDim.x <= ceil(n_samples / 256)
__global__ void __launch_bounds__(kPpoThreads) ppo_input_stats_kernel(const PpoInputStatsArgs a) {
  __shared__ double red[2][kPpoThreads];
  const carl_ppo_batch_t& b = a.b;
  const int tid = (int)threadIdx.x;
  const int n_in = a.n_in;
  const int spt = kPpoThreads / n_in;          // samples of one pass
  const int i = tid % n_in, so = tid / n_in;   // this thread's input slot and its sample within a pass
  const bool active = so < spt;
  const bool is_ctx = i < a.n_ctx;
  const size_t pitch = (size_t)b.row_pitch;
  const size_t D = (size_t)b.obs_dim;
  const float sh = a.shift[i];
  const float* const ctx_row = b.ctx_table + (size_t)a.ctx_rows[is_ctx ? i : 0] * b.ctx_stride;
  const int od = is_ctx ? 0 : i - a.n_ctx;     // the observation entry of an observation slot (0: an address never read)
  // (n_samples < 2^31, host-checked: 32-bit unsigned sample indices, one 32-bit division per sample)
  const unsigned n_s = (unsigned)a.n_samples, n_l = (unsigned)b.n_lanes;
  const unsigned n_pass = (n_s + (unsigned)spt - 1u) / (unsigned)spt;
  double s1 = 0.0, s2 = 0.0;
  // The loads of kInputAhead of the thread's passes are issued before the dependent float64 chain of those passes, as the
  // return walk below issues its rows ahead: a persistent grid holds 4 wavefronts per compute unit, so one load in flight
  // per thread leaves the launch waiting on memory latency.  A pass past the end loads sample 0 (always inside the
  // buffer) and adds nothing, so no load sits behind a branch; the chain's order is the samples' order as before.
  if (active) {
#pragma unroll 1
    for (unsigned p0 = blockIdx.x; p0 < n_pass; p0 += (unsigned)kInputAhead * gridDim.x) {
      bool ok[kInputAhead];
      const float* src[kInputAhead];
      int cid[kInputAhead];
      float x[kInputAhead];
#pragma unroll
      for (int k = 0; k < kInputAhead; ++k) {
        const unsigned p = p0 + (unsigned)k * gridDim.x;
        unsigned m = p * (unsigned)spt + (unsigned)so;
        ok[k] = p < n_pass && m < n_s;
        m = ok[k] ? m : 0u;
        const unsigned t = m / n_l;
        const unsigned lane = m - t * n_l;
        src[k] = t == 0 ? b.obs0 + ((size_t)lane * D + od) : b.obs + (((size_t)(t - 1) * pitch + lane) * D + od);
        if (is_ctx) cid[k] = b.context_id[(size_t)t * pitch + lane];
      }
#pragma unroll
      for (int k = 0; k < kInputAhead; ++k)
        x[k] = is_ctx ? ctx_row[min(max(cid[k], 0), b.n_contexts - 1)] : *src[k];
#pragma unroll
      for (int k = 0; k < kInputAhead; ++k) {
        if (ok[k]) {
          const double d = (double)(x[k] - sh);  // one fp32 subtraction: the input transform's first operation
          s1 += d;
          s2 += d * d;                           // (the product of two widened floats is exact)
        }
      }
    }
  }
  red[0][tid] = s1;
  red[1][tid] = s2;
  __syncthreads();
  if (tid < 2 * CARL_POLICY_MAX_IN) {
    const int q = tid / CARL_POLICY_MAX_IN, j = tid % CARL_POLICY_MAX_IN;
    double s = 0.0;
    if (j < n_in)
      for (int k = 0; k < spt; ++k) s += red[q][k * n_in + j];
    a.partial[((size_t)blockIdx.x * 2 + q) * CARL_POLICY_MAX_IN + j] = s;
  }
}

// ---- the discounted return of every lane, for reward scaling (VecNormalize's rule).  One thread owns one lane's column and
// walks it forward; the loads of kReturnRows rows are issued before the dependent chain of those rows, as gae_kernel's
// and context_trace_kernel's.  pitch is never 0 here.
constexpr int kReturnThreads = 256;
constexpr int kReturnRows = 8;

struct PpoReturnStatsArgs {
  int n_lanes, n_steps, pitch;
  float gamma;
  const float* reward;
  const uint8_t* terminated;
  const uint8_t* truncated;
  float* ret;        // [n_lanes], read and written back
  float* ret_rows;   // [n_steps][pitch], nullable
  double* partial;   // [gridDim.x][2]
};

__global__ void __launch_bounds__(kReturnThreads) ppo_return_stats_kernel(const PpoReturnStatsArgs a) {
#pragma clang fp contract(off)
  __shared__ double red[kReturnThreads];
  const int lane = (int)blockIdx.x * kReturnThreads + (int)threadIdx.x;
  const bool live = lane < a.n_lanes;
  const size_t n = (size_t)a.pitch;
  double s1 = 0.0, s2 = 0.0;
  if (live) {
    float r = a.ret[lane];
#pragma unroll 1
    for (int t0 = 0; t0 < a.n_steps; t0 += kReturnRows) {
      float rw[kReturnRows];
      uint8_t dn[kReturnRows];
#pragma unroll
      for (int k = 0; k < kReturnRows; ++k) {
        if (t0 + k < a.n_steps) {  // (uniform)
          const size_t i = (size_t)(t0 + k) * n + lane;
          rw[k] = a.reward[i];
          dn[k] = a.terminated[i] | a.truncated[i];
        }
      }
#pragma unroll
      for (int k = 0; k < kReturnRows; ++k) {
        if (t0 + k < a.n_steps) {
          const float gr = a.gamma * r;
          r = gr + rw[k];
          if (a.ret_rows != nullptr) a.ret_rows[(size_t)(t0 + k) * n + lane] = r;
          const double d = (double)r;
          s1 += d;
          s2 += d * d;
          if (dn[k] != 0) r = 0.0f;
        }
      }
    }
    a.ret[lane] = r;
  }
  const double t1 = ppo_block_sum(red, s1);
  const double t2 = ppo_block_sum(red, s2);
  if (threadIdx.x == 0) {
    a.partial[(size_t)blockIdx.x * 2] = t1;
    a.partial[(size_t)blockIdx.x * 2 + 1] = t2;
  }
}

// One thread: the slabs in order, the batch mean and M2, Chan's merge into the running triple, the scale.  Every operation
// float64, each rounded on its own -- carl_policy_stats_merge's text for one entry, without a shift.
__global__ void __launch_bounds__(64)
    ppo_return_merge_kernel(const double* __restrict__ partial, const int n_slabs, const long long n_b_i, int64_t* count,
                            double* mean, double* m2, const double eps, float* scale) {
#pragma clang fp contract(off)
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double S1 = 0.0, S2 = 0.0;
  for (int w = 0; w < n_slabs; ++w) {
    S1 += partial[(size_t)w * 2];
    S2 += partial[(size_t)w * 2 + 1];
  }
  const double n_b = (double)n_b_i;
  const double mean_b = S1 / n_b;
  double M2_b = S2 - S1 * S1 / n_b;
  M2_b = M2_b > 0.0 ? M2_b : 0.0;
  const int64_t c0 = count[0], c1 = c0 + (int64_t)n_b_i;
  const double cnt = (double)c0, nn = (double)c1;
  double mu = mean_b, M = M2_b;
  if (c0 > 0) {  // Chan et al.'s pairwise update
    const double delta = mean_b - mean[0];
    mu = mean[0] + delta * (n_b / nn);
    M = (m2[0] + M2_b) + delta * delta * (cnt * n_b / nn);
  }
  count[0] = c1;
  mean[0] = mu;
  m2[0] = M;
  const double var = M / nn;
  scale[0] = (float)(1.0 / sqrt(var + eps));
}

}  // namespace carl
