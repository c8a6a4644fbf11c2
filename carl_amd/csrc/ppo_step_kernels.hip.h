// ppo_step_kernels.hip.h -- the kernels of PPO's minibatch step (include/carl_amd.h: carl_ppo_adv_stats, carl_adam_step).
// Included by carl_ppo_step.hip only.  No device function of another header is called, no existing kernel is instantiated.
//
// Both kernels sum in float64 in an order that is a fixed function of the launch shape: a thread chains its own elements
// in index order, a wavefront adds its 64 values by a shuffle tree, thread 0 adds the wavefronts' sums from LDS in
// wavefront order.  No floating-point atomics, no hand-over between workgroups: the same call twice gives the same bits.
// Floating-point contraction is off in both, so every product and every sum is rounded on its own.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/carl_amd.h"

namespace carl {

constexpr int kAdvThreads = 256;    // one workgroup per minibatch
constexpr int kAdvAhead = 8;        // gathers of a thread in flight before the dependent adds
constexpr int kAdamThreads = 1024;  // the one workgroup of an Adam step
constexpr int kAdamAhead = 4;
constexpr long long kAdamMaxFloats = 1ll << 18;  // 256 elements per thread and pass: what one workgroup takes in tens of microseconds

// Sum of v over a workgroup of THREADS threads, returned in EVERY thread.  `red`: THREADS / 64 + 1 doubles of LDS.
template <int THREADS>
__device__ __forceinline__ double step_block_sum(double* red, double v) {
#pragma clang fp contract(off)
  constexpr int kWaves = THREADS / 64;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);  // lanes past the tree's edge add values never used
  const int tid = (int)threadIdx.x;
  __syncthreads();  // (a previous sum's result has been read by everyone)
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) {
    double s = red[0];
    for (int w = 1; w < kWaves; ++w) s += red[w];
    red[kWaves] = s;
  }
  __syncthreads();
  return red[kWaves];
}

// ---- one epoch's advantage mean and scale: workgroup k takes minibatch k
struct PpoAdvStatsArgs {
  const float* advantage;
  long long storage_floats;
  const int32_t* idx;
  int n_total, batch_size;
  double eps;
  float* adv_norm;  // [gridDim.x][2]
};

// Preconditions (host, carl_ppo_step.hip): n_total >= 1, batch_size >= 1, gridDim.x == ceil(n_total / batch_size)
__global__ void __launch_bounds__(kAdvThreads) ppo_adv_stats_kernel(const PpoAdvStatsArgs a) {
#pragma clang fp contract(off)
  __shared__ double red[kAdvThreads / 64 + 1];
  const int tid = (int)threadIdx.x;
  const long long first = (long long)blockIdx.x * a.batch_size;
  const long long left = (long long)a.n_total - first;
  const int n = (int)(left < a.batch_size ? left : a.batch_size);  // >= 1
  const int32_t* const idx = a.idx + first;
  if (n == 1) {  // the identity: what passing no adv_norm does
    if (tid == 0) a.adv_norm[(size_t)blockIdx.x * 2] = 0.0f, a.adv_norm[(size_t)blockIdx.x * 2 + 1] = 1.0f;
    return;
  }
  const long long j0 = idx[0];
  const bool in0 = j0 >= 0 && j0 < a.storage_floats;
  const double c = in0 ? (double)a.advantage[j0] : 0.0;  // (an index outside the storage: the shift is 0)
  double s1 = 0.0, s2 = 0.0;
  // kAdvAhead of the thread's gathers are issued before the dependent float64 chain, as ppo_input_stats_kernel issues
  // its passes: a sample past the end or outside the storage loads element 0 (storage_floats >= 1) and adds nothing.
#pragma unroll 1
  for (int i0 = tid; i0 < n; i0 += kAdvAhead * kAdvThreads) {
    bool ok[kAdvAhead];
    long long j[kAdvAhead];
    float x[kAdvAhead];
#pragma unroll
    for (int k = 0; k < kAdvAhead; ++k) {
      const int i = i0 + k * kAdvThreads;
      j[k] = idx[i < n ? i : 0];
      ok[k] = i < n && j[k] >= 0 && j[k] < a.storage_floats;
    }
#pragma unroll
    for (int k = 0; k < kAdvAhead; ++k) x[k] = a.advantage[ok[k] ? j[k] : 0];
#pragma unroll
    for (int k = 0; k < kAdvAhead; ++k) {
      if (ok[k]) {
        const double d = (double)x[k] - c;
        s1 += d;
        s2 += d * d;
      }
    }
  }
  const double S1 = step_block_sum<kAdvThreads>(red, s1);
  const double S2 = step_block_sum<kAdvThreads>(red, s2);
  if (tid == 0) {
    const double nn = (double)n;
    const double mean = c + S1 / nn;
    double var = (S2 - S1 * S1 / nn) / (nn - 1.0);
    var = var > 0.0 ? var : 0.0;
    a.adv_norm[(size_t)blockIdx.x * 2] = (float)mean;
    a.adv_norm[(size_t)blockIdx.x * 2 + 1] = (float)(1.0 / (sqrt(var) + a.eps));
  }
}

// ---- the global-norm clip and Adam over up to CARL_ADAM_MAX_TENSORS tensors: one workgroup, the norm, then the update
struct AdamArgs {
  int n_tensors;
  long long n[CARL_ADAM_MAX_TENSORS];
  float* param[CARL_ADAM_MAX_TENSORS];
  const float* grad[CARL_ADAM_MAX_TENSORS];
  float* m[CARL_ADAM_MAX_TENSORS];
  float* v[CARL_ADAM_MAX_TENSORS];
  double lr, beta1, beta2, eps, max_grad_norm;
  int64_t* step;
  double* beta_pow;
  double* norm_out;  // nullable
};

// Preconditions (host): gridDim.x == 1; the tensors' elements together <= kAdamMaxFloats
__global__ void __launch_bounds__(kAdamThreads) adam_step_kernel(const AdamArgs a) {
#pragma clang fp contract(off)
  __shared__ double red[kAdamThreads / 64 + 1];
  const int tid = (int)threadIdx.x;
  // every thread reads the state before the sum's barriers; thread 0 writes it behind them
  const int64_t step = a.step[0];
  const double bp1 = a.beta_pow[0] * a.beta1, bp2 = a.beta_pow[1] * a.beta2;
  double s = 0.0;
  for (int t = 0; t < a.n_tensors; ++t) {
    const float* const g = a.grad[t];
    const long long n = a.n[t];
#pragma unroll 1
    for (long long i0 = tid; i0 < n; i0 += (long long)kAdamAhead * kAdamThreads) {
      float x[kAdamAhead];
#pragma unroll
      for (int k = 0; k < kAdamAhead; ++k) {
        const long long i = i0 + (long long)k * kAdamThreads;
        x[k] = i < n ? g[i] : 0.0f;
      }
#pragma unroll
      for (int k = 0; k < kAdamAhead; ++k) {
        const double d = (double)x[k];
        s += d * d;  // (a slot past the end adds +0.0 to a sum that is never -0.0)
      }
    }
  }
  const double norm = sqrt(step_block_sum<kAdamThreads>(red, s));
  const double ratio = a.max_grad_norm / (norm + 1e-6);  // (+inf: no clip)
  const double coef = ratio < 1.0 ? ratio : 1.0;
  if (tid == 0) {
    a.step[0] = step + 1;
    a.beta_pow[0] = bp1;
    a.beta_pow[1] = bp2;
    if (a.norm_out != nullptr) a.norm_out[0] = norm, a.norm_out[1] = coef;
  }
  const double omb1 = 1.0 - a.beta1, omb2 = 1.0 - a.beta2;
  const double step_size = a.lr / (1.0 - bp1), sqrt_bc2 = sqrt(1.0 - bp2);
  for (int t = 0; t < a.n_tensors; ++t) {
    const float* const g = a.grad[t];
    float* const p = a.param[t];
    float* const m = a.m[t];
    float* const v = a.v[t];
    const long long n = a.n[t];
    for (long long i = tid; i < n; i += kAdamThreads) {
      const double gd = (double)g[i] * coef;
      const float mf = (float)(a.beta1 * (double)m[i] + omb1 * gd);
      const float vf = (float)(a.beta2 * (double)v[i] + omb2 * gd * gd);
      m[i] = mf;
      v[i] = vf;
      p[i] = (float)((double)p[i] - step_size * (double)mf / (sqrt((double)vf) / sqrt_bc2 + a.eps));
    }
  }
}

}  // namespace carl
