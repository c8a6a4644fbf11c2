// ppo_step_device.hip.h -- what the kernels of PPO's minibatch step share (ppo_step_kernels.hip.h: the one-set kernels;
// ppo_sets_kernels.hip.h: a population's): the launch constants, the workgroup sum and the argument structs.  No kernel is
// defined here; no device function of another header is called.
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

}  // namespace carl
