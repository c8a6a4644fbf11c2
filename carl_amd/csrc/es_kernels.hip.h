// es_kernels.hip.h -- evolution strategies on the device (include/carl_amd.h: carl_es_t): the antithetic perturbation of
// a centre parameter vector into packed weight sets, and the gradient estimate that regenerates the same noise from its
// counter instead of reading it back.  The noise rule, the two-rounding arithmetic and the summation order are the
// header's; nothing here is shared with the rollout kernels but Philox and u01 (carl_device.hip.h), so those compile
// as they did.
#pragma once

#include "carl_device.hip.h"

namespace carl {

constexpr uint32_t kSubEsNoise = 0x40000000u;  // last counter word of the noise stream (include/carl_amd.h)
constexpr int kEsThreads = 256;
constexpr int kEsSlicePairs = 16;                             // carl_es_slice_pairs(): pairs of one summation slice
constexpr int kEsGradBlocks = 32;                             // Philox blocks (two parameters each) of one workgroup
constexpr int kEsGradSlices = kEsThreads / kEsGradBlocks;     // slices a workgroup sums side by side

// the Philox block of parameters 2 * block and 2 * block + 1 of pair `pair`
__device__ __forceinline__ u32x4 es_words(const carl_es_t& es, uint32_t block, uint32_t pair) {
  return philox4x32_10(u32x4{block, pair, es.generation, kSubEsNoise}, (uint32_t)es.seed, (uint32_t)(es.seed >> 32));
}

// carl_policy_sampling_t's Gaussian rule (carl_device.hip.h: normal_from_words)
__device__ __forceinline__ float es_normal(uint32_t a, uint32_t b) { return normal_from_words(a, b); }

// One thread per (pair, Philox block): floats 2k and 2k + 1 of sets 2i and 2i + 1, as one 8-byte store each (set_floats
// is a multiple of 4 and params 16-byte aligned), so a wavefront writes two contiguous 512-byte runs.  Threads of the
// shift | scale | clip section and the padding draw nothing and copy the centre's bits.
__global__ __launch_bounds__(kEsThreads) void es_perturb_kernel(carl_es_t es, const float* __restrict__ center,
                                                                float* __restrict__ params, float* __restrict__ noise) {
#pragma clang fp contract(off)
  const int half = es.set_floats >> 1;
  const int t = (int)blockIdx.x * kEsThreads + (int)threadIdx.x;
  if (t >= es.n_pairs * half) return;
  const int i = t / half, k = t - i * half, j = 2 * k;
  const float c0 = center[j], c1 = center[j + 1];
  float2 plus{c0, c1}, minus{c0, c1};
  if (j < es.n_noisy) {
    const u32x4 w = es_words(es, (uint32_t)k, (uint32_t)i);
    float* nz = noise != nullptr ? noise + (size_t)i * (size_t)es.n_noisy + j : nullptr;
    const float z0 = es_normal(w.x, w.y);
    const float d0 = es.sigma * z0;
    plus.x = c0 + d0;
    minus.x = c0 - d0;
    if (nz != nullptr) nz[0] = z0;
    if (j + 1 < es.n_noisy) {
      const float z1 = es_normal(w.z, w.w);
      const float d1 = es.sigma * z1;
      plus.y = c1 + d1;
      minus.y = c1 - d1;
      if (nz != nullptr) nz[1] = z1;
    }
  }
  float* row = params + (size_t)(2 * i) * (size_t)es.set_floats + j;
  *reinterpret_cast<float2*>(row) = plus;
  *reinterpret_cast<float2*>(row + es.set_floats) = minus;
}

// grad[j] = sum_i weight[i] * z_ij in the header's order.  A workgroup owns kEsGradBlocks Philox blocks; its threads
// (g, b) sum kEsGradSlices slices of block b side by side, each sequentially over its pairs, and thread (0, b) then adds
// the slice sums in slice order -- through LDS, no atomics, so the result does not depend on the grid.
__global__ __launch_bounds__(kEsThreads) void es_gradient_kernel(carl_es_t es, const float* __restrict__ weight,
                                                                 float* __restrict__ grad) {
#pragma clang fp contract(off)
  __shared__ float2 part[kEsGradSlices][kEsGradBlocks];
  const int b = (int)threadIdx.x % kEsGradBlocks, g = (int)threadIdx.x / kEsGradBlocks;
  const int k = (int)blockIdx.x * kEsGradBlocks + b, j = 2 * k;
  const bool live = j < es.n_noisy;
  const int n_slices = (es.n_pairs + kEsSlicePairs - 1) / kEsSlicePairs;
  float2 total{0.0f, 0.0f};
  for (int s0 = 0; s0 < n_slices; s0 += kEsGradSlices) {  // (workgroup-uniform: every thread reaches both barriers)
    const int s = s0 + g;
    float2 p{0.0f, 0.0f};
    if (live && s < n_slices) {
      const int i0 = s * kEsSlicePairs;
      const int i1 = i0 + kEsSlicePairs < es.n_pairs ? i0 + kEsSlicePairs : es.n_pairs;  // (the last slice may be ragged)
      for (int i = i0; i < i1; ++i) {
        const float wt = weight[i];
        const u32x4 w = es_words(es, (uint32_t)k, (uint32_t)i);
        p.x = p.x + wt * es_normal(w.x, w.y);
        p.y = p.y + wt * es_normal(w.z, w.w);
      }
    }
    part[g][b] = p;
    __syncthreads();
    if (g == 0) {
      const int ns = n_slices - s0 < kEsGradSlices ? n_slices - s0 : kEsGradSlices;
      for (int q = 0; q < ns; ++q) {
        total.x = total.x + part[q][b].x;
        total.y = total.y + part[q][b].y;
      }
    }
    __syncthreads();
  }
  if (g == 0 && live) {
    grad[j] = total.x;
    if (j + 1 < es.n_noisy) grad[j + 1] = total.y;
  }
}

}  // namespace carl
