// ppo_kernels.hip.h -- the kernels of the PPO update on the device (include/carl_amd.h: carl_policy_context_trace,
// carl_ppo_grad): ppo_net_kernel<H> (ppo_net_kernel.hip.h), and here the two that are not templates, the slab reduction
// and the trace walk.  Included by carl_ppo.hip only, so the library holds one definition of each of the two: the Brax
// unit runs its trace through carl_ppo.hip's launch_context_trace (ppo_host.hpp) and has a reduction of its own.  The
// layout, the argument structs and the tile helpers are ppo_device.hip.h's; carl_device.hip.h's select_context is
// called, not changed.
#pragma once

#include "ppo_net_kernel.hip.h"

namespace carl {

// One thread per output (ppo_reduce_body.inc, which the population's reduction includes too)
__global__ void __launch_bounds__(256) ppo_reduce_kernel(const PpoReduceArgs a) {
#include "ppo_reduce_body.inc"
}

// ---- the context each step ran in (include/carl_amd.h: carl_policy_context_trace).  One thread owns one lane's column
// and walks it forward; the flag loads of kTraceRows rows are issued before the dependent chain of those rows, as
// gae_kernel's.  pitch is never 0 here.
constexpr int kTraceRows = 8;

__global__ void __launch_bounds__(kTraceThreads)
    context_trace_kernel(const carl_batch_t b, const int32_t* __restrict__ ctx_idx0, const uint32_t* __restrict__ episode0,
                         const uint8_t* __restrict__ terminated, const uint8_t* __restrict__ truncated, const int n_steps,
                         const int pitch, int32_t* __restrict__ context_id) {
  const int lane = (int)blockIdx.x * kTraceThreads + (int)threadIdx.x;
  if (lane >= b.n_lanes) return;
  const size_t n = (size_t)pitch;
  const uint64_t glane = (uint64_t)(b.lane_offset + lane);
  const bool autoreset = (b.flags & CARL_FLAG_AUTORESET) != 0;
  int c = ctx_idx0[lane];
  uint32_t e = episode0[lane];
#pragma unroll 1
  for (int t0 = 0; t0 < n_steps; t0 += kTraceRows) {
    uint8_t te[kTraceRows], tr[kTraceRows];
#pragma unroll
    for (int k = 0; k < kTraceRows; ++k) {
      if (t0 + k < n_steps) {  // (uniform)
        const size_t i = (size_t)(t0 + k) * n + lane;
        te[k] = terminated[i];
        tr[k] = truncated[i];
      }
    }
#pragma unroll
    for (int k = 0; k < kTraceRows; ++k) {
      if (t0 + k < n_steps) {
        context_id[(size_t)(t0 + k) * n + lane] = c;
        if (autoreset && (te[k] | tr[k]) != 0) {  // reset_lane's order: the selector, then the episode counter
          c = select_context(b, c, glane, e);
          e += 1u;
        }
      }
    }
  }
}

}  // namespace carl
