// brax_stats_kernels.hip.h -- input statistics inside the episodes launch of the Brax closed-loop rollout
// (include/carl_amd.h: carl_brax_evaluate_policy_stats): the policy type that selects the variant in Group<K>::run
// (brax_kernels.hip.h: Pol::kStats, beside Pol::kEpisodes), the tap BraxPolicy::act (brax_policy_kernels.hip.h) hands the
// raw inputs to, and the kernel around them.  The step, the records and the engine state are the episodes twin's
// (brax_episodes_kernels.hip.h), and so are the launch shape and the LDS: nothing is added to policy_layout_of.
//
// What is gathered is carl_evaluate_policy_stats' contract: for every live env-step and every policy input i,
// d_i = fp32(x_i - shift_i) -- normalize_input's first operation -- and d_i * d_i.  Where:
//   act, first phase   the lane that normalises entry i of its env also leaves d_i in row i of the env's h2 rows, which
//                      are dead until layer 2 writes them; the env's first lane leaves `live` (1 / 0) in the first of the
//                      env's four summary-total rows, which the episodes mode reserves and never uses.  An env past the
//                      end of the batch has such a lane too and marks 0; what its d rows hold is never looked at.
//   behind the phase's hand-over (the phase_sync that is there anyway), before layer 1:
//                      lane i < n_in of the WAVEFRONT owns input i.  It walks the wavefront's kEnvs envs in env order --
//                      row r is base[r * kEnvs + env], one run of consecutive floats -- and adds d and d * d of the live
//                      ones, both widened to float64 first (the square of an fp32 value is exact in float64), into two
//                      float64 step sums that start at +0.0; the step sums are then added to the two float64 registers
//                      the lane keeps for the whole launch, over all the wavefront's fragments.
//   behind the fragment loop
//                      lanes 0 .. CARL_POLICY_MAX_IN - 1 write the wavefront's slab partial[blockIdx.x * waves + wave]
//                      once, in full: +0.0 at and beyond n_in, and everywhere for a wavefront that ran no fragment.
// No barrier, no atomics, no fp32 accumulation: every slab entry is a fixed sequence of float64 additions of exact terms.
// Cost per wavefront-step: at most kEnvs pairs of LDS reads, conversions and float64 adds in n_in lanes, four VGPRs.
#pragma once

#include "brax_episodes_kernels.hip.h"

namespace carl {
namespace brax {

// BraxPolicy::act's tap: one per act() call, around the wavefront's running sums
struct InputStatsTap {
  static constexpr bool kOn = true;
  bool live;   // the env takes this step as one of the steps episodes_out.steps counts
  int lane;    // the lane's index in its wavefront: the input it owns
  double& s1;  // the wavefront's sums of input `lane`
  double& s2;

  template <class LdsT>
  __device__ __forceinline__ void put(const LdsT& m, int row, float raw, float shift) const {
#pragma clang fp contract(off)
    m.at(row) = raw - shift;
  }
  // every env column of the wavefront has a first lane, the columns past the end of the batch included
  template <class LdsT>
  __device__ __forceinline__ void mark(const LdsT& m, int row) const {
    if (m.sub == 0) m.atu(row) = live ? 1u : 0u;
  }
  template <int kSub, class LdsT>
  __device__ __forceinline__ void gather(const LdsT& m, int d_row, int live_row, int n_in) const {
#pragma clang fp contract(off)
    constexpr int kEnvs = Group<kSub>::kEnvs;
    if (lane < n_in) {
      const float* d = m.base + (d_row + lane) * kEnvs;
      const uint32_t* on = reinterpret_cast<const uint32_t*>(m.base) + live_row * kEnvs;
      double t1 = 0.0, t2 = 0.0;
#pragma unroll
      for (int e = 0; e < kEnvs; ++e) {
        const double v = on[e] != 0u ? (double)d[e] : 0.0;  // (a select, not a product: a dead row may hold anything)
        t1 += v;
        t2 += v * v;
      }
      s1 += t1;
      s2 += t2;
    }
  }
};

struct BraxStatsPolicy : BraxEpisodesPolicy {
  static constexpr bool kStats = true;
  double* partial;  // [grid * waves per workgroup][2][CARL_POLICY_MAX_IN]; validated by the host (carl_brax_policy_stats.hip)

  // BraxPolicy::act with the tap; no per-step action record (the episodes mode has none)
  template <int kSub, class LdsT>
  __device__ __forceinline__ void act_stats(const LdsT& m, int rows, const carl_batch_t& b, int cidx, int env, bool active,
                                            bool live, int lane, int obs_dim, int n_act, double& s1, double& s2) const {
    this->template act<kSub>(m, rows, b, cidx, env, active, obs_dim, n_act, nullptr, InputStatsTap{live, lane, s1, s2});
  }

  // behind the fragment loop: the wavefront's slab, every entry of it
  __device__ __forceinline__ void store_stats(int slab, int lane, double s1, double s2) const {
    if (lane < CARL_POLICY_MAX_IN) {
      double* out = partial + (size_t)slab * 2 * CARL_POLICY_MAX_IN;
      const bool own = lane < p.n_in;
      out[lane] = own ? s1 : 0.0;
      out[CARL_POLICY_MAX_IN + lane] = own ? s2 : 0.0;
    }
  }
};

// brax_episodes_kernel's statistics twin, one instance per instance of it.
template <bool MULTI, int K, bool TASK = false, bool PLANAR = false>
__global__ void __launch_bounds__(kLanes * max_waves_per_wg(TASK)) __attribute__((amdgpu_waves_per_eu(CARL_BRAX_WAVES_PER_EU(TASK))))
brax_episodes_stats_kernel(const carl_batch_t b, const carl_brax_sys_t* __restrict__ sys_dev, const Prepared prep,
                           const carl_step_io_t io, const BraxStatsPolicy pol, const int max_steps) {
  Group<K>::template run<2, MULTI, TASK, PLANAR, false, BraxStatsPolicy>(b, sys_dev, prep, io, nullptr, nullptr, max_steps, pol);
}

// max_steps == 0: the slabs of the launch shape of one step, all zeros
__global__ void __launch_bounds__(256) brax_stats_zero_kernel(double* const partial, const size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) partial[i] = 0.0;
}

}  // namespace brax
}  // namespace carl
