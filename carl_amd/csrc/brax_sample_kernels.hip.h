// brax_sample_kernels.hip.h -- sampled actions and their log-probabilities inside the Brax closed-loop rollout
// (include/carl_amd.h: carl_brax_rollout_policy_sampled): the policy type that selects the variant in Group<K>::run
// (brax_kernels.hip.h: Pol::kSampled, beside Pol::kEpisodes / Pol::kStats), the hook BraxPolicy::act
// (brax_policy_kernels.hip.h) hands the head's outputs to, and the kernel around them.  The network, the step, the
// records, the summary mode and the fragment hand-over are the deterministic twin's (brax_policy_kernels.hip.h), and so
// are the launch shape and the LDS: nothing is added to policy_layout_of.
//
// A diagonal Gaussian over the model's actuators, mean the head's outputs, one state-independent log_std per weight set
// and actuator.  Where:
//   head layer         the lane that computes head unit u draws Philox block u >> 1 of the env-step itself -- counter
//                      (genv lo, genv hi, episode counter - 1, 0x40000000 | (u >> 1) << 28 | elapsed), all of it in the
//                      lane's registers at the top of the step -- BEFORE the row's products and reduces it at once to
//                      z_u, the one float it needs (the four words are dead again while the products run); behind the
//                      products it leaves a_u = fma(exp(log_std_u), z_u, mu_u) where the deterministic head leaves mu_u
//                      (the env's io row, io->action) and lp_u in row u of the policy rows that are dead by then: the
//                      h2 rows with one hidden layer, the h1 rows otherwise.
//   behind the head layer's hand-over (the phase_sync that is there anyway)
//                      the env's first lane sums lp_0 .. lp_{n_act - 1} in index order and stores log_prob[t][env],
//                      behind the wavefront-uniform branch of the other per-step stores; log_prob == NULL is a
//                      wavefront-uniform runtime branch too, not a second set of instances.
// Two lanes that share a block (actuators 2k and 2k + 1 on different lanes: kSub > 1) each run its ten rounds; one draw and
// a hand-over through LDS would cost a phase_sync per step for a few dozen integer multiplies.  An env past the end of the
// batch is not `active`: it draws nothing and stores nothing.  A draw is a function of the env's own counters, so the
// tail fragment of a split group continues the stream of its head, and the summary launch takes the transitions launch's
// actions.
#pragma once

#include "brax_policy_kernels.hip.h"

namespace carl {
namespace brax {

constexpr uint32_t kSubBraxSample = 0x40000000u;  // | block << 28 | elapsed (the reset draws: 0x80000000 | block, draw_u)

// BraxPolicy::layer's hook on the head: one per act() call
struct GaussianHead {
  static constexpr bool kOn = true;
  uint64_t seed, genv;
  uint32_t episode;      // the index of the episode the step belongs to
  uint32_t tag;          // kSubBraxSample | elapsed
  const float* log_std;  // the row of the env's weight set
  int lp_row;            // the first of the n_act dead policy rows that take lp_u

  __device__ __forceinline__ float draw(int u) const {
    const u32x4 wd = lane_words(seed, genv, episode, tag | ((uint32_t)(u >> 1) << 28));
    const bool odd = (u & 1) != 0;
    return normal_from_words(odd ? wd.z : wd.x, odd ? wd.w : wd.y);
  }
  template <class LdsT>
  __device__ __forceinline__ float action(const LdsT& m, int u, float mu, float z) const {
#pragma clang fp contract(off)
    const float ls = log_std[u];
    m.at(lp_row + u) = __fmaf_rn(-0.5f * z, z, -ls - 0.918938533204672742f);
    return __fmaf_rn(expf(ls), z, mu);
  }
};

struct BraxSampledPolicy : BraxPolicy {
  static constexpr bool kSampled = true;
  uint64_t seed;         // sample_seed
  const float* log_std;  // [n_sets][n_act]; validated by the host (carl_brax_policy_sample.hip)
  float* log_prob;       // [T][n_lanes], or NULL

  // BraxPolicy::act with the Gaussian head.  genv / episode / elapsed: the env's global index, episode counter and step
  // count in its episode, as run() holds them at the top of the step; log_prob[lp_at] takes the step's log-probability
  // when `per_step` (wavefront-uniform) and there is a log_prob array.  `use`: act()'s hook behind the input phase.
  template <int kSub, class LdsT, class Use = NoInputUse>
  __device__ __forceinline__ void act_sampled(const LdsT& m, int rows, const carl_batch_t& b, int cidx, int env, bool active,
                                              uint64_t genv, uint32_t episode, int elapsed, int obs_dim, int n_act,
                                              float* __restrict__ action_out, bool per_step, size_t lp_at,
                                              const Use& use = Use()) const {
    const int lp_row = rows + kPolicyXRows + (p.n_hidden == 1 ? kPolicyHRows : 0);
    const GaussianHead head{seed, genv, episode - 1u, kSubBraxSample | (uint32_t)elapsed,
                            log_std + (size_t)(active ? env / p.lanes_per_set : 0) * n_act, lp_row};
    this->template act<kSub>(m, rows, b, cidx, env, active, obs_dim, n_act, action_out, NoInputTap(), head, use);
    if (per_step && log_prob != nullptr) {
      if (active && m.sub == 0) {
#pragma clang fp contract(off)
        float lp = m.at(lp_row);
        for (int j = 1; j < n_act; ++j) lp += m.at(lp_row + j);
        log_prob[lp_at] = lp;
      }
    }
  }
};

// brax_policy_kernel's sampled twin, one instance per instance of it.
template <bool MULTI, int K, bool TASK = false, bool PLANAR = false>
__global__ void __launch_bounds__(kLanes * max_waves_per_wg(TASK)) __attribute__((amdgpu_waves_per_eu(CARL_BRAX_WAVES_PER_EU(TASK))))
brax_policy_sampled_kernel(const carl_batch_t b, const carl_brax_sys_t* __restrict__ sys_dev, const Prepared prep,
                           const carl_step_io_t io, const BraxSampledPolicy pol, const int n_steps) {
  Group<K>::template run<2, MULTI, TASK, PLANAR, false, BraxSampledPolicy>(b, sys_dev, prep, io, nullptr, nullptr, n_steps, pol);
}

}  // namespace brax
}  // namespace carl
