// brax_value_kernels.hip.h -- a critic inside the sampled Brax closed-loop rollout (include/carl_amd.h:
// carl_brax_rollout_policy_valued): the policy type that selects the variant in Group<K>::run (brax_kernels.hip.h:
// Pol::kValued, beside Pol::kSampled), the hook BraxPolicy::act (brax_policy_kernels.hip.h) runs behind its input phase,
// and the kernel around them.  The actor, its draws, the step, the records and the fragment hand-over are the sampled
// twin's (brax_sample_kernels.hip.h), and so are the launch shape and the LDS: nothing is added to policy_layout_of.
//
// The critic is a second packed network of one output that reads the actor's transformed inputs, the x rows.  Its layers
// are BraxPolicy::layer's, split over the env's lanes as the actor's are, with the critic's block and activation; they
// use the h1 / h2 rows, which are dead outside act()'s layers (the log-probability terms a sampled head leaves there are
// summed before act_sampled returns), and the head's one unit lands in the fourth summary-total row: rows 0 - 2 hold the
// totals of a transitions launch with a summary, row 0 the statistics tap's mark in the episodes mode, row 3 is written
// by no other mode.  Where:
//   value       in the step, behind the input phase's hand-over and before the actor's layers write h1 / h2: the order
//               changes no actor result.  Three more phase_syncs per step (one per critic layer).
//   boot_value  in run()'s done block, under a wavefront-uniform ballot of the envs a step truncated alone, before the
//               io rows are rewritten: the terminal observation is normalised into the observation part of the x rows,
//               whose context part still holds the episode's values.
//   last_value  behind the step loop of the fragment that ran the launch's last step, on the env's current context
//               (r.cidx, after any reset of that step) and the observation in the io rows.
// The two cold sites share one function that is NOT inlined, so that the step loop's registers do not carry them; it takes
// scalars and pointers only (a reference to the kernel's policy argument would put a copy of it in scratch memory).
#pragma once

#include "brax_sample_kernels.hip.h"

namespace carl {
namespace brax {

// what BraxPolicy::layer needs of the lane's LDS view, for code that is not inlined into run(): the float rows and the
// lane's coordinates.  The rows as an LDS pointer, not a generic one: the function then addresses LDS as run() does, and
// no generic pointer to LDS is built at the call (whose null check the gfx950 back end of ROCm's clang stops at:
// "V_CMP_NE_U32 0, $src_shared_base: illegal operand", as brax_kernels.hip.h notes for the episodes mode's stores).
typedef __attribute__((address_space(3))) float lds_float;
template <int kEnvs>
struct RowView {
  lds_float* base;
  int env, sub;
  __device__ __forceinline__ lds_float& at(int row) const { return base[row * kEnvs + env]; }
};

// The critic's layers on the x rows [X, X + n_in) -> V in the fourth summary-total row, and in dst[0] when `go` (the
// env's first lane stores it).  w: the block of the env's critic set; act / nh / w0 / w1: its activation and hidden
// layers.  Wavefront-uniform call; ends on a phase_sync.
template <int kSub, class LdsT>
__device__ __forceinline__ void critic_layers(const LdsT& m, int X, const float* __restrict__ w, int act, int n_in, int nh,
                                              int w0, int w1, bool go, float* __restrict__ dst) {
  BraxPolicy net{};  // (layer() reads the activation alone)
  net.p.activation = act;
  const int H1 = X + kPolicyXRows, H2 = H1 + kPolicyHRows, V = H2 + kPolicyHRows + 3;
  // packed offsets (include/carl_amd.h): per layer W then b, the head one row
  const int d1 = nh > 0 ? w0 : 1, d2 = nh > 1 ? w1 : 1;
  const int p_w0 = 0, p_b0 = d1 * n_in;
  const int p_w1 = p_b0 + d1, p_b1 = p_w1 + (nh > 0 ? d2 * d1 : 0);
  const int p_w2 = p_b1 + (nh > 0 ? d2 : 0), p_b2 = p_w2 + (nh > 1 ? d2 : 0);
  if (nh == 0) {
    net.template layer<kSub, false>(m, w, p_w0, p_b0, n_in, 1, X, V, go, dst);
  } else {
    net.template layer<kSub, true>(m, w, p_w0, p_b0, n_in, w0, X, H1, go, nullptr);
    if (nh > 1) {
      net.template layer<kSub, true>(m, w, p_w1, p_b1, w0, w1, H1, H2, go, nullptr);
      net.template layer<kSub, false>(m, w, p_w2, p_b2, w1, 1, H2, V, go, dst);
    } else {
      net.template layer<kSub, false>(m, w, p_w1, p_b1, w0, 1, H1, V, go, dst);
    }
  }
}

// The cold sites' shared body: the observation in rows [io, io + obs_dim) -> the observation part of the x rows by the
// actor's transform (xf: the shift | scale | clip section of the env's actor set), then the critic.
template <int kSub, int kEnvs>
__device__ __noinline__ void critic_on_io(lds_float* base, int env_w, int sub, int io, int X, int obs_dim, int n_ctx, int n_in,
                                          const float* __restrict__ xf, const float* __restrict__ w, int act, int nh, int w0,
                                          int w1, bool go, float* __restrict__ dst) {
  const RowView<kEnvs> m{base, env_w, sub};
  if (go) {
    const float clip = xf[2 * n_in];
    for (int d = sub; d < obs_dim; d += kSub)
      m.at(X + n_ctx + d) = normalize_input(m.at(io + d), xf[n_ctx + d], xf[n_in + n_ctx + d], clip);
  }
  Group<kSub>::phase_sync();
  critic_layers<kSub>(m, X, w, act, n_in, nh, w0, w1, go, dst);
}

struct BraxValuedPolicy : BraxSampledPolicy {
  static constexpr bool kValued = true;
  carl_policy_t critic;  // validated by the host (carl_brax_policy_value.hip); its shift | scale | clip section is not read
  int critic_set_floats;
  int xf_at;             // where the actor's shift | scale | clip section begins in its packed set
  float* value;          // [T][n_lanes]
  float* last_value;     // [n_lanes]
  float* boot_value;     // [T][n_lanes], or NULL

  // (an env past the end of the batch reads nothing: its set index may lie past the last set)
  __device__ __forceinline__ const float* critic_set(int env, bool go) const {
    return critic.params + (size_t)(go ? env / critic.lanes_per_set : 0) * critic_set_floats;
  }

  // act()'s hook behind the input phase: the critic on the step's inputs
  struct StepValue {
    static constexpr bool kOn = true;
    const BraxValuedPolicy& pol;
    int env;
    float* dst;  // value[t][env], or NULL
    template <int kSub, class LdsT>
    __device__ __forceinline__ void run(const LdsT& m, int X, bool active) const {
      // The layer sizes, opaque to the optimiser inside the step loop: as loop invariants their products (the packed
      // offsets, the rows' piece bounds) are computed ahead of the loop and kept in registers all through the step.
      int n_in = pol.critic.n_in, nh = pol.critic.n_hidden;
      int w0 = nh > 0 ? pol.critic.width[0] : 0, w1 = nh > 1 ? pol.critic.width[1] : 0;
      asm volatile("" : "+s"(n_in), "+s"(nh), "+s"(w0), "+s"(w1));
      critic_layers<kSub>(m, X, pol.critic_set(env, active), pol.critic.activation, n_in, nh, w0, w1, active, dst);
    }
  };

  // BraxSampledPolicy::act_sampled with the critic behind the input phase (run() calls the policy's act_sampled: this one
  // for a valued policy); value[lp_at] takes V when `per_step`.
  template <int kSub, class LdsT>
  __device__ __forceinline__ void act_sampled(const LdsT& m, int rows, const carl_batch_t& b, int cidx, int env, bool active,
                                              uint64_t genv, uint32_t episode, int elapsed, int obs_dim, int n_act,
                                              float* __restrict__ action_out, bool per_step, size_t lp_at) const {
    const StepValue use{*this, env, per_step ? value + lp_at : nullptr};
    BraxSampledPolicy::template act_sampled<kSub>(m, rows, b, cidx, env, active, genv, episode, elapsed, obs_dim, n_act,
                                                  action_out, per_step, lp_at, use);
  }

  // the context part of the env's x rows <- the transformed values of context cidx (act()'s input phase writes the same)
  template <int kSub, class LdsT>
  __device__ __forceinline__ void put_context(const LdsT& m, int rows, const carl_batch_t& b, int cidx, int env,
                                              bool go) const {
    if (go) {
      const float* __restrict__ xf = p.params + (size_t)(env / p.lanes_per_set) * set_floats + xf_at;
      const float clip = xf[2 * p.n_in];
      for (int k = 0; k < p.n_ctx; ++k)
        if (m.sub == k % kSub)
          m.at(rows + k) = normalize_input(b.ctx_table[(size_t)p.ctx_rows[k] * b.ctx_stride + cidx], xf[k], xf[p.n_in + k],
                                           clip);
    }
  }

  // V of [the context part of the env's x rows as it is, the observation in the env's io rows] -> dst[0], for the envs
  // with `go`.  Wavefront-uniform call; ends on a phase_sync.
  template <int kSub, class LdsT>
  __device__ __forceinline__ void value_of_io(const LdsT& m, int rows, int env, bool go, int obs_dim, float* dst) const {
    const float* xf = p.params + (size_t)(go ? env / p.lanes_per_set : 0) * set_floats + xf_at;
    critic_on_io<kSub, Group<kSub>::kEnvs>((lds_float*)m.base, m.env, m.sub, m.lay.io, rows, obs_dim, p.n_ctx, p.n_in, xf, critic_set(env, go),
                                      critic.activation, critic.n_hidden, critic.n_hidden > 0 ? critic.width[0] : 0,
                                      critic.n_hidden > 1 ? critic.width[1] : 0, go, dst);
  }
};

// brax_policy_sampled_kernel's valued twin, one instance per instance of it.
template <bool MULTI, int K, bool TASK = false, bool PLANAR = false>
__global__ void __launch_bounds__(kLanes * max_waves_per_wg(TASK)) __attribute__((amdgpu_waves_per_eu(CARL_BRAX_WAVES_PER_EU(TASK))))
brax_policy_valued_kernel(const carl_batch_t b, const carl_brax_sys_t* __restrict__ sys_dev, const Prepared prep,
                          const carl_step_io_t io, const BraxValuedPolicy pol, const int n_steps) {
  Group<K>::template run<2, MULTI, TASK, PLANAR, false, BraxValuedPolicy>(b, sys_dev, prep, io, nullptr, nullptr, n_steps, pol);
}

}  // namespace brax
}  // namespace carl
