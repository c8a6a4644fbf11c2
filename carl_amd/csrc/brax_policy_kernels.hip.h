// brax_policy_kernels.hip.h -- the policy of the Brax closed-loop rollout (include/carl_amd.h: carl_brax_rollout_policy):
// what Group<K>::run's MODE 2 (brax_kernels.hip.h) calls at the top of every env step, and the kernel around it.
//
// The network and its arithmetic are carl_rollout_policy's (include/carl_amd.h; policy_kernels.hip.h: normalize_input,
// activate, tanh_fast -- called here, not restated): x = [context values of the env's current context, observation] ->
// input transform -> hidden layers -> linear head, every product an explicit fma in input order, bias first.  What
// differs is where it runs.  A classic-control lane evaluates the whole network in its own registers from a weight set
// its workgroup staged in LDS.  A Brax env is kSub lanes of a wavefront whose step code already exchanges everything
// through per-env LDS rows, so the env's lanes SPLIT each layer: lane `sub` computes output units sub, sub + kSub, ... from
// the layer's input rows and writes them to the layer's output rows, a phase_sync hands over to the next layer.  The rows
// are the kPolicyRows that policy_layout_of adds behind the step's: x [32] | h1 [64] | h2 [64] (| the summary totals).
//
// Weights stay in global memory, in the packed form the host passes (no padding, no transposition), and are read through
// the vector cache 16 bytes at a time: a wavefront's 64 / K envs straddle weight-set boundaries (lanes_per_set is a
// multiple of 256 envs, 64 / K divides nothing), and under the balanced fragment schedule a workgroup runs many groups, so
// a workgroup has no one weight set to stage.  A packed row W[u][.] starts wherever the rows before it end, not on a
// 16-byte boundary: the lane reads the aligned 16-byte pieces that cover the row (the block of a set is 16-byte aligned
// and padded to a multiple of four floats, so every piece lies inside it); in the first and the last piece a select
// keeps the accumulator where an element belongs to a neighbouring row, the pieces in between are four plain fmas -- the
// row's own elements are added in input order, exactly once.
#pragma once

#include "brax_kernels.hip.h"
#include "classic_control.hip.h"
#include "policy_kernels.hip.h"

namespace carl {
namespace brax {

// act()'s tap on the raw inputs: none.  brax_stats_kernels.hip.h has the one that gathers input statistics.
struct NoInputTap {
  static constexpr bool kOn = false;
};

// act()'s hook on the head's outputs: none, the action is the head's outputs as they come.  brax_sample_kernels.hip.h has
// the one that draws a Gaussian action around them.
struct PlainHead {
  static constexpr bool kOn = false;
};

// act()'s hook between the input phase and the layers: none.  brax_value_kernels.hip.h has the one that evaluates a
// critic on the x rows there, while the h1 / h2 rows are still dead.
struct NoInputUse {
  static constexpr bool kOn = false;
};

struct BraxPolicy {
  static constexpr bool kEpisodes = false;  // (run(): not the episodes variant -- brax_episodes_kernels.hip.h)
  static constexpr bool kStats = false;     // (nor its statistics variant -- brax_stats_kernels.hip.h)
  static constexpr bool kSampled = false;   // (nor the sampled variant -- brax_sample_kernels.hip.h)
  static constexpr bool kValued = false;    // (nor its valued variant -- brax_value_kernels.hip.h)
  carl_policy_t p;            // validated by the host (carl_brax_policy.hip)
  int set_floats;             // floats per packed weight set
  carl_policy_summary_t sum;  // per-env totals; all NULL: none
  float* cur_obs;             // [N][obs_dim] the envs' current observation, in and out

  // out rows [out_row, out_row + n_out) = act(b + W in), W [n_out][n_in] row-major at w + p_w, b at w + p_b; lane `sub`
  // of the env computes units sub, sub + kSub, ...  ACT: the hidden activation is applied; else (the head) the unit is
  // also stored to gout[u] when gout != NULL -- with a `head` (Head::kOn) what is put and stored is head.action(u, unit),
  // for which the lane calls head.draw(u) before the row's products.
  template <int kSub, bool ACT, class LdsT, class Head = PlainHead>
  __device__ __forceinline__ void layer(const LdsT& m, const float* __restrict__ w, int p_w, int p_b, int n_in, int n_out,
                                        int in_row, int out_row, bool active, float* __restrict__ gout,
                                        const Head& head = Head()) const {
    if (active) {
      for (int u = m.sub; u < n_out; u += kSub) {
        [[maybe_unused]] float drawn = 0.0f;
        if constexpr (Head::kOn) drawn = head.draw(u);
        float acc = w[p_b + u];
        const int a = p_w + u * n_in, end = a + n_in;  // the row's floats [a, end); its aligned pieces start at a & ~3
        // a piece that reaches into a neighbouring row (the first and the last one may): a select per element
        auto edge_piece = [&](int e) {
          const pvf4 ww = *reinterpret_cast<const pvf4*>(w + e);
          const float wv[4] = {ww.x, ww.y, ww.z, ww.w};
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int i = e + c - a;
            const bool own = (unsigned)i < (unsigned)n_in;  // (an element of the row before or after: not added)
            const float f = __fmaf_rn(wv[c], m.at(in_row + (own ? i : 0)), acc);
            acc = own ? f : acc;
          }
        };
        int e = a & ~3;
        if (e < a) {
          edge_piece(e);
          e += 4;
        }
        for (; e + 4 <= end; e += 4) {  // the pieces inside the row: four fmas per 16 bytes, input rows at constant offsets
          const pvf4 ww = *reinterpret_cast<const pvf4*>(w + e);
          const int i = e - a;
          acc = __fmaf_rn(ww.x, m.at(in_row + i), acc);
          acc = __fmaf_rn(ww.y, m.at(in_row + i + 1), acc);
          acc = __fmaf_rn(ww.z, m.at(in_row + i + 2), acc);
          acc = __fmaf_rn(ww.w, m.at(in_row + i + 3), acc);
        }
        if (e < end) edge_piece(e);
        if constexpr (ACT) {
          float h[1] = {acc};
          activate(h, p.activation, 1);
          m.at(out_row + u) = h[0];
        } else {
          if constexpr (Head::kOn) acc = head.action(m, u, acc, drawn);
          m.at(out_row + u) = acc;
          if (gout != nullptr) gout[u] = acc;
        }
      }
    }
    Group<kSub>::phase_sync();
  }

  // The env's io rows hold its observation [obs_dim]: leave its action [n_act] there, and in action_out[0, n_act) when
  // that is not NULL.  `rows`: the first of the env's policy rows; cidx: the env's current context.  Wavefront-uniform call.
  // `tap` (Tap::kOn): sees every raw input beside its shift where the first phase normalises it, marks the env before that
  // phase's hand-over and gathers behind it, while h2 and the summary-total rows are still dead.
  // `head` (Head::kOn): the head layer's hook, see layer().
  // `use` (Use::kOn): runs behind the first phase's hand-over, when the x rows hold the transformed inputs and before the
  // layers write h1 / h2; it may use h1, h2 and the fourth summary-total row and must end on a phase_sync.
  template <int kSub, class LdsT, class Tap = NoInputTap, class Head = PlainHead, class Use = NoInputUse>
  __device__ __forceinline__ void act(const LdsT& m, int rows, const carl_batch_t& b, int cidx, int env, bool active,
                                      int obs_dim, int n_act, float* __restrict__ action_out, const Tap& tap = Tap(),
                                      const Head& head = Head(), const Use& use = Use()) const {
    const int X = rows, H1 = rows + kPolicyXRows, H2 = H1 + kPolicyHRows;
    const int n_in = p.n_in, n_ctx = p.n_ctx, nh = p.n_hidden;
    const int w0 = nh > 0 ? p.width[0] : 0, w1 = nh > 1 ? p.width[1] : 0;
    // packed offsets (include/carl_amd.h): per layer W then b; then shift | scale | clip
    const int d1 = nh > 0 ? w0 : n_act, d2 = nh > 1 ? w1 : n_act;
    const int p_w0 = 0, p_b0 = d1 * n_in;
    const int p_w1 = p_b0 + d1, p_b1 = p_w1 + (nh > 0 ? d2 * d1 : 0);
    const int p_w2 = p_b1 + (nh > 0 ? d2 : 0), p_b2 = p_w2 + (nh > 1 ? n_act * d2 : 0);
    const int p_shift = p_b2 + (nh > 1 ? n_act : 0), p_scale = p_shift + n_in, p_clip = p_scale + n_in;
    // (an env past the end of the batch reads nothing: its set index may lie past the last set)
    const float* __restrict__ w = p.params + (size_t)(active ? env / p.lanes_per_set : 0) * set_floats;
    if (active) {
      const float clip = w[p_clip];
      for (int k = 0; k < n_ctx; ++k)  // (wavefront-uniform k: the row index is a scalar load from the kernel arguments)
        if (m.sub == k % kSub) {
          const float raw = b.ctx_table[(size_t)p.ctx_rows[k] * b.ctx_stride + cidx];
          m.at(X + k) = normalize_input(raw, w[p_shift + k], w[p_scale + k], clip);
          if constexpr (Tap::kOn) tap.put(m, H2 + k, raw, w[p_shift + k]);
        }
      for (int d = m.sub; d < obs_dim; d += kSub) {
        const float raw = m.at(m.lay.io + d);
        m.at(X + n_ctx + d) = normalize_input(raw, w[p_shift + n_ctx + d], w[p_scale + n_ctx + d], clip);
        if constexpr (Tap::kOn) tap.put(m, H2 + n_ctx + d, raw, w[p_shift + n_ctx + d]);
      }
    }
    if constexpr (Tap::kOn) tap.mark(m, H2 + kPolicyHRows);
    Group<kSub>::phase_sync();
    if constexpr (Tap::kOn) tap.template gather<kSub>(m, H2, H2 + kPolicyHRows, n_in);
    if constexpr (Use::kOn) use.template run<kSub>(m, X, active);
    if (nh == 0) {
      layer<kSub, false>(m, w, p_w0, p_b0, n_in, n_act, X, m.lay.io, active, action_out, head);
    } else {
      layer<kSub, true>(m, w, p_w0, p_b0, n_in, w0, X, H1, active, nullptr);
      if (nh > 1) {
        layer<kSub, true>(m, w, p_w1, p_b1, w0, w1, H1, H2, active, nullptr);
        layer<kSub, false>(m, w, p_w2, p_b2, w1, n_act, H2, m.lay.io, active, action_out, head);
      } else {
        layer<kSub, false>(m, w, p_w1, p_b1, w0, n_act, H1, m.lay.io, active, action_out, head);
      }
    }
  }
};

// brax_kernel's closed-loop twin: MODE 2 of the same run().  Never F32 (the host refuses CARL_FLAG_BRAX_FP32).
template <bool MULTI, int K, bool TASK = false, bool PLANAR = false>
__global__ void __launch_bounds__(kLanes * max_waves_per_wg(TASK)) __attribute__((amdgpu_waves_per_eu(CARL_BRAX_WAVES_PER_EU(TASK))))
brax_policy_kernel(const carl_batch_t b, const carl_brax_sys_t* __restrict__ sys_dev, const Prepared prep,
                   const carl_step_io_t io, const BraxPolicy pol, const int n_steps) {
  Group<K>::template run<2, MULTI, TASK, PLANAR, false, BraxPolicy>(b, sys_dev, prep, io, nullptr, nullptr, n_steps, pol);
}

}  // namespace brax
}  // namespace carl
