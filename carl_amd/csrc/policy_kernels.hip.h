// policy_kernels.hip.h -- the closed-loop fused rollout (include/carl_amd.h: carl_rollout_policy).
//
// The open-loop staged rollout (engine_kernels.hip.h: rollout_staged_body) with the loader wave replaced by a small
// fp32 MLP that every compute lane evaluates at every step.  A lane's state, its counters and its context inputs stay
// in registers for the whole launch, as in carl_rollout; the workgroup's weight set sits in LDS and is read as
// wave-uniform broadcasts (every lane of a wave reads the same 16 bytes: ds_read_b128, no bank conflicts).
//
// Per step and lane: x = [context values of the lane's current context..., observation...] -> input transform ->
// hidden layers -> head -> action (argmax / raw Box value) -> the family's unchanged step through step_lane (the
// generic done path: finish_episodes, the same arithmetic as every other kernel of the engine, so replaying the
// recorded actions with carl_rollout reproduces the transitions bit for bit).
//
// Two output modes:
//   transitions  the records go through the LdsSink and storer-wave drain of the staged rollout (drain_records), and
//                the action taken is one more [T][pitch] column, drained by the same waves;
//   summary      no per-step stores at all: each lane writes its episode count / return sum / length sum once.
// A kernel of its own (policy_episodes_kernel, carl_evaluate_policy) runs the summary layout until each lane has
// finished K episodes and writes one record per finished episode.
//
// Weights in LDS (floats, every section on a 16-byte boundary), K = the family's F + D rounded up to 4, H = the
// padded hidden width of the instantiation (0: a linear policy, else 32 or 64):
//   W1 [H][K] | b1 [H] | W2 [H][H] | b2 [H] | Wh^T [HI][4] | bh [4] | shift [K] | scale [K] | clip [4]
// HI = K when H == 0, else H.  Input slot of context input k: k (k < n_ctx); of observation entry d: F + d.  Every
// slot, row and column the policy does not use holds 0, a padded input slot is never written (0), and a padded hidden
// unit is forced to exact 0 after its activation (activate): its zero weights would turn an infinite input into NaN
// (fma(0, inf, y)), and the zero head weights would carry that NaN into every output.  So the padding changes no
// result, only the instruction count (up to the sign of a zero sum: fma(0, 0, -0) = +0).
#pragma once

#include "engine_kernels.hip.h"

namespace carl {

constexpr int kPolicyLanes = kRolloutLanes;  // lanes per workgroup = the weight-set quantum (carl_policy_lane_quantum)
constexpr int kPolicyThreadsSummary = kPolicyLanes;
constexpr int kPolicyThreadsTransitions = kPolicyLanes + kStorers * kWave;  // + the storer waves of the staged drain

// head outputs of a family: n_actions (discrete) or 1 (Box); host-validated against carl_policy_t::n_out
template <class Fam>
struct policy_outputs : std::integral_constant<int, std::is_same_v<typename Fam::Action, float> ? 1
                                                    : (std::is_same_v<Fam, CartPole> ? 2 : 3)> {};

template <class Fam, int H>
struct PolicyLayout {
  static constexpr int K = (Fam::F + Fam::D + 3) / 4 * 4;
  static constexpr int HI = H == 0 ? K : H;
  static constexpr int kW1 = 0, kB1 = kW1 + H * K, kW2 = kB1 + H, kB2 = kW2 + H * H, kWh = kB2 + H, kBh = kWh + HI * 4;
  static constexpr int kShift = kBh + 4, kScale = kShift + K, kClip = kScale + K;
  static constexpr int kFloats = kClip + 4;
  static constexpr size_t kBytes = (size_t)kFloats * sizeof(float);
};

// LDS of a sampled launch's log_prob column (LOGP): [2][chunk][256] floats, after the action column
template <bool LOGP>
__host__ __device__ constexpr size_t policy_logp_lds_bytes(int chunk) {
  return LOGP ? (size_t)2 * chunk * kPolicyLanes * 4 : 0;
}
// transitions mode: steps per LDS record buffer -- 8 like carl_rollout where the records and the action column (the
// staged rollout's buffers), the log_prob column of a sampled launch that stores one (LOGP), the largest weight set
// and the family's static tables fit a compute unit; 4 otherwise (Acrobot: 24-byte observations)
template <class Fam, bool LOGP = false>
__host__ __device__ constexpr int policy_chunk() {
  return rollout_staged_lds_bytes<Fam, 8>() + policy_logp_lds_bytes<LOGP>(8) + PolicyLayout<Fam, 64>::kBytes +
                     static_lds_bytes<Fam>() <= kCuLdsBytes ? 8 : 4;
}
template <class Fam, int H, bool SUMMARY, bool LOGP = false>
__host__ __device__ constexpr size_t policy_lds_bytes() {
  constexpr int CHUNK = policy_chunk<Fam, LOGP>();
  return PolicyLayout<Fam, H>::kBytes +
         (SUMMARY ? 0 : rollout_staged_lds_bytes<Fam, CHUNK>() + policy_logp_lds_bytes<LOGP>(CHUNK));
}

// Copy weight set `set` from its packed form (include/carl_amd.h) into the padded LDS layout; every thread of the
// workgroup, the caller synchronises.
template <class Fam, int H>
__device__ __forceinline__ void stage_policy(float* w, const carl_policy_t& pol, int set_floats, int set) {
  using L = PolicyLayout<Fam, H>;
  const float* src = pol.params + (size_t)set * set_floats;
  const int n_in = pol.n_in, n_ctx = pol.n_ctx, n_out = pol.n_out;
  const int nh = pol.n_hidden;
  const int w0 = nh > 0 ? pol.width[0] : 0, w1 = nh > 1 ? pol.width[1] : 0;
  // packed offsets of layer l = 0 .. nh (dims[l] -> dims[l + 1]; the last one is the head)
  const int dims[CARL_POLICY_MAX_HIDDEN + 2] = {n_in, nh > 0 ? w0 : n_out, nh > 1 ? w1 : n_out, n_out};
  int p_w[CARL_POLICY_MAX_HIDDEN + 1] = {0, 0, 0}, p_b[CARL_POLICY_MAX_HIDDEN + 1] = {0, 0, 0};
  int off = 0;
#pragma unroll
  for (int l = 0; l <= CARL_POLICY_MAX_HIDDEN; ++l) {
    if (l <= nh) {
      p_w[l] = off;
      off += dims[l + 1] * dims[l];
      p_b[l] = off;
      off += dims[l + 1];
    }
  }
  const int p_w0 = p_w[0], p_b0 = p_b[0], p_w1 = p_w[1], p_b1 = p_b[1];
  const int p_shift = off, p_scale = p_shift + n_in, p_clip = p_scale + n_in;
  // packed input index of LDS input slot s, or -1
  auto in_of = [&](int s) -> int {
    if (s < n_ctx) return s;
    if (s >= Fam::F && s < Fam::F + Fam::D) return n_ctx + (s - Fam::F);
    return -1;
  };
  // head layer: packed W, b and input width
  const int hw = p_w[nh], hb = p_b[nh], hin = dims[nh];
  for (int e = threadIdx.x; e < L::kFloats; e += blockDim.x) {
    float v = 0.0f;
    if (e < L::kB1) {  // W1 [H][K]
      const int j = e / L::K, s = e % L::K, i = in_of(s);
      if (j < w0 && i >= 0) v = src[p_w0 + j * n_in + i];
    } else if (e < L::kW2) {
      const int j = e - L::kB1;
      if (j < w0) v = src[p_b0 + j];
    } else if (e < L::kB2) {  // W2 [H][H]
      const int j = (e - L::kW2) / (H > 0 ? H : 1), i = (e - L::kW2) % (H > 0 ? H : 1);
      if (j < w1 && i < w0) v = src[p_w1 + j * w0 + i];
    } else if (e < L::kWh) {
      const int j = e - L::kB2;
      if (j < w1) v = src[p_b1 + j];
    } else if (e < L::kBh) {  // Wh^T [HI][4]
      const int j = (e - L::kWh) / 4, k = (e - L::kWh) % 4;
      const int i = H == 0 ? in_of(j) : (j < hin ? j : -1);
      if (k < n_out && i >= 0) v = src[hw + k * hin + i];
    } else if (e < L::kShift) {
      const int k = e - L::kBh;
      if (k < n_out) v = src[hb + k];
    } else if (e < L::kScale) {
      const int i = in_of(e - L::kShift);
      if (i >= 0) v = src[p_shift + i];
    } else if (e < L::kClip) {
      const int i = in_of(e - L::kScale);
      if (i >= 0) v = src[p_scale + i];
    } else {
      v = src[p_clip];
    }
    w[e] = v;
  }
}

typedef float pvf4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ pvf4 bcast4(const float* p) { return *reinterpret_cast<const pvf4*>(p); }

// tanh(v) = 1 - 2 / (e^{2v} + 1): v_exp_f32 + v_rcp_f32 (e^{2v} = inf for large v gives 1, 0 for very negative v -1)
__device__ __forceinline__ float tanh_fast(float v) {
#pragma clang fp contract(off)
  const float e = __expf(2.0f * v);
  return 1.0f - __fdividef(2.0f, e + 1.0f);
}

// h = act(h) on the `width` real units; the padded units [width, N) become exact 0 (one select each)
template <int N>
__device__ __forceinline__ void activate(float (&h)[N], int act, int width) {
  if (act == CARL_POLICY_TANH) {
#pragma unroll
    for (int j = 0; j < N; ++j) h[j] = tanh_fast(h[j]);
  } else if (act == CARL_POLICY_RELU) {
#pragma unroll
    for (int j = 0; j < N; ++j) h[j] = fmaxf(h[j], 0.0f);
  }
  if (width < N) {  // (wave-uniform: a full-width layer pays nothing)
#pragma unroll
    for (int j = 0; j < N; ++j) h[j] = j < width ? h[j] : 0.0f;
  }
}

// out[j] = b[j] + sum_i W[j][i] in[i] (i ascending, one fma each); W rows of IN floats at w, biases at b
template <int OUT, int IN>
__device__ __forceinline__ void dense_layer(const float* w, const float* b, const float (&in)[IN], float (&out)[OUT]) {
  static_assert(IN % 4 == 0 && OUT % 4 == 0, "LDS rows are read as float4");
#pragma unroll
  for (int j0 = 0; j0 < OUT; j0 += 4) {
    const pvf4 bb = bcast4(b + j0);
    float acc[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
    for (int i = 0; i < IN; i += 4) {
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const pvf4 ww = bcast4(w + (j0 + jj) * IN + i);
        acc[jj] = __fmaf_rn(ww.x, in[i], acc[jj]);
        acc[jj] = __fmaf_rn(ww.y, in[i + 1], acc[jj]);
        acc[jj] = __fmaf_rn(ww.z, in[i + 2], acc[jj]);
        acc[jj] = __fmaf_rn(ww.w, in[i + 3], acc[jj]);
      }
    }
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) out[j0 + jj] = acc[jj];
  }
}

// head: y[k] = bh[k] + sum_j Wh[k][j] in[j]; Wh stored transposed, one float4 = (Wh[0..3][j])
template <int IN>
__device__ __forceinline__ void head_layer(const float* wt, const float* b, const float (&in)[IN], float (&y)[4]) {
  const pvf4 bb = bcast4(b);
  y[0] = bb.x, y[1] = bb.y, y[2] = bb.z, y[3] = bb.w;
#pragma unroll
  for (int j = 0; j < IN; ++j) {
    const pvf4 ww = bcast4(wt + 4 * j);
    y[0] = __fmaf_rn(ww.x, in[j], y[0]);
    y[1] = __fmaf_rn(ww.y, in[j], y[1]);
    y[2] = __fmaf_rn(ww.z, in[j], y[2]);
    y[3] = __fmaf_rn(ww.w, in[j], y[3]);
  }
}

// x_slot = min(max((v - shift) * scale, -clip), clip); a NaN (a NaN input, or 0 * inf) becomes -clip: fmaxf returns
// the operand that is not NaN
__device__ __forceinline__ float normalize_input(float v, float shift, float scale, float clip) {
#pragma clang fp contract(off)
  return fminf(fmaxf((v - shift) * scale, -clip), clip);
}

// The policy's head outputs y[0, n_out) for input slots x (LDS layout above)
template <class Fam, int H>
__device__ __forceinline__ void policy_head(const float* w, const float (&x)[PolicyLayout<Fam, H>::K], int n_hidden,
                                            int act, int w0, int w1, float (&y)[4]) {
  using L = PolicyLayout<Fam, H>;
  if constexpr (H == 0) {
    head_layer<L::K>(w + L::kWh, w + L::kBh, x, y);
  } else {
    float h1[H];
    dense_layer<H, L::K>(w + L::kW1, w + L::kB1, x, h1);
    activate(h1, act, w0);
    if (n_hidden > 1) {  // (wave-uniform)
      float h2[H];
      dense_layer<H, H>(w + L::kW2, w + L::kB2, h1, h2);
      activate(h2, act, w1);
      head_layer<H>(w + L::kWh, w + L::kBh, h2, y);
    } else {
      head_layer<H>(w + L::kWh, w + L::kBh, h1, y);
    }
  }
}

// The policy's deterministic action for input slots x: the first maximal head output (discrete), y[0] (Box).  It keeps
// its own copy of policy_head's forward pass: calling policy_head from here moves the register allocation of the
// deterministic kernels (same results; profiles/policy_sample_isa_identity.txt holds their code unchanged).
template <class Fam, int H>
__device__ __forceinline__ typename Fam::Action policy_action(const float* w, const float (&x)[PolicyLayout<Fam, H>::K],
                                                              int n_hidden, int act, int w0, int w1) {
  using L = PolicyLayout<Fam, H>;
  float y[4];
  if constexpr (H == 0) {
    head_layer<L::K>(w + L::kWh, w + L::kBh, x, y);
  } else {
    float h1[H];
    dense_layer<H, L::K>(w + L::kW1, w + L::kB1, x, h1);
    activate(h1, act, w0);
    if (n_hidden > 1) {  // (wave-uniform)
      float h2[H];
      dense_layer<H, H>(w + L::kW2, w + L::kB2, h1, h2);
      activate(h2, act, w1);
      head_layer<H>(w + L::kWh, w + L::kBh, h2, y);
    } else {
      head_layer<H>(w + L::kWh, w + L::kBh, h1, y);
    }
  }
  if constexpr (std::is_same_v<typename Fam::Action, float>) {
    return y[0];
  } else {
    int best = 0;
    float top = y[0];
#pragma unroll
    for (int k = 1; k < policy_outputs<Fam>::value; ++k) {
      const bool gt = y[k] > top;  // first maximal index wins
      best = gt ? k : best;
      top = gt ? y[k] : top;
    }
    return best;
  }
}

// How a step's action comes from the network: ModePick, the deterministic policy (carl_rollout_policy /
// carl_evaluate_policy: policy_action), or SampledPick, whose choose() returns a sampled action and, when kLogProb, its
// log-probability in `lp`.
template <class Fam>
struct ModePick {
  static constexpr bool kSampled = false, kLogProb = false;
};

// Sampled actions (include/carl_amd.h: carl_policy_sampling_t).  The Philox block is drawn and reduced to the one
// float the rule needs (u, or the Gaussian z) BEFORE the network runs, so its four words are dead again by the time
// the hidden layers need their registers.  The counter reads the lane's episode counter, which load_staged_lane has
// fetched up front for every lane.
template <class Fam, bool LOGP>
struct SampledPick {
  static constexpr bool kSampled = true, kLogProb = LOGP;
  uint64_t seed;
  float sigma;  // Box: exp(log_std) of the workgroup's weight set
  float lp0;    // Box: -log_std - ln(2 pi) / 2

  // the workgroup's values (one weight set per workgroup: wave-uniform, scalar loads)
  static __device__ __forceinline__ SampledPick of(const carl_policy_sampling_t& smp, const carl_policy_t& pol) {
    SampledPick p{smp.seed, 1.0f, 0.0f};
    if constexpr (std::is_same_v<typename Fam::Action, float>) {
      const float ls = smp.log_std[(int)blockIdx.x * kPolicyLanes / pol.lanes_per_set];
      p.sigma = expf(ls);
      p.lp0 = -ls - 0.918938533204672742f;
    }
    return p;
  }

  template <int H>
  __device__ __forceinline__ typename Fam::Action choose(const float* w, const float (&x)[PolicyLayout<Fam, H>::K],
                                                         int n_hidden, int act, int w0, int w1, uint64_t glane,
                                                         const LaneRegs<Fam>& r, float& lp) const {
#pragma clang fp contract(off)
    const u32x4 wd = lane_words(seed, glane, r.episode - 1u, kSubSample | (uint32_t)r.elapsed);
    float y[4];
    if constexpr (std::is_same_v<typename Fam::Action, float>) {
      const float z = normal_from_words(wd.x, wd.y);
      policy_head<Fam, H>(w, x, n_hidden, act, w0, w1, y);
      if constexpr (LOGP) lp = __fmaf_rn(-0.5f * z, z, lp0);
      return __fmaf_rn(sigma, z, y[0]);
    } else {
      constexpr int NA = policy_outputs<Fam>::value;
      const float u = u01(wd.x);
      policy_head<Fam, H>(w, x, n_hidden, act, w0, w1, y);
      float m = y[0];
#pragma unroll
      for (int k = 1; k < NA; ++k) m = fmaxf(m, y[k]);
      float c[NA];  // prefix sums of exp(y_k - m); c[NA - 1] = S
      float s = 0.0f;
#pragma unroll
      for (int k = 0; k < NA; ++k) c[k] = s = s + expf(y[k] - m);
      const float t = u * s;
      int a = NA - 1;
      float ya = y[NA - 1];
#pragma unroll
      for (int k = NA - 2; k >= 0; --k) {  // the first k with t < c_k
        const bool in = t < c[k];
        a = in ? k : a;
        ya = in ? y[k] : ya;
      }
      if constexpr (LOGP) lp = (ya - m) - logf(s);
      return a;
    }
  }
};

// summary mode's sink: step_lane writes nothing anywhere (flags are lazy: only the done path would write them)
template <class Fam>
struct NullSink {
  static constexpr bool kLazyFlags = true;
  __device__ __forceinline__ void put_reward(float) const {}
  __device__ __forceinline__ void put_flags(bool, bool) const {}
  __device__ __forceinline__ void put_obs(const float (&)[Fam::D]) const {}
  __device__ __forceinline__ float* final_obs_ptr() const { return nullptr; }
};

// storer wave `which`: the action column of steps [t0, t0 + steps), one 1 KiB row piece per step (as drain_records)
__device__ __forceinline__ void drain_actions(const char* buf, void* action, size_t n, int cols, int lane_base, int l,
                                              int which, int t0, int steps) {
  const int valid = min(kPolicyLanes, cols - lane_base);  // a multiple of 16
  for (int u = which; u < steps; u += kStorers) {
    const char* src = buf + (size_t)u * kPolicyLanes * 4 + 16 * l;
    char* dst = reinterpret_cast<char*>(action) + ((size_t)(t0 + u) * n + lane_base) * 4 + 16 * l;
    if (4 * l < valid) __builtin_nontemporal_store(*reinterpret_cast<const pvf4*>(src), reinterpret_cast<pvf4*>(dst));
  }
}

// Preconditions (host, carl_policy.hip): a classic family; the policy validated against it; SUMMARY or a staged row
// layout (pitch % 16 == 0, 16-byte aligned arrays); lanes_per_set % kPolicyLanes == 0 and n_sets * lanes_per_set >= n_lanes.
template <class Fam, int H, bool SUMMARY>
__global__ void __launch_bounds__(SUMMARY ? kPolicyThreadsSummary : kPolicyThreadsTransitions)
    policy_rollout_kernel(const carl_batch_t b, const carl_step_io_t io, const carl_policy_t pol, const int set_floats,
                          const carl_policy_summary_t sum, const int n_steps) {
  using Pick = ModePick<Fam>;
  const Pick pick{};
  float* const log_prob = nullptr;
#include "policy_rollout_body.inc"
}

// carl_rollout_policy_sampled (carl_policy_sample.hip); LOGP: transitions mode with the log_prob column
template <class Fam, int H, bool SUMMARY, bool LOGP>
__global__ void __launch_bounds__(SUMMARY ? kPolicyThreadsSummary : kPolicyThreadsTransitions)
    policy_rollout_sampled_kernel(const carl_batch_t b, const carl_step_io_t io, const carl_policy_t pol,
                                  const int set_floats, const carl_policy_summary_t sum, const int n_steps,
                                  const carl_policy_sampling_t smp) {
  static_assert(!(SUMMARY && LOGP), "a summary stores no per-step column");
  using Pick = SampledPick<Fam, LOGP>;
  const Pick pick = Pick::of(smp, pol);
  float* const log_prob = smp.log_prob;
#include "policy_rollout_body.inc"
}

// episodes mode's sink: no per-step store; put_flags keeps the terminated bit in the caller's register.  kLazyFlags:
// step_lane calls put_flags on the done path only, and the constant also selects finish_episodes' Philox predraw path,
// so the reset draws are those of every other kernel.
template <class Fam>
struct TermSink {
  static constexpr bool kLazyFlags = true;
  bool* te;
  __device__ __forceinline__ void put_reward(float) const {}
  __device__ __forceinline__ void put_flags(bool t, bool) const { *te = t; }
  __device__ __forceinline__ void put_obs(const float (&)[Fam::D]) const {}
  __device__ __forceinline__ float* final_obs_ptr() const { return nullptr; }
};

// episodes mode without input statistics: the body's `if constexpr (Stats::kOn)` statements are discarded, no code
// (policy_stats_kernels.hip.h: InputStats gathers them, in a kernel of its own)
template <class Fam, int H>
struct NoInputStats {
  static constexpr bool kOn = false;
};

// Episodes mode (include/carl_amd.h: carl_evaluate_policy): the summary instantiation's layout -- 256 threads, four
// compute waves, one weight set in LDS, no storer waves -- with a per-lane `live` predicate.  A lane is live while it
// has finished fewer than K episodes and taken fewer than max_steps steps; the step runs through step_lane's
// active_in path, so a frozen lane's registers stay as they are while it still takes part in the wave-level
// operations inside (the done ballot, the finished-episode log's ballot + atomic).  Padding lanes are never live.
// There is no barrier in the step loop: a wave leaves it as soon as none of its lanes is live, checked every step.
// Each finished episode is written straight to row `done_eps` of the record arrays; the sentinels once, at the end.
// Preconditions (host, carl_policy.hip): as policy_rollout_kernel's summary mode; K >= 1; K * n_lanes < 2^31.
template <class Fam, int H>
__global__ void __launch_bounds__(kPolicyThreadsSummary)
    policy_episodes_kernel(const carl_batch_t b, const carl_policy_t pol, const int set_floats,
                           const carl_policy_episodes_t ep, const int n_episodes, const int max_steps) {
  using Pick = ModePick<Fam>;
  const Pick pick{};
  using Stats = NoInputStats<Fam, H>;
  [[maybe_unused]] Stats istats;
#include "policy_episodes_body.inc"
}

// carl_evaluate_policy_sampled (carl_policy_sample.hip)
template <class Fam, int H>
__global__ void __launch_bounds__(kPolicyThreadsSummary)
    policy_episodes_sampled_kernel(const carl_batch_t b, const carl_policy_t pol, const int set_floats,
                                   const carl_policy_episodes_t ep, const int n_episodes, const int max_steps,
                                   const carl_policy_sampling_t smp) {
  using Pick = SampledPick<Fam, false>;
  const Pick pick = Pick::of(smp, pol);
  using Stats = NoInputStats<Fam, H>;
  [[maybe_unused]] Stats istats;
#include "policy_episodes_body.inc"
}

}  // namespace carl
