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

// transitions mode: steps per LDS record buffer -- 8 like carl_rollout where the records and the action column (the
// staged rollout's buffers), the largest weight set and the family's static tables fit a compute unit; 4 otherwise
// (Acrobot: 24-byte observations)
template <class Fam>
__host__ __device__ constexpr int policy_chunk() {
  return rollout_staged_lds_bytes<Fam, 8>() + PolicyLayout<Fam, 64>::kBytes + static_lds_bytes<Fam>() <= kCuLdsBytes ? 8 : 4;
}
template <class Fam, int H, bool SUMMARY>
__host__ __device__ constexpr size_t policy_lds_bytes() {
  return PolicyLayout<Fam, H>::kBytes + (SUMMARY ? 0 : rollout_staged_lds_bytes<Fam, policy_chunk<Fam>()>());
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

// The policy's action for input slots x (LDS layout above)
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
  using L = PolicyLayout<Fam, H>;
  using SK = LdsSink<Fam>;
  using Action = typename Fam::Action;
  constexpr int CHUNK = policy_chunk<Fam>();
  extern __shared__ float lds_dyn[];
  stage_family_tables<Fam>();
  float* const wts = lds_dyn;
  char* const out_buf = reinterpret_cast<char*>(lds_dyn) + L::kBytes;         // [2][CHUNK] records (transitions)
  char* const act_buf = out_buf + (size_t)2 * CHUNK * SK::kStepBytes;         // [2][CHUNK][256] actions
  const int lane_base = (int)blockIdx.x * kPolicyLanes;
  stage_policy<Fam, H>(wts, pol, set_floats, lane_base / pol.lanes_per_set);
  const GlobalCtx ctx{b.ctx_table, b.ctx_stride};
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const bool compute = wave < kPolicyLanes / kWave;
  const int hl = threadIdx.x % kWave;
  const int storer = wave - kPolicyLanes / kWave;
  const int lane = lane_base + (compute ? (int)threadIdx.x : 0);
  const bool active = compute && lane < b.n_lanes;
  const uint64_t glane = (uint64_t)(b.lane_offset + lane);
  const size_t n = (size_t)io.row_pitch;
  const int n_cols = (b.n_lanes + 15) & ~15;
  if (!SUMMARY && !compute) zero_flag_rows<Fam, CHUNK>(out_buf, hl, storer);
  __syncthreads();

  if (compute) {
    LaneRegs<Fam> r{};
    load_staged_lane<Fam>(b, ctx, lane, active, r);
    float* const final_base = (!SUMMARY && io.final_obs != nullptr && active) ? io.final_obs + (size_t)lane * Fam::D : nullptr;
    const int n_ctx = pol.n_ctx, n_hidden = pol.n_hidden, act = pol.activation;
    const int w0 = pol.width[0], w1 = pol.width[1];  // (w1: read only when n_hidden == 2)
    const float clip = wts[L::kClip];
    float x[L::K];
#pragma unroll
    for (int s = 0; s < L::K; ++s) x[s] = 0.0f;
    int x_cidx = -1;  // context whose values x[0, n_ctx) hold
    int ep_count = 0, len_sum = 0;
    float ret_sum = 0.0f;
    int buf = 0;
    for (int t0 = 0; t0 < n_steps; t0 += CHUNK, buf ^= 1) {
      const int steps = min(CHUNK, n_steps - t0);
      if constexpr (predraw_of<Fam>::value) predraw<Fam>(b, glane, r);
      char* const rec = out_buf + (size_t)buf * CHUNK * SK::kStepBytes;
      Action* const my_act = reinterpret_cast<Action*>(act_buf + (size_t)buf * CHUNK * kPolicyLanes * 4) + threadIdx.x;
#pragma unroll 1
      for (int u = 0; u < steps; ++u) {
        // context inputs: re-read when some lane of the wave moved to another context (a reset under a round-robin /
        // random selector, or the launch's first step)
        if (ballot(r.cidx != x_cidx) != 0ull) {
#pragma unroll
          for (int k = 0; k < Fam::F; ++k)
            if (k < n_ctx) x[k] = normalize_input(ctx.get(pol.ctx_rows[k], r.cidx), wts[L::kShift + k], wts[L::kScale + k], clip);
          x_cidx = r.cidx;
        }
        float o[Fam::D];
        Fam::observe(r.s, r.aux, o);
#pragma unroll
        for (int d = 0; d < Fam::D; ++d)
          x[Fam::F + d] = normalize_input(o[d], wts[L::kShift + Fam::F + d], wts[L::kScale + Fam::F + d], clip);
        const Action a = policy_action<Fam, H>(wts, x, n_hidden, act, w0, w1);
        const int before = r.n_new_episodes;
        if constexpr (SUMMARY) {
          step_lane<Fam, GlobalCtx, true, NullSink<Fam>>(b, ctx, NullSink<Fam>{}, b.max_episode_steps, true, lane, glane,
                                                          a, r);
        } else {
          my_act[u * kPolicyLanes] = a;
          const SK sink{rec + (size_t)u * SK::kStepBytes, final_base, n * Fam::D, t0 + u, (int)threadIdx.x};
          step_lane<Fam, GlobalCtx, true, SK>(b, ctx, sink, b.max_episode_steps, true, lane, glane, a, r);
        }
        const bool fin = r.n_new_episodes != before;  // (valid lanes only: finish_episodes counts those)
        ep_count += fin ? 1 : 0;
        len_sum += fin ? r.fin_length : 0;
        ret_sum = fin ? ret_sum + r.fin_return : ret_sum;
      }
      if constexpr (!SUMMARY) __syncthreads();
    }
    if (active) {
      store_lane<Fam>(b, ctx, lane, r);
      if (sum.episodes != nullptr) {
        sum.episodes[lane] = ep_count;
        sum.return_sum[lane] = ret_sum;
        sum.length_sum[lane] = len_sum;
      }
    }
  } else if constexpr (!SUMMARY) {
    // storer waves: the previous chunk's records and actions while the compute waves run the current one
    int buf = 0;
    for (int t0 = 0; t0 < n_steps; t0 += CHUNK, buf ^= 1) {
      if (t0 > 0) {
        drain_records<Fam>(out_buf + (size_t)(buf ^ 1) * CHUNK * SK::kStepBytes, io, n, n_cols, lane_base, hl, storer,
                           t0 - CHUNK, CHUNK);
        drain_actions(act_buf + (size_t)(buf ^ 1) * CHUNK * kPolicyLanes * 4, const_cast<void*>(io.action), n, n_cols,
                      lane_base, hl, storer, t0 - CHUNK, CHUNK);
      }
      __syncthreads();
    }
    if (n_steps > 0) {
      const int last_t0 = ((n_steps - 1) / CHUNK) * CHUNK;
      drain_records<Fam>(out_buf + (size_t)(buf ^ 1) * CHUNK * SK::kStepBytes, io, n, n_cols, lane_base, hl, storer,
                         last_t0, n_steps - last_t0);
      drain_actions(act_buf + (size_t)(buf ^ 1) * CHUNK * kPolicyLanes * 4, const_cast<void*>(io.action), n, n_cols,
                    lane_base, hl, storer, last_t0, n_steps - last_t0);
    }
  }
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
  using L = PolicyLayout<Fam, H>;
  using Action = typename Fam::Action;
  constexpr int CHUNK = policy_chunk<Fam>();
  extern __shared__ float lds_dyn[];
  stage_family_tables<Fam>();
  float* const wts = lds_dyn;
  const int lane_base = (int)blockIdx.x * kPolicyLanes;
  stage_policy<Fam, H>(wts, pol, set_floats, lane_base / pol.lanes_per_set);
  const GlobalCtx ctx{b.ctx_table, b.ctx_stride};
  const int lane = lane_base + (int)threadIdx.x;
  const bool active = lane < b.n_lanes;
  const uint64_t glane = (uint64_t)(b.lane_offset + lane);
  const size_t n = (size_t)b.n_lanes;
  __syncthreads();

  LaneRegs<Fam> r{};
  load_staged_lane<Fam>(b, ctx, lane, active, r);
  const int n_ctx = pol.n_ctx, n_hidden = pol.n_hidden, act = pol.activation;
  const int w0 = pol.width[0], w1 = pol.width[1];  // (w1: read only when n_hidden == 2)
  const float clip = wts[L::kClip];
  float x[L::K];
#pragma unroll
  for (int s = 0; s < L::K; ++s) x[s] = 0.0f;
  int x_cidx = -1;  // context whose values x[0, n_ctx) hold
  int done_eps = 0, steps = 0;
  bool live = active;
  // (ballot(live) == 0: every lane of the wave is done -- a wave-uniform exit from both loops)
  for (int t0 = 0; t0 < max_steps && ballot(live) != 0ull; t0 += CHUNK) {
    if constexpr (predraw_of<Fam>::value) predraw<Fam>(b, glane, r);
    const int n_u = min(CHUNK, max_steps - t0);
#pragma unroll 1
    for (int u = 0; u < n_u; ++u) {
      if (ballot(live) == 0ull) break;
      if (ballot(r.cidx != x_cidx) != 0ull) {
#pragma unroll
        for (int k = 0; k < Fam::F; ++k)
          if (k < n_ctx) x[k] = normalize_input(ctx.get(pol.ctx_rows[k], r.cidx), wts[L::kShift + k], wts[L::kScale + k], clip);
        x_cidx = r.cidx;
      }
      float o[Fam::D];
      Fam::observe(r.s, r.aux, o);
#pragma unroll
      for (int d = 0; d < Fam::D; ++d)
        x[Fam::F + d] = normalize_input(o[d], wts[L::kShift + Fam::F + d], wts[L::kScale + Fam::F + d], clip);
      const Action a = policy_action<Fam, H>(wts, x, n_hidden, act, w0, w1);
      const int before = r.n_new_episodes, cidx = r.cidx;
      bool te = false;
      step_lane<Fam, GlobalCtx, false, TermSink<Fam>>(b, ctx, TermSink<Fam>{&te}, b.max_episode_steps, live, lane,
                                                       glane, a, r);
      steps += live ? 1 : 0;
      if (r.n_new_episodes != before) {  // (live lanes only: finish_episodes counts valid lanes that stepped)
        const size_t at = (size_t)done_eps * n + lane;
        ep.ret[at] = r.fin_return;
        ep.length[at] = r.fin_length;
        ep.context_id[at] = cidx;
        ep.terminated[at] = (uint8_t)te;
        done_eps += 1;
      }
      live = live && done_eps < n_episodes;
    }
  }
  if (active) {
    store_lane<Fam>(b, ctx, lane, r);
    ep.episodes[lane] = done_eps;
    ep.steps[lane] = steps;
    for (int k = done_eps; k < n_episodes; ++k) {
      const size_t at = (size_t)k * n + lane;
      ep.ret[at] = __builtin_nanf("");
      ep.length[at] = 0;
      ep.context_id[at] = -1;
      ep.terminated[at] = 0;
    }
  }
}

}  // namespace carl
