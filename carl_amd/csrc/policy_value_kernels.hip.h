// policy_value_kernels.hip.h -- the closed-loop rollout with a critic (include/carl_amd.h: carl_rollout_policy_valued)
// and the GAE kernel (carl_gae).  Included by carl_policy_value.hip only: the kernels of policy_kernels.hip.h are read,
// none is changed, so every earlier kernel compiles to the code it had (profiles/policy_value_isa_identity.txt).
//
// policy_rollout_valued_kernel is the transitions-mode body of policy_rollout_body.inc with a second network:
//   * two weight regions in LDS, the actor's and the critic's, each PolicyLayout<Fam, H> bytes, H the larger of the two
//     padded widths.  A network with hidden layers is staged by stage_policy<Fam, H> (its padding); a LINEAR network
//     (n_hidden == 0) in an H > 0 instance is staged in the H = 0 layout at the start of its region and evaluated by the
//     H = 0 code (policy_action<Fam, 0> / SampledPick::choose<0> / policy_head<Fam, 0>) under a wave-uniform branch:
//     stage_policy's H > 0 layout has no place for a head that reads the inputs.  Either way a network's arithmetic is
//     that of the instance it would run in alone, so actions and log-probabilities keep their bits.
//   * V = y[0] of policy_head on the critic's region, from the same x[] registers, BEFORE the action is chosen: the two
//     forward passes never overlap, and while the critic's hidden arrays are live neither the action, its log-probability
//     nor the sampled pick's draw is (the order changes no result).  The critic's own shift / scale / clip section is
//     not read.
//   * value and boot_value are two more [2][CHUNK][256] fp32 LDS columns after action and log_prob, drained by the storer
//     waves in 16-byte non-temporal stores (drain_actions).  The boot column is lazy like the flag rows: all zero, written
//     only under a wave-uniform ballot(truncated && !terminated) branch, re-zeroed by the storer after each drain.
//   * ValuedSink wraps LdsSink: put_flags also keeps the two flags in the caller's registers, and final_obs_ptr() hands
//     finish_episodes a per-lane LDS slot, so the terminal observation is at hand without touching step_lane.  The slot
//     is copied on to io.final_obs when the caller asked for it.  The boot evaluation overwrites the observation slots
//     of x[] (the next step rewrites them anyway) and keeps the context slots: they still hold the context the episode
//     ran in, the re-read for a moved lane happens at the top of the next step.
//   * after the last step each lane evaluates the critic once more on its current input: last_value.
#pragma once

#include "policy_kernels.hip.h"

namespace carl {

// steps per LDS record buffer: 8 where the records, the action / log_prob (SAMPLED) / value / boot columns, both weight
// regions at H = 64, the terminal-observation slots and the family's static tables fit a compute unit; 4 otherwise
template <class Fam>
__host__ __device__ constexpr size_t valued_slot_bytes() {
  return (size_t)kPolicyLanes * Fam::D * sizeof(float);
}
template <class Fam, int H, bool SAMPLED>
__host__ __device__ constexpr size_t valued_lds_bytes_at(int chunk) {
  return 2 * PolicyLayout<Fam, H>::kBytes + (size_t)2 * chunk * LdsSink<Fam>::kStepBytes +
         (size_t)(SAMPLED ? 4 : 3) * 2 * chunk * kPolicyLanes * 4 + valued_slot_bytes<Fam>();
}
template <class Fam, bool SAMPLED>
__host__ __device__ constexpr int valued_chunk() {
  return valued_lds_bytes_at<Fam, 64, SAMPLED>(8) + static_lds_bytes<Fam>() <= kCuLdsBytes ? 8 : 4;
}
template <class Fam, int H, bool SAMPLED>
__host__ __device__ constexpr size_t valued_lds_bytes() {
  return valued_lds_bytes_at<Fam, H, SAMPLED>(valued_chunk<Fam, SAMPLED>());
}

// a network's region: stage_policy's layout of the instance, or the H = 0 layout for a linear network (see above)
template <class Fam, int H>
__device__ __forceinline__ void stage_network(float* w, const carl_policy_t& pol, int set_floats, int set) {
  if constexpr (H == 0) {
    stage_policy<Fam, 0>(w, pol, set_floats, set);
  } else {
    using L = PolicyLayout<Fam, H>;
    using L0 = PolicyLayout<Fam, 0>;
    if (pol.n_hidden == 0) {  // (kernel argument: the whole workgroup takes one side)
      stage_policy<Fam, 0>(w, pol, set_floats, set);
      // shift | scale | clip once more where the H layout keeps them: the kernel reads the input transform from there
      static_assert(L::kShift >= L0::kFloats, "the copy must not overlap the H = 0 layout");
      __syncthreads();
      for (int e = threadIdx.x; e < 2 * L::K + 4; e += blockDim.x) w[L::kShift + e] = w[L0::kShift + e];
    } else {
      stage_policy<Fam, H>(w, pol, set_floats, set);
    }
  }
}

// V(x): the critic's one head output
template <class Fam, int H>
__device__ __forceinline__ float critic_value(const float* w, const float (&x)[PolicyLayout<Fam, H>::K], int n_hidden,
                                              int act, int w0, int w1) {
  float y[4];
  if constexpr (H == 0) {
    policy_head<Fam, 0>(w, x, 0, act, 0, 0, y);
  } else {
    if (n_hidden == 0)  // (wave-uniform)
      policy_head<Fam, 0>(w, x, 0, act, 0, 0, y);
    else
      policy_head<Fam, H>(w, x, n_hidden, act, w0, w1, y);
  }
  return y[0];
}

// LdsSink plus what the critic needs of a step: the flags in registers, the terminal observation in an LDS slot
template <class Fam>
struct ValuedSink {
  static constexpr bool kLazyFlags = true;
  LdsSink<Fam> base;
  float* slot;  // this lane's terminal-observation slot in LDS
  bool* te;
  bool* tr;
  __device__ __forceinline__ void put_reward(float r) const { base.put_reward(r); }
  __device__ __forceinline__ void put_flags(bool t, bool u) const {
    base.put_flags(t, u);
    *te = t;
    *tr = u;
  }
  __device__ __forceinline__ void put_obs(const float (&o)[Fam::D]) const { base.put_obs(o); }
  __device__ __forceinline__ float* final_obs_ptr() const { return slot; }
};

// storer wave `which`: the lazy boot column of steps [t0, t0 + steps) as drain_actions, each drained row zeroed again
__device__ __forceinline__ void drain_boot(char* buf, float* boot, size_t n, int cols, int lane_base, int l, int which,
                                           int t0, int steps) {
  const int valid = min(kPolicyLanes, cols - lane_base);  // a multiple of 16
  for (int u = which; u < steps; u += kStorers) {
    char* src = buf + (size_t)u * kPolicyLanes * 4 + 16 * l;
    char* dst = reinterpret_cast<char*>(boot) + ((size_t)(t0 + u) * n + lane_base) * 4 + 16 * l;
    if (4 * l < valid) __builtin_nontemporal_store(*reinterpret_cast<const pvf4*>(src), reinterpret_cast<pvf4*>(dst));
    *reinterpret_cast<pvf4*>(src) = pvf4{0.0f, 0.0f, 0.0f, 0.0f};
  }
}

// Preconditions (host, carl_policy_value.hip): those of policy_rollout_kernel's transitions mode; the critic validated
// against the actor (same inputs, same set layout, n_out 1); val.value and val.last_value non-NULL, val.boot_value only
// with CARL_FLAG_AUTORESET; the columns on 16-byte boundaries; n_steps >= 1.
template <class Fam, int H, bool SAMPLED>
__global__ void __launch_bounds__(kPolicyThreadsTransitions)
    policy_rollout_valued_kernel(const carl_batch_t b, const carl_step_io_t io, const carl_policy_t pol, const int set_floats,
                                 const carl_policy_t crit, const int crit_set_floats, const carl_policy_summary_t sum,
                                 const int n_steps, const carl_policy_sampling_t smp, const carl_policy_value_t val) {
  using L = PolicyLayout<Fam, H>;
  using SK = LdsSink<Fam>;
  using Action = typename Fam::Action;
  using Pick = std::conditional_t<SAMPLED, SampledPick<Fam, true>, ModePick<Fam>>;
  constexpr int CHUNK = valued_chunk<Fam, SAMPLED>();
  constexpr size_t kCol = (size_t)CHUNK * kPolicyLanes * 4;  // one buffer of one column
  extern __shared__ float lds_dyn[];
  stage_family_tables<Fam>();
  float* const wts = lds_dyn;
  float* const cwts = lds_dyn + L::kFloats;
  char* const out_buf = reinterpret_cast<char*>(lds_dyn) + 2 * L::kBytes;  // [2][CHUNK] records
  char* const act_buf = out_buf + (size_t)2 * CHUNK * SK::kStepBytes;      // [2][CHUNK][256] actions
  char* const lp_buf = act_buf + 2 * kCol;                                 // log-probs (SAMPLED)
  char* const val_buf = lp_buf + (SAMPLED ? 2 * kCol : 0);                 // values
  char* const boot_buf = val_buf + 2 * kCol;                               // lazy boot values
  float* const slots = reinterpret_cast<float*>(boot_buf + 2 * kCol);      // [256][D] terminal observations
  const int lane_base = (int)blockIdx.x * kPolicyLanes;
  stage_network<Fam, H>(wts, pol, set_floats, lane_base / pol.lanes_per_set);
  stage_network<Fam, H>(cwts, crit, crit_set_floats, lane_base / crit.lanes_per_set);
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
  if (!compute) {
    zero_flag_rows<Fam, CHUNK>(out_buf, hl, storer);
    for (int u = storer; u < 2 * CHUNK; u += kStorers)
      *reinterpret_cast<pvf4*>(boot_buf + (size_t)u * kPolicyLanes * 4 + 16 * hl) = pvf4{0.0f, 0.0f, 0.0f, 0.0f};
  }
  __syncthreads();

  if (compute) {
    Pick pick{};
    if constexpr (SAMPLED) pick = Pick::of(smp, pol);
    LaneRegs<Fam> r{};
    load_staged_lane<Fam>(b, ctx, lane, active, r);
    float* const final_base = (io.final_obs != nullptr && active) ? io.final_obs + (size_t)lane * Fam::D : nullptr;
    const bool autoreset = (b.flags & CARL_FLAG_AUTORESET) != 0;
    const bool want_boot = val.boot_value != nullptr;
    const int n_ctx = pol.n_ctx, n_hidden = pol.n_hidden, act = pol.activation;
    const int pol_w0 = pol.width[0], pol_w1 = pol.width[1];  // (w1: read only when n_hidden == 2)
    const int c_hidden = crit.n_hidden, c_act = crit.activation, crit_w0 = crit.width[0], crit_w1 = crit.width[1];
    // the actor's input transform (stage_network keeps it at the H layout's offsets in either layout)
    const bool a_lin = H > 0 && n_hidden == 0;
    const float* const shift = wts + L::kShift;
    const float* const scale = wts + L::kScale;
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
      // this lane's entry of step 0 in the chunk's action column; the other columns lie at constant offsets from it
      char* const my_col = act_buf + buf * kCol + 4 * threadIdx.x;
      constexpr size_t kLp = 2 * kCol, kVal = (SAMPLED ? 4 : 2) * kCol, kBoot = kVal + 2 * kCol;
#pragma unroll 1
      for (int u = 0; u < steps; ++u) {
        if (ballot(r.cidx != x_cidx) != 0ull) {  // (as policy_rollout_body.inc)
#pragma unroll
          for (int k = 0; k < Fam::F; ++k)
            if (k < n_ctx) x[k] = normalize_input(ctx.get(pol.ctx_rows[k], r.cidx), shift[k], scale[k], clip);
          x_cidx = r.cidx;
        }
        float o[Fam::D];
        Fam::observe(r.s, r.aux, o);
#pragma unroll
        for (int d = 0; d < Fam::D; ++d) x[Fam::F + d] = normalize_input(o[d], shift[Fam::F + d], scale[Fam::F + d], clip);
        // The layer widths, opaque to the optimiser from here on.  activate() zeroes the padded units with one select per
        // unit on `j < width`; with loop-invariant widths the compiler computes those 64 lane masks per layer once,
        // ahead of the step loop, and keeps them: 128 SGPRs per layer, four layers here, spilled to VGPR lanes and from
        // there to scratch.  Opaque, each mask is one scalar compare next to its select.
        int w0 = pol_w0, w1 = pol_w1, c_w0 = crit_w0, c_w1 = crit_w1;
        asm volatile("" : "+s"(w0), "+s"(w1), "+s"(c_w0), "+s"(c_w1));
        // the critic first: while it runs, nothing of the action's choice is live yet (the order changes no result)
        char* const my = my_col + (size_t)u * kPolicyLanes * 4;
        *reinterpret_cast<float*>(my + kVal) = critic_value<Fam, H>(cwts, x, c_hidden, c_act, c_w0, c_w1);
        [[maybe_unused]] float lp;
        Action a;
        if constexpr (SAMPLED) {
          if constexpr (H == 0) {
            a = pick.template choose<0>(wts, x, 0, act, 0, 0, glane, r, lp);
          } else {
            if (a_lin)  // (wave-uniform)
              a = pick.template choose<0>(wts, x, 0, act, 0, 0, glane, r, lp);
            else
              a = pick.template choose<H>(wts, x, n_hidden, act, w0, w1, glane, r, lp);
          }
        } else {
          if constexpr (H == 0) {
            a = policy_action<Fam, 0>(wts, x, 0, act, 0, 0);
          } else {
            if (a_lin)
              a = policy_action<Fam, 0>(wts, x, 0, act, 0, 0);
            else
              a = policy_action<Fam, H>(wts, x, n_hidden, act, w0, w1);
          }
        }
        *reinterpret_cast<Action*>(my) = a;
        if constexpr (SAMPLED) *reinterpret_cast<float*>(my + kLp) = lp;
        const int before = r.n_new_episodes;
        bool te = false, tr = false;  // (put_flags runs on the done path only)
        float* const slot = slots + threadIdx.x * Fam::D;
        const ValuedSink<Fam> sink{SK{rec + (size_t)u * SK::kStepBytes, nullptr, n * Fam::D, t0 + u, (int)threadIdx.x}, slot,
                                   &te, &tr};
        step_lane<Fam, GlobalCtx, true, ValuedSink<Fam>>(b, ctx, sink, b.max_episode_steps, true, lane, glane, a, r);
        const bool fin = r.n_new_episodes != before;  // (valid lanes only: finish_episodes counts those)
        ep_count += fin ? 1 : 0;
        len_sum += fin ? r.fin_length : 0;
        ret_sum = fin ? ret_sum + r.fin_return : ret_sum;
        if (ballot(te || tr) != 0ull) {  // the slot holds the terminal observation of a lane that was reset
          if (final_base != nullptr && (te || tr) && autoreset) {
            float* const dst = final_base + (size_t)(t0 + u) * n * Fam::D;
#pragma unroll
            for (int d = 0; d < Fam::D; ++d) dst[d] = slot[d];
          }
          const bool cut = tr && !te;
          if (want_boot && ballot(cut) != 0ull) {
            // x[0, n_ctx) still holds the context the episode ran in; the observation slots are rewritten next step
#pragma unroll
            for (int d = 0; d < Fam::D; ++d)
              x[Fam::F + d] = normalize_input(slot[d], shift[Fam::F + d], scale[Fam::F + d], clip);
            const float v = critic_value<Fam, H>(cwts, x, c_hidden, c_act, c_w0, c_w1);
            if (cut) *reinterpret_cast<float*>(my + kBoot) = v;
          }
        }
      }
      __syncthreads();
    }
    // V of the input after the last step
    if (ballot(r.cidx != x_cidx) != 0ull) {
#pragma unroll
      for (int k = 0; k < Fam::F; ++k)
        if (k < n_ctx) x[k] = normalize_input(ctx.get(pol.ctx_rows[k], r.cidx), shift[k], scale[k], clip);
    }
    float o[Fam::D];
    Fam::observe(r.s, r.aux, o);
#pragma unroll
    for (int d = 0; d < Fam::D; ++d) x[Fam::F + d] = normalize_input(o[d], shift[Fam::F + d], scale[Fam::F + d], clip);
    const float v_last = critic_value<Fam, H>(cwts, x, c_hidden, c_act, crit_w0, crit_w1);
    if (active) {
      val.last_value[lane] = v_last;
      store_lane<Fam>(b, ctx, lane, r);
      if (sum.episodes != nullptr) {
        sum.episodes[lane] = ep_count;
        sum.return_sum[lane] = ret_sum;
        sum.length_sum[lane] = len_sum;
      }
    }
  } else {
    // storer waves: the previous chunk's records and columns while the compute waves run the current one
    auto drain = [&](int b_, int t0, int steps) {
      drain_records<Fam>(out_buf + (size_t)b_ * CHUNK * SK::kStepBytes, io, n, n_cols, lane_base, hl, storer, t0, steps);
      drain_actions(act_buf + b_ * kCol, const_cast<void*>(io.action), n, n_cols, lane_base, hl, storer, t0, steps);
      if constexpr (SAMPLED) drain_actions(lp_buf + b_ * kCol, smp.log_prob, n, n_cols, lane_base, hl, storer, t0, steps);
      drain_actions(val_buf + b_ * kCol, val.value, n, n_cols, lane_base, hl, storer, t0, steps);
      if (val.boot_value != nullptr)
        drain_boot(boot_buf + b_ * kCol, val.boot_value, n, n_cols, lane_base, hl, storer, t0, steps);
    };
    int buf = 0;
    for (int t0 = 0; t0 < n_steps; t0 += CHUNK, buf ^= 1) {
      if (t0 > 0) drain(buf ^ 1, t0 - CHUNK, CHUNK);
      __syncthreads();
    }
    const int last_t0 = ((n_steps - 1) / CHUNK) * CHUNK;
    drain(buf ^ 1, last_t0, n_steps - last_t0);
  }
}

// ---- GAE (include/carl_amd.h: carl_gae).  One thread owns one lane's column and walks it from T - 1 down to 0; the
// loads of kGaeRows rows are issued before the dependent chain of those rows, so a wave keeps up to 5 * kGaeRows
// row pieces (256 bytes of fp32, 64 of flags) in flight.  g.row_pitch is never 0 here; gl = fp32(gamma) * fp32(lambda).
constexpr int kGaeThreads = 64;
constexpr int kGaeRows = 8;

template <bool BOOT>
__global__ void __launch_bounds__(kGaeThreads) gae_kernel(const carl_gae_t g, const float gl) {
  const int lane = (int)blockIdx.x * kGaeThreads + (int)threadIdx.x;
  if (lane >= g.n_lanes) return;
  const size_t n = (size_t)g.row_pitch;
  const float gamma = g.gamma;
  float adv = 0.0f;
  float v_next = g.last_value[lane];
#pragma unroll 1
  for (int t1 = g.n_steps; t1 > 0; t1 -= kGaeRows) {
    float rw[kGaeRows], v[kGaeRows], bt[kGaeRows];
    uint8_t te[kGaeRows], tr[kGaeRows];
#pragma unroll
    for (int k = 0; k < kGaeRows; ++k) {
      const int t = t1 - 1 - k;
      if (t >= 0) {  // (uniform)
        const size_t i = (size_t)t * n + lane;
        rw[k] = g.reward[i];
        v[k] = g.value[i];
        te[k] = g.terminated[i];
        tr[k] = g.truncated[i];
        if constexpr (BOOT) bt[k] = g.boot_value[i];
      }
    }
#pragma unroll
    for (int k = 0; k < kGaeRows; ++k) {
      const int t = t1 - 1 - k;
      if (t >= 0) {
#pragma clang fp contract(off)
        const size_t i = (size_t)t * n + lane;
        const bool term = te[k] != 0, trunc = tr[k] != 0;
        const bool done = term || trunc;
        float vn = done ? 0.0f : v_next;  // selects: a masked-out NaN must not reach the result
        if constexpr (BOOT) vn = (trunc && !term) ? bt[k] : vn;
        const float delta = __fmaf_rn(gamma, vn, rw[k]) - v[k];
        adv = __fmaf_rn(gl, done ? 0.0f : adv, delta);
        g.advantage[i] = adv;
        g.ret[i] = adv + v[k];
        v_next = v[k];
      }
    }
  }
}

}  // namespace carl
