// policy_rollout_body.inc -- the body of policy_rollout_kernel and policy_rollout_sampled_kernel (policy_kernels.hip.h),
// included textually inside each: the compiler then sees every kernel's arguments as kernel arguments, so the
// deterministic kernels compile to exactly the code they had before the sampled ones shared their body (a body function
// taking the arguments changes where the kernel-argument loads land).  In scope: Fam, H, SUMMARY, the kernel
// arguments b, io, pol, set_floats, sum, n_steps; `Pick` (ModePick / SampledPick) and `pick`, which chooses each
// step's action; `log_prob`: the destination of the log-probabilities when Pick::kLogProb (transitions mode), one more
// [T][pitch] column of LDS after the actions, drained by the storer waves.
  using L = PolicyLayout<Fam, H>;
  using SK = LdsSink<Fam>;
  using Action = typename Fam::Action;
  constexpr int CHUNK = policy_chunk<Fam, Pick::kLogProb>();
  extern __shared__ float lds_dyn[];
  stage_family_tables<Fam>();
  float* const wts = lds_dyn;
  char* const out_buf = reinterpret_cast<char*>(lds_dyn) + L::kBytes;         // [2][CHUNK] records (transitions)
  char* const act_buf = out_buf + (size_t)2 * CHUNK * SK::kStepBytes;         // [2][CHUNK][256] actions
  char* const lp_buf = act_buf + (size_t)2 * CHUNK * kPolicyLanes * 4;        // [2][CHUNK][256] log-probs (kLogProb)
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
        [[maybe_unused]] float lp;  // (Pick::kLogProb)
        Action a;
        if constexpr (Pick::kSampled)
          a = pick.template choose<H>(wts, x, n_hidden, act, w0, w1, glane, r, lp);
        else
          a = policy_action<Fam, H>(wts, x, n_hidden, act, w0, w1);
        const int before = r.n_new_episodes;
        if constexpr (SUMMARY) {
          step_lane<Fam, GlobalCtx, true, NullSink<Fam>>(b, ctx, NullSink<Fam>{}, b.max_episode_steps, true, lane, glane,
                                                          a, r);
        } else {
          my_act[u * kPolicyLanes] = a;
          if constexpr (Pick::kLogProb)
            reinterpret_cast<float*>(lp_buf + (size_t)buf * CHUNK * kPolicyLanes * 4)[u * kPolicyLanes + threadIdx.x] = lp;
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
        if constexpr (Pick::kLogProb)
          drain_actions(lp_buf + (size_t)(buf ^ 1) * CHUNK * kPolicyLanes * 4, log_prob, n, n_cols, lane_base, hl,
                        storer, t0 - CHUNK, CHUNK);
      }
      __syncthreads();
    }
    if (n_steps > 0) {
      const int last_t0 = ((n_steps - 1) / CHUNK) * CHUNK;
      drain_records<Fam>(out_buf + (size_t)(buf ^ 1) * CHUNK * SK::kStepBytes, io, n, n_cols, lane_base, hl, storer,
                         last_t0, n_steps - last_t0);
      drain_actions(act_buf + (size_t)(buf ^ 1) * CHUNK * kPolicyLanes * 4, const_cast<void*>(io.action), n, n_cols,
                    lane_base, hl, storer, last_t0, n_steps - last_t0);
      if constexpr (Pick::kLogProb)
        drain_actions(lp_buf + (size_t)(buf ^ 1) * CHUNK * kPolicyLanes * 4, log_prob, n, n_cols, lane_base, hl, storer,
                      last_t0, n_steps - last_t0);
    }
  }
