// policy_episodes_body.inc -- the body of policy_episodes_kernel and policy_episodes_sampled_kernel
// (policy_kernels.hip.h), included textually inside each, as policy_rollout_body.inc.  In scope: Fam, H, the kernel
// arguments b, pol, set_floats, ep, n_episodes, max_steps; `Pick` (ModePick / SampledPick without log-probabilities) and `pick`,
// which chooses each step's action; `Stats` and `istats` (NoInputStats: nothing, or policy_stats_kernels.hip.h's InputStats,
// which gathers the raw inputs' sums of every live lane-step).
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
  if constexpr (Stats::kOn) istats.begin(wts + L::kFloats);

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
        if constexpr (Stats::kOn) istats.flush_context(ctx, pol, wts, n_ctx, x_cidx);
#pragma unroll
        for (int k = 0; k < Fam::F; ++k)
          if (k < n_ctx) x[k] = normalize_input(ctx.get(pol.ctx_rows[k], r.cidx), wts[L::kShift + k], wts[L::kScale + k], clip);
        x_cidx = r.cidx;
      }
      float o[Fam::D];
      Fam::observe(r.s, r.aux, o);
      if constexpr (Stats::kOn) istats.add_step(live, o, wts);
#pragma unroll
      for (int d = 0; d < Fam::D; ++d)
        x[Fam::F + d] = normalize_input(o[d], wts[L::kShift + Fam::F + d], wts[L::kScale + Fam::F + d], clip);
      [[maybe_unused]] float lp;  // (Pick::kLogProb)
      Action a;
      if constexpr (Pick::kSampled)
        a = pick.template choose<H>(wts, x, n_hidden, act, w0, w1, glane, r, lp);
      else
        a = policy_action<Fam, H>(wts, x, n_hidden, act, w0, w1);
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
    if constexpr (Stats::kOn) istats.flush(ctx, pol, wts, n_ctx, x_cidx);
  }
  if constexpr (Stats::kOn) istats.store(wts + L::kFloats, n_ctx, pol.n_in);
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
