"""Every sampled closed-loop policy kernel (carl_policy_sample.hip: policy_rollout_sampled_kernel<Fam, H, SUMMARY,
LOGP> and policy_episodes_sampled_kernel<Fam, H>: 6 step types x H in {0, 32, 64} x transitions with log_prob,
transitions, summary, episodes = 72 instances) against a float64 reference of the sampling rule (include/carl_amd.h:
carl_policy_sampling_t; sampling_ref.py) on the exact host reference of the packed policy (oracle_policy_forward).

One chain per case (run_and_check): a transitions launch with log_prob from a snapshot, teacher-forced the way
test_gpu_policy_sampling.teacher does (inputs x, episode index e, elapsed before every lane-step), the words drawn with
glane = lane_offset + lane, and each lane's weight set and log_std its own (lane // lanes_per_set).
  - Categorical actions equal SR.categorical64 on y64 wherever t = u S is further than SR.categorical_tolerance from a
    prefix-sum boundary; the exempted share stays below 1e-3 over the module (a two-layer tanh net's forward bound
    alone exempts ~1e-3 of its lane-steps: per launch 2e-3 and one lane-step; counted, printed at module end).
  - Box actions: |a - (y64 + sigma z64)| <= bound(y) + sigma dz + |a| 2^-23, dz = SR.gaussian_z_bound (the existing
    derived bound), sigma = exp of the lane's own set's fp32 log_std.
  - log_prob, discrete: y64[a] - logsumexp(y64) at the device's own action a.  The device computes (y_a - m) - logf(S)
    from outputs within B (the forward pass's bound) of y64: y_a - m is off by at most 2 B; every exp(y_k - m) by 2 B
    relative, so S is too and log S by 2 B absolute; then a few fp32 ulps of each rounding (y_k - m, expf, the n - 1
    sums, logf, the last subtraction) of |y_a - m|, 1 and |log_prob|: SR.categorical_log_prob_bound.
  - log_prob, Box: -z64^2 / 2 - log_std - ln(2 pi) / 2, from the words (not from (a - mu) / sigma, which loses every
    digit at small sigma).  The device's fma(-z/2, z, lp0) is off by |z| dz plus the roundings of lp0 and of the fma:
    SR.gaussian_log_prob_bound.
  Both log_prob bounds are also capped at the earlier 1e-5 abs + 1e-5 rel: never looser than that.
  - Then each other variant is pinned bit for bit to that launch: rollout() of the recorded actions (records, state);
    the transitions launch without log_prob (actions, records, state); the summary launch (the exact reduction,
    host_summary; state); evaluate_policy(..., deterministic=False) (test_gpu_policy_episodes.exact_case: counts,
    steps, returns with their NaN sentinels, lengths, context ids, terminated, each lane's state at its stop step).

Padding lanes (lanes [n, carl_rollout_pitch(n)) of a transitions launch's last workgroup) run as clones of lane n - 1:
its state, context, weight set, episode index and elapsed count -- but they draw with their OWN global lane id
lane_offset + lane.  So at step 0 a padding lane's action and log_prob are the rule applied to lane n - 1's input with
the padding lane's words (checked with the bounds and the exemption of a real lane); later steps depend on those
draws.  The padding columns of the action and log_prob rows are written, nothing past them and no row >= T."""
import numpy as np
import pytest
import torch

import sampling_ref as SR
from carl_amd import _lib
from carl_amd.policy import MLPPolicy
from oracle import oracle as O
from test_gpu_policy_episodes import exact_case
from test_gpu_policy_kernels import (CTX_MODES, OPTIONS, STEP_TYPES, assert_same_state, canary_out, check_canaries,
                                     check_summary_canary, make_engine, make_policy, summary_canary)
from test_gpu_policy_rollout import engine_state, host_summary
from test_gpu_policy_sampling import teacher, words, zero_head_policy

pytestmark = pytest.mark.gpu

SEED = 0x5A3D1E5EED0F
VARIANTS = ("transitions_log_prob", "transitions", "summary", "episodes")
ACTS = ["identity", "relu", "tanh"]
LOG_STDS = [-20.0, -0.5, 0.0, 2.0]
LAUNCHED = set()  # (step type, H, variant) of every sampled launch made
STATS = {"exempt": 0, "lane_steps": 0, "lp_worst_frac": 0.0}


def step_type_of(eng):
    if eng.family == _lib.ACROBOT and eng.b.flags & _lib.FLAG_ACROBOT_FP32:
        return "acrobot_fast"
    return next(s for s, (f, o) in STEP_TYPES.items() if f == eng.family and not o)


def padded_hidden(pol):
    """carl_policy.hip: policy_padded_hidden"""
    return 0 if not pol.widths else 32 if max(pol.widths) <= 32 else 64


def launched(eng, pol, variant):
    LAUNCHED.add((step_type_of(eng), padded_hidden(pol), variant))


@pytest.fixture(scope="module", autouse=True)
def every_instance_and_statistics(request):
    yield
    line = (f"sampled policies: {STATS['exempt']} of {STATS['lane_steps']} discrete lane-steps exempted near a prefix-sum "
            f"boundary; largest log_prob |err| / bound {STATS['lp_worst_frac']:.3f}; {len(LAUNCHED)} of 72 instances "
            "launched")
    capman = request.config.pluginmanager.getplugin("capturemanager")
    if capman is not None:
        with capman.global_and_fixture_disabled():
            print("\n" + line)
    else:
        print("\n" + line)
    assert STATS["exempt"] < 1e-3 * max(STATS["lane_steps"], 1)
    if MATRIX_RUN == set(MATRIX_IDS):  # (the whole matrix ran: not a -k selection)
        want = {(s, H, v) for s in STEP_TYPES for H in (0, 32, 64) for v in VARIANTS}
        assert want <= LAUNCHED, sorted(want - LAUNCHED)


def check_rule(pol, x, w, a, lp, sets):
    """the sampling rule on inputs x [N, n_in] with words w (4 x [N]) and weight sets `sets` [N] against the device's
    actions a [N] and log-probabilities lp [N] (module docstring)"""
    r = O.policy_forward(pol.params, pol.n_in, pol.widths, pol.n_out, pol.activation, x, sets)
    a = np.asarray(a).reshape(-1)
    lp = np.asarray(lp, np.float64).reshape(-1)
    if pol.discrete:
        u = SR.u_categorical(w[0]).reshape(-1).astype(np.float64)
        want, margin = SR.categorical64(r.y64, u)
        clear = margin > SR.categorical_tolerance(r.y64, r.bound)
        STATS["exempt"] += int((~clear).sum())
        STATS["lane_steps"] += a.size
        assert (~clear).sum() <= 2e-3 * a.size + 1, (~clear).mean()  # (module-wide: below 1e-3)
        np.testing.assert_array_equal(a[clear], want[clear])
        lp_ref = SR.categorical_log_prob64(r.y64, a)
        lp_bound = SR.categorical_log_prob_bound(r.y64, r.bound, a)
    else:
        ls = pol.log_std[sets]
        sigma = np.exp(ls.astype(np.float64))
        z = SR.z_gaussian64(w[0], w[1]).reshape(-1)
        want = r.y64[:, 0] + sigma * z
        err = np.abs(a.astype(np.float64) - want)
        bound = r.bound[:, 0] + sigma * SR.gaussian_z_bound(z) + np.abs(want) * 2.0 ** -23
        assert np.all(err <= bound), (err.max(), int(np.argmax(err - bound)))
        lp_ref = SR.gaussian_log_prob64(z, ls)
        lp_bound = SR.gaussian_log_prob_bound(z, ls)
    lim = np.minimum(lp_bound, 1e-5 + 1e-5 * np.abs(lp_ref))
    err = np.abs(lp - lp_ref)
    STATS["lp_worst_frac"] = max(STATS["lp_worst_frac"], float((err / lim).max()) if err.size else 0.0)
    assert np.all(err <= lim), (err.max(), lp[np.argmax(err / lim)], lp_ref[np.argmax(err / lim)])
    return r


def lane_sets(pol, n):
    return np.arange(n) // pol.lanes_per_set if pol.n_sets > 1 else np.zeros(n, np.int64)


def run_and_check(eng, pol, T, K=2, out=None, summary_out=None, plain=True, seed=SEED):
    """the chain of the module docstring; returns (transitions output with log_prob, x, e, el, episodes count or None)"""
    kw = dict(deterministic=False, sample_seed=seed)
    n = eng.n
    sets = lane_sets(pol, n)
    snap = eng.snapshot()
    out = eng.rollout_policy(pol, T, out=out, log_prob=True, **kw)
    launched(eng, pol, "transitions_log_prob")
    after = engine_state(eng)
    acts = out["action"][:T]
    x, e, el = teacher(eng, pol, snap, acts)
    w = words(eng, e, el, seed)
    check_rule(pol, x.reshape(-1, pol.n_in), w, acts.cpu().numpy(), out["log_prob"][:T].cpu().numpy(), np.tile(sets, T))
    # replay through rollout()
    eng.restore(snap)
    ref = eng.rollout(acts, out=eng.alloc_rollout(T))
    for k in ("obs", "reward", "terminated", "truncated"):
        assert torch.equal(out[k][:T], ref[k]), k
    assert_same_state(after, engine_state(eng))
    # the transitions launch without log_prob
    if plain:
        eng.restore(snap)
        p = eng.rollout_policy(pol, T, **kw)
        launched(eng, pol, "transitions")
        for k in ("action", "obs", "reward", "terminated", "truncated"):
            x1, x2 = p[k][:T], out[k][:T]
            if x1.dtype == torch.float32:
                x1, x2 = x1.view(torch.int32), x2.view(torch.int32)
            assert torch.equal(x1, x2), k
        assert_same_state(after, engine_state(eng))
    eng.restore(snap)
    if not eng.auto_reset:
        with pytest.raises(ValueError, match="auto_reset"):
            eng.rollout_policy(pol, T, mode="summary", **kw)
        with pytest.raises(ValueError, match="auto_reset"):
            eng.evaluate_policy(pol, K, T, **kw)
        return out, x, e, el, None
    # summary = the exact reduction, same state
    s = eng.rollout_policy(pol, T, mode="summary", out=summary_out, **kw)
    launched(eng, pol, "summary")
    assert_same_state(after, engine_state(eng))
    count, ret_sum, len_sum = host_summary(snap, {k: v[:T] for k, v in out.items()}, T)
    np.testing.assert_array_equal(s["episodes"].cpu().numpy(), count)
    np.testing.assert_array_equal(s["return_sum"].cpu().numpy(), ret_sum)
    np.testing.assert_array_equal(s["length_sum"].cpu().numpy(), len_sum)
    # episodes mode: each lane's first K episodes of the same transitions
    _, ep_count = exact_case(eng, pol, K, T, transitions=(snap, out), **kw)
    launched(eng, pol, "episodes")
    return out, x, e, el, ep_count


# ---------------------------------------------------------------- 1 + 2. every instance through every variant
def _matrix():
    """(step type, widths, activation, context mode, clip, log_std, wide head) per case: H = 0, 32, 64 for each step
    type; activation, context mode and clip cycled; Box families cycle log_std; every other discrete case has a wide
    head (logit gaps up to 30 - 90)"""
    shapes = {0: [()], 32: [(31,), (32, 7)], 64: [(64,), (33, 64)]}
    cases = []
    for si, s in enumerate(STEP_TYPES):
        box = STEP_TYPES[s][0] in (_lib.PENDULUM, _lib.MOUNTAINCAR_CONT)
        for hi, H in enumerate((0, 32, 64)):
            k = len(cases)
            ws = shapes[H][si % len(shapes[H])]
            cases.append((s, ws, ACTS[(si + hi) % 3], CTX_MODES[k % 5], 2.0 if k % 2 else None,
                          LOG_STDS[k % 4] if box else None, not box and (si + hi) % 2 == 0))
    return cases


MATRIX = _matrix()
MATRIX_IDS = [f"{s}-" + ("x".join(map(str, w)) or "linear") + f"-{a}-{c}" + ("-clip" if cl else "")
              + (f"-logstd{ls:g}" if ls is not None else "") + ("-wide" if wide else "")
              for s, w, a, c, cl, ls, wide in MATRIX]
MATRIX_RUN = set()


def widen_head(eng, pol, clip, gap=60.0):
    """pol with its last logit's bias lowered by `gap`: that logit trails the mode by 30 - 90 on every lane-step, so its
    exp(y_k - m) vanishes below S's resolution, while (three actions) the other two still make a real choice.  (A bias
    moves the logits by exact amounts: the forward bound, and with it the exempted share, stays as small as it was.)"""
    layers = [(W.astype(np.float64), b.astype(np.float64)) for W, b in pol.layers]
    W, b = layers[-1]
    b = b.copy()
    b[-1] -= gap
    layers[-1] = (W, b)
    return MLPPolicy.for_env(eng, layers, pol.activation, input_shift=pol.shift, input_scale=pol.scale,
                             input_clip=clip, context_features=pol.ctx_rows)


@pytest.mark.parametrize("step_type, widths, act, ctx, clip, log_std, wide", MATRIX, ids=MATRIX_IDS)
def test_sampled_kernel_matrix(step_type, widths, act, ctx, clip, log_std, wide):
    """n = 1000 (a partial last workgroup, 8 padding lanes); episodes cut at 12 steps and half the lanes reset after 5
    warm-up steps, so that with K = 3 and T = 33 lanes both finish K episodes and fall short of it"""
    k = MATRIX.index((step_type, widths, act, ctx, clip, log_std, wide))
    family, opts = STEP_TYPES[step_type]
    eng = make_engine(family, 1000, seed=100 + k, max_episode_steps=12, **opts)
    rng = np.random.default_rng(2000 + k)
    pol = make_policy(eng, widths, act, rng, ctx, clip=clip, log_std=log_std)
    if wide:
        pol = widen_head(eng, pol, clip)
    a0 = torch.zeros(eng.n, dtype=torch.int32 if eng.info.action_is_discrete else torch.float32, device=eng.device)
    for _ in range(5):  # (per-call steps: the teacher reads the observation buffer, which a launch does not refresh)
        eng.step(a0)
    eng.reset(torch.arange(eng.n, device=eng.device) % 2)
    out, x, _, _, count = run_and_check(eng, pol, 33, K=3, seed=SEED + k)
    assert (count == 3).any() and (count < 3).any(), np.bincount(count)
    if wide:
        y = O.policy_forward(pol.params, pol.n_in, pol.widths, pol.n_out, pol.activation, x.reshape(-1, pol.n_in)).y64
        gap = np.sort(y.max(axis=1, keepdims=True) - y, axis=1)[:, 1:]  # the non-mode gaps of each lane-step
        assert gap[:, -1].min() >= 30 and gap[:, -1].max() <= 90, (gap[:, -1].min(), gap[:, -1].max())
        if gap.shape[1] > 1:
            assert (gap[:, 0] < 2).mean() > 0.05, "the other two logits must make a real choice"
        assert np.all(out["action"][:33].cpu().numpy() != pol.n_out - 1)
    MATRIX_RUN.add(MATRIX_IDS[k])


# ---------------------------------------------------------------- 3. launch shapes, with canaries
def launch_shape_case(step_type, n, T):
    family, opts = STEP_TYPES[step_type]
    eng = make_engine(family, n, seed=n + T, n_contexts=max(1, min(64, n)), max_episode_steps=6, **opts)
    box = family in (_lib.PENDULUM, _lib.MOUNTAINCAR_CONT)
    pol = make_policy(eng, (33,), "relu", np.random.default_rng(n * 31 + T), "all", clip=2.0,
                      log_std=-0.5 if box else None)
    full, view, spec, P0 = canary_out(eng, T, log_prob=True)
    bufs, sview = summary_canary(eng)
    out, x, e, el, _ = run_and_check(eng, pol, T, K=1, out=view, summary_out=sview, plain=False, seed=SEED + n + T)
    check_canaries(eng, T, full, spec, P0, sampled=True)
    check_summary_canary(eng, bufs)
    if P0 > n:  # step 0 of the padding lanes: lane n - 1's input, their own words
        pad = np.arange(n, P0)
        m = pad.size
        w = words(eng, np.full((1, m), e[0, n - 1]), np.full((1, m), el[0, n - 1]), SEED + n + T, lanes=pad)
        check_rule(pol, np.repeat(x[0, n - 1:n], m, axis=0), w, full["action"][0, n:P0].cpu().numpy(),
                   full["log_prob"][0, n:P0].cpu().numpy(), np.zeros(m, np.int64))


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 7, 8, 9, 13, 17])
@pytest.mark.parametrize("step_type", list(STEP_TYPES))
def test_step_counts(step_type, T):
    launch_shape_case(step_type, 257, T)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 255, 256, 257, 4112])
@pytest.mark.parametrize("step_type", list(STEP_TYPES))
def test_lane_counts(step_type, n):
    launch_shape_case(step_type, n, 13)


# ---------------------------------------------------------------- 4. weight sets
def stacked_policy(eng, n_sets, lanes_per_set, rng, widths=(33, 7), act="relu"):
    """n_sets distinct weight sets (Box families: each with its own log_std)"""
    box = not eng.info.action_is_discrete
    sets = [make_policy(eng, widths, act, np.random.default_rng(rng.integers(1 << 30)), "all", clip=3.0,
                        log_std=LOG_STDS[s % 4] + 0.125 * s if box else None) for s in range(n_sets)]
    return MLPPolicy.stack(sets, lanes_per_set)


@pytest.mark.parametrize("lanes_per_set", [256, 512])
@pytest.mark.parametrize("step_type", ["cartpole", "pendulum", "acrobot_fast", "mountaincar_cont"])
def test_each_lane_uses_its_own_weight_set(step_type, lanes_per_set):
    n = 1000  # the last set only partly filled, and one set more than the lanes need
    family, opts = STEP_TYPES[step_type]
    eng = make_engine(family, n, seed=lanes_per_set, max_episode_steps=10, **opts)
    pol = stacked_policy(eng, -(-n // lanes_per_set) + 1, lanes_per_set, np.random.default_rng(lanes_per_set + family))
    assert 3 <= pol.n_sets <= 5
    run_and_check(eng, pol, 21, K=1, plain=False)


# ---------------------------------------------------------------- 5. engine options and offsets
SAMPLED_OPTIONS = {**OPTIONS, "lane_offset_hi": (_lib.PENDULUM, dict(lane_offset=5_000_000_000))}


@pytest.mark.parametrize("option", list(SAMPLED_OPTIONS))
def test_engine_options(option):
    family, opts = SAMPLED_OPTIONS[option]
    n = 600
    eng = make_engine(family, n, seed=7, **opts)
    rng = np.random.default_rng(7)
    if option.startswith("lane_offset"):  # the weight-set index is LOCAL: lane // lanes_per_set, whatever the offset
        run_and_check(eng, stacked_policy(eng, 3, 256, rng, widths=(31,), act="identity"), 29)
        return
    box = family in (_lib.PENDULUM, _lib.MOUNTAINCAR_CONT)
    pol = make_policy(eng, (32, 32), "relu", rng, "all", clip=2.0, log_std=-0.5 if box else None)
    run_and_check(eng, pol, 29)


@pytest.mark.parametrize("family", [_lib.CARTPOLE, _lib.ACROBOT])
def test_equal_logits_take_the_words_of_global_lanes(family):
    """an engine of n lanes at lane_offset L draws the words of global lanes L .. L + n - 1 (the counter's hi word
    non-zero): exact, as test_equal_logits_take_the_documented_words"""
    n, T, L = 512, 200 if family == _lib.CARTPOLE else 600, 5_000_000_000
    eng = make_engine(family, n, _lib.SEL_RANDOM, n_contexts=16, seed=3, lane_offset=L)
    pol = zero_head_policy(eng, widths=(8,))
    snap = eng.snapshot()
    out = eng.rollout_policy(pol, T, deterministic=False, sample_seed=SEED, log_prob=True)
    acts = out["action"][:T]
    assert bool((out["terminated"] | out["truncated"]).any()), "the launch must cross auto-resets"
    _, e, el = teacher(eng, pol, snap, acts)
    w = SR.sample_words(SEED, np.broadcast_to(L + np.arange(n, dtype=np.uint64), (T, n)), e, el)
    na = int(eng.info.n_actions)
    np.testing.assert_array_equal(acts.cpu().numpy(), SR.categorical_equal_logits(SR.u_categorical(w[0]), na))
    np.testing.assert_allclose(out["log_prob"][:T].cpu().numpy(), np.full((T, n), -np.log(na)), rtol=2.5e-7, atol=0)
    lo = SR.sample_words(SEED, np.broadcast_to(np.arange(n, dtype=np.uint64) + (L & 0xFFFFFFFF), (T, n)), e, el)
    assert (SR.categorical_equal_logits(SR.u_categorical(lo[0]), na) != acts.cpu().numpy()).mean() > 0.3
