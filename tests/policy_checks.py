"""How a closed-loop policy test case (policy_cases.py) is run on the GPU and compared, shared by test_gpu_policy_*.py:
engine-state capture and comparison, teacher forcing, the deterministic and the sampled launch chains with their
canaries, and the episodes mode against its transitions.  STATS / SAMPLED_STATS / LAUNCHED count what the checks saw;
the module-scoped fixtures of test_gpu_policy_kernels.py and test_gpu_policy_sampled_kernels.py print them.  A plain
module: importing it allocates nothing and touches no device."""
import numpy as np
import pytest
import torch

import sampling_ref as SR
from carl_amd import _lib
from oracle import oracle as O
from policy_cases import STATE_KEYS, STEP_TYPES, host_records, host_summary, make_engine, make_policy, words


# ---------------------------------------------------------------- engine state, teacher forcing
def engine_state(eng):
    return {k: getattr(eng, k).clone() for k in STATE_KEYS}


def assert_same_state(a, b, finite=False, lanes=None):
    """two engine_state()s hold the same bits (so +0 differs from -0, and a NaN context value in ctx_obs equals itself).
    finite: every float buffer of both sides is finite as well; lanes: of those lanes only"""
    for k in STATE_KEYS:
        x, y = a[k], b[k]
        if lanes is not None:
            x, y = x[..., lanes], y[..., lanes]
        if x.is_floating_point():
            assert x.dtype == y.dtype == torch.float32, k
            assert not finite or bool(torch.isfinite(x).all() and torch.isfinite(y).all()), k
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), k


def teacher(eng, pol, snap, actions):
    """per-call replay of the recorded actions from `snap`, reading the engine before each step: the float32 inputs the
    policy must have seen [T, n, n_in] (context values of the lane's context, then its observation) and each lane-step's
    counter fields (episode index e = episode counter - 1, elapsed before the step) [T, n]"""
    eng.restore(snap)
    tab = eng.ctx_table.cpu().numpy()
    xs, es, els = [], [], []
    for t in range(actions.shape[0]):
        cidx = eng.ctx_idx.cpu().numpy().astype(np.int64)
        xs.append(np.concatenate([tab[pol.ctx_rows][:, cidx].T, eng.obs.cpu().numpy()], axis=1).astype(np.float32))
        es.append(eng.episode.cpu().numpy().astype(np.int64) - 1)
        els.append(eng.elapsed.cpu().numpy().astype(np.int64))
        eng.step(actions[t].contiguous())
    torch.cuda.synchronize()
    return np.stack(xs), np.stack(es), np.stack(els)


def replay(eng, snap, actions, stop):
    """per-call replay of the recorded actions from snap: ctx_idx before every step [T, n], and every lane's engine state
    at its own stop step"""
    eng.restore(snap)
    T = int(actions.shape[0])
    stop_d = torch.as_tensor(stop, device=eng.device)
    final = engine_state(eng)
    ctx = []
    for t in range(T):
        ctx.append(eng.ctx_idx.cpu().numpy().copy())
        eng.step(actions[t].contiguous())
        m = stop_d == t + 1
        for k in STATE_KEYS:
            final[k] = torch.where(m, getattr(eng, k), final[k])
    torch.cuda.synchronize()
    return np.stack(ctx) if ctx else np.zeros((0, eng.n), np.int32), final


# ---------------------------------------------------------------- the deterministic launch
# tanh over the deterministic checks: discrete lane-steps exempted by the tie rule (and of those, how many the device
# actually resolved differently from the float64 argmax), the largest Box |err| / bound, the largest |pre-activation|
# of the saturated cases (test_gpu_policy_kernels.py fills that one, and reports all of them at its end).
STATS = {"exempt": 0, "exempt_disagree": 0, "lane_steps": 0, "worst_frac": 0.0, "max_pre": 0.0}


def check_actions(pol, x, acts, sets=None, exact=None):
    """acts [T, n] against the exact host reference of the packed policy (oracle.policy_forward) on inputs x
    [T, n, n_in]; sets [n]: each lane's weight set.  exact (default: identity / relu policies): bit for bit (+0 == -0);
    else (tanh: v_exp_f32 / v_rcp_f32) within the reference's derived bound -- Box actions always, discrete actions
    wherever the top two float64 outputs are further apart than twice the bound (the exempted lane-steps go to STATS)."""
    T, n, n_in = x.shape
    r = O.policy_forward(pol.params, n_in, pol.widths, pol.n_out, pol.activation, x.reshape(-1, n_in),
                         None if sets is None else np.tile(sets, T))
    a = np.asarray(acts).reshape(-1)
    exact = pol.activation != "tanh" if exact is None else exact
    if exact:
        np.testing.assert_array_equal(a, r.action if pol.discrete else r.y32[:, 0])
        return
    if not pol.discrete:
        err = np.abs(a.astype(np.float64) - r.y64[:, 0])
        assert np.all(err <= r.bound[:, 0] * (1 + 1e-9)), (err.max(), r.bound[:, 0][np.argmax(err - r.bound[:, 0])])
        STATS["worst_frac"] = max(STATS["worst_frac"], float((err / np.maximum(r.bound[:, 0], 1e-300)).max()))
        return
    srt = np.sort(r.y64, axis=1)
    clear = (srt[:, -1] - srt[:, -2]) > 2 * r.bound.max(axis=1)
    np.testing.assert_array_equal(a[clear], np.argmax(r.y64, axis=1)[clear])
    STATS["exempt"] += int((~clear).sum())
    STATS["exempt_disagree"] += int((a[~clear] != np.argmax(r.y64, axis=1)[~clear]).sum())
    STATS["lane_steps"] += a.size
    assert (~clear).mean() <= 0.02, (~clear).mean()


def assert_replays(eng, out, T, after):
    """from the launch's snapshot (restored by the caller), rollout() of the recorded actions gives the launch's records
    and engine state bit for bit"""
    ref = eng.rollout(out["action"][:T], out=eng.alloc_rollout(T))
    for k in ("obs", "reward", "terminated", "truncated"):
        assert torch.equal(out[k][:T], ref[k]), k
    assert_same_state(after, engine_state(eng))


def assert_summary_reduces(eng, s, snap, out, T, after):
    """a summary launch's result s is the exact reduction of the transitions `out`, and it left the same engine state"""
    assert_same_state(after, engine_state(eng))
    count, ret_sum, len_sum = host_summary(snap, {k: v[:T] for k, v in out.items()}, T)
    np.testing.assert_array_equal(s["episodes"].cpu().numpy(), count)
    np.testing.assert_array_equal(s["return_sum"].cpu().numpy(), ret_sum)
    np.testing.assert_array_equal(s["length_sum"].cpu().numpy(), len_sum)
    return count


def check_deterministic_launch(eng, pol, T, sets=None, out=None, summary_out=None, exact=None):
    """transitions launch from a snapshot -> teacher-forced reference (the inputs are read from the engine itself, not
    from the policy's bookkeeping: check_actions), replay through rollout, summary = reduction; returns (out, the
    teacher-forced inputs [T, n, n_in])"""
    snap = eng.snapshot()
    out = eng.rollout_policy(pol, T, out=out)
    after = engine_state(eng)
    acts = out["action"][:T]
    x = teacher(eng, pol, snap, acts)[0]
    check_actions(pol, x, acts.cpu().numpy(), sets, exact)
    eng.restore(snap)
    assert_replays(eng, out, T, after)
    eng.restore(snap)
    if not eng.auto_reset:
        with pytest.raises(ValueError, match="auto_reset"):
            eng.rollout_policy(pol, T, mode="summary")
        return out, x
    s = eng.rollout_policy(pol, T, mode="summary", out=summary_out)
    assert_summary_reduces(eng, s, snap, out, T, after)
    return out, x


# ---------------------------------------------------------------- canaries round the output buffers
# the log_prob column's canary: a float32 bit pattern no log-probability of these tests takes (1.03e7), compared as int32
LOG_PROB_FILL = 0x4B1D4B1D


def canary_out(eng, T, extra_rows=3, log_prob=False):
    """rollout_policy buffers of T + extra_rows rows, NaN / 0xAB / -7 filled (log_prob: a "log_prob" column as well,
    LOG_PROB_FILL); pitch wider than n where n % 16 == 0"""
    n, P0 = eng.n, eng._row_pitch()
    P = P0 + 32 if n % 16 == 0 else P0
    adt = torch.int32 if eng.info.action_is_discrete else torch.float32
    spec = {"obs": ((eng.D,), torch.float32, float("nan")), "reward": ((), torch.float32, float("nan")),
            "terminated": ((), torch.uint8, 0xAB), "truncated": ((), torch.uint8, 0xAB),
            "action": ((), adt, -7 if adt == torch.int32 else float("nan"))}
    if log_prob:
        spec["log_prob"] = ((), torch.float32, LOG_PROB_FILL)
    full = {}
    for k, (tail, dt, fill) in spec.items():
        if dt == torch.float32 and isinstance(fill, int):  # a bit pattern
            full[k] = torch.full((T + extra_rows, P) + tail, fill, dtype=torch.int32, device=eng.device).view(dt)
        else:
            full[k] = torch.full((T + extra_rows, P) + tail, fill, dtype=dt, device=eng.device)
    return full, {k: v[:, :n] for k, v in full.items()}, spec, P0


def is_canary(t, fill):
    if t.dtype == torch.float32 and isinstance(fill, int):
        return t.view(torch.int32) == fill
    return torch.isnan(t) if t.dtype == torch.float32 and fill != fill else t == fill


def check_canaries(eng, T, full, spec, P0, sampled=False):
    """sampled: the padding lanes draw their own actions, so their first step is not lane n - 1's
    (sampled_launch_shape_case checks it against the reference rule instead)"""
    n = eng.n
    for k, t in full.items():
        fill = spec[k][2]
        assert bool(is_canary(t[T:], fill).all()), f"{k}: a row >= T was written"
        assert bool(is_canary(t[:, P0:], fill).all()), f"{k}: a column >= carl_rollout_pitch(n) was written"
        assert not bool(is_canary(t[:T, :n], fill).any()), f"{k}: a lane's record is missing"
        assert not bool(is_canary(t[:T, n:P0], fill).any()), f"{k}: a padding lane's record is missing"
    if sampled:
        return
    # the padding lanes are clones of the last lane: the same first step
    for k in ("action", "reward"):
        assert bool((full[k][0, n:P0] == full[k][0, n - 1]).all()), k


def summary_canary(eng):
    n = eng.n
    bufs = {"episodes": torch.full((n + 24,), -5, dtype=torch.int32, device=eng.device),
            "return_sum": torch.full((n + 24,), float("nan"), device=eng.device),
            "length_sum": torch.full((n + 24,), -5, dtype=torch.int32, device=eng.device)}
    return bufs, {k: v[8: 8 + n] for k, v in bufs.items()}


def check_summary_canary(eng, bufs):
    n = eng.n
    for k, b in bufs.items():
        fill = float("nan") if b.dtype == torch.float32 else -5
        assert bool(is_canary(b[:8], fill).all()) and bool(is_canary(b[8 + n:], fill).all()), k


def deterministic_launch_shape_case(step_type, n, T):
    family, opts = STEP_TYPES[step_type]
    eng = make_engine(family, n, seed=n + T, n_contexts=max(1, min(64, n)), **opts)
    pol = make_policy(eng, (33,), "relu", np.random.default_rng(n * 31 + T), "all", clip=2.0)
    full, view, spec, P0 = canary_out(eng, T)
    bufs, sview = summary_canary(eng)
    check_deterministic_launch(eng, pol, T, out=view, summary_out=sview)
    check_canaries(eng, T, full, spec, P0)
    check_summary_canary(eng, bufs)


# ---------------------------------------------------------------- the episodes mode
def exact_case(eng, pol, K, T, warm=0, transitions=None, **kw):
    """evaluate_policy against a transitions-mode rollout_policy of T = max_steps steps from the same engine state: each
    lane's first K episodes and its stop step derived from its transition rows (host_records), the recorded actions
    replayed per call for the context each episode ran in and each lane's engine state at its own stop step (replay).
    evaluate_policy from the snapshot must give all of it bit for bit: counts, steps, every record, every sentinel, the
    engine state.  Returns (the result, the counts).  transitions: (snapshot, rollout_policy output) of a launch already
    made from that snapshot, instead of a new one; kw: the sampling arguments of both launches (deterministic=False,
    sample_seed=...)"""
    if transitions is not None:
        snap, out = transitions
    else:
        if warm:  # lanes mid-episode at the launch: the running episode counts with its full length and return
            eng.rollout_policy(pol, warm, mode="summary")
        snap = eng.snapshot()
        out = eng.rollout_policy(pol, T, **kw)
    count, stop, ret, length, term, at_step = host_records(snap, out, K, T)
    ctx_before, want_state = replay(eng, snap, out["action"][:T], stop)
    cid = np.full((K, eng.n), -1, np.int32)
    has = at_step >= 0
    cid[has] = ctx_before[at_step[has], np.nonzero(has)[1]]
    eng.restore(snap)
    res = eng.evaluate_policy(pol, K, T, **kw)
    np.testing.assert_array_equal(res["episodes"].cpu().numpy(), count)
    np.testing.assert_array_equal(res["steps"].cpu().numpy(), stop)
    np.testing.assert_array_equal(res["return"].cpu().numpy().view(np.int32), ret.view(np.int32))  # NaN sentinels too
    np.testing.assert_array_equal(res["length"].cpu().numpy(), length)
    np.testing.assert_array_equal(res["context_id"].cpu().numpy(), cid)
    np.testing.assert_array_equal(res["terminated"].cpu().numpy(), term)
    assert_same_state(want_state, engine_state(eng))
    return res, count


# ---------------------------------------------------------------- the sampled launch
SAMPLED_SEED = 0x5A3D1E5EED0F
SAMPLED_VARIANTS = ("transitions_log_prob", "transitions", "summary", "episodes")
LAUNCHED = set()  # (step type, H, variant) of every sampled launch check_sampled_launch made
SAMPLED_STATS = {"exempt": 0, "lane_steps": 0, "lp_worst_frac": 0.0}


def launched(eng, pol, variant):
    if eng.family == _lib.ACROBOT and eng.b.flags & _lib.FLAG_ACROBOT_FP32:
        step_type = "acrobot_fast"
    else:
        step_type = next(s for s, (f, o) in STEP_TYPES.items() if f == eng.family and not o)
    H = 0 if not pol.widths else 32 if max(pol.widths) <= 32 else 64  # carl_policy.hip: policy_padded_hidden
    LAUNCHED.add((step_type, H, variant))


def check_rule(pol, x, w, a, lp, sets):
    """the sampling rule (include/carl_amd.h: carl_policy_sampling_t) in float64 on the exact host reference of the
    packed policy, inputs x [N, n_in] with words w (4 x [N]) and weight sets `sets` [N], against the device's actions
    a [N] and log-probabilities lp [N].
      - Categorical actions equal SR.categorical64 on y64 wherever t = u S is further than SR.categorical_tolerance from
        a prefix-sum boundary (a two-layer tanh net's forward bound alone exempts ~1e-3 of its lane-steps: per call 2e-3
        and one lane-step; counted in SAMPLED_STATS, whose share test_gpu_policy_sampled_kernels.py holds below 1e-3).
      - Box actions: |a - (y64 + sigma z64)| <= bound(y) + sigma dz + |a| 2^-23, dz = SR.gaussian_z_bound, sigma = exp of
        the lane's own set's fp32 log_std.
      - log_prob, discrete: y64[a] - logsumexp(y64) at the device's own action a.  The device computes (y_a - m) - logf(S)
        from outputs within B (the forward pass's bound) of y64: y_a - m is off by at most 2 B; every exp(y_k - m) by
        2 B relative, so S is too and log S by 2 B absolute; then a few fp32 ulps of each rounding (y_k - m, expf, the
        n - 1 sums, logf, the last subtraction) of |y_a - m|, 1 and |log_prob|: SR.categorical_log_prob_bound.
      - log_prob, Box: -z64^2 / 2 - log_std - ln(2 pi) / 2, from the words (not from (a - mu) / sigma, which loses every
        digit at small sigma).  The device's fma(-z/2, z, lp0) is off by |z| dz plus the roundings of lp0 and of the
        fma: SR.gaussian_log_prob_bound.
      Both log_prob bounds are also capped at 1e-5 abs + 1e-5 rel."""
    r = O.policy_forward(pol.params, pol.n_in, pol.widths, pol.n_out, pol.activation, x, sets)
    a = np.asarray(a).reshape(-1)
    lp = np.asarray(lp, np.float64).reshape(-1)
    if pol.discrete:
        u = SR.u_categorical(w[0]).reshape(-1).astype(np.float64)
        want, margin = SR.categorical64(r.y64, u)
        clear = margin > SR.categorical_tolerance(r.y64, r.bound)
        SAMPLED_STATS["exempt"] += int((~clear).sum())
        SAMPLED_STATS["lane_steps"] += a.size
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
    SAMPLED_STATS["lp_worst_frac"] = max(SAMPLED_STATS["lp_worst_frac"], float((err / lim).max()) if err.size else 0.0)
    assert np.all(err <= lim), (err.max(), lp[np.argmax(err / lim)], lp_ref[np.argmax(err / lim)])
    return r


def check_sampled_launch(eng, pol, T, K=2, out=None, summary_out=None, plain=True, seed=SAMPLED_SEED):
    """One chain: a transitions launch with log_prob from a snapshot, teacher-forced (inputs x, episode index e, elapsed
    before every lane-step), the words drawn with glane = lane_offset + lane, and each lane's weight set and log_std its
    own (lane // lanes_per_set): check_rule.  Then each other variant is pinned bit for bit to that launch: rollout() of
    the recorded actions (records, state); plain: the transitions launch without log_prob (actions, records, state); the
    summary launch (the exact reduction, host_summary; state); evaluate_policy(..., deterministic=False) (exact_case).
    Returns (transitions output with log_prob, x, e, el, episodes count or None)"""
    kw = dict(deterministic=False, sample_seed=seed)
    sets = np.arange(eng.n) // pol.lanes_per_set if pol.n_sets > 1 else np.zeros(eng.n, np.int64)
    snap = eng.snapshot()
    out = eng.rollout_policy(pol, T, out=out, log_prob=True, **kw)
    launched(eng, pol, "transitions_log_prob")
    after = engine_state(eng)
    acts = out["action"][:T]
    x, e, el = teacher(eng, pol, snap, acts)
    w = words(eng, e, el, seed)
    check_rule(pol, x.reshape(-1, pol.n_in), w, acts.cpu().numpy(), out["log_prob"][:T].cpu().numpy(), np.tile(sets, T))
    eng.restore(snap)
    assert_replays(eng, out, T, after)
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
    s = eng.rollout_policy(pol, T, mode="summary", out=summary_out, **kw)
    launched(eng, pol, "summary")
    assert_summary_reduces(eng, s, snap, out, T, after)
    # episodes mode: each lane's first K episodes of the same transitions
    _, ep_count = exact_case(eng, pol, K, T, transitions=(snap, out), **kw)
    launched(eng, pol, "episodes")
    return out, x, e, el, ep_count


def sampled_launch_shape_case(step_type, n, T):
    """Padding lanes (lanes [n, carl_rollout_pitch(n)) of a transitions launch's last workgroup) run as clones of lane
    n - 1: its state, context, weight set, episode index and elapsed count -- but they draw with their OWN global lane
    id lane_offset + lane.  So at step 0 a padding lane's action and log_prob are the rule applied to lane n - 1's input
    with the padding lane's words (checked with the bounds and the exemption of a real lane); later steps depend on
    those draws.  The padding columns of the action and log_prob rows are written, nothing past them and no row >= T."""
    family, opts = STEP_TYPES[step_type]
    eng = make_engine(family, n, seed=n + T, n_contexts=max(1, min(64, n)), max_episode_steps=6, **opts)
    box = family in (_lib.PENDULUM, _lib.MOUNTAINCAR_CONT)
    pol = make_policy(eng, (33,), "relu", np.random.default_rng(n * 31 + T), "all", clip=2.0,
                      log_std=-0.5 if box else None)
    full, view, spec, P0 = canary_out(eng, T, log_prob=True)
    bufs, sview = summary_canary(eng)
    seed = SAMPLED_SEED + n + T
    out, x, e, el, _ = check_sampled_launch(eng, pol, T, K=1, out=view, summary_out=sview, plain=False, seed=seed)
    check_canaries(eng, T, full, spec, P0, sampled=True)
    check_summary_canary(eng, bufs)
    if P0 > n:  # step 0 of the padding lanes: lane n - 1's input, their own words
        pad = np.arange(n, P0)
        m = pad.size
        w = words(eng, np.full((1, m), e[0, n - 1]), np.full((1, m), el[0, n - 1]), seed, lanes=pad)
        check_rule(pol, np.repeat(x[0, n - 1:n], m, axis=0), w, full["action"][0, n:P0].cpu().numpy(),
                   full["log_prob"][0, n:P0].cpu().numpy(), np.zeros(m, np.int64))
