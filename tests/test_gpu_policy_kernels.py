"""Every closed-loop policy kernel (policy_rollout_kernel<Fam, H, SUMMARY>: 6 step types x H in {0, 32, 64} x both
modes) against the exact host reference of the packed policy (oracle/carl_oracle.c: oracle_policy_forward).

Teacher forcing: the inputs are read from the engine itself, not from the policy's bookkeeping -- the launch runs from
a snapshot, the snapshot is restored, and the engine is stepped per call with the recorded actions, reading each lane's
context id and observation before each step.  identity / relu policies are compared bit for bit (+0 == -0); tanh
ones (v_exp_f32 / v_rcp_f32) within the reference's derived bound: Box actions always, discrete actions wherever the
top two float64 outputs are further apart than twice the bound (the exempted lane-steps are counted and printed).
Each case also replays the actions through carl_rollout (same bits) and checks that a summary launch is the exact
reduction of the transitions and leaves the same engine state."""
import numpy as np
import pytest
import torch

from carl_amd import _lib
from carl_amd.engine import VecEngine
from carl_amd.policy import MLPPolicy
from oracle import oracle as O
from test_gpu_policy_rollout import STATE_KEYS, OBS_NORM, context_table, defaults, engine_state, host_summary

pytestmark = pytest.mark.gpu


def assert_same_state(a, b):
    """bit for bit (a NaN context value in ctx_obs compares equal to itself)"""
    for k in STATE_KEYS:
        x, y = a[k], b[k]
        if x.dtype == torch.float32:
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), k

# step type -> (family, engine options): AcrobotFast is Acrobot under acrobot_fp32
STEP_TYPES = {"cartpole": (_lib.CARTPOLE, {}), "pendulum": (_lib.PENDULUM, {}), "acrobot": (_lib.ACROBOT, {}),
              "acrobot_fast": (_lib.ACROBOT, {"acrobot_fp32": True}), "mountaincar": (_lib.MOUNTAINCAR, {}),
              "mountaincar_cont": (_lib.MOUNTAINCAR_CONT, {})}
ACTS = ["identity", "tanh", "relu"]
CTX_MODES = ["all", "none", "one", "permuted", "repeated"]


def _matrix():
    """(widths, activation, context mode, clip, saturate) per case.  Padded hidden width H: 0 (linear), 32 (widths
    <= 32), 64.  The linear kernel takes every context mode, with and without a binding clip; the hidden shapes cycle
    through the context modes and clips; every other tanh case has saturating first-layer weights (half of them with
    a binding clip)."""
    cases = [((), "identity", ctx, 2.0 if j % 2 else None, False) for j, ctx in enumerate(CTX_MODES)]
    shapes = [(w,) for w in (1, 4, 31, 32, 33, 64)] + [(64, 64), (33, 7), (5, 64), (32, 32)]
    n_tanh = 0
    for ws in shapes:
        for a in ACTS:
            k = len(cases)
            if a == "tanh":
                cases.append((ws, a, CTX_MODES[k % 5], 2.0 if n_tanh % 4 in (1, 2) else None, n_tanh % 2 == 0))
                n_tanh += 1
            else:
                cases.append((ws, a, CTX_MODES[k % 5], 2.0 if k % 2 else None, False))
    return cases


MATRIX = _matrix()
MATRIX_IDS = [("x".join(map(str, w)) or "linear") + f"-{a}-{c}" + ("-clip" if cl else "") + ("-sat" if sat else "")
              for w, a, c, cl, sat in MATRIX]


def make_engine(family, n, selector=_lib.SEL_ROUND_ROBIN, n_contexts=64, seed=0, **opts):
    rng = np.random.default_rng(seed)
    eng = VecEngine(family, context_table(family, n_contexts, rng), n, "cuda", selector=selector,
                    auto_reset=opts.pop("auto_reset", True), seed=seed, **opts)
    eng.reset()
    return eng


def ctx_rows(eng, mode, rng):
    vis = list(eng.ctx_obs_rows)
    return {"all": vis, "none": [], "one": vis[-1:], "permuted": list(rng.permutation(vis)),
            "repeated": [vis[0], vis[-1], vis[0]]}[mode]


def make_policy(eng, widths, act, rng, ctx="all", clip=None, saturate=False, log_std=None):
    """A random policy over the given context rows, inputs centred / scaled to about +-1 (clip: a bound that binds);
    saturate: first-layer pre-activations up to 100 on the engine's current inputs (tanh then returns exactly +-1 for
    many units; first_layer_pre measures what a launch reached); log_std: a Box policy's, for sampled launches."""
    rows = ctx_rows(eng, ctx, rng)
    d = defaults(eng.family)[rows] if rows else np.zeros(0)
    o_shift, o_scale = OBS_NORM[eng.family]
    shift = np.concatenate([d, o_shift])
    scale = np.concatenate([4.0 / np.maximum(np.abs(d), 1e-3), o_scale]) * rng.uniform(0.8, 1.25, len(rows) + eng.D)
    n_out = int(eng.info.n_actions) if eng.info.action_is_discrete else 1
    dims = [len(rows) + eng.D, *widths, n_out]
    layers = [(rng.normal(0, 1.5 / np.sqrt(i), (o, i)), rng.normal(0, 0.3, o)) for i, o in zip(dims[:-1], dims[1:])]
    if saturate:
        layers[0] = saturate_units(eng, rows, shift, scale, clip, *layers[0])
    return MLPPolicy.for_env(eng, layers, act, input_shift=shift, input_scale=scale, input_clip=clip,
                             context_features=rows, log_std=log_std)


def saturate_units(eng, rows, shift, scale, clip, W, b):
    """(W, b) with each unit scaled so that its largest |pre-activation| over the lanes' current inputs is 100"""
    x0 = np.concatenate([eng.ctx_table.cpu().numpy()[rows][:, eng.ctx_idx.cpu().numpy()].T, eng.obs.cpu().numpy()], 1)
    lim = np.inf if clip is None else clip
    pre = np.clip((x0 - shift) * scale, -lim, lim) @ W.T + b
    c = 100.0 / np.maximum(np.abs(pre).max(axis=0), 1e-6)
    return W * c[:, None], b * c


def teacher_inputs(eng, pol, snap, actions):
    """[T, n, n_in] float32 inputs the policy must have seen: context values of the lane's context, then its
    observation, read from the engine before each per-call step of the recorded actions."""
    eng.restore(snap)
    tab = eng.ctx_table.cpu().numpy()
    xs = []
    for t in range(actions.shape[0]):
        cidx = eng.ctx_idx.cpu().numpy().astype(np.int64)
        obs = eng.obs.cpu().numpy()
        xs.append(np.concatenate([tab[pol.ctx_rows][:, cidx].T, obs], axis=1).astype(np.float32))
        eng.step(actions[t].contiguous())
    torch.cuda.synchronize()
    return np.stack(xs)


def first_layer_pre(pol, x, sets=None):
    """float64 first-layer pre-activations [T * n, width] of the inputs x [T, n, n_in] (one weight set)"""
    assert sets is None and pol.n_sets == 1
    z = np.clip((x.reshape(-1, x.shape[-1]).astype(np.float64) - pol.shift) * pol.scale.astype(np.float64),
                -float(pol.clip), float(pol.clip))
    W, b = pol.layers[0]
    return z @ W.astype(np.float64).T + b


# tanh over the GPU suite: discrete lane-steps exempted by the tie rule (and of those, how many the device actually
# resolved differently from the float64 argmax), the largest Box |err| / bound, the largest |pre-activation| of the
# saturated cases.  Reported at the end of the module (report_tanh_statistics).
STATS = {"exempt": 0, "exempt_disagree": 0, "lane_steps": 0, "worst_frac": 0.0, "max_pre": 0.0}


@pytest.fixture(scope="module", autouse=True)
def report_tanh_statistics(request):
    yield
    if STATS["lane_steps"] == 0 and STATS["worst_frac"] == 0.0:
        return
    line = (f"tanh policies: {STATS['exempt']} of {STATS['lane_steps']} discrete lane-steps exempted by the tie rule "
            f"({STATS['exempt_disagree']} of them resolved differently from the float64 argmax); largest Box |err| / "
            f"bound {STATS['worst_frac']:.3f}; saturated cases reached |pre-activation| {STATS['max_pre']:.1f}")
    capman = request.config.pluginmanager.getplugin("capturemanager")
    if capman is not None:
        with capman.global_and_fixture_disabled():
            print("\n" + line)
    else:
        print("\n" + line)


def check_actions(pol, x, acts, sets=None, exact=None):
    """acts [T, n] against the reference on inputs x [T, n, n_in]; sets [n]: each lane's weight set."""
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


def run_and_check(eng, pol, T, sets=None, out=None, summary_out=None, exact=None):
    """transitions launch -> teacher-forced reference, replay through rollout, summary = reduction; returns (out, the
    teacher-forced inputs [T, n, n_in])"""
    snap = eng.snapshot()
    out = eng.rollout_policy(pol, T, out=out)
    after = engine_state(eng)
    acts = out["action"][:T]
    x = teacher_inputs(eng, pol, snap, acts)
    check_actions(pol, x, acts.cpu().numpy(), sets, exact)
    eng.restore(snap)
    ref = eng.rollout(acts, out=eng.alloc_rollout(T))
    for k in ("obs", "reward", "terminated", "truncated"):
        assert torch.equal(out[k][:T], ref[k]), k
    assert_same_state(after, engine_state(eng))
    eng.restore(snap)
    if not eng.auto_reset:
        with pytest.raises(ValueError, match="auto_reset"):
            eng.rollout_policy(pol, T, mode="summary")
        return out, x
    s = eng.rollout_policy(pol, T, mode="summary", out=summary_out)
    assert_same_state(after, engine_state(eng))
    count, ret_sum, len_sum = host_summary(snap, {k: v[:T] for k, v in out.items()}, T)
    np.testing.assert_array_equal(s["episodes"].cpu().numpy(), count)
    np.testing.assert_array_equal(s["return_sum"].cpu().numpy(), ret_sum)
    np.testing.assert_array_equal(s["length_sum"].cpu().numpy(), len_sum)
    return out, x


# ---------------------------------------------------------------- a. every instance, every shape
@pytest.mark.parametrize("widths, act, ctx, clip, saturate", MATRIX, ids=MATRIX_IDS)
@pytest.mark.parametrize("step_type", list(STEP_TYPES))
def test_kernel_matrix(step_type, widths, act, ctx, clip, saturate):
    k = MATRIX.index((widths, act, ctx, clip, saturate))
    family, opts = STEP_TYPES[step_type]
    eng = make_engine(family, 1000, seed=k, **opts)
    rng = np.random.default_rng(1000 * k + family)
    pol = make_policy(eng, widths, act, rng, ctx, clip=clip, saturate=saturate)
    _, x = run_and_check(eng, pol, 37)
    if saturate:  # the first layer really reaches the saturated range
        pre = first_layer_pre(pol, x)
        STATS["max_pre"] = max(STATS["max_pre"], float(np.abs(pre).max()))
        assert np.abs(pre).max() >= 50 and (np.abs(pre) > 10).mean() >= 0.02, (np.abs(pre).max(), (np.abs(pre) > 10).mean())


@pytest.mark.parametrize("family", [_lib.PENDULUM, _lib.MOUNTAINCAR_CONT])
def test_tanh_saturates_to_exactly_one(family):
    """A Box head that reads one tanh unit (weight 1, bias 0) returns that unit's value itself: wherever the float64
    pre-activation is beyond +-10 (|v| up to ~100 here) the device's tanh must be exactly +-1 (1 - 2 / (e^20 + 1) is
    within half an ulp of 1); elsewhere within the bound (check_actions)"""
    eng = make_engine(family, 1000, seed=family)
    rng = np.random.default_rng(family)
    pol = make_policy(eng, (4,), "tanh", rng, "all", saturate=True)
    head = np.zeros((1, 4))
    head[0, 0] = 1.0
    W, b = pol.layers[0]
    b = b.copy()
    b[0] = 0.0  # unit 0: W x alone, whose inputs spread on both sides of 0
    W, b = saturate_units(eng, pol.ctx_rows, pol.shift, pol.scale, None, W.astype(np.float64), b.astype(np.float64))
    pol = MLPPolicy.for_env(eng, [(W, b), (head, np.zeros(1))], "tanh", input_shift=pol.shift,
                            input_scale=pol.scale, context_features=pol.ctx_rows)
    out, x = run_and_check(eng, pol, 37)
    pre = first_layer_pre(pol, x)[:, 0]
    a = out["action"].cpu().numpy().reshape(-1).astype(np.float64)
    hi, lo = pre > 10, pre < -10
    assert np.abs(pre).max() >= 50 and hi.sum() >= 200 and lo.sum() >= 200, (np.abs(pre).max(), hi.sum(), lo.sum())
    np.testing.assert_array_equal(a[hi], 1.0)
    np.testing.assert_array_equal(a[lo], -1.0)
    STATS["max_pre"] = max(STATS["max_pre"], float(np.abs(pre).max()))


@pytest.mark.parametrize("step_type", [s for s, (f, _) in STEP_TYPES.items() if f not in (_lib.PENDULUM, _lib.MOUNTAINCAR_CONT)])
def test_tied_head_rows_take_the_first_index(step_type):
    family, opts = STEP_TYPES[step_type]
    eng = make_engine(family, 1000, seed=3, **opts)
    rng = np.random.default_rng(3)
    pol = make_policy(eng, (33,), "tanh", rng)
    W, b = pol.layers[-1]
    W[1:] = W[0]
    b[1:] = b[0]  # every output identical: action 0, exactly
    pol = MLPPolicy.for_env(eng, pol.layers, "tanh", input_shift=pol.shift, input_scale=pol.scale,
                            context_features=pol.ctx_rows)
    out, _ = run_and_check(eng, pol, 21, exact=True)
    assert int(out["action"].abs().sum()) == 0
    if W.shape[0] == 3:  # rows 1 and 2 identical and far above row 0: action 1, never 2
        b[0] = -1e6
        pol = MLPPolicy.for_env(eng, pol.layers, "tanh", input_shift=pol.shift, input_scale=pol.scale,
                                context_features=pol.ctx_rows)
        out = eng.rollout_policy(pol, 21)
        assert bool((out["action"] == 1).all())



# ---------------------------------------------------------------- b. launch shapes
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
    """sampled: the padding lanes draw their own actions, so their first step is not lane n - 1's (the sampled module
    checks it against the reference rule instead)"""
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


def launch_shape_case(step_type, n, T):
    family, opts = STEP_TYPES[step_type]
    eng = make_engine(family, n, seed=n + T, n_contexts=max(1, min(64, n)), **opts)
    pol = make_policy(eng, (33,), "relu", np.random.default_rng(n * 31 + T), "all", clip=2.0)
    full, view, spec, P0 = canary_out(eng, T)
    bufs, sview = summary_canary(eng)
    run_and_check(eng, pol, T, out=view, summary_out=sview)
    check_canaries(eng, T, full, spec, P0)
    check_summary_canary(eng, bufs)


@pytest.mark.parametrize("T", [1, 2, 3, 5, 7, 8, 9, 13])
@pytest.mark.parametrize("step_type", list(STEP_TYPES))
def test_step_counts(step_type, T):
    launch_shape_case(step_type, 257, T)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 255, 256, 257, 4112])
@pytest.mark.parametrize("step_type", list(STEP_TYPES))
def test_lane_counts(step_type, n):
    launch_shape_case(step_type, n, 13)


# ---------------------------------------------------------------- c. weight sets
@pytest.mark.parametrize("lanes_per_set", [256, 512])
@pytest.mark.parametrize("step_type", ["cartpole", "pendulum", "acrobot", "mountaincar_cont"])
def test_each_lane_uses_its_own_weight_set(step_type, lanes_per_set):
    n = 1000  # the last set only partly filled, and one set more than the lanes need
    family, opts = STEP_TYPES[step_type]
    eng = make_engine(family, n, seed=lanes_per_set, **opts)
    n_sets = -(-n // lanes_per_set) + 1
    rng = np.random.default_rng(lanes_per_set + family)
    sets = [make_policy(eng, (33, 7), "relu", np.random.default_rng(rng.integers(1 << 30)), "all", clip=3.0)
            for _ in range(n_sets)]
    pol = MLPPolicy.stack(sets, lanes_per_set)
    run_and_check(eng, pol, 21, sets=np.arange(n) // lanes_per_set)


# ---------------------------------------------------------------- d. engine options
OPTIONS = {
    "acrobot_fp32": (_lib.ACROBOT, dict(acrobot_fp32=True)),
    "cartpole_recompute": (_lib.CARTPOLE, dict(cartpole_recompute=True)),
    "max_episode_steps_cartpole": (_lib.CARTPOLE, dict(max_episode_steps=5)),
    "max_episode_steps_pendulum": (_lib.PENDULUM, dict(max_episode_steps=5)),
    "lane_offset": (_lib.MOUNTAINCAR, dict(lane_offset=1000)),
    "sel_host": (_lib.CARTPOLE, dict(selector=_lib.SEL_HOST)),
    "sel_random": (_lib.ACROBOT, dict(selector=_lib.SEL_RANDOM)),
    "selector_stride": (_lib.ACROBOT, dict(selector_stride=3)),
    "ctx_obs_rows_subset": (_lib.CARTPOLE, dict(ctx_obs_rows=[5, 0, 3])),
    "no_auto_reset": (_lib.CARTPOLE, dict(auto_reset=False)),
}


@pytest.mark.parametrize("option", list(OPTIONS))
def test_engine_options(option):
    family, opts = OPTIONS[option]
    n = 600
    eng = make_engine(family, n, seed=7, **opts)
    rng = np.random.default_rng(7)
    if option == "lane_offset":  # the weight-set index is LOCAL: lane // lanes_per_set, whatever the offset
        sets = [make_policy(eng, (31,), "identity", np.random.default_rng(s), "all", clip=2.0) for s in range(3)]
        run_and_check(eng, MLPPolicy.stack(sets, 256), 29, sets=np.arange(n) // 256)
        return
    pol = make_policy(eng, (32, 32), "relu", rng, "all", clip=2.0)
    run_and_check(eng, pol, 29)


def test_finished_episode_log_reduces_to_the_summary():
    n, T, off = 1000, 60, 5000
    eng = make_engine(_lib.CARTPOLE, n, seed=9, lane_offset=off, fin_capacity=1 << 17)
    pol = make_policy(eng, (64,), "tanh", np.random.default_rng(9), "all", clip=2.0)
    snap = eng.snapshot()
    out = eng.rollout_policy(pol, T)
    lanes, rets, lens, dropped = (v.cpu().numpy() if hasattr(v, "cpu") else v for v in eng.drain_finished())
    assert dropped == 0 and lanes.size > n
    assert lanes.min() >= off and lanes.max() < off + n  # global lane ids
    count, ret_sum, len_sum = host_summary(snap, out, T)
    loc = (lanes - off).astype(np.int64)
    got_ret = np.zeros(n, np.float32)
    for lane, r in zip(loc, rets):  # per lane, the log holds its episodes in step order
        got_ret[lane] = np.float32(got_ret[lane] + np.float32(r))
    np.testing.assert_array_equal(np.bincount(loc, minlength=n), count)
    np.testing.assert_array_equal(np.bincount(loc, weights=lens, minlength=n).astype(np.int64), len_sum)
    np.testing.assert_array_equal(got_ret, ret_sum)
    eng.restore(snap)
    s = eng.rollout_policy(pol, T, mode="summary")
    np.testing.assert_array_equal(s["episodes"].cpu().numpy(), count)
    np.testing.assert_array_equal(s["return_sum"].cpu().numpy(), got_ret)
    np.testing.assert_array_equal(s["length_sum"].cpu().numpy(), len_sum)


# ---------------------------------------------------------------- findings: summaries without auto-reset, padding
def test_summary_without_auto_reset_is_refused_on_the_device_path():
    import ctypes as C

    eng = make_engine(_lib.CARTPOLE, 512, auto_reset=False)
    pol = make_policy(eng, (8,), "relu", np.random.default_rng(0))
    with pytest.raises(ValueError, match="auto_reset"):
        eng.rollout_policy(pol, 40, mode="summary")
    # the C entry point decides the same for a caller that does not go through VecEngine
    res = eng.alloc_policy_summary()
    params = pol.device_params(eng.device)
    p = pol.struct(eng.n, params.data_ptr())
    summ = _lib.PolicySummary(res["episodes"].data_ptr(), res["return_sum"].data_ptr(), res["length_sum"].data_ptr())
    with torch.cuda.device(eng.device):
        rc = eng.lib.carl_rollout_policy(C.byref(eng.b), C.byref(p), None, 40, C.byref(summ), eng._stream())
    torch.cuda.synchronize()
    assert rc == _lib.ERR_UNSUPPORTED, (rc, int(res["episodes"].max()))


@pytest.mark.parametrize("width", [33, 64])
@pytest.mark.parametrize("family", [_lib.CARTPOLE, _lib.PENDULUM])
def test_infinite_inputs_leave_the_padding_inert(family, width):
    """clip = inf and an input that becomes +-inf (scale = inf): every real tanh unit is exactly +-1 on both sides, so
    the head is bit-exact -- and a padded unit must not turn fma(0, inf, .) into a NaN output"""
    eng = make_engine(family, 1000, seed=width)
    rng = np.random.default_rng(width)
    D = eng.D
    scale = np.ones(D)
    scale[D - 1] = np.inf  # CartPole theta_dot, Pendulum theta_dot: non-zero after a reset
    layers = [(rng.normal(0, 1, (width, D)), rng.normal(0, 0.3, width)),
              (rng.normal(0, 1, (pol_out(eng), width)), rng.normal(0, 0.3, pol_out(eng)))]
    pol = MLPPolicy.for_env(eng, layers, "tanh", input_scale=scale, context_features=[])
    out, _ = run_and_check(eng, pol, 16, exact=True)
    a = out["action"].float()
    assert not bool(torch.isnan(a).any())


def pol_out(eng):
    return int(eng.info.n_actions) if eng.info.action_is_discrete else 1


@pytest.mark.parametrize("clip, widths, act", [(3.0, (33,), "relu"), (None, (33,), "tanh"), (None, (), "identity")])
def test_nan_and_infinite_context_values(clip, widths, act):
    """Pendulum's "gravity" feature is read by no step (the physics uses "g"): a NaN there is a NaN policy input,
    which the transform maps to -clip (fmaxf returns the operand that is not NaN); an inf one to +clip"""
    eng = make_engine(_lib.PENDULUM, 1000, seed=4)
    tab = eng.ctx_table.clone()
    tab[0, ::2] = float("nan")
    tab[0, 1::2] = float("inf")
    eng.set_contexts_device(tab, eng.ctx_idx.clone())
    eng.reset()
    rng = np.random.default_rng(4)
    n_in = 1 + eng.D
    dims = [n_in, *widths, 1]
    layers = [(rng.normal(0, 1, (o, i)), rng.normal(0, 0.3, o)) for i, o in zip(dims[:-1], dims[1:])]
    if act == "identity":  # linear: the head must see the context input, but an infinite one times w is +-inf
        clip = 3.0
    pol = MLPPolicy.for_env(eng, layers, act, input_clip=clip, context_features=[0])
    out, _ = run_and_check(eng, pol, 16, exact=True)
    assert not bool(torch.isnan(out["action"]).any())


# ---------------------------------------------------------------- e. through the user-facing API
@pytest.mark.parametrize("as_dict, features", [(True, None), (False, None), (True, ["masspole", "gravity", "length"]),
                                               (False, ["length", "tau", "gravity"]), (True, [])],
                         ids=["dict", "box", "dict-subset", "box-subset", "no-context"])
def test_rollout_policy_sees_what_flatten_observation_gives(as_dict, features):
    from carl_amd.context.context_space import UniformFloatContextFeature as U
    from carl_amd.context.sampler import ContextSampler
    from carl_amd.context.selection import StaticSelector
    from carl_amd.envs import CARLCartPole
    from carl_amd.wrappers import FlattenObservation

    n, T = 1000, 24
    sampler = ContextSampler([U("gravity", lower=5, upper=15), U("length", lower=0.3, upper=1.0),
                              U("masspole", lower=0.05, upper=0.3), U("tau", lower=0.01, upper=0.03)],
                             CARLCartPole.get_context_space(), seed=0)
    env = CARLCartPole(contexts=sampler.sample_context_table(n), num_envs=n, device="cuda:0",
                       context_selector=StaticSelector, seed=0, obs_context_as_dict=as_dict,
                       obs_context_features=features)
    flat = FlattenObservation(env)
    obs, _ = flat.reset(seed=0)
    n_in = int(obs.shape[1])
    torch.manual_seed(0)
    seq = torch.nn.Sequential(torch.nn.Linear(n_in, 33), torch.nn.ReLU(), torch.nn.Linear(33, 2))
    with torch.no_grad():
        seq[0].weight.mul_(torch.linspace(0.5, 4.0, n_in))  # every input matters, each with its own weight
    pol = MLPPolicy.from_sequential(env, seq)
    snap = env.env.snapshot()
    out = env.rollout_policy(pol, T)
    acts = out["action"]
    env.env.restore(snap)
    seq64 = seq.double()
    for t in range(T):
        x = obs.cpu().numpy().astype(np.float32)
        r = O.policy_forward(pol.params, n_in, pol.widths, pol.n_out, "relu", x)
        with torch.no_grad():
            y = seq64(torch.as_tensor(x, dtype=torch.float64)).numpy()
        np.testing.assert_allclose(y, r.y64, rtol=1e-9, atol=1e-9)  # the packed block is the Sequential
        np.testing.assert_array_equal(acts[t].cpu().numpy(), r.action, err_msg=f"step {t}")
        obs, *_ = flat.step(acts[t].contiguous())
