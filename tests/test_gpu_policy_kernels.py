"""Every deterministic closed-loop policy kernel (policy_rollout_kernel<Fam, H, SUMMARY>: 6 step types x H in {0, 32,
64} x both modes) against the exact host reference of the packed policy (oracle/carl_oracle.c: oracle_policy_forward),
teacher-forced from the engine itself: policy_checks.check_deterministic_launch over the shape matrix, launch shapes
with canaries, weight sets, engine options, saturated tanh, ties, non-finite inputs, and the user-facing API."""
import numpy as np
import pytest
import torch

from carl_amd import _lib
from carl_amd.policy import MLPPolicy
from oracle import oracle as O
from policy_cases import (ACTS, CTX_MODES, HIDDEN_SHAPES, OPTIONS, STEP_TYPES, first_layer_pre, host_summary, make_engine,
                          make_policy, n_outputs, saturate_units, stacked_policy)
from policy_checks import STATS, check_actions, check_deterministic_launch, deterministic_launch_shape_case

pytestmark = pytest.mark.gpu


def _matrix():
    """(widths, activation, context mode, clip, saturate) per case.  Padded hidden width H: 0 (linear), 32 (widths
    <= 32), 64.  The linear kernel takes every context mode, with and without a binding clip; the hidden shapes cycle
    through the context modes and clips; every other tanh case has saturating first-layer weights (half of them with
    a binding clip)."""
    cases = [((), "identity", ctx, 2.0 if j % 2 else None, False) for j, ctx in enumerate(CTX_MODES)]
    n_tanh = 0
    for ws in HIDDEN_SHAPES:
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


# ---------------------------------------------------------------- a. every instance, every shape
@pytest.mark.parametrize("widths, act, ctx, clip, saturate", MATRIX, ids=MATRIX_IDS)
@pytest.mark.parametrize("step_type", list(STEP_TYPES))
def test_kernel_matrix(step_type, widths, act, ctx, clip, saturate):
    k = MATRIX.index((widths, act, ctx, clip, saturate))
    family, opts = STEP_TYPES[step_type]
    eng = make_engine(family, 1000, seed=k, **opts)
    rng = np.random.default_rng(1000 * k + family)
    pol = make_policy(eng, widths, act, rng, ctx, clip=clip, saturate=saturate)
    _, x = check_deterministic_launch(eng, pol, 37)
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
    out, x = check_deterministic_launch(eng, pol, 37)
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
    out, _ = check_deterministic_launch(eng, pol, 21, exact=True)
    assert int(out["action"].abs().sum()) == 0
    if W.shape[0] == 3:  # rows 1 and 2 identical and far above row 0: action 1, never 2
        b[0] = -1e6
        pol = MLPPolicy.for_env(eng, pol.layers, "tanh", input_shift=pol.shift, input_scale=pol.scale,
                                context_features=pol.ctx_rows)
        out = eng.rollout_policy(pol, 21)
        assert bool((out["action"] == 1).all())


# ---------------------------------------------------------------- b. launch shapes, with canaries
@pytest.mark.parametrize("T", [1, 2, 3, 5, 7, 8, 9, 13])
@pytest.mark.parametrize("step_type", list(STEP_TYPES))
def test_step_counts(step_type, T):
    deterministic_launch_shape_case(step_type, 257, T)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 255, 256, 257, 4112])
@pytest.mark.parametrize("step_type", list(STEP_TYPES))
def test_lane_counts(step_type, n):
    deterministic_launch_shape_case(step_type, n, 13)


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
    check_deterministic_launch(eng, pol, 21, sets=np.arange(n) // lanes_per_set)


def test_258_weight_sets():
    """a population-sized block: workgroup w stages weight set lane_base / lanes_per_set = w for w up to 257, over two
    chunks of steps (8 + 1); relu, so every action is compared bit for bit.  The negative control: the same actions
    against each lane's neighbouring set do not pass"""
    n_sets, lanes_per_set, T = 258, 256, 9
    n = n_sets * lanes_per_set
    eng = make_engine(_lib.CARTPOLE, n, seed=258)
    pol = stacked_policy(eng, n_sets, lanes_per_set, np.random.default_rng(258))
    assert pol.n_sets == n_sets and pol.activation == "relu"
    assert np.unique(pol.params, axis=0).shape[0] == n_sets  # the sets are distinct
    sets = np.arange(n) // lanes_per_set
    out, x = check_deterministic_launch(eng, pol, T, sets=sets)
    acts = out["action"][:T].cpu().numpy()
    assert 0.2 < acts.mean() < 0.8  # (both actions occur: a wrong set is visible)
    with pytest.raises(AssertionError):
        check_actions(pol, x, acts, (sets + 1) % n_sets)


# ---------------------------------------------------------------- d. engine options
@pytest.mark.parametrize("option", list(OPTIONS))
def test_engine_options(option):
    family, opts = OPTIONS[option]
    n = 600
    eng = make_engine(family, n, seed=7, **opts)
    rng = np.random.default_rng(7)
    if option == "lane_offset":  # the weight-set index is LOCAL: lane // lanes_per_set, whatever the offset
        sets = [make_policy(eng, (31,), "identity", np.random.default_rng(s), "all", clip=2.0) for s in range(3)]
        check_deterministic_launch(eng, MLPPolicy.stack(sets, 256), 29, sets=np.arange(n) // 256)
        return
    pol = make_policy(eng, (32, 32), "relu", rng, "all", clip=2.0)
    check_deterministic_launch(eng, pol, 29)


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
              (rng.normal(0, 1, (n_outputs(eng), width)), rng.normal(0, 0.3, n_outputs(eng)))]
    pol = MLPPolicy.for_env(eng, layers, "tanh", input_scale=scale, context_features=[])
    out, _ = check_deterministic_launch(eng, pol, 16, exact=True)
    a = out["action"].float()
    assert not bool(torch.isnan(a).any())


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
    out, _ = check_deterministic_launch(eng, pol, 16, exact=True)
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
