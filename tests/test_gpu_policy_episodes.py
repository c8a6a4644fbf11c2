"""The episodes mode of the closed-loop rollout (VecEngine.evaluate_policy / carl_evaluate_policy) on the GPU, bit for bit
against the first K episodes of a transitions-mode launch from the same engine state (policy_checks.exact_case) over
step types, selectors and policy shapes; the finished-episode log, weight sets, the full size, refusals, max_steps = 0
and the env entry point.  (The observation is a function of the state: equal state bits are equal observations.)"""
import numpy as np
import pytest
import torch

from carl_amd import _lib
from carl_amd.policy import MLPPolicy, episode_stats, flattened_context_rows
from policy_cases import SELECTORS, STEP_TYPES, host_records, make_engine, make_policy, random_policy
from policy_checks import assert_same_state, engine_state, exact_case

pytestmark = pytest.mark.gpu

H_SHAPES = {0: ((), "identity"), 32: ((32,), "tanh"), 64: ((64, 33), "relu")}


# ---------------------------------------------------------------- 1 + 2. exact records and engine state
CASES = [(s, sel) for s in STEP_TYPES for sel in SELECTORS]


@pytest.mark.parametrize("step_type, sel", CASES, ids=[f"{s}-{sel}" for s, sel in CASES])
def test_records_and_state_equal_the_transitions(step_type, sel):
    """lanes 4 096 and 1 000 (a partial last workgroup), K in {1, 3}, H cycled over the cases; episodes cut at 30
    steps, so that T = 30 K + 10 lets every lane finish and T = 10 K + 5 (the cap) leaves lanes short of K"""
    c = CASES.index((step_type, sel))
    family, opts = STEP_TYPES[step_type]
    short = finished = 0
    for j, (n, K) in enumerate(((4096, 1 + 2 * (c % 2)), (1000, 3 - 2 * (c % 2)))):
        eng = make_engine(family, n, selector=SELECTORS[sel], seed=c * 7 + j, max_episode_steps=30, **opts)
        widths, act = H_SHAPES[(0, 32, 64)[(c + j) % 3]]
        pol = make_policy(eng, widths, act, np.random.default_rng(c * 13 + j), "all", clip=3.0)
        T = 10 * K + 5 if j == c % 2 else 30 * K + 10
        res, count = exact_case(eng, pol, K, T, warm=3 + c % 5)
        short += int((count < K).sum())
        finished += int(count.sum())
    assert short > 0, "the capped launch must leave some lanes short of K"
    assert finished > 0


# ---------------------------------------------------------------- 3. the finished-episode log
def test_finished_episode_log_holds_exactly_the_counted_episodes():
    n, K, T, off = 1000, 3, 400, 5000
    eng = make_engine(_lib.CARTPOLE, n, seed=9, lane_offset=off, fin_capacity=1 << 16)
    pol = make_policy(eng, (64,), "tanh", np.random.default_rng(9), "all", clip=2.0)
    eng.drain_finished()
    res = eng.evaluate_policy(pol, K, T)
    lanes, rets, lens, dropped = (v.cpu().numpy() if hasattr(v, "cpu") else v for v in eng.drain_finished())
    assert dropped == 0 and lanes.min() >= off and lanes.max() < off + n
    count = res["episodes"].cpu().numpy()
    assert int(count.sum()) == lanes.size and int((count == K).sum()) > n // 2
    ret, length = res["return"].cpu().numpy(), res["length"].cpu().numpy()
    seen = np.zeros(n, np.int64)
    for lane, r, ln in zip(lanes - off, rets, lens):  # per lane, the log holds its episodes in step order
        k = seen[lane]
        assert k < count[lane]
        assert np.float32(r).view(np.int32) == ret[k, lane].view(np.int32) and ln == length[k, lane]
        seen[lane] += 1
    np.testing.assert_array_equal(seen, count)


# ---------------------------------------------------------------- 4. weight sets
def test_each_lane_runs_its_own_weight_set():
    n, K, T = 1000, 2, 300
    eng = make_engine(_lib.ACROBOT, n, selector=_lib.SEL_ROUND_ROBIN, seed=4, max_episode_steps=60)
    sets = [make_policy(eng, (33,), "relu", np.random.default_rng(s), "all", clip=3.0) for s in range(4)]
    snap = eng.snapshot()
    res = eng.evaluate_policy(MLPPolicy.stack(sets, 256), K, T)
    after = engine_state(eng)
    for s, p in enumerate(sets):
        eng.restore(snap)
        one = eng.evaluate_policy(p, K, T)
        lanes = slice(256 * s, min(n, 256 * (s + 1)))
        for k in res:
            assert torch.equal(res[k][..., lanes], one[k][..., lanes]) or (
                k == "return" and torch.equal(res[k][..., lanes].view(torch.int32), one[k][..., lanes].view(torch.int32))), (s, k)
        assert_same_state(after, engine_state(eng), lanes=lanes)


# ---------------------------------------------------------------- 5. full size
def test_full_size_cartpole():
    n, K, T = 65536, 2, 1100
    eng = make_engine(_lib.CARTPOLE, n, selector=_lib.SEL_STATIC, n_contexts=4096, seed=21)
    pol = random_policy(eng, seed=21)  # 2 x 64 tanh
    snap = eng.snapshot()
    out = eng.rollout_policy(pol, T)
    count, stop, ret, length, term, at_step = host_records(snap, out, K, T)
    del out
    eng.restore(snap)
    res = eng.evaluate_policy(pol, K, T)
    ctx = snap["ctx_idx"].cpu().numpy()  # (a static selector: each lane keeps its context)
    np.testing.assert_array_equal(res["episodes"].cpu().numpy(), count)
    np.testing.assert_array_equal(res["steps"].cpu().numpy(), stop)
    np.testing.assert_array_equal(res["return"].cpu().numpy().view(np.int32), ret.view(np.int32))
    np.testing.assert_array_equal(res["length"].cpu().numpy(), length)
    np.testing.assert_array_equal(res["context_id"].cpu().numpy(), np.where(at_step >= 0, ctx[None, :], -1))
    np.testing.assert_array_equal(res["terminated"].cpu().numpy(), term)
    assert int(count.sum()) > n
    s = episode_stats(res, n_contexts=4096)
    assert s["count"] == count.sum() and s["context_count"].sum() == count.sum()


# ---------------------------------------------------------------- 6. refusals, max_steps = 0, the env entry point
def test_python_refusals_and_zero_steps():
    eng = make_engine(_lib.CARTPOLE, 600, seed=1)
    pol = make_policy(eng, (8,), "relu", np.random.default_rng(1))
    other = make_policy(make_engine(_lib.PENDULUM, 256, seed=1), (8,), "relu", np.random.default_rng(1))
    with pytest.raises(ValueError, match="family"):
        eng.evaluate_policy(other, 1, 10)
    with pytest.raises(ValueError, match="n_episodes"):
        eng.evaluate_policy(pol, 0, 10)
    with pytest.raises(ValueError, match="max_steps"):
        eng.evaluate_policy(pol, 1, -1)
    bad = {"wrong dtype": ("length", lambda t: t.to(torch.int64)), "wrong shape": ("return", lambda t: t[:1]),
           "missing": ("steps", None), "not contiguous": ("context_id", lambda t: t.t().contiguous().t()),
           "on the host": ("episodes", lambda t: t.cpu())}
    for case, (k, f) in bad.items():
        out = eng.alloc_policy_episodes(2)
        if f is None:
            del out[k]
        else:
            out[k] = f(out[k])
        with pytest.raises(ValueError, match="evaluate_policy output"):
            eng.evaluate_policy(pol, 2, 10, out=out)
    before = engine_state(eng)
    out = {k: v.fill_(7) for k, v in eng.alloc_policy_episodes(2).items()}  # every element is written
    res = eng.evaluate_policy(pol, 2, 0, out=out)
    assert res is out
    assert int(res["episodes"].abs().sum()) == 0 and int(res["steps"].abs().sum()) == 0
    assert bool(torch.isnan(res["return"]).all()) and int(res["length"].abs().sum()) == 0
    assert bool((res["context_id"] == -1).all()) and int(res["terminated"].sum()) == 0
    assert_same_state(before, engine_state(eng))
    eng.auto_reset = False
    with pytest.raises(ValueError, match="auto_reset"):
        eng.evaluate_policy(pol, 1, 10)


def test_env_entry_point_resets_and_counts_whole_episodes():
    from carl_amd.context.context_space import UniformFloatContextFeature as U
    from carl_amd.context.sampler import ContextSampler
    from carl_amd.context.selection import RoundRobinSelector
    from carl_amd.envs import CARLCartPole

    n, K = 2048, 3
    sampler = ContextSampler([U("length", lower=0.3, upper=1.0)], CARLCartPole.get_context_space(), seed=0)
    env = CARLCartPole(contexts=sampler.sample_context_table(16), num_envs=n, device="cuda:0",
                       context_selector=RoundRobinSelector, seed=0)
    env.reset(seed=0)
    rng = np.random.default_rng(0)
    n_in = len(flattened_context_rows(env)[0]) + 4
    pol = MLPPolicy.for_env(env, [(rng.normal(0, 1, (16, n_in)), rng.normal(0, 0.1, 16)), (rng.normal(0, 1, (2, 16)), None)],
                            "tanh", input_scale=np.r_[np.zeros(n_in - 4), np.ones(4)])
    env.rollout_policy(pol, 17, mode="summary")  # mid-episode: evaluate_policy must reset first
    eng, seen = env.env, {}
    launch = eng.evaluate_policy

    def spy(*a, **kw):  # the engine state evaluate_policy starts from
        seen["snap"] = eng.snapshot()
        return launch(*a, **kw)

    eng.evaluate_policy = spy
    res = env.evaluate_policy(pol, K, 20000, seed=3)
    del eng.evaluate_policy
    assert int(seen["snap"]["elapsed"].abs().sum()) == 0  # every lane starts a whole episode
    eng.restore(seen["snap"])
    want, _ = exact_case(eng, pol, K, int(res["steps"].max()))
    for k in res:
        assert torch.equal(res[k].view(torch.int32) if k == "return" else res[k],
                           want[k].view(torch.int32) if k == "return" else want[k]), k
    assert bool((res["episodes"] == K).all())
    s = episode_stats(res, n_contexts=16)
    assert s["count"] == n * K and s["context_count"].sum() == n * K
    r = res["return"].double().cpu().numpy().reshape(-1)
    np.testing.assert_allclose([s["mean_return"], s["std_return"]], [r.mean(), r.std()], rtol=1e-12)
