"""The closed-loop fused rollout (VecEngine.rollout_policy / carl_rollout_policy) by its properties, with one tanh test
policy and tolerances of its own rather than the exact reference of the kernel matrices: replay of the recorded actions
is bit-exact, the actions are the policy's (float64 forward pass), context moves are seen, a known controller balances,
weight sets go to their lanes, the summary is the reduction of the transitions, and the full-size launch holds the same."""
import numpy as np
import pytest
import torch

from carl_amd import _lib
from carl_amd.engine import VecEngine
from carl_amd.policy import MLPPolicy
from policy_cases import (FAMILIES, SELECTORS, context_table, defaults, forward64, host_summary, make_engine,
                          random_policy)
from policy_checks import assert_same_state, engine_state

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- 1. replay, bit-exact
@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("sel", list(SELECTORS))
def test_replay_of_recorded_actions_is_bit_exact(family, sel):
    for n in (4096, 1000):
        for final_obs in (False, True):
            eng = make_engine(family, n, SELECTORS[sel], seed=family * 10 + n % 7)
            pol = random_policy(eng, seed=family)
            T = 48
            snap = eng.snapshot()
            out = eng.rollout_policy(pol, T, final_obs=final_obs)
            after = engine_state(eng)
            acts = out["action"]
            assert acts.dtype == (torch.int32 if eng.info.action_is_discrete else torch.float32)
            if eng.info.action_is_discrete:
                counts = torch.bincount(acts.reshape(-1).long(), minlength=int(eng.info.n_actions))
                assert int((counts > 0).sum()) >= 2, f"the test policy must vary its actions: {counts.tolist()}"
            else:
                assert float(acts.std()) > 0.1
            eng.restore(snap)
            ref_out = eng.alloc_rollout(T, final_obs=final_obs)
            ref = eng.rollout(acts, out=ref_out)
            for k in ("obs", "reward", "terminated", "truncated") + (("final_obs",) if final_obs else ()):
                assert torch.equal(out[k], ref[k]), (family, sel, n, final_obs, k)
            assert_same_state(after, engine_state(eng), finite=True)


# ---------------------------------------------------------------- 2. the action is the policy's
@pytest.mark.parametrize("family", list(FAMILIES))
def test_actions_are_the_policys(family):
    n, T = 1000, 32
    rng = np.random.default_rng(family)
    eng = VecEngine(family, context_table(family, n, rng), n, "cuda", selector=_lib.SEL_STATIC, auto_reset=True,
                    seed=3, ctx_idx0=np.arange(n))
    eng.reset()
    pol = random_policy(eng, seed=family + 100, clip=1.0)
    obs0 = eng.obs.cpu().numpy().copy()
    ctx = eng.ctx_table.cpu().numpy()[pol.ctx_rows][:, np.arange(n)].T.astype(np.float64)  # [n, n_ctx]
    out = eng.rollout_policy(pol, T)
    obs = out["obs"].cpu().numpy()
    acts = out["action"].cpu().numpy()
    near, clipped = 0, 0
    for t in range(T):
        prev = obs0 if t == 0 else obs[t - 1]
        x = np.concatenate([ctx, prev.astype(np.float64)], axis=1)
        clipped += int((np.abs((x - pol.shift) * pol.scale) > 1.0).sum())
        y = forward64(pol, x)
        if eng.info.action_is_discrete:
            top = y.max(axis=1)
            second = np.sort(y, axis=1)[:, -2]
            clear = (top - second) > 1e-4 * (1 + np.abs(top))
            near += int((~clear).sum())
            np.testing.assert_array_equal(acts[t][clear], y.argmax(axis=1)[clear], err_msg=f"step {t}")
        else:
            err = np.abs(acts[t] - y[:, 0]) / (1 + np.abs(y[:, 0]))
            assert err.max() <= 2e-5, (t, err.max())
    assert clipped > 0, "the clip of the input transform must be exercised"
    print(f"family {family}: {near} near-ties of {n * T} lane-steps")
    assert near <= 0.01 * n * T


# ---------------------------------------------------------------- 3. context moves are seen
def test_action_follows_the_context_at_each_auto_reset():
    n, T = 4096, 300
    table = np.tile(defaults(_lib.CARTPOLE), (2, 1))
    table[0, 0], table[1, 0] = 9.8, 12.0  # gravity
    eng = VecEngine(_lib.CARTPOLE, table, n, "cuda", selector=_lib.SEL_ROUND_ROBIN, auto_reset=True, seed=5)
    eng.reset()
    # a linear policy of gravity alone: y = [0, g - 10.9] -> action 1 in context 1, 0 in context 0
    pol = MLPPolicy.for_env(eng, [(np.array([[0, 0, 0, 0, 0], [1, 0, 0, 0, 0]], float), np.array([0.0, -10.9]))],
                            context_features=[0])
    c0 = eng.ctx_idx.cpu().numpy().copy()
    out = eng.rollout_policy(pol, T)
    acts = out["action"].cpu().numpy()
    done = (out["terminated"] | out["truncated"]).cpu().numpy().astype(np.int64)
    moves = np.concatenate([np.zeros((1, n), np.int64), np.cumsum(done, axis=0)[:-1]])  # resets before step t
    want = (c0[None, :] + moves) % 2
    np.testing.assert_array_equal(acts, want)
    assert done.sum() > n, "lanes must move between the contexts inside the launch"


# ---------------------------------------------------------------- 4. it controls
def test_linear_controller_keeps_the_pole_up():
    n, T = 4096, 500
    eng = VecEngine(_lib.CARTPOLE, defaults(_lib.CARTPOLE)[None], n, "cuda", selector=_lib.SEL_STATIC, auto_reset=True,
                    seed=7)
    eng.reset()
    # action 1 iff 0.1 x + 0.5 x_dot + 10 theta + 2 theta_dot > 0: keeps all 4 096 default-context lanes of the CPU
    # oracle (float64) up for 500 steps
    w = np.array([0.1, 0.5, 10.0, 2.0])
    pol = MLPPolicy.for_env(eng, [(np.stack([np.zeros(4), w]), np.zeros(2))], context_features=[])
    out = eng.rollout_policy(pol, T)
    fell = out["terminated"].any(dim=0).cpu().numpy()
    assert 1 - fell.mean() >= 0.99, fell.mean()
    zero = MLPPolicy.for_env(eng, [(np.zeros((2, 4)), np.zeros(2))], context_features=[])
    eng.reset()
    out = eng.rollout_policy(zero, T)
    assert out["terminated"].any(dim=0).float().mean().item() > 0.99  # always pushing left: every lane falls


# ---------------------------------------------------------------- 5. weight sets
@pytest.mark.parametrize("lanes_per_set", [256, 1024])
def test_each_lane_uses_its_weight_set(lanes_per_set):
    n = 4 * lanes_per_set
    eng = make_engine(_lib.PENDULUM, n, _lib.SEL_ROUND_ROBIN)
    consts = [-1.5, -0.25, 0.75, 1.75]
    sets = [MLPPolicy.for_env(eng, [(np.zeros((4, 3 + len(eng.ctx_obs_rows))), np.zeros(4)), (np.zeros((1, 4)), [c])])
            for c in consts]
    pol = MLPPolicy.stack(sets, lanes_per_set)
    out = eng.rollout_policy(pol, 24)
    want = np.repeat(np.asarray(consts, np.float32), lanes_per_set)
    np.testing.assert_array_equal(out["action"].cpu().numpy(), np.broadcast_to(want, (24, n)))


# ---------------------------------------------------------------- 6. summary = reduction of transitions
@pytest.mark.parametrize("family", [_lib.CARTPOLE, _lib.MOUNTAINCAR, _lib.PENDULUM])
def test_summary_is_the_exact_reduction_of_transitions(family):
    n, T = 4096, 240
    eng = make_engine(family, n, _lib.SEL_ROUND_ROBIN, seed=11)
    pol = random_policy(eng, seed=7, widths=(32, 32))
    snap = eng.snapshot()
    out = eng.rollout_policy(pol, T)
    after = engine_state(eng)
    eng.restore(snap)
    s = eng.rollout_policy(pol, T, mode="summary")
    assert_same_state(after, engine_state(eng), finite=True)
    count, ret_sum, len_sum = host_summary(snap, out, T)
    assert count.sum() > 0
    np.testing.assert_array_equal(s["episodes"].cpu().numpy(), count)
    np.testing.assert_array_equal(s["return_sum"].cpu().numpy(), ret_sum)
    np.testing.assert_array_equal(s["length_sum"].cpu().numpy(), len_sum)


# ---------------------------------------------------------------- 7. full size
def test_full_size_cartpole_both_modes():
    n, T = 65536, 1000
    eng = make_engine(_lib.CARTPOLE, n, _lib.SEL_RANDOM, n_contexts=4096, seed=21)
    pol = random_policy(eng, seed=21)
    snap = eng.snapshot()
    out = eng.rollout_policy(pol, T)
    after = engine_state(eng)
    eng.restore(snap)
    s = eng.rollout_policy(pol, T, mode="summary")
    assert_same_state(after, engine_state(eng), finite=True)
    assert int(s["episodes"].sum()) == int((out["terminated"] | out["truncated"]).sum())
    # replay from the snapshot; compare a seeded sample of lanes
    eng.restore(snap)
    ref = eng.rollout(out["action"])
    lanes = torch.as_tensor(np.random.default_rng(0).choice(n, 2048, replace=False), device=eng.device)
    for k in ("obs", "reward", "terminated", "truncated"):
        assert torch.equal(out[k][:, lanes], ref[k][:, lanes]), k
    assert_same_state(after, engine_state(eng), finite=True)
