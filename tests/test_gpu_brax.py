"""HIP Brax lane engine (through the C ABI) against the fp64 oracle of the same specification
(oracle/brax_spring.c).  PARITY WITH BRAX ITSELF IS UNPINNED (brax 0.12.1 is neither in the reference tree nor
installable) -- these tests pin the LDS-resident kernel against an independent fp64
implementation, per transition.

Tolerance: north_star's "within 1e-5 fp32 (bit-exact for discrete done flags ...)", asserted as a MAXIMUM of
|d| / (1 + |x|) over every observation entry and the reward of every lane-step whose DISCRETE decisions agree
with the oracle's (tests/brax_parity_util.py: the contact set of every substep, hashed on both sides, and the
`terminated` flag); lanes where a contact switched inside the rounding interval are excluded AND COUNTED
(bound: 0.5 % of lane-steps), like the threshold-edge done flags of tests/test_gpu_parity.py.  Round 2 missed the
bar (Humanoid: 11.7 % of entries beyond 1e-5) because a float32 pose carries ~1e-7 of rounding that the constraint
springs multiply by k dt / m = 20 .. 47 per substep; since round 3 the kernel holds the pose, and forms every pose
DIFFERENCE (anchor separation, relative joint rotation and its angles, contact depth, forward progress), in
float64, and keeps forces / impulses / velocities in float32 (profiles/r03_brax_parity_percentiles.txt).
Discrete outputs (truncation, counters, context ids) are exact."""
import numpy as np
import pytest
import torch

from carl_amd.envs.brax.models import ant_sys
from brax_parity_util import Parity, assert_parity, step_both
from oracle import brax as B
from oracle import oracle as O

pytestmark = pytest.mark.gpu

# per-family tolerance of the every-width test where it is not north_star's 1e-5 (filled from the measured
# profiles/r03_brax_parity_percentiles.txt; an entry here is a stated, failed bar)
TOL: dict = {}

NAMES = ["gravity", "friction", "elasticity", "ang_damping", "mass_torso", "viscosity", "target_distance",
         "target_direction", "target_radius"]
DEFAULT = np.array([-9.8, 1.0, 0.0, -0.05, 10.0, 0.0, 100.0, 1.0, 5.0])


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want) / (1.0 + np.abs(want))


def context_rows(rng, n):
    """BASELINE config 4: mass_torso ~ U(5,15), gravity ~ U(-15,-5), friction ~ U(0.3,1.5)"""
    rows = np.tile(DEFAULT, (n, 1))
    rows[:, 0] = rng.uniform(-15, -5, n)
    rows[:, 1] = rng.uniform(0.3, 1.5, n)
    rows[:, 4] = rng.uniform(5, 15, n)
    return rows.astype(np.float32).astype(np.float64)


def engine(sys_table, rows, n, device, **kw):
    from carl_amd.brax_engine import BraxVecEngine

    return BraxVecEngine(sys_table, len(NAMES), rows, n, device, **kw)


def test_reset_matches_oracle(device):
    s = ant_sys(NAMES)
    rng = np.random.default_rng(0)
    n, n_ctx = 1000, 13
    rows = context_rows(rng, n_ctx)
    kw = dict(selector=O.SEL_ROUND_ROBIN, selector_stride=2, seed=77, lane_offset=5_000_000_000)
    eng = engine(s, rows, n, device, **kw)
    ora = B.Engine(s, rows, n, **kw)
    for _ in range(2):
        obs = eng.reset().cpu().numpy()
        want = ora.reset()
        np.testing.assert_array_equal(eng.ctx_idx.cpu().numpy(), ora.ctx_idx)
        np.testing.assert_array_equal(eng.n_calls.cpu().numpy(), ora.n_calls)
        assert rel_err(eng.state_np(), ora.state).max() < 2e-6  # fp32 Box-Muller / kinematics
        assert rel_err(obs, want).max() < 5e-6
        np.testing.assert_array_equal(eng.ctx_obs.cpu().numpy(), rows[ora.ctx_idx].T.astype(np.float32))
    mask = (rng.random(n) < 0.25).astype(np.uint8)
    before = eng.state.clone()
    eng.reset(torch.as_tensor(mask))
    ora.reset(mask)
    keep = torch.as_tensor(mask == 0, device=device)
    assert torch.equal(eng.state[:, keep], before[:, keep])
    assert rel_err(eng.state_np(), ora.state).max() < 2e-6


def test_stepwise_parity_with_resync(device):
    s = ant_sys(NAMES)
    rng = np.random.default_rng(1)
    n = 2048
    rows = context_rows(rng, n)
    kw = dict(selector=O.SEL_STATIC, seed=5, ctx_idx0=np.arange(n))
    eng = engine(s, rows, n, device, max_episode_steps=40, branch_record=True, **kw)
    ora = B.Engine(s, rows, n, max_steps=40, **kw)
    eng.reset()
    ora.reset()
    par = Parity()
    for t in range(90):
        a = rng.uniform(-1.2, 1.2, (n, 8)).astype(np.float32)
        step_both(eng, ora, a, par, t)
        if par.flag_mismatch == 0:
            np.testing.assert_array_equal(eng.elapsed.cpu().numpy(), ora.elapsed)
            np.testing.assert_array_equal(eng.episodes_done.cpu().numpy(), ora.episodes_done)
    assert_parity(par, "ant")
    assert int(eng.episodes_done.sum()) >= n  # truncation at 40 + falls


def test_rollout_equals_repeated_step_bit_exact(device):
    s = ant_sys(NAMES)
    rng = np.random.default_rng(2)
    n, T = 500, 30
    rows = context_rows(rng, 7)
    acts = torch.as_tensor(rng.uniform(-1, 1, (T, n, 8)).astype(np.float32), device=device)
    kw = dict(selector=O.SEL_RANDOM, seed=3, max_episode_steps=11, fin_capacity=1 << 14)
    e1, e2 = engine(s, rows, n, device, **kw), engine(s, rows, n, device, **kw)
    e1.reset()
    e2.reset()
    out = e1.rollout(acts, e1.alloc_rollout(T, final_obs=True))
    for t in range(T):
        obs, rew, term, trunc = e2.step(acts[t])
        assert torch.equal(out["obs"][t], obs) and torch.equal(out["reward"][t], rew)
        assert torch.equal(out["terminated"][t], term) and torch.equal(out["truncated"][t], trunc)
        d = (term | trunc).bool()
        assert torch.equal(out["final_obs"][t][d], e2.final_obs[d])
    for name in ("state", "elapsed", "ctx_idx", "episode", "n_calls", "ep_return", "episodes_done", "ctx_obs"):
        assert torch.equal(getattr(e1, name), getattr(e2, name)), name
    l1, r1, n1, _ = e1.drain_finished()
    l2, r2, n2, _ = e2.drain_finished()
    assert sorted(zip(l1.tolist(), r1.tolist(), n1.tolist())) == sorted(zip(l2.tolist(), r2.tolist(), n2.tolist()))
    assert l1.numel() == int(e1.episodes_done.sum()) > 0


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float64])
def test_half_precision_actions_are_widened_once_for_the_brax_entry_points(device, dtype):
    """A policy under autocast emits float16 / bfloat16 actions.  The classic-control lean rollout reads them as they
    are (CARL_ACTION_F16 / BF16); the Brax entry points take float32 only -- the engine widens such actions once, so
    rollout / step return exactly what the float32 widening gives (it used to raise INVALID_ARGUMENT)."""
    s = ant_sys(NAMES)
    rng = np.random.default_rng(9)
    n, T = 96, 5
    rows = context_rows(rng, 5)
    a16 = torch.as_tensor(rng.uniform(-1, 1, (T, n, 8)).astype(np.float32), device=device).to(dtype)
    kw = dict(selector=O.SEL_STATIC, seed=3)
    e1, e2 = engine(s, rows, n, device, **kw), engine(s, rows, n, device, **kw)
    e1.reset()
    e2.reset()
    o1 = e1.rollout(a16)
    o2 = e2.rollout(a16.to(torch.float32))
    for k in ("obs", "reward", "terminated", "truncated"):
        assert torch.equal(o1[k], o2[k]), k
    obs1, *_ = e1.step(a16[0])
    obs2, *_ = e2.step(a16[0].float())
    assert torch.equal(obs1, obs2) and torch.equal(e1.state, e2.state)


@pytest.mark.parametrize("width", [0, 16])
def test_large_batch_fragment_schedule_equals_repeated_step_bit_exact(device, width):
    """More env groups than the chip holds wavefronts: the rollout kernel then runs as many workgroups as are resident
    and cuts each workgroup's (group, step) work into one piece per wavefront -- groups are split between two wavefronts
    at a step boundary and handed over through the state record (brax_kernels.hip.h: run(), "fragments").  A fused
    rollout must still be, bit for bit, the sequence of per-call steps (which never split a group), with episodes
    ending and auto-resetting inside the launch, and every env's counters must come out the same."""
    s = ant_sys(NAMES)
    if width:
        s.lanes_per_env = width  # 4 envs per wavefront: 7 500 groups for 30 000 envs
    rng = np.random.default_rng(12)
    n, T = 30000, 7  # 30 000 / 7 envs per wavefront = 4 286 groups > 3 072 resident wavefronts; T not a divisor of anything
    rows = context_rows(rng, 64)
    acts = torch.as_tensor(rng.uniform(-1, 1, (T, n, 8)).astype(np.float32), device=device)
    kw = dict(selector=O.SEL_ROUND_ROBIN, seed=5, max_episode_steps=5)
    e1, e2 = engine(s, rows, n, device, **kw), engine(s, rows, n, device, **kw)
    e1.reset()
    e2.reset()
    out = e1.rollout(acts, e1.alloc_rollout(T, final_obs=True))
    for t in range(T):
        obs, rew, term, trunc = e2.step(acts[t])
        assert torch.equal(out["obs"][t], obs) and torch.equal(out["reward"][t], rew), t
        assert torch.equal(out["terminated"][t], term) and torch.equal(out["truncated"][t], trunc), t
        d = (term | trunc).bool()
        assert torch.equal(out["final_obs"][t][d], e2.final_obs[d]), t
    for name in ("state", "elapsed", "ctx_idx", "episode", "n_calls", "ep_return", "episodes_done", "ctx_obs", "last_return",
                 "last_length"):
        assert torch.equal(getattr(e1, name), getattr(e2, name)), name
    assert int(e1.episodes_done.min()) >= 1  # TimeLimit 5 < T: every env finished an episode inside the launch
    # ... and a second launch continues from the first one's records
    out2 = e1.rollout(acts[:3].contiguous())
    for t in range(3):
        obs, rew, term, trunc = e2.step(acts[t])
        assert torch.equal(out2["obs"][t], obs) and torch.equal(out2["reward"][t], rew)


def test_lane_sharding_is_invariant(device):
    s = ant_sys(NAMES)
    rng = np.random.default_rng(4)
    n, T, G = 512, 12, 4
    rows = context_rows(rng, n)
    acts = torch.as_tensor(rng.uniform(-1, 1, (T, n, 8)).astype(np.float32), device=device)
    full = engine(s, rows, n, device, selector=O.SEL_STATIC, seed=8, ctx_idx0=np.arange(n))
    full.reset()
    out = full.rollout(acts)
    m = n // G
    for g in range(G):
        sl = slice(g * m, (g + 1) * m)
        sh = engine(s, rows[sl], m, device, selector=O.SEL_STATIC, seed=8, lane_offset=g * m, ctx_idx0=np.arange(m))
        sh.reset()
        o = sh.rollout(acts[:, sl].contiguous())
        assert torch.equal(o["obs"], out["obs"][:, sl]) and torch.equal(o["reward"], out["reward"][:, sl])


def test_config4_full_size_properties(device):
    """BASELINE config 4 shape on one GPU: 32 768 contexts over mass_torso / gravity / friction"""
    s = ant_sys(NAMES)
    rng = np.random.default_rng(6)
    n, T = 32768, 60
    rows = context_rows(rng, n)
    eng = engine(s, rows, n, device, selector=O.SEL_STATIC, seed=0, ctx_idx0=np.arange(n), fin_capacity=1 << 20)
    obs0 = eng.reset().clone()
    assert obs0.shape == (n, 27) and float((obs0[:, 0] - 0.55).abs().max()) <= 0.1 + 1e-5
    quat = obs0[:, 1:5]
    assert float((quat.norm(dim=1) - 1).abs().max()) < 1e-5
    acts = torch.as_tensor(rng.uniform(-1, 1, (T, n, 8)).astype(np.float32), device=device)
    out = eng.rollout(acts)
    assert torch.isfinite(out["obs"]).all() and torch.isfinite(out["reward"]).all()
    assert float((out["obs"][..., 1:5].norm(dim=-1) - 1).abs().max()) < 1e-4  # unit quaternions
    z = out["obs"][..., 0]
    term = out["terminated"].bool()
    # done rule: torso z outside [0.2, 1.0] <=> terminated (obs of done lanes is the RESET obs, so
    # check on lanes that did not finish)
    assert bool(((z >= 0.2) & (z <= 1.0))[~term].all())
    done = (out["terminated"] | out["truncated"]).bool()
    assert torch.equal(done.sum(0).to(torch.int32), eng.episodes_done)
    lanes, rets, lens, dropped = eng.drain_finished()
    assert dropped == 0 and lanes.numel() == int(done.sum())
    # the per-lane gravity context acts: under the same random policy, ants in strong gravity
    # ride lower on their springy legs than ants in weak gravity (lanes that never reset)
    g = torch.as_tensor(rows[:, 0], device=device)
    alive = eng.episodes_done == 0
    z_end = out["obs"][-1][:, 0]
    assert float(z_end[alive & (g < -12)].mean()) < float(z_end[alive & (g > -8)].mean()) - 0.005


def test_env_api(device):
    from carl_amd.context.selection import StaticSelector
    from carl_amd.envs import CARLBraxAnt

    env = CARLBraxAnt()
    assert env.observation_space["obs"].shape == (27,) and env.action_space.shape == (8,)
    env._progress_instance()
    env._update_context()
    obs, info = env.reset()
    assert obs["obs"].shape == (27,) and obs["obs"].dtype == np.float32 and info == {"context_id": 0}
    # the contexts setter fills every feature's default, goal features included (reference:
    # carl_env.py:135-137; examples/sample_contexts_with_brax.ipynb cell 7 shows all nine)
    assert list(obs["context"]) == list(CARLBraxAnt.get_context_features())
    o, r, term, trunc, info = env.step(env.action_space.sample())
    assert isinstance(r, float) and trunc is False and o["obs"].shape == (27,)
    with pytest.raises(RuntimeError):
        CARLBraxAnt(contexts={0: {"bogus": 1.0}})
    n = 256
    rows = context_rows(np.random.default_rng(0), n)
    from carl_amd.context.table import ContextTable

    benv = CARLBraxAnt(batch_size=n, contexts=ContextTable(NAMES, rows), context_selector=StaticSelector)
    obs, info = benv.reset(seed=1)
    assert obs["obs"].shape == (n, 27) and obs["context"]["gravity"].shape == (n,)
    o, r, term, trunc, info = benv.step(torch.zeros(n, 8, device=device))
    assert r.shape == (n,) and term.dtype == torch.bool
    assert benv.observation_space["obs"].shape == (n, 27) and benv.action_space.shape == (n, 8)


# ------------------------------------------------------------------ Halfcheetah
def _cheetah():
    from carl_amd.envs import CARLBraxHalfcheetahStiffness as CARLBraxHalfcheetah  # + joint_stiffness (config 5)
    from carl_amd.envs.brax.models import halfcheetah_sys

    feats = CARLBraxHalfcheetah.get_context_features()
    names = list(feats)
    default = np.array([float(f.default_value) for f in feats.values()])
    return halfcheetah_sys(names), names, default


def _cheetah_rows(rng, n, default, names):
    """BASELINE config 5 shape: joint_stiffness scale ~ U(0.5, 2), gravity ~ U(-15, -5)"""
    rows = np.tile(default, (n, 1))
    rows[:, names.index("joint_stiffness")] = rng.uniform(0.5, 2.0, n)
    rows[:, names.index("gravity")] = rng.uniform(-15, -5, n)
    return rows.astype(np.float32).astype(np.float64)


def test_halfcheetah_stepwise_parity_and_reset(device):
    from carl_amd.brax_engine import BraxVecEngine

    s, names, default = _cheetah()
    rng = np.random.default_rng(11)
    n = 2048
    rows = _cheetah_rows(rng, n, default, names)
    kw = dict(selector=O.SEL_STATIC, seed=6, ctx_idx0=np.arange(n))
    eng = BraxVecEngine(s, len(names), rows, n, device, max_episode_steps=25, branch_record=True, **kw)
    ora = B.Engine(s, rows, n, max_steps=25, **kw)
    obs = eng.reset().cpu().numpy()
    want = ora.reset()
    assert obs.shape == (n, 17) and rel_err(obs, want).max() < 5e-6
    assert rel_err(eng.state_np(), ora.state).max() < 2e-6
    par = Parity()
    for t in range(60):
        a = rng.uniform(-1.2, 1.2, (n, 6)).astype(np.float32)
        o, rew, term, trunc, out = step_both(eng, ora, a, par, t)
        assert not term.any() and not out.terminated.any()
        np.testing.assert_array_equal(eng.elapsed.cpu().numpy(), ora.elapsed)
    assert_parity(par, "halfcheetah")  # k = 15000 x up to 2 (joint_stiffness context), 16 substeps per env step
    # planar: y and the roll / yaw quaternion components stay zero
    st = eng.state64().permute(1, 2, 0)  # [link, 13, env]
    assert float(st[:, 1].abs().max()) < 1e-5 and float(st[:, 4].abs().max()) < 1e-5


def test_halfcheetah_rollout_equals_step_and_env_api(device):
    from carl_amd.brax_engine import BraxVecEngine
    from carl_amd.context.selection import StaticSelector
    from carl_amd.context.table import ContextTable
    from carl_amd.envs import CARLBraxHalfcheetah

    s, names, default = _cheetah()
    rng = np.random.default_rng(12)
    n, T = 256, 20
    rows = _cheetah_rows(rng, n, default, names)
    acts = torch.as_tensor(rng.uniform(-1, 1, (T, n, 6)).astype(np.float32), device=device)
    kw = dict(selector=O.SEL_STATIC, seed=1, ctx_idx0=np.arange(n), max_episode_steps=9)
    e1 = BraxVecEngine(s, len(names), rows, n, device, **kw)
    e2 = BraxVecEngine(s, len(names), rows, n, device, **kw)
    e1.reset()
    e2.reset()
    out = e1.rollout(acts)
    for t in range(T):
        o, r, te, tr = e2.step(acts[t])
        assert torch.equal(out["obs"][t], o) and torch.equal(out["reward"][t], r) and torch.equal(out["truncated"][t], tr)
    assert torch.equal(e1.state, e2.state)
    from carl_amd.envs import CARLBraxHalfcheetahStiffness

    env = CARLBraxHalfcheetahStiffness(batch_size=n, contexts=ContextTable(names, rows), context_selector=StaticSelector)
    obs, info = env.reset(seed=0)
    assert obs["obs"].shape == (n, 17) and env.action_space.shape == (n, 6)
    assert "joint_stiffness" in obs["context"] and obs["context"]["mass_bthigh"].shape == (n,)
    single = CARLBraxHalfcheetah()  # the reference's class: no extension feature in its context / spaces
    assert "joint_stiffness" not in single.get_context_features()
    o, _ = single.reset()
    assert o["obs"].shape == (17,)
    o, r, te, tr, _ = single.step(np.zeros(6, np.float32))
    assert te is False and tr is False


# ------------------------------------------------------------------ goal-directed mode (a14)
def test_goal_reward_epilogue_matches_oracle_and_reference_test(device):
    """BraxWalkerGoalWrapper fused into the kernels (carl/envs/brax/brax_walker_goal_wrapper.py:
    113-140).  The reference's only behavioural Brax test asserts the wrapped reward is >= 0
    over 10 x 10 random steps (test/test_language_goals.py:125-166): same assertion here, plus
    parity of reward / success / integrated position with the oracle."""
    from carl_amd.brax_engine import BraxVecEngine

    s = ant_sys(NAMES)
    s.goal_mode = 1
    rng = np.random.default_rng(21)
    n = 512
    rows = np.tile(DEFAULT, (n, 1))
    codes = np.array([1, 3, 2, 4, 12, 32, 14, 34, 112, 332, 114, 334, 212, 232, 414, 434], dtype=np.float64)
    rows[:, 6] = rng.uniform(0.05, 3.0, n)        # target_distance
    rows[:, 7] = codes[rng.integers(0, 16, n)]    # target_direction
    rows[:, 8] = rng.uniform(0.1, 0.5, n)         # target_radius
    rows = rows.astype(np.float32).astype(np.float64)
    kw = dict(selector=O.SEL_STATIC, seed=2, ctx_idx0=np.arange(n))
    eng = BraxVecEngine(s, len(NAMES), rows, n, device, max_episode_steps=60, branch_record=True, **kw)
    ora = B.Engine(s, rows, n, max_steps=60, **kw)
    eng.reset()
    ora.reset()
    n_success = 0
    par = Parity()
    for t in range(100):
        pos0 = eng.goal_pos.t().cpu().numpy().astype(np.float64)
        o, rew, term, trunc, out = step_both(eng, ora, rng.uniform(-1, 1, (n, 8)).astype(np.float32), par, t, sync_goal=True)
        assert float(rew.min()) >= 0.0  # the reference's own assertion
        ok = eng.success.cpu().numpy()
        # lanes where a contact switched within rounding this step differ in their velocities, hence in the
        # integrated position: judge the epilogue on the lanes whose branch record agrees with the oracle's
        sig = eng.branch_sig.cpu().numpy().view(np.uint32)
        same = sig[:, 0] == ora.branch_sig[:, 0]
        agree = ok == ora.success
        assert agree.mean() >= 0.999  # success flips only within rounding of the radius (1e-3 everywhere)
        n_success += int(ok.sum())
        done = ((term | trunc) != 0).cpu().numpy()
        live = same & agree & ~done  # (a done env's position is back at the origin on both sides)
        assert rel_err(eng.goal_pos.t().cpu().numpy(), ora.goal_pos)[live].max() < 1e-5
        if not agree.all():
            break
    assert n_success > 0  # some lanes with tiny target distances did reach their goal
    # the progress reward replaces the env reward: it is part of the parity record.  A success flip shows up as a
    # `terminated` mismatch and is excluded with the contact flips.
    assert_parity(par, "ant goal mode")


def test_goal_mode_through_the_env_api(device):
    """contexts whose goals differ switch the env into goal mode (carl_brax_env.py:195-223);
    info carries `success` (brax_walker_goal_wrapper.py:121,135-139)"""
    from carl_amd.envs import CARLBraxAnt

    contexts = {0: {"target_distance": 8.957, "target_direction": 112}, 1: {"target_distance": 11.77, "target_direction": 334}}
    env = CARLBraxAnt(contexts=contexts)
    assert env.env.sys.goal_mode == 1
    obs, info = env.reset()
    assert info["success"] == 0 and info["context_id"] == 0
    for _ in range(10):
        obs, r, te, tr, info = env.step(env.action_space.sample())
        assert r >= 0 and info["success"] in (0, 1)
    same = {0: {"target_distance": 5.0, "target_direction": 1}, 1: {"target_distance": 5.0, "target_direction": 1}}
    assert CARLBraxAnt(contexts=same).env.sys.goal_mode == 0
    benv = CARLBraxAnt(batch_size=64, contexts=contexts)
    obs, info = benv.reset()
    o, r, te, tr, info = benv.step(torch.zeros(64, 8, device=device))
    assert info["success"].shape == (64,) and float(r.min()) >= 0
    out = benv.env.rollout(torch.zeros(5, 64, 8, device=device))
    assert out["success"].shape == (5, 64)


# ------------------------------------------------------------------ Humanoid (BASELINE config 5)
def _humanoid():
    from carl_amd.envs import CARLBraxHumanoidStiffness as CARLBraxHumanoid  # + joint_stiffness (config 5)
    from carl_amd.envs.brax.models import humanoid_sys

    feats = CARLBraxHumanoid.get_context_features()
    names = list(feats)
    default = np.array([float(f.default_value) for f in feats.values()])
    return humanoid_sys(names), names, default


def _humanoid_rows(rng, n, default, names):
    rows = np.tile(default, (n, 1))
    rows[:, names.index("gravity")] = rng.uniform(-15, -5, n)
    rows[:, names.index("friction")] = rng.uniform(0.3, 1.5, n)
    rows[:, names.index("mass_torso")] = rng.uniform(5, 15, n)
    rows[:, names.index("mass_left_shin")] = rng.uniform(3, 6, n)
    return rows.astype(np.float32).astype(np.float64)


def test_humanoid_stepwise_parity_and_reset(device):
    """11 links with 2- and 3-dof joints, 244-dim observation (q, qd, com inertia, com velocity,
    actuator forces), COM-based forward reward, uniform velocity reset noise."""
    from carl_amd.brax_engine import BraxVecEngine

    s, names, default = _humanoid()
    rng = np.random.default_rng(31)
    n = 1024
    rows = _humanoid_rows(rng, n, default, names)
    kw = dict(selector=O.SEL_STATIC, seed=8, ctx_idx0=np.arange(n))
    eng = BraxVecEngine(s, len(names), rows, n, device, max_episode_steps=12, branch_record=True, **kw)
    ora = B.Engine(s, rows, n, max_steps=12, **kw)
    obs = eng.reset().cpu().numpy()
    want = ora.reset()
    assert obs.shape == (n, 244) and rel_err(obs, want).max() < 5e-6
    assert rel_err(eng.state_np(), ora.state).max() < 2e-6
    assert np.all(obs[:, -23:] == 0)
    par = Parity()
    for t in range(30):
        a = rng.uniform(-0.5, 0.5, (n, 17)).astype(np.float32)
        step_both(eng, ora, a, par, t)
    assert_parity(par, "humanoid")  # k_pos 20000 at dt 0.0015, 10 substeps, 2- and 3-dof joints, contacts, terminations


def test_humanoid_rollout_equals_step_and_env_api(device):
    from carl_amd.brax_engine import BraxVecEngine
    from carl_amd.context.selection import StaticSelector
    from carl_amd.context.table import ContextTable
    from carl_amd.envs import CARLBraxHumanoid

    s, names, default = _humanoid()
    rng = np.random.default_rng(32)
    n, T = 200, 12  # ragged last wavefront
    rows = _humanoid_rows(rng, n, default, names)
    acts = torch.as_tensor(rng.uniform(-0.4, 0.4, (T, n, 17)).astype(np.float32), device=device)
    kw = dict(selector=O.SEL_STATIC, seed=2, ctx_idx0=np.arange(n), max_episode_steps=7)
    e1 = BraxVecEngine(s, len(names), rows, n, device, **kw)
    e2 = BraxVecEngine(s, len(names), rows, n, device, **kw)
    e1.reset()
    e2.reset()
    out = e1.rollout(acts)
    for t in range(T):
        o, r, te, tr = e2.step(acts[t])
        assert torch.equal(out["obs"][t], o) and torch.equal(out["reward"][t], r)
        assert torch.equal(out["truncated"][t], tr) and torch.equal(out["terminated"][t], te)
    assert torch.equal(e1.state, e2.state)
    from carl_amd.envs import CARLBraxHumanoidStiffness

    env = CARLBraxHumanoidStiffness(batch_size=n, contexts=ContextTable(names, rows), context_selector=StaticSelector)
    obs, info = env.reset(seed=0)
    assert obs["obs"].shape == (n, 244) and env.action_space.shape == (n, 17)
    assert obs["context"]["mass_left_lower_arm"].shape == (n,)
    single = CARLBraxHumanoid()
    o, _ = single.reset()
    assert o["obs"].shape == (244,)
    o, r, te, tr, _ = single.step(np.zeros(17, np.float32))
    assert te is False and tr is False and 4.0 < r < 6.5  # healthy reward 5 + small forward term


# ------------------------------------------------------------------ lanes-per-env variants
def _planar(cls_name, fn_name):
    import importlib

    cls = getattr(importlib.import_module("carl_amd.envs"), cls_name)
    fn = getattr(importlib.import_module("carl_amd.envs.brax.models"), fn_name)
    feats = cls.get_context_features()
    names = list(feats)
    return fn(names), names, np.array([float(f.default_value) for f in feats.values()])


@pytest.mark.parametrize("lanes_per_env", [2, 4, 7, 9, 11, 16])
@pytest.mark.parametrize("model", ["ant", "halfcheetah", "humanoid", "hopper", "walker2d", "inverted_pendulum",
                                   "humanoidstandup", "inverted_double_pendulum", "reacher", "pusher"])
def test_every_lane_group_width_matches_oracle(device, model, lanes_per_env):
    """The host picks the lanes per env (one per link, rounded up to an instantiated width: 2, 4, 7,
    9, 11, 16) from the model and the batch size
    (carl_brax.hip: brax_lanes_per_env); `carl_brax_sys_t::lanes_per_env` pins it so that every instantiation is
    checked on every model, with a ragged last wavefront and auto-reset inside the window.  (Since round 5 a hint
    narrower than the model's link count is rounded UP to one lane per link -- the kernels keep a lane's link in
    registers -- so the small hints exercise the rounding, the large ones the wider instantiations.)"""
    from carl_amd.brax_engine import BraxVecEngine

    if model == "ant":
        s, names, default = ant_sys(NAMES), NAMES, DEFAULT
    elif model == "halfcheetah":
        s, names, default = _cheetah()
    elif model == "humanoid":
        s, names, default = _humanoid()
    elif model == "hopper":
        s, names, default = _planar("CARLBraxHopper", "hopper_sys")
    elif model == "walker2d":
        s, names, default = _planar("CARLBraxWalker2d", "walker2d_sys")
    elif model == "humanoidstandup":
        s, names, default = _planar("CARLBraxHumanoidStandup", "humanoidstandup_sys")
    elif model == "inverted_double_pendulum":
        s, names, default = _planar("CARLBraxInvertedDoublePendulum", "inverted_double_pendulum_sys")
    elif model == "reacher":
        s, names, default = _planar("CARLBraxReacher", "reacher_sys")
    elif model == "pusher":
        s, names, default = _planar("CARLBraxPusher", "pusher_sys")
    else:
        s, names, default = _planar("CARLBraxInvertedPendulum", "inverted_pendulum_sys")
    s.lanes_per_env = lanes_per_env  # the ABI's launch hint (rounded up to a width instantiated for the model)
    rng = np.random.default_rng(100 + lanes_per_env)
    n = 812 + 3  # ragged last wavefront for every width
    rows = np.tile(default, (n, 1))
    rows[:, names.index("gravity")] = rng.uniform(-15, -5, n)
    rows = rows.astype(np.float32).astype(np.float64)
    kw = dict(selector=O.SEL_STATIC, seed=9, ctx_idx0=np.arange(n))
    eng = BraxVecEngine(s, len(names), rows, n, device, max_episode_steps=4, branch_record=True, **kw)
    ora = B.Engine(s, rows, n, max_steps=4, **kw)
    obs = eng.reset().cpu().numpy()
    assert rel_err(obs, ora.reset()).max() < 5e-6
    if model == "pusher":  # even lanes: the fork sweeps into the puck within the first step (pair contacts)
        from test_brax_oracle import pusher_contact_state

        eng.set_state64(pusher_contact_state(s, n))
    lo = float(s.act_lo[0])
    par = Parity()
    for t in range(9):
        a = rng.uniform(lo, -lo, (n, s.n_act)).astype(np.float32)
        o, rew, term, trunc, out = step_both(eng, ora, a, par, t)
        done = (term.cpu().numpy() | trunc.cpu().numpy()) != 0
        if par.flag_mismatch == 0:
            # the observation returned on a done step is the reset observation of the next episode
            assert rel_err(o.cpu().numpy()[done], out.obs[done]).max(initial=0.0) < 5e-6
            np.testing.assert_array_equal(eng.elapsed.cpu().numpy(), ora.elapsed)
    # 7 335 lane-steps per case: the same excluded-share bound as the headline tests
    assert_parity(par, f"{model}/{lanes_per_env}", tol=TOL.get(model, 1e-5))


def test_new_planar_families_env_api_and_rules(device):
    """CARLBraxHopper / Walker2d / InvertedPendulum through the CARL-shaped API: spaces, context
    observation, the pitch / pole-angle health rule and the velocity clip against the oracle."""
    from carl_amd.brax_engine import BraxVecEngine
    from carl_amd.envs import CARLBraxHopper, CARLBraxInvertedPendulum, CARLBraxWalker2d

    for cls, dims in ((CARLBraxHopper, (11, 3)), (CARLBraxWalker2d, (17, 6)), (CARLBraxInvertedPendulum, (4, 1))):
        env = cls(batch_size=64, device=device)
        obs, info = env.reset(seed=0)
        assert obs["obs"].shape == (64, dims[0]) and env.action_space.shape == (64, dims[1])
        o, r, te, tr, info = env.step(torch.zeros((64, dims[1]), device=device))
        assert torch.isfinite(o["obs"]).all() and not te.any()
        single = cls()
        o, _ = single.reset()
        assert o["obs"].shape == (dims[0],)
    # hopper: a pitched, fast torso terminates and shows a clipped velocity, exactly like the oracle
    s, names, default = _planar("CARLBraxHopper", "hopper_sys")
    n = 64
    kw = dict(selector=O.SEL_STATIC, seed=3)
    eng = BraxVecEngine(s, len(names), default[None], n, device, **kw)
    ora = B.Engine(s, default[None], n, **kw)
    eng.reset()
    ora.reset()
    q = np.array(s.init_q[:6], dtype=np.float64)
    q[2] = 0.25
    qd = np.zeros(6)
    qd[0] = 50.0
    st = eng.state_np().copy()
    st[::2] = B.forward_kinematics(s, q, qd).reshape(-1)
    eng.set_state64(st)
    ora.state[:] = eng.state_np()
    a = np.zeros((n, 3), np.float32)
    o, r, te, tr = eng.step(torch.as_tensor(a))
    out = ora.step(a)
    np.testing.assert_array_equal(te.cpu().numpy(), out.terminated)
    assert te.cpu().numpy()[::2].all() and not te.cpu().numpy()[1::2].any()
    fo = eng.final_obs.cpu().numpy()
    assert np.all(fo[::2, 5] == 10.0) and rel_err(fo[::2], out.final_obs[::2]).max() < 1e-4


def test_config5_full_size_properties(device):
    """BASELINE config 5 shape on one GPU: Halfcheetah + Humanoid, 32 768 contexts each (65 536
    together) with joint_stiffness variation; episodic returns gathered with the reporting helper
    (an RCCL all-gather under torchrun, the identity in one process)."""
    from carl_amd.brax_engine import BraxVecEngine
    from carl_amd.distributed import all_gather_episode_stats, reduce_episode_summary

    n, T = 32768, 24
    rng = np.random.default_rng(50)
    for make, n_act, lo in ((_cheetah, 6, 1.0), (_humanoid, 17, 0.4)):
        s, names, default = make()
        rows = np.tile(default, (n, 1))
        js = names.index("joint_stiffness")
        rows[:, js] = rng.uniform(0.5, 2.0, n)
        rows[:, names.index("gravity")] = rng.uniform(-15, -5, n)
        rows = rows.astype(np.float32).astype(np.float64)
        eng = BraxVecEngine(s, len(names), rows, n, device, selector=O.SEL_STATIC, seed=0, ctx_idx0=np.arange(n),
                            max_episode_steps=16)
        eng.reset()
        acts = torch.as_tensor(rng.uniform(-lo, lo, (T, n, n_act)).astype(np.float32), device=device)
        out = eng.rollout(acts)
        assert torch.isfinite(out["obs"]).all() and torch.isfinite(out["reward"]).all()
        done = (out["terminated"] | out["truncated"]).bool()
        assert torch.equal(done.sum(0).to(torch.int32), eng.episodes_done)
        assert int(out["truncated"][15].sum()) >= int(0.5 * n)  # TimeLimit(16) fires at step index 15 for survivors
        # the per-env joint_stiffness context acts: softer constraint springs let the joints separate
        # more under the same load -> larger anchor gap (measured on the final state, non-root joints)
        st = eng.state64().cpu().numpy()
        soft, stiff = rows[:, js] < 0.7, rows[:, js] > 1.6
        gaps = []
        for sel in (soft, stiff):
            idx = np.nonzero(sel)[0][:256]
            g = []
            for e in idx:
                q, qd = B.inverse_kinematics(s, st[e].reshape(-1))
                re = B.forward_kinematics(s, q, qd).reshape(s.n_links, 13)  # the nearest consistent pose
                g.append(np.abs(re[:, :3] - st[e][:, :3]).max())
            gaps.append(np.mean(g))
        assert gaps[0] > 1.3 * gaps[1], gaps
        stats = all_gather_episode_stats(eng)
        assert stats["last_return"].shape == (n,) and int(stats["episodes_done"].sum()) == int(done.sum())
        summary = reduce_episode_summary(eng)
        assert summary["episodes"] == float(done.sum()) and summary["mean_length"] <= 16


def test_lane_width_is_a_pure_scheduling_choice_and_autotune_restores_state(device):
    """Every launchable lane-group width produces bit-identical transitions (same per-link
    arithmetic, same summation order), so ``BraxVecEngine.autotune`` may pick by time alone; the
    probe must leave all engine state untouched."""
    from carl_amd.brax_engine import BraxVecEngine

    s, names, default = _humanoid()
    rng = np.random.default_rng(77)
    n, T = 333, 6
    rows = _humanoid_rows(rng, n, default, names)
    acts = torch.as_tensor(rng.uniform(-0.4, 0.4, (T, n, 17)).astype(np.float32), device=device)
    ref = None
    for hint in [0] + BraxVecEngine(s, len(names), rows, n, device).lane_widths():
        eng = BraxVecEngine(s, len(names), rows, n, device, selector=O.SEL_STATIC, seed=3, ctx_idx0=np.arange(n),
                            max_episode_steps=4)
        eng.sys.lanes_per_env = hint
        eng.reset()
        out = eng.rollout(acts)
        cur = (out["obs"].clone(), out["reward"].clone(), out["terminated"].clone(), eng.state.clone())
        if ref is None:
            ref = cur
        else:
            assert all(torch.equal(a, b) for a, b in zip(ref, cur)), hint
    s2 = ant_sys(NAMES)
    eng = engine(s2, context_rows(rng, 512), 512, device, selector=O.SEL_STATIC, seed=1, ctx_idx0=np.arange(512),
                 branch_record=True)
    assert eng.lane_widths() == [9, 16]  # one lane per link or wider
    eng.reset()
    eng.step(torch.zeros((512, 8), device=device))
    before = {k: getattr(eng, k).clone() for k in ("state", "elapsed", "episode", "n_calls", "ep_return", "obs", "reward",
                                                   "terminated", "truncated", "done", "branch_sig")}
    rng_state = torch.cuda.get_rng_state(torch.device(device))
    best = eng.autotune()
    assert best in eng.lane_widths() and eng.sys.lanes_per_env == best and set(eng.autotune_ms) == set(eng.lane_widths())
    assert all(torch.equal(v, getattr(eng, k)) for k, v in before.items())
    assert torch.equal(rng_state, torch.cuda.get_rng_state(torch.device(device)))  # the caller's RNG stream is untouched
    assert set(eng._tuned) == {False, True}  # both launch-length classes probed HERE: step / rollout never stop to probe
    # a probe launch that raises leaves the engine as it was: width, state, and the probing switch
    width = int(eng.sys.lanes_per_env)
    real, calls = eng.rollout, [0]

    def failing_rollout(*a, **k):
        calls[0] += 1
        if calls[0] == 3:  # (the second width's warm-up launch)
            raise RuntimeError("probe launch failed")
        return real(*a, **k)

    eng.rollout = failing_rollout
    with pytest.raises(RuntimeError, match="probe launch failed"):
        eng._probe_widths(2, 1)
    del eng.rollout
    assert int(eng.sys.lanes_per_env) == width and not eng._tuning
    assert all(torch.equal(v, getattr(eng, k)) for k, v in before.items())
    eng.step(torch.zeros((512, 8), device=device))  # and keeps working


def test_snapshot_restores_branch_sig_and_dense_rows_are_required(device):
    """``snapshot`` / ``restore`` -- the one list of buffers a launch writes (``capture_step``'s warm-up, ``autotune``'s
    probes) -- include the per-step branch signature; and a Brax rollout into rows padded beyond the lane count (the
    classic families' staged layout) is refused with a ValueError before anything is padded or launched."""
    s = ant_sys(NAMES)
    rng = np.random.default_rng(31)
    n, T = 333, 3
    eng = engine(s, context_rows(rng, n), n, device, selector=O.SEL_STATIC, seed=2, ctx_idx0=np.arange(n),
                 branch_record=True)
    eng.reset()
    eng.branch_sig.fill_(-1)  # (no hash of a step: the step below overwrites every lane's record)
    snap = eng.snapshot()
    assert "branch_sig" in snap
    eng.step(torch.as_tensor(rng.uniform(-1, 1, (n, 8)).astype(np.float32), device=device))
    assert not torch.equal(eng.branch_sig, snap["branch_sig"])
    eng.restore(snap)
    for k, v in snap.items():
        assert torch.equal(getattr(eng, k), v), k
    P = (n + 15) // 16 * 16
    padded = {"obs": torch.zeros((T, P, eng.D), device=device)[:, :n], "reward": torch.zeros((T, P), device=device)[:, :n],
              "terminated": torch.zeros((T, P), dtype=torch.uint8, device=device)[:, :n],
              "truncated": torch.zeros((T, P), dtype=torch.uint8, device=device)[:, :n]}
    acts = torch.as_tensor(rng.uniform(-1, 1, (T, n, 8)).astype(np.float32), device=device)
    with pytest.raises(ValueError, match="dense rows only"):
        eng.rollout(acts, padded)
    torch.cuda.synchronize()
    for k, v in snap.items():  # nothing launched
        assert torch.equal(getattr(eng, k), v), k
    assert not any(bool(t.any()) for t in padded.values())


def test_reacher_env_api_and_goal_stays_put(device):
    """CARLBraxReacher through the CARL-shaped API (reference class carl/envs/brax/carl_reacher.py:9-39):
    spaces, goal inside the 0.2 disc and fixed over an episode, reward = -distance - |a|^2, no
    termination; mass context reaches the physics (a heavier arm swings less under the same torque)."""
    from carl_amd.envs import CARLBraxReacher

    n = 256
    env = CARLBraxReacher(batch_size=n, device=device)
    obs, info = env.reset(seed=0)
    o0 = obs["obs"].cpu().numpy().astype(np.float64)
    assert o0.shape == (n, 11) and env.action_space.shape == (n, 2)
    assert np.hypot(o0[:, 4], o0[:, 5]).max() <= 0.2
    g = torch.Generator(device="cpu").manual_seed(0)
    for t in range(30):
        a = (torch.rand((n, 2), generator=g) * 2 - 1).to(device)
        o, r, te, tr, info = env.step(a)
        on = o["obs"].cpu().numpy().astype(np.float64)
        np.testing.assert_allclose(on[:, 4:6], o0[:, 4:6], atol=2e-4)
        want = -np.linalg.norm(on[:, 8:11], axis=1) - (a.cpu().numpy().astype(np.float64) ** 2).sum(1)
        np.testing.assert_allclose(r.cpu().numpy(), want, rtol=1e-5, atol=1e-5)
        assert not te.any() and not tr.any()
    single = CARLBraxReacher()
    o, _ = single.reset()
    assert o["obs"].shape == (11,)


def test_pusher_env_api_goal_context_and_contact(device):
    """CARLBraxPusher through the CARL-shaped API (reference class carl/envs/brax/carl_pusher.py:9-103):
    spaces, the goal_position_* context shows up as the observation's goal block and moves the reward,
    the puck keeps 0.17 from the goal at reset, and the fork pushes the puck on the device as it does in
    the oracle (bit-for-bit the same contact set: compared through the puck's displacement)."""
    from carl_amd.brax_engine import BraxVecEngine
    from carl_amd.envs import CARLBraxPusher
    from test_brax_oracle import pusher_contact_state

    feats = CARLBraxPusher.get_context_features()
    names = list(feats)
    default = {k: float(f.default_value) for k, f in feats.items()}
    n = 64
    contexts = {i: dict(default, gravity=-1e-6, goal_position_x=0.2 + 0.005 * i, goal_position_y=0.05 - 0.003 * i)
                for i in range(n)}
    env = CARLBraxPusher(contexts=contexts, batch_size=n, device=device)
    obs, info = env.reset(seed=0)
    o = obs["obs"].cpu().numpy().astype(np.float64)
    assert o.shape == (n, 23) and env.action_space.shape == (n, 7)
    cid = info["context_id"].cpu().numpy()
    np.testing.assert_allclose(o[:, 20], 0.2 + 0.005 * cid, rtol=1e-6)
    np.testing.assert_allclose(o[:, 21], 0.05 - 0.003 * cid, rtol=1e-5, atol=1e-7)
    assert np.hypot(o[:, 17] - o[:, 20], o[:, 18] - o[:, 21]).min() >= 0.17 - 1e-6
    a = torch.zeros((n, 7), device=device)
    o2, r, te, tr, _ = env.step(a)
    on = o2["obs"].cpu().numpy().astype(np.float64)
    want = -np.linalg.norm(on[:, 17:20] - on[:, 20:23], axis=1) - 0.5 * np.linalg.norm(on[:, 17:20] - on[:, 14:17], axis=1)
    np.testing.assert_allclose(r.cpu().numpy(), want, rtol=1e-5, atol=1e-5)
    assert not te.any() and not tr.any()
    # contact on the device vs the oracle, free-running for 8 steps
    s, names, dflt = _planar("CARLBraxPusher", "pusher_sys")
    rows = dflt[None].copy()
    rows[:, 0] = -1e-6
    m = 32
    kw = dict(selector=O.SEL_STATIC, seed=1)
    eng = BraxVecEngine(s, len(names), rows, m, device, **kw)
    ora = B.Engine(s, rows, m, **kw)
    eng.reset()
    ora.reset()
    st = pusher_contact_state(s, m)
    eng.set_state64(st)
    ora.state[:] = eng.state_np()
    act = np.zeros((m, 7), np.float32)
    act[:, 0] = 2.0
    for t in range(8):
        eng.step(torch.as_tensor(act))
        ora.step(act)
    got = eng.state_np().reshape(m, 8, 13)[:, 7, :3]
    wnt = ora.state.reshape(m, 8, 13)[:, 7, :3]
    assert np.all(got[0::2, 1] - st.reshape(m, 8, 13)[0::2, 7, 1] > 0.08)
    np.testing.assert_allclose(got, wnt, atol=2e-4)


def test_reference_brax_env_test_over_every_class(device):
    """The reference's own Brax test (test/test_brax_env.py:8-23), statement for statement, on this
    package: every CARL class exported by ``envs.brax`` builds with its defaults, progresses its
    instance, updates its context and resets.  (Plus: all ten reference classes are there, and the
    default reset observation has the class's dimension and is finite.)"""
    import inspect

    import carl_amd.envs.brax as brax_envs

    seen = []
    for env_name, env_obj in inspect.getmembers(brax_envs):
        if inspect.isclass(env_obj) and "CARL" in env_name and env_name != "CARLBraxEnv":
            env_obj.get_context_features()
            env = env_obj()
            env._progress_instance()
            env._update_context()
            obs, info = env.reset()
            assert np.isfinite(obs["obs"]).all() and obs["obs"].shape == env.observation_space["obs"].shape
            seen.append(env_name)
    # the reference's ten classes, plus this build's two opt-in variants with the joint_stiffness feature
    assert sorted(seen) == sorted(
        ["CARLBrax" + n for n in ("Ant", "Halfcheetah", "Hopper", "Humanoid", "HumanoidStandup", "InvertedDoublePendulum",
                                  "InvertedPendulum", "Pusher", "Reacher", "Walker2d")]
        + ["CARLBraxHalfcheetahStiffness", "CARLBraxHumanoidStiffness"])


def test_language_goals_as_the_reference_tests_them(device):
    """test/test_language_goals.py:86-121 (wrapper selection: ``position`` is None before reset, set after)
    and :170-260 (TestLanguageWrapper: ``state["obs"]["goal"]`` is a string naming the context's distance
    and direction on reset and on every step; without ``use_language_goals`` there is no goal entry),
    with the reference's own context sampling."""
    from carl_amd.context.context_space import CategoricalContextFeature, NormalFloatContextFeature
    from carl_amd.context.sampler import ContextSampler
    from carl_amd.envs import CARLBraxAnt, CARLBraxHalfcheetah
    from carl_amd.envs.brax.brax_walker_goal_wrapper import DIRECTION_NAMES, directions

    def sampled(cls):
        dists = [NormalFloatContextFeature("target_distance", mu=9.8, sigma=1, upper=50, lower=-40),
                 CategoricalContextFeature("target_direction", choices=directions)]
        return ContextSampler(context_distributions=dists, context_space=cls.get_context_space(),
                              seed=0).sample_contexts(n_contexts=10)

    for cls in (CARLBraxAnt, CARLBraxHalfcheetah):
        env = cls(contexts=sampled(cls), use_language_goals=True)
        assert env.env.sys.goal_mode == 1 and env.position is None
        state, info = env.reset()
        assert env.position is not None and info is not None
        for _ in range(10):
            assert type(state) is dict and type(state["obs"]) is dict and type(state["obs"]["goal"]) is str
            goal = state["obs"]["goal"]
            assert str(env.context["target_distance"]) in goal and DIRECTION_NAMES[env.context["target_direction"]] in goal
            assert goal.startswith("The distance to the goal is ") and "Move within" in goal
            assert state["obs"]["obs"].shape == env.observation_space["obs"].shape
            state, _, _, _, _ = env.step(env.action_space.sample())
        plain = cls(contexts=sampled(cls))
        state, _ = plain.reset()
        for _ in range(3):
            assert "goal" not in state and not isinstance(state["obs"], dict)
            state, _, _, _, _ = plain.step(plain.action_space.sample())
    # a batch: one sentence per env, following the envs' context ids
    contexts = sampled(CARLBraxAnt)
    benv = CARLBraxAnt(batch_size=32, contexts=contexts, use_language_goals=True)
    obs, info = benv.reset(seed=0)
    texts, ids = obs["obs"]["goal"], info["context_id"].tolist()
    assert len(texts) == 32 and obs["obs"]["obs"].shape == (32, 27) and benv.position.shape == (32, 2)
    keys = list(contexts)
    for t, cid in zip(texts, ids):
        assert t == CARLBraxAnt.describe_goal(benv.contexts[keys[cid]])
    # goals that do not vary: no goal wrapper, hence no language wrapper either (carl_brax_env.py:216-218)
    same = {0: {"target_distance": 5.0, "target_direction": 1}, 1: {"target_distance": 5.0, "target_direction": 1}}
    env = CARLBraxAnt(contexts=same, use_language_goals=True)
    state, _ = env.reset()
    assert not isinstance(state["obs"], dict) and env.position is None


def test_every_mass_feature_at_the_reference_lower_bound_constructs_and_stays_finite(device):
    """The reference accepts any ``mass_<link>`` in (0.1, inf) (carl/envs/brax/carl_halfcheetah.py:37-57) -- there
    the value never reaches the physics (Quirk B1); here it does, and below a model-specific fraction of its
    default the explicit spring integration would blow up.  Default ``mass_check="warn"``: every such context
    CONSTRUCTS, the kernel runs the env at the stability floor (carl_brax_ctx_map_t::mass_ratio_floor), the
    context observation keeps the sampled value, one RuntimeWarning names the features; "error" refuses."""
    import inspect
    import warnings

    import carl_amd.envs.brax as brax_envs
    from carl_amd.envs.brax.feature_tables import MASS_BOUNDS

    lower = float(MASS_BOUNDS[0])
    n_classes = 0
    for env_name, cls in inspect.getmembers(brax_envs):
        if not (inspect.isclass(cls) and "CARL" in env_name and env_name != "CARLBraxEnv"):
            continue
        feats = cls.get_context_features()
        mass = [k for k in feats if k.startswith("mass_")]
        if not mass:
            continue
        n_classes += 1
        default = {k: float(f.default_value) for k, f in feats.items() if k not in ("target_distance", "target_direction", "target_radius")}
        # one context per mass feature at the bound, plus one with ALL of them there
        contexts = {i: dict(default, **{m: lower * 1.001}) for i, m in enumerate(mass)}
        contexts[len(mass)] = dict(default, **{m: lower * 1.001 for m in mass})
        n = len(contexts)
        with pytest.warns(RuntimeWarning, match="stays stable"):
            env = cls(contexts=contexts, batch_size=n, device=device, seed=0)
        with pytest.raises(ValueError):
            cls(contexts=contexts, batch_size=n, device=device, seed=0, mass_check="error")
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # contexts at the defaults: silent
            cls(batch_size=2, device=device)
        obs, info = env.reset(seed=0)
        cid = info["context_id"].cpu().numpy()
        for i, m in enumerate(mass):  # the observation shows what was sampled, not the clamp
            assert float(obs["context"][m][cid == i][0]) == pytest.approx(lower * 1.001, rel=1e-6)
        g = torch.Generator(device="cpu").manual_seed(1)
        lo, hi = env.action_space.low[0], env.action_space.high[0]
        for t in range(60):
            a = torch.rand((n, env.action_space.shape[1]), generator=g) * float(hi[0] - lo[0]) + float(lo[0])
            o, r, te, tr, _ = env.step(a.to(device))
            assert bool(torch.isfinite(o["obs"]).all()) and bool(torch.isfinite(r).all()), (env_name, t)
    assert n_classes >= 10


def wide_brax_rows(rng, n, default, names, fam):
    """context rows far outside BASELINE's distributions but inside the reference's declared bounds (carl_ant.py:21-49 and the
    like): gravity log-uniform in [-50, -2], friction in [0.1, 10], elasticity U(0, 0.8), ang_damping U(-0.5, 0), every link mass
    x [1, 3] (lighter links: the documented stability floors), joint_stiffness up to the model's measured ceiling"""
    from carl_amd.envs.brax.feature_tables import JOINT_STIFFNESS_CEILING

    def logu(lo, hi):
        return np.exp(rng.uniform(np.log(lo), np.log(hi), n))

    rows = np.tile(default, (n, 1))
    rows[:, names.index("gravity")] = -logu(2.0, 50.0)
    rows[:, names.index("friction")] = logu(0.1, 10.0)
    rows[:, names.index("elasticity")] = rng.uniform(0.0, 0.8, n)
    if "ang_damping" in names:
        rows[:, names.index("ang_damping")] = -rng.uniform(0.0, 0.5, n)
    for k, nm in enumerate(names):
        if nm.startswith("mass_"):
            rows[:, k] = default[k] * logu(1.0, 3.0)
    if "joint_stiffness" in names:
        rows[:, names.index("joint_stiffness")] = logu(0.3, JOINT_STIFFNESS_CEILING.get(fam, 2.0))
    return rows.astype(np.float32).astype(np.float64)


def brax_wide_context_case(cls, n, steps, rng, device):
    """free-run `steps` env steps from reset under random actions, then re-compute ONE env step of every lane with the float64
    restatement from the engine's own state: (error per lane, agreeing-lane mask, blown-up mask)"""
    from carl_amd.brax_engine import BraxVecEngine
    from carl_amd.envs.brax.models import SYSTEMS

    feats = cls.get_context_features()
    names = list(feats)
    default = np.array([float(f.default_value) for f in feats.values()])
    fam = cls.env_name
    s = SYSTEMS[fam](names)
    amp = 0.4 if "humanoid" in fam else 1.0
    rows = wide_brax_rows(rng, n, default, names, fam)
    eng = BraxVecEngine(s, len(names), rows, n, device, selector=O.SEL_STATIC, seed=1, ctx_idx0=np.arange(n), auto_reset=False,
                        max_episode_steps=10_000, branch_record=True)
    eng.reset()
    g = torch.Generator(device=device).manual_seed(3)
    for _ in range(steps):
        eng.step((torch.rand((n, s.n_act), generator=g, device=device) * 2 - 1) * amp)
    st = eng.state_np()
    fin0 = np.isfinite(st.reshape(n, -1)).all(1)
    ora = B.Engine(s, rows, n, selector=O.SEL_STATIC, ctx_idx0=np.arange(n), autoreset=False, max_steps=10_000)
    ora.reset()
    ora.state[:] = np.where(fin0.reshape((n,) + (1,) * (st.ndim - 1)), st, ora.state)
    ora.elapsed[:] = eng.elapsed.cpu().numpy()
    a = (rng.uniform(-1, 1, (n, s.n_act)) * amp).astype(np.float32)
    obs, rew, term, trunc = eng.step(torch.as_tensor(a))
    out = ora.step(a)
    sig = eng.branch_sig.cpu().numpy().view(np.uint32)
    o = obs.cpu().numpy()
    fin = fin0 & np.isfinite(o).all(1) & np.isfinite(out.obs).all(1) & (np.abs(o).max(1) < 1e4)
    flag = (term.cpu().numpy() != 0) != (out.terminated != 0)
    agree = (sig[:, 0] == ora.branch_sig[:, 0]) & ~flag & fin
    e = np.where(fin, np.maximum(rel_err(o, out.obs).max(1), rel_err(rew.cpu().numpy(), out.reward)), 0.0)
    return e, agree, ~fin, rows, names


def test_every_brax_class_over_wide_contexts(device):
    """All twelve classes (the ten reference classes + the two ...Stiffness variants) far outside BASELINE's context distributions (`wide_brax_rows`): no env leaves the finite range,
    the excluded share (contact record / flag differs) stays below 1e-3, and north_star's 1e-5 holds as a MAXIMUM on the
    agreeing lanes -- with ONE recorded exception: a Humanoid under 2.5-5 g whose joints are stiffened x 3-6
    (`CARLBraxHumanoidStiffness`: gravity <= -24 AND joint_stiffness >= 2.7; measured 16 of 8 192 lanes up to 2.6e-4,
    DESIGN 7), bounded here at 1 % of the lanes and 2e-3."""
    import inspect

    import carl_amd.envs.brax as brax_envs

    rng = np.random.default_rng(2026)
    n_classes = 0
    for cname, cls in inspect.getmembers(brax_envs):
        if not (inspect.isclass(cls) and cname.startswith("CARLBrax") and cname != "CARLBraxEnv"):
            continue
        n_classes += 1
        n = 2048
        e, agree, blown, rows, names = brax_wide_context_case(cls, n, 40, rng, device)
        assert not blown.any(), (cname, int(blown.sum()))
        assert agree.mean() >= 0.999, (cname, agree.mean())
        above = agree & (e > 1e-5)
        if cname == "CARLBraxHumanoidStiffness":
            assert above.sum() <= n // 100 and e[agree].max() <= 2e-3, (cname, int(above.sum()), e[agree].max())
            corner = (rows[:, names.index("gravity")] <= -20.0) & (rows[:, names.index("joint_stiffness")] >= 2.0)
            assert corner[above].all(), "a lane above the bar outside the recorded corner"
        else:
            assert not above.any(), (cname, int(above.sum()), e[agree].max())
    assert n_classes == 12


def test_joint_stiffness_above_the_measured_ceiling_warns_or_refuses(device):
    """``joint_stiffness`` (this build's extension feature, declared bounds (0.01, 100)) scales the constraint stiffness; above
    a model-specific scale the explicit spring integration leaves the finite range (tools/stiffness_stability_sweep.py:
    Halfcheetah all envs at x 2.5 with a torso at 0.8 x default and at x 3.0 with the default torso, none at x 2.0; Humanoid
    none at x 6, all at x 10 / 0.8).  BASELINE config 5's U(0.5, 2) constructs silently; above the ceiling the constructor
    warns once (the physics is not clamped) or, with mass_check="error", refuses."""
    import warnings

    from carl_amd.envs import CARLBraxHalfcheetahStiffness, CARLBraxHumanoidStiffness
    from carl_amd.envs.brax.feature_tables import JOINT_STIFFNESS_CEILING

    for cls, fam in ((CARLBraxHalfcheetahStiffness, "halfcheetah"), (CARLBraxHumanoidStiffness, "humanoid")):
        feats = cls.get_context_features()
        default = {k: float(f.default_value) for k, f in feats.items() if k not in ("target_distance", "target_direction", "target_radius")}
        top = JOINT_STIFFNESS_CEILING[fam]
        inside = {0: dict(default, joint_stiffness=0.5), 1: dict(default, joint_stiffness=top)}
        above = {0: dict(default), 1: dict(default, joint_stiffness=top * 1.5)}
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            env = cls(contexts=inside, batch_size=2, device=device, seed=0)
        with pytest.warns(RuntimeWarning, match="joint_stiffness"):
            cls(contexts=above, batch_size=2, device=device, seed=0)
        with pytest.raises(ValueError, match="joint_stiffness"):
            cls(contexts=above, batch_size=2, device=device, seed=0, mass_check="error")
        env.reset(seed=0)
        g = torch.Generator(device="cpu").manual_seed(2)
        lo, hi = env.action_space.low[0], env.action_space.high[0]
        for _ in range(100):  # at the ceiling the envs stay finite
            a = torch.rand((2, env.action_space.shape[1]), generator=g) * float(hi[0] - lo[0]) + float(lo[0])
            o, r, *_ = env.step(a.to(device))
            assert bool(torch.isfinite(o["obs"]).all()) and bool(torch.isfinite(r).all())


def test_config4_and_config5_full_size_step_parity(device):
    """BASELINE configs 4 and 5 at their full sizes (Ant x 32 768; Halfcheetah + Humanoid x 32 768 each with the
    joint_stiffness classes): the engines run the whole batch; the fp64 oracle re-computes every lane (Ant) or every
    fourth lane (config 5) of one env step from the engine's own state after a few free-running steps -- north_star's
    1e-5 as a maximum on the lanes whose contact decisions agree, the excluded share bounded."""
    from carl_amd.brax_engine import BraxVecEngine

    n = 32768
    rng = np.random.default_rng(60)
    cases = [("ant", ant_sys(NAMES), NAMES, context_rows(rng, n), 1, 1.0)]
    s, names, default = _cheetah()
    cases.append(("halfcheetah", s, names, _cheetah_rows(rng, n, default, names), 4, 1.0))
    s, names, default = _humanoid()
    rows = np.tile(default, (n, 1))
    rows[:, names.index("joint_stiffness")] = rng.uniform(0.5, 2.0, n)
    rows[:, names.index("gravity")] = rng.uniform(-15, -5, n)
    cases.append(("humanoid", s, names, rows.astype(np.float32).astype(np.float64), 4, 0.4))
    for label, s, names, rows, stride, amp in cases:
        eng = BraxVecEngine(s, len(names), rows, n, device, selector=O.SEL_STATIC, seed=1, ctx_idx0=np.arange(n),
                            auto_reset=False, max_episode_steps=10_000, branch_record=True)
        eng.reset()
        g = torch.Generator(device=device).manual_seed(3)
        for _ in range(5):  # away from the reset pose: contacts, limits, motion
            eng.step((torch.rand((n, s.n_act), generator=g, device=device) * 2 - 1) * amp)
        sel = np.arange(0, n, stride)
        ora = B.Engine(s, rows[sel], len(sel), selector=O.SEL_STATIC, ctx_idx0=np.arange(len(sel)), autoreset=False,
                       max_steps=10_000)
        ora.reset()
        ora.state[:] = eng.state_np()[sel]
        ora.elapsed[:] = eng.elapsed.cpu().numpy()[sel]
        a = (rng.uniform(-1, 1, (n, s.n_act)) * amp).astype(np.float32)
        obs, rew, term, trunc = eng.step(torch.as_tensor(a))
        out = ora.step(a[sel])
        sig = eng.branch_sig.cpu().numpy().view(np.uint32)[sel]
        flag = (term.cpu().numpy()[sel] != 0) != (out.terminated != 0)
        agree = (sig[:, 0] == ora.branch_sig[:, 0]) & ~flag
        e = np.maximum(rel_err(obs.cpu().numpy()[sel], out.obs).max(1), rel_err(rew.cpu().numpy()[sel], out.reward))
        print(f"{label}: {len(sel)} lanes, agreeing max {e[agree].max():.2e}, excluded {1 - agree.mean():.5f}")
        assert agree.mean() >= 0.999 and e[agree].max() <= 1e-5, (label, e[agree].max(), agree.mean())
        assert bool(torch.isfinite(obs).all())


@pytest.mark.parametrize("fam", ["ant", "halfcheetah", "humanoid"])
def test_committed_brax_transitions(fam, device, golden_dir):
    """The committed (self-derived: made from the fp64 restatement, NOT brax output) transition fixtures of BASELINE
    configs 4 / 5 through the HIP kernel: observation and reward within north_star's 1e-5 on the rows whose contact
    record equals the fixture's, flags exact."""
    import os

    from carl_amd.brax_engine import BraxVecEngine
    from carl_amd.envs.brax.models import SYSTEMS

    g = np.load(os.path.join(golden_dir, f"transitions_brax_{fam}.npz"))
    names = [str(x) for x in g["names"]]
    s = SYSTEMS[fam](names)
    rows = g["ctx"].astype(np.float64)
    n = len(rows)
    eng = BraxVecEngine(s, len(names), rows, n, device, selector=O.SEL_STATIC, ctx_idx0=np.arange(n), auto_reset=False,
                        max_episode_steps=1 << 30, branch_record=True)
    eng.reset()
    eng.set_state64(g["state"].reshape(n, s.n_links, 13))
    obs, rew, term, trunc = eng.step(torch.as_tensor(g["action"]))
    sig = eng.branch_sig.cpu().numpy().view(np.uint32)
    same = sig[:, 0] == g["branch_sig"][:, 0]
    assert same.mean() >= 0.999, same.mean()  # at most 1e-3 of the rows excluded
    np.testing.assert_array_equal(term.cpu().numpy()[same], g["terminated"][same])
    e = np.maximum(rel_err(obs.cpu().numpy(), g["obs"]).max(1), rel_err(rew.cpu().numpy(), g["reward"]))
    assert e[same].max() <= 1e-5, e[same].max()


@pytest.mark.parametrize("model", ["halfcheetah", "hopper", "walker2d"])
def test_planar_substep_agrees_with_the_general_substep(device, model):
    """Planar models (root on two world slides + hinges about y, geometry in the y = 0 plane) are stepped by
    brax_kernels.hip.h's substep_planar -- the same records, phases and formulas without the zero components -- unless the
    batch carries CARL_FLAG_BRAX_GENERIC.  From the same state one env step of the two paths must agree to rounding on every
    lane that took the same contact decisions (compared through the branch record), with identical flags; and the state
    stays in the plane (up to the rounding residue of reset's float32 kinematics, which the planar substep leaves alone)."""
    from carl_amd import envs as E
    from carl_amd.brax_engine import BraxVecEngine
    from carl_amd.envs.brax.models import SYSTEMS

    cls = {"halfcheetah": E.CARLBraxHalfcheetahStiffness, "hopper": E.CARLBraxHopper, "walker2d": E.CARLBraxWalker2d}[model]
    feats = cls.get_context_features()
    names = list(feats)
    n = 4096
    rng = np.random.default_rng(21)
    rows = np.tile([float(f.default_value) for f in feats.values()], (n, 1))
    rows[:, names.index("gravity")] = rng.uniform(-15, -5, n)
    rows[:, names.index("friction")] = rng.uniform(0.3, 1.5, n)
    rows = rows.astype(np.float32).astype(np.float64)
    kw = dict(selector=O.SEL_STATIC, seed=9, ctx_idx0=np.arange(n), branch_record=True)
    s = SYSTEMS[cls.env_name](names)
    fast = BraxVecEngine(s, len(names), rows, n, device, **kw)
    slow = BraxVecEngine(SYSTEMS[cls.env_name](names), len(names), rows, n, device, generic_substep=True, **kw)
    fast.reset()
    slow.reset()
    assert torch.equal(fast.state, slow.state)
    amp = float(max(s.act_hi[: s.n_act]))
    worst, agree_share = 0.0, []
    for t in range(25):
        slow.set_state64(fast.state64())
        for name in ("elapsed", "episode", "ep_return", "ctx_idx", "n_calls", "episodes_done"):
            getattr(slow, name).copy_(getattr(fast, name))
        a = torch.as_tensor(rng.uniform(-amp, amp, (n, s.n_act)).astype(np.float32), device=device)
        o1, r1, te1, tr1 = fast.step(a)
        o2, r2, te2, tr2 = slow.step(a)
        assert torch.equal(tr1, tr2)
        same = (fast.branch_sig[:, 0] == slow.branch_sig[:, 0]) & (te1 == te2)
        agree_share.append(float(same.float().mean()))
        d = (o1.double() - o2.double()).abs() / (1 + o2.double().abs())
        dr = (r1.double() - r2.double()).abs() / (1 + r2.double().abs())
        worst = max(worst, float(d[same.bool()].max()), float(dr[same.bool()].max()))
        st = fast.state64()  # [N, L, 13]: p, r (w x y z), v, w
        # y position, r.x, r.z, v.y, w.x, w.z: what the float32 forward kinematics of reset left there (<= 1e-5: velocities of a reset draw), never more
        assert float(st[:, :, [1, 4, 6, 8, 10, 12]].abs().max()) <= 2e-5
    print(f"{model}: planar vs general substep, 25 steps x {n} envs: max |d| / (1 + |x|) {worst:.2e} on agreeing lanes "
          f"(share {min(agree_share):.5f})")
    assert worst <= 2e-6 and min(agree_share) >= 0.999


def test_reference_viscosity_rule_moves_the_angular_damping(device):
    """`CARLBraxEnv(viscosity="reference")` (Quirk B2, carl_brax_env.py:276-279: the viscosity context overwrites
    ang_damping): an env whose viscosity column holds x steps exactly like a default-rule env whose ang_damping column
    holds x -- whatever its own ang_damping column says; under the default rule viscosity is observed only."""
    from carl_amd.context.selection import StaticSelector
    from carl_amd.envs import CARLBraxAnt

    n = 64
    base = CARLBraxAnt.get_default_context()
    mk = lambda **kv: {i: {**base, **kv} for i in range(n)}  # noqa: E731
    a = CARLBraxAnt(contexts=mk(ang_damping=-0.8), batch_size=n, device=device, context_selector=StaticSelector, seed=1, autotune=False)
    b = CARLBraxAnt(contexts=mk(ang_damping=-0.05, viscosity=-0.8), batch_size=n, device=device, context_selector=StaticSelector,
                    seed=1, autotune=False, viscosity="reference")
    c = CARLBraxAnt(contexts=mk(ang_damping=-0.05, viscosity=-0.8), batch_size=n, device=device, context_selector=StaticSelector,
                    seed=1, autotune=False)  # default rule: viscosity does nothing
    for e in (a, b, c):
        e.reset(seed=1)
    g = torch.Generator(device=device).manual_seed(0)
    differs = False
    for t in range(12):
        act = torch.rand((n, 8), generator=g, device=device) * 2 - 1
        oa, ob, oc = a.step(act)[0]["obs"], b.step(act)[0]["obs"], c.step(act)[0]["obs"]
        assert torch.equal(oa, ob), t
        differs |= not torch.equal(oa, oc)
    assert differs
    assert float(b.step(act)[0]["context"]["viscosity"][0]) == pytest.approx(-0.8)  # still observed as sampled


@pytest.mark.parametrize("fam", ["ant", "halfcheetah", "humanoid", "inverted_double_pendulum"])
def test_float32_substeps_are_opt_in_close_and_self_consistent(fam, device):
    """CARL_FLAG_BRAX_FP32 (round 6, VERDICT r05 "Next" #7): the substeps' pose algebra in float32 -- brax's own precision
    under JAX's default -- as an OPT-IN flag that tells what the float64 parity bar costs.  Never on by default; reset is
    untouched (bit-identical states); one env step from identical states stays close to the float64 path (loose bounds:
    this is NOT a parity claim -- the measured deviation from the float64 restatement is in
    profiles/r06_brax_fp32_deviation.txt); a float32 rollout equals repeated float32 steps bit for bit; the task models
    refuse the flag."""
    from carl_amd import _lib
    from carl_amd.brax_engine import BraxVecEngine
    from carl_amd.envs.brax.models import SYSTEMS, reacher_sys

    names = list({"ant": NAMES}.get(fam) or [])
    if fam == "ant":
        s = ant_sys(NAMES)
        rows = context_rows(np.random.default_rng(3), 1024)
    else:
        from carl_amd import envs as E

        cls = {"halfcheetah": E.CARLBraxHalfcheetah, "humanoid": E.CARLBraxHumanoid,
               "inverted_double_pendulum": E.CARLBraxInvertedDoublePendulum}[fam]
        names = list(cls.get_context_features())
        s = SYSTEMS[cls.env_name](names)
        rows = np.tile([float(f.default_value) for f in cls.get_context_features().values()], (1024, 1))
    n, T = 1024, 6
    kw = dict(selector=O.SEL_STATIC, seed=9, ctx_idx0=np.arange(n), max_episode_steps=1000)
    e64 = BraxVecEngine(s, len(names), rows, n, device, **kw)
    e32 = BraxVecEngine(s, len(names), rows, n, device, pose_float32=True, **kw)
    e32b = BraxVecEngine(s, len(names), rows, n, device, pose_float32=True, **kw)
    assert not (e64.b.flags & _lib.FLAG_BRAX_FP32) and (e32.b.flags & _lib.FLAG_BRAX_FP32)
    for e in (e64, e32, e32b):
        e.reset()
    assert torch.equal(e64.state, e32.state)  # reset does not know the flag
    g = torch.Generator(device=device).manual_seed(4)
    lo, hi = float(min(s.act_lo[: s.n_act])), float(max(s.act_hi[: s.n_act]))
    acts = torch.rand((T, n, s.n_act), generator=g, device=device) * (hi - lo) + lo
    out = e32b.rollout(acts)
    differs = False
    for t in range(T):
        e64._state_storage.copy_(e32._state_storage)  # the same state in: one env step's deviation
        for k in ("elapsed", "ep_return", "episode", "n_calls", "ctx_idx"):
            getattr(e64, k).copy_(getattr(e32, k))
        o64, r64, te64, _ = e64.step(acts[t])
        o32, r32, te32, tr32 = e32.step(acts[t])
        assert bool(torch.isfinite(o32).all()) and bool(torch.isfinite(r32).all())
        d = (o32 - o64).abs() / (1 + o64.abs())
        same = te32 == te64
        # loose: one env step (10-20 substeps) of float32 pose rounding amplified by the constraint springs; contacts that
        # switch within rounding move single lanes further (excluded by the quantile)
        assert float(d[same].quantile(0.99)) < 2e-3 and float(d[same].median()) < 2e-4, (fam, t, float(d.max()))
        differs |= not torch.equal(o32, o64)
        assert torch.equal(out["obs"][t], o32) and torch.equal(out["reward"][t], r32), (fam, t)  # rollout == repeated step
        assert torch.equal(out["terminated"][t], te32) and torch.equal(out["truncated"][t], tr32)
    assert differs  # the flag does something
    assert torch.equal(e32.state, e32b.state)
    with pytest.raises(ValueError, match="task"):
        BraxVecEngine(reacher_sys(), 1, [[0.0]], 4, device, pose_float32=True)
