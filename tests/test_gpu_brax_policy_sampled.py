"""The sampled closed-loop rollout of the Brax families (include/carl_amd.h: carl_brax_rollout_policy_sampled;
BraxVecEngine.rollout_policy(deterministic=False)) on the GPU.  Every launch is held to the rule itself and to the
other launches:

  * the rule: a per-call replay of the recorded actions reads, before every step, the env's context values, observation,
    episode counter and step count from the engine; brax_sampling_cases.check_rule draws each actuator's z in float64 from
    those counters and holds every action and every log-probability to the derived bounds -- no env-step is exempted;
  * the other launches, from the same snapshot, bit for bit: `rollout` of the recorded actions, the launch without
    log_prob, the summary launch, the horizon split into two launches, another lane width.

Shapes: 300 envs in two weight sets of 256 with different log_std rows (one wavefront holds envs of both sets at every
width), 8 steps under a TimeLimit of 3 (every env crosses auto-resets inside the launch)."""
import numpy as np
import pytest
import torch

import brax_policy_cases as BP
import brax_sampling_cases as BS
import policy_checks as PC
import value_cases as VC
from carl_amd import _lib
from carl_amd.brax_policy import BraxMLPPolicy

pytestmark = pytest.mark.gpu

N, T = 300, 8
RECORDS = ("obs", "reward", "terminated", "truncated")


def _first_of_each_class():
    """one (model, width) per kernel class: lean, multi-hinge, general, planar"""
    seen = {}
    for m, w in BP.instance_cases():
        seen.setdefault(BP.MODELS[m], (m, w))
    assert len(seen) == 4
    return set(seen.values())


ALL_NETWORKS = _first_of_each_class()


def launch(eng, pol, steps, log_prob=True, **kw):
    return eng.rollout_policy(pol, steps, deterministic=False, sample_seed=BS.SEED, log_prob=log_prob, **kw)


def sets_of(eng, pol):
    return (np.arange(eng.n) // (pol.lanes_per_set or (1 << 30))).astype(np.int32)


def same_bits(a, b, what):
    if a.is_floating_point():
        a, b = a.view(torch.int32), b.view(torch.int32)
    assert torch.equal(a, b), what


def check_against_rule(eng, pol, snap, out, steps):
    """teacher-forced: the counters and inputs come from the engine's own per-call replay of the recorded actions"""
    acts = out["action"][:steps]
    x, es, els = PC.teacher(eng, pol, snap, acts)
    assert es.min() >= 0 and els.min() >= 0
    n, M = eng.n, steps * eng.n
    genv = int(eng.b.lane_offset) + np.arange(n)
    lp = out["log_prob"][:steps].cpu().numpy().reshape(M) if "log_prob" in out else None
    z, mu, wa, wl = BS.check_rule(pol, x.reshape(M, -1), np.tile(genv, steps), es.reshape(M), els.reshape(M),
                                  np.tile(sets_of(eng, pol), steps), BS.SEED, acts.cpu().numpy().reshape(M, -1), lp)
    return x, es, els, z.reshape(steps, n, -1), mu.reshape(steps, n, -1), wa, wl


def check_pinned(eng, pol, snap, out, steps, after, split=3):
    """the transitions launch with log_prob `out` from `snap`, against the other launches from the same snapshot"""
    eng.restore(snap)
    PC.assert_replays(eng, out, steps, after)                      # rollout of the recorded actions: records and state
    eng.restore(snap)
    plain = launch(eng, pol, steps, log_prob=False)                 # the same launch without log_prob
    assert "log_prob" not in plain
    for k in RECORDS + ("action",):
        same_bits(plain[k], out[k][:steps], k)
    PC.assert_same_state(after, PC.engine_state(eng))
    if eng.auto_reset:
        eng.restore(snap)
        s = launch(eng, pol, steps, log_prob=False, mode="summary")  # the summary launch: state, and totals = the reduction
        PC.assert_summary_reduces(eng, s, snap, out, steps, after)
        same_bits(eng.obs, out["obs"][steps - 1], "obs after the summary launch")
    eng.restore(snap)
    a, b = launch(eng, pol, split), launch(eng, pol, steps - split)  # the horizon in two launches
    for k in RECORDS + ("action", "log_prob"):
        same_bits(torch.cat([a[k], b[k]]), out[k][:steps], k)
    PC.assert_same_state(after, PC.engine_state(eng))


@pytest.mark.parametrize("model,width", BP.instance_cases(), ids=str)
def test_every_kernel_instance_against_the_rule_and_pinned(device, model, width):
    """cases 1 and 2: every instantiated (class, width) with the 2 x 64 tanh network, one instance per class with the
    1 x 32 relu and the linear network as well; the tanh launch is then pinned bit for bit to its replay, its twin without
    log_prob, the summary launch and the 3 + 5 split"""
    seed = 9000 + 100 * list(BP.MODELS).index(model) + width
    eng = BS.make_engine(model, width, N, device, seed)
    assert BP.launch_shape(eng.b, eng.sys, BS.make_policy(eng, (), "identity", 0).struct(N, 0x10), T)[1].lanes_per_env == width
    nets = BP.NETWORKS if (model, width) in ALL_NETWORKS else BP.NETWORKS[:1]
    for k, (widths, act) in enumerate(nets):
        pol = BS.two_set_policy(eng, widths, act, seed + 10 * k)
        assert pol.log_std.shape == (2, eng.sys.n_act) and (pol.log_std[0] != pol.log_std[1]).all()
        snap = eng.snapshot()
        out = launch(eng, pol, T)
        after = PC.engine_state(eng)
        assert tuple(out["action"].shape) == (T, N, eng.sys.n_act) and tuple(out["log_prob"].shape) == (T, N)
        assert out["log_prob"].dtype == torch.float32
        same_bits(eng.obs, out["obs"][T - 1], "obs after the launch")
        x, es, els, z, mu, wa, wl = check_against_rule(eng, pol, snap, out, T)
        PC.assert_same_state(after, PC.engine_state(eng))  # (the per-call replay ends in the launch's state)
        assert es.max() >= 2 and els.max() == 2  # TimeLimit 3 inside 8 steps: every env crossed auto-resets, e advanced
        done = (out["terminated"] | out["truncated"]).bool()
        assert int(done.sum(0).min()) >= 2
        print(f"{model}/{width} {act}{list(widths)}: worst action |err| / bound {wa:.3f}, log_prob {wl:.3f}")
        if k == 0:
            check_pinned(eng, pol, snap, out, T, after)
    assert len(torch.unique(eng.ctx_idx)) >= 3


def test_fragment_hand_over(device):
    """case 3: Ant pinned to 16 lanes per env, 6 steps, the smallest env count whose launch cuts a group between two
    wavefronts: the tail fragment continues its head's stream (the single launch meets the teacher-forced rule), and the cut
    changes no bit relative to 9 lanes per env, which does not cut this batch"""
    steps = 6
    s = BP.build_model("ant")[0]

    def plan(n, width):
        s.lanes_per_env = width
        b = _lib.Batch()
        b.n_lanes, b.flags = n, _lib.FLAG_AUTORESET
        code, sh = BP.launch_shape(b, s, _lib.Policy(), steps)
        assert code == 0 and sh.lanes_per_env == width
        return sh

    def waits(n, width):
        sh = plan(n, width)
        return sh, [f for f in BP.fragments(sh, n, steps) if f[5]]

    lo = 1  # the smallest group count (4 envs per group at 16 lanes) with fewer wavefronts than groups
    while lo < 1 << 13:
        sh = plan(4 * (lo - 1) + 1, 16)
        if sh.grid * sh.waves_per_workgroup < lo:
            break
        lo += 1
    n = 4 * (lo - 1) + 1
    shape, wait = waits(n, 16)
    assert wait, "no wait_head fragment"
    assert not waits(n, 9)[1], "9 lanes per env cuts this batch too"
    print(f"hand-over from {n} envs: {shape.grid} x {shape.waves_per_workgroup} wavefronts, {len(wait)} tail fragments")
    eng = BS.make_engine("ant", 16, n, device, 13, max_episode_steps=4)
    pol = BS.make_policy(eng, (64, 64), "tanh", 14, log_std=np.linspace(-1.0, 0.2, 8))
    snap = eng.snapshot()
    out = launch(eng, pol, steps)
    after = PC.engine_state(eng)
    check_against_rule(eng, pol, snap, out, steps)
    PC.assert_same_state(after, PC.engine_state(eng))
    eng.restore(snap)
    eng.sys.lanes_per_env = 9
    whole = launch(eng, pol, steps)
    for k in RECORDS + ("action", "log_prob"):
        same_bits(whole[k], out[k], k)
    PC.assert_same_state(after, PC.engine_state(eng))


def test_zero_variance_limit(device):
    """case 4: log_std = -200: exp gives 0 and fma(0, z, mu) = mu -- the deterministic launch's actions bit for bit, a
    finite log_prob inside the rule's bound"""
    eng = BS.make_engine("ant", 9, N, device, 41)
    pol = BS.make_policy(eng, (64, 64), "tanh", 42, log_std=-200.0)
    snap = eng.snapshot()
    det = eng.rollout_policy(pol, T)
    after = PC.engine_state(eng)
    eng.restore(snap)
    out = launch(eng, pol, T)
    for k in RECORDS + ("action",):
        same_bits(out[k], det[k], k)
    PC.assert_same_state(after, PC.engine_state(eng))
    assert bool(torch.isfinite(out["log_prob"]).all()) and float(out["log_prob"].min()) > 8 * (200 - 0.92) - 8 * 20
    check_against_rule(eng, pol, snap, out, T)


def test_draws_are_independent(device):
    """case 5: the z recovered from one Ant launch with the linear network (mu is the host's fp32 reference bit for bit,
    log_std 0) -- 300 * 8 * 8 draws: mean, variance, the correlation inside a Philox block and between neighbouring
    envs inside the 5-sigma bounds of the rule itself; so are the float64 reference draws of the same counters"""
    eng = BS.make_engine("ant", 9, N, device, 51)
    pol = BS.make_policy(eng, (), "identity", 52, log_std=0.0)
    snap = eng.snapshot()
    out = launch(eng, pol, T)
    x, es, els, z64, mu64, _, _ = check_against_rule(eng, pol, snap, out, T)
    mu32 = BP.reference_actions(pol, x.reshape(T * N, -1))[0].reshape(T, N, -1)
    z = out["action"].cpu().numpy().astype(np.float64) - mu32.astype(np.float64)
    assert z.size == 300 * 8 * 8
    assert np.abs(z - z64).max() < 1e-4  # (the recovered draws are the reference's, up to the roundings of mu and the fma)
    print("reference: mean %.4f var %.4f pair %.4f env %.4f" % BS.assert_independent(z64))
    print("device:    mean %.4f var %.4f pair %.4f env %.4f" % BS.assert_independent(z))


def test_canaries(device):
    """case 6: buffers with rows beyond T, the log_prob buffer included, keep their fill there and lose it below"""
    eng = BS.make_engine("hopper", 4, 70, device, 61)
    pol = BS.make_policy(eng, (32,), "relu", 62, log_std=-0.5)
    extra = 3
    spec = {"obs": ((eng.D,), torch.float32, float("nan")), "reward": ((), torch.float32, float("nan")),
            "terminated": ((), torch.uint8, 0xAB), "truncated": ((), torch.uint8, 0xAB),
            "action": ((eng.sys.n_act,), torch.float32, float("nan")), "log_prob": ((), torch.float32, PC.LOG_PROB_FILL)}
    full = {}
    for k, (tail, dt, fill) in spec.items():
        if isinstance(fill, int) and dt == torch.float32:
            full[k] = torch.full((T + extra, 70) + tail, fill, dtype=torch.int32, device=device).view(dt)
        else:
            full[k] = torch.full((T + extra, 70) + tail, fill, dtype=dt, device=device)
    snap = eng.snapshot()
    out = launch(eng, pol, T, out=full)
    assert out is full
    torch.cuda.synchronize()
    for k, t in full.items():
        assert bool(PC.is_canary(t[T:], spec[k][2]).all()), f"{k}: a row >= T was written"
        assert not bool(PC.is_canary(t[:T], spec[k][2]).any()), f"{k}: a record is missing"
    check_against_rule(eng, pol, snap, out, T)
    with pytest.raises(ValueError, match="log_prob"):
        launch(eng, pol, T, out={**full, "log_prob": full["log_prob"][:, :69]})
    with pytest.raises(ValueError, match="log_prob"):
        launch(eng, pol, T, out={**full, "log_prob": full["log_prob"].double()})
    with pytest.raises(ValueError, match="log_prob=True"):
        eng.rollout_policy(pol, T, log_prob=True)
    with pytest.raises(ValueError, match="log_prob=True"):
        launch(eng, pol, T, mode="summary")


@pytest.mark.parametrize("mode", ["redraw", "first_state", "none"])
def test_auto_reset_modes(device, mode):
    """case 6: both auto-reset modes (and none) run once each: the rule from the engine's own counters, and the replay"""
    kw = dict(auto_reset=False) if mode == "none" else dict(autoreset_mode=mode)
    eng = BS.make_engine("halfcheetah", 7, 70, device, 71, **kw)
    if mode == "first_state":
        eng.reset()  # (the first_state copy is taken by an explicit reset)
    pol = BS.make_policy(eng, (32,), "relu", 72, log_std=-0.3)
    snap = eng.snapshot()
    out = launch(eng, pol, T)
    after = PC.engine_state(eng)
    check_against_rule(eng, pol, snap, out, T)
    check_pinned(eng, pol, snap, out, T, after)


def test_goal_wrapper_and_env_front_end(device):
    """case 6: the goal wrapper once, and CARLBraxEnv.rollout_policy with the sampling keywords"""
    from carl_amd.envs import CARLBraxAnt

    contexts = {k: {"target_distance": d, "target_direction": c, "target_radius": 0.3}
                for k, (d, c) in enumerate([(0.05, 112), (0.4, 334), (1.0, 1), (2.0, 32)])}
    env = CARLBraxAnt(batch_size=64, contexts=contexts, obs_context_features=["target_distance", "target_direction"],
                      device=device)
    env.reset(seed=3)
    eng = env.env
    assert eng.sys.goal_mode == 1
    rng = np.random.default_rng(3)
    pol = BraxMLPPolicy.for_env(env, BP.make_layers(rng, 2 + eng.D, (16,), eng.sys.n_act), "relu", log_std=-1.0)
    snap = eng.snapshot()
    out = env.rollout_policy(pol, 5, deterministic=False, sample_seed=BS.SEED, log_prob=True)
    after, goal_after = PC.engine_state(eng), eng.goal_pos.clone()
    eng.restore(snap)
    ref = eng.rollout(out["action"], eng.alloc_rollout(5))
    for k in RECORDS + ("success",):
        same_bits(out[k], ref[k], k)
    PC.assert_same_state(after, PC.engine_state(eng))
    assert torch.equal(goal_after, eng.goal_pos)
    check_against_rule(eng, pol, snap, out, 5)

    env = CARLBraxAnt(batch_size=64, obs_context_features=["gravity", "friction"], device=device)
    env.reset(seed=4)
    pol = BraxMLPPolicy.from_sequential(env, torch.nn.Sequential(torch.nn.Linear(29, 16), torch.nn.Tanh(),
                                                                 torch.nn.Linear(16, 8)), log_std=np.full(8, -0.7))
    assert pol.log_std.shape == (1, 8)
    out = env.rollout_policy(pol, 4, deterministic=False, sample_seed=1, log_prob=True)
    assert tuple(out["action"].shape) == (4, 64, 8) and tuple(out["log_prob"].shape) == (4, 64)
    assert bool(torch.isfinite(out["action"]).all()) and bool(torch.isfinite(out["log_prob"]).all())
    again = env.rollout_policy(pol, 4, deterministic=False, sample_seed=2)
    assert "log_prob" not in again
    # an on_device policy with its own [n_sets, n_act] log_std tensor
    dev = BraxMLPPolicy.on_device(pol, pol.device_params(device).clone(), 256,
                                  log_std=torch.full((1, 8), -0.7, device=device))
    env.reset(seed=4)
    twin = env.rollout_policy(dev, 4, deterministic=False, sample_seed=1, log_prob=True)
    same_bits(twin["action"], out["action"], "action")
    same_bits(twin["log_prob"], out["log_prob"], "log_prob")


def test_gae_on_brax_rows(device):
    """case 7: LaneEngine.gae on a Brax rollout's dense rows against value_cases.gae_ref, bit for bit"""
    steps, n = 5, 70
    eng = BS.make_engine("hopper", 4, n, device, 81, max_episode_steps=2)
    pol = BS.make_policy(eng, (32,), "relu", 82, log_std=-0.5)
    out = launch(eng, pol, steps)
    rng = np.random.default_rng(83)
    value = rng.normal(size=(steps, n)).astype(np.float32)
    last = rng.normal(size=n).astype(np.float32)
    done = (out["terminated"] | out["truncated"]).bool()
    assert bool(done.any()) and not bool(done.all())
    res = eng.gae(out["reward"], torch.as_tensor(value).to(device), out["terminated"], out["truncated"],
                  torch.as_tensor(last).to(device), 0.99, 0.95)
    a, r = VC.gae_ref(out["reward"].cpu().numpy(), value, out["terminated"].cpu().numpy(), out["truncated"].cpu().numpy(),
                      last, 0.99, 0.95, boot_value=None)
    np.testing.assert_array_equal(res["advantage"].cpu().numpy().view(np.int32), a.view(np.int32))
    np.testing.assert_array_equal(res["return"].cpu().numpy().view(np.int32), r.view(np.int32))
