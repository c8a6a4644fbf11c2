"""The closed-loop rollout of the Brax families (include/carl_amd.h: carl_brax_rollout_policy; BraxVecEngine.rollout_policy)
on the GPU.  The policy runs inside the rollout kernel (brax_kernels.hip.h: run(), MODE 2), so every launch is held to
two references:

  * the open-loop kernel: `rollout` of the recorded actions from the same snapshot gives the launch's observations,
    rewards and flags bit for bit, and the same engine state -- the step code of the two modes is one text;
  * the host: the recorded actions against oracle.policy_forward on the inputs a per-call replay of those actions reads
    from the engine before each step (context values of the env's current context, then its observation).  relu and
    identity networks bit for bit; tanh (v_exp_f32 / v_rcp_f32) within the bound the oracle derives.  The oracle takes
    at most four outputs: the head is evaluated in row slices of at most four (brax_policy_cases.reference_actions).

Shapes: 77 envs (a ragged last wavefront at every width), 12 steps under a TimeLimit of 5 (auto-resets inside the
launch), a round-robin selector over 5 contexts of which gravity and friction are policy inputs."""
import numpy as np
import pytest
import torch

import brax_policy_cases as BP
from brax_kernel_cases import touch_down
from carl_amd import _lib
from carl_amd.brax_policy import BraxMLPPolicy
from oracle import oracle as O
from policy_cases import host_summary

pytestmark = pytest.mark.gpu

N, T, TIME_LIMIT, N_CTX = 77, 12, 5, 5
STATE = ("state", "elapsed", "ctx_idx", "episode", "n_calls", "ep_return", "episodes_done", "ctx_obs", "last_return",
         "last_length")
RECORDS = ("obs", "reward", "terminated", "truncated")


def make_engine(model, width, n, device, seed, **kw):
    from carl_amd.brax_engine import BraxVecEngine

    s, names, default = BP.build_model(model)
    s.lanes_per_env = width
    rng = np.random.default_rng(seed)
    rows = BP.context_rows(rng, N_CTX, default, names)
    kw.setdefault("max_episode_steps", TIME_LIMIT)
    eng = BraxVecEngine(s, len(names), rows, n, device, selector=O.SEL_ROUND_ROBIN, seed=seed,
                        ctx_obs_rows=[names.index("gravity"), names.index("friction")], **kw)
    assert width in eng.lane_widths()
    eng.reset()
    if model in BP.GROUND:  # half the envs 5 mm deep in the ground: the contact path from the first step on
        eng.set_state64(touch_down(eng.sys, eng.state64().cpu().numpy()))
    return eng


def make_policy(eng, widths, act, seed):
    rng = np.random.default_rng(seed)
    n_in = 2 + eng.D
    shift, scale, clip = BP.transform(rng, n_in)
    shift[0] += -10.0  # gravity ~ -10: centred like a normalised input
    return BraxMLPPolicy.for_env(eng, BP.make_layers(rng, n_in, widths, eng.sys.n_act), act, shift, scale, clip)


def engine_state(eng):
    return {k: getattr(eng, k).clone() for k in STATE}


def assert_same_state(a, b):
    for k in STATE:
        x, y = a[k], b[k]
        if x.is_floating_point():
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), k


def teacher(eng, pol, snap, actions):
    """per-call replay of the recorded actions from `snap`: the float32 inputs the policy must have seen [T, n, n_in]"""
    eng.restore(snap)
    tab = eng.ctx_table.cpu().numpy()
    xs = []
    for t in range(actions.shape[0]):
        cidx = eng.ctx_idx.cpu().numpy().astype(np.int64)
        xs.append(np.concatenate([tab[pol.ctx_rows][:, cidx].T, eng.obs.cpu().numpy()], axis=1).astype(np.float32))
        eng.step(actions[t].contiguous())
    torch.cuda.synchronize()
    return np.stack(xs)


def check_actions(pol, x, acts, sets=None):
    """acts [T, n, n_act] against the host reference on inputs x [T, n, n_in]; sets [n]: each env's weight set"""
    steps, n, n_in = x.shape
    y32, y64, bound = BP.reference_actions(pol, x.reshape(-1, n_in), None if sets is None else np.tile(sets, steps))
    a = np.asarray(acts).reshape(-1, pol.n_out)
    assert np.isfinite(a).all()
    if pol.activation != "tanh":
        np.testing.assert_array_equal(a, y32)  # (+0 == -0)
        return 0.0
    err = np.abs(a.astype(np.float64) - y64)
    assert np.all(err <= bound * (1 + 1e-9)), (err.max(), bound.flat[np.argmax(err - bound)])
    return float((err / np.maximum(bound, 1e-300)).max())


def check_launch(eng, pol, steps, sets=None, summary=True):
    """One transitions launch from the engine's current state against both references; then (summary) the summary launch
    from the same snapshot against the exact reduction of the transitions.  Leaves the engine after the launch."""
    snap = eng.snapshot()
    obs0 = eng.obs.clone()
    out = eng.rollout_policy(pol, steps)
    after = engine_state(eng)
    assert tuple(out["action"].shape) == (steps, eng.n, eng.sys.n_act)
    assert torch.equal(eng.obs, out["obs"][steps - 1])  # the launch leaves every env's last observation in `obs`
    acts = out["action"]
    x = teacher(eng, pol, snap, acts)
    np.testing.assert_array_equal(x[0, :, len(pol.ctx_rows):], obs0.cpu().numpy())
    worst = check_actions(pol, x, acts.cpu().numpy(), sets)
    # the per-call replay is the open-loop reference too: same state; and the fused open-loop rollout gives the same rows
    assert_same_state(after, engine_state(eng))
    eng.restore(snap)
    ref = eng.rollout(acts, eng.alloc_rollout(steps))
    for k in RECORDS:
        a, b = out[k], ref[k]
        if a.is_floating_point():
            a, b = a.view(torch.int32), b.view(torch.int32)
        assert torch.equal(a, b), k
    assert_same_state(after, engine_state(eng))
    if summary:
        eng.restore(snap)
        s = eng.rollout_policy(pol, steps, mode="summary")
        assert_same_state(after, engine_state(eng))
        assert torch.equal(eng.obs, out["obs"][steps - 1])
        count, ret_sum, len_sum = host_summary(snap, out, steps)
        np.testing.assert_array_equal(s["episodes"].cpu().numpy(), count)
        np.testing.assert_array_equal(s["return_sum"].cpu().numpy().view(np.int32), ret_sum.view(np.int32))
        np.testing.assert_array_equal(s["length_sum"].cpu().numpy(), len_sum)
    return out, worst


@pytest.mark.parametrize("model,width", BP.instance_cases(), ids=str)
def test_every_kernel_instance(device, model, width):
    """case 1: every instantiated (class, width) -- tests/test_brax_policy_abi.py holds this list against the kernel table"""
    seed = 7000 + 100 * list(BP.MODELS).index(model) + width
    eng = make_engine(model, width, N, device, seed)
    shape = BP.launch_shape(eng.b, eng.sys, make_policy(eng, (), "identity", 0).struct(N, 0x10), T)[1]
    assert shape.lanes_per_env == width
    for k, (widths, act) in enumerate(BP.NETWORKS):
        pol = make_policy(eng, widths, act, seed + k)
        out, worst = check_launch(eng, pol, T)
        done = (out["terminated"] | out["truncated"]).bool()
        assert int(done.sum(0).min()) >= 2  # TimeLimit 5 inside 12 steps: every env auto-reset inside the launch
        a = out["action"]
        assert float(a.abs().max()) > 1.0 and float((a.abs() < 1.0).float().mean()) > 0.05  # clipped and unclipped actions
        print(f"{model}/{width} {act}{list(widths)}: worst |err| / bound {worst:.3f}")
    assert len(torch.unique(eng.ctx_idx)) >= 3  # the round-robin selector moved the envs over the contexts


def test_two_weight_sets_inside_one_wavefront(device):
    """case 2: Ant at 9 lanes per env is 7 envs per wavefront; 512 envs in sets of 256: wavefront 36 holds envs 252 .. 258,
    of both sets.  Every env matches its own set (and would not match the other)."""
    n, steps = 512, 6
    eng = make_engine("ant", 9, n, device, 11)
    assert (256 // 7) * 7 < 256 < (256 // 7 + 1) * 7  # a wavefront straddles the boundary
    pols = [make_policy(eng, (64, 64), "relu", 100 + k) for k in range(2)]
    pol = BraxMLPPolicy.stack(pols, 256)
    sets = (np.arange(n) // 256).astype(np.int32)
    snap = eng.snapshot()
    out, _ = check_launch(eng, pol, steps, sets)
    # the other set's actions differ for every env: the check above cannot pass by ignoring the set index
    x = teacher(eng, pol, snap, out["action"][:1])[0]
    assert (BP.reference_actions(pol, x, 1 - sets)[0] != out["action"][0].cpu().numpy()).any(axis=1).all()


def test_fragment_hand_over(device):
    """case 3: Ant pinned to 16 lanes per env, 6 steps, the smallest env count whose launch cuts a group between two
    wavefronts (a wait_head fragment in carl_brax_fragment_plan of the launch-shape query): the second wavefront starts
    from the observation, the state and the summary totals the first one left."""
    steps = 6
    s = BP.build_model("ant")[0]
    s.lanes_per_env = 16

    def waits(n):
        eng_b = _lib.Batch()
        eng_b.n_lanes, eng_b.flags = n, _lib.FLAG_AUTORESET
        p = _lib.Policy()
        code, sh = BP.launch_shape(eng_b, s, p, steps)
        assert code == 0 and sh.lanes_per_env == 16
        return sh, [f for f in BP.fragments(sh, n, steps) if f[5]]

    # group counts are searched (4 envs per group; the first env of a new group is the smallest count that has it).
    # Every smaller group count is looked at: its launch has a wavefront for every group, and such a launch hands nothing
    # over (tests/test_brax_policy_abi.py: test_a_wavefront_per_group_hands_nothing_over); the counts just below and a
    # spread of smaller ones are also planned in full.
    def wavefronts(g):
        b = _lib.Batch()
        b.n_lanes, b.flags = 4 * (g - 1) + 1, _lib.FLAG_AUTORESET
        code, sh = BP.launch_shape(b, s, _lib.Policy(), steps)
        assert code == 0 and sh.lanes_per_env == 16
        return sh.grid * sh.waves_per_workgroup

    lo = 1
    while lo < 1 << 13 and wavefronts(lo) >= lo:
        lo += 1
    n = 4 * (lo - 1) + 1
    for g in {lo - 1, lo - 2, lo // 2, 13, 12, 1} - {0, lo}:
        if 0 < g < lo:
            assert not waits(4 * g)[1], g
    shape, wait = waits(n)
    assert wait, "no wait_head fragment"
    print(f"hand-over from {n} envs: {shape.grid} x {shape.waves_per_workgroup} wavefronts, {len(wait)} tail fragments")
    eng = make_engine("ant", 16, n, device, 13)
    pol = make_policy(eng, (64, 64), "tanh", 14)
    out, _ = check_launch(eng, pol, steps)
    done = (out["terminated"] | out["truncated"]).bool()
    assert int(done.sum(0).min()) >= 1
    assert all(0 <= f[2] < -(-n // 4) for f in wait)  # (the split groups are groups of this batch: checked above with all)


@pytest.mark.parametrize("model,width,mode", [("hopper", 4, "redraw"), ("ant", 9, "first_state")], ids=str)
def test_summary_mode(device, model, width, mode):
    """case 4: summary = the exact reduction of the transitions launch, same end state; also into caller buffers with
    canaries round them, under both auto-reset modes; without auto-reset it is refused"""
    eng = make_engine(model, width, N, device, 21, autoreset_mode=mode)
    if mode == "first_state":
        eng.reset()  # (the first_state copy is taken by an explicit reset)
    pol = make_policy(eng, (32,), "relu", 22)
    snap = eng.snapshot()
    out, _ = check_launch(eng, pol, T)
    eng.restore(snap)
    full = {"episodes": torch.full((N + 16,), -5, dtype=torch.int32, device=device),
            "return_sum": torch.full((N + 16,), float("nan"), device=device),
            "length_sum": torch.full((N + 16,), -5, dtype=torch.int32, device=device)}
    view = {k: v[8: 8 + N] for k, v in full.items()}
    s = eng.rollout_policy(pol, T, out=view, mode="summary")
    count, ret_sum, len_sum = host_summary(snap, out, T)
    assert count.min() >= 2
    np.testing.assert_array_equal(s["episodes"].cpu().numpy(), count)
    np.testing.assert_array_equal(s["return_sum"].cpu().numpy().view(np.int32), ret_sum.view(np.int32))
    np.testing.assert_array_equal(s["length_sum"].cpu().numpy(), len_sum)
    for k, v in full.items():
        edge = torch.cat([v[:8], v[8 + N:]])
        assert bool((torch.isnan(edge) if v.is_floating_point() else edge == -5).all()), k
    s0 = eng.rollout_policy(pol, 0, mode="summary")  # no step: zeros
    assert all(int(v.abs().sum()) == 0 for v in s0.values())
    plain = make_engine(model, width, N, device, 21, auto_reset=False)
    with pytest.raises(ValueError, match="auto_reset"):
        plain.rollout_policy(pol, T, mode="summary")
    check_launch(plain, pol, T, summary=False)  # transitions mode works without auto-reset


def test_observation_hand_over_from_reset_step_and_rollout(device):
    """case 5: the launch starts from the env's true current observation whatever ran before it -- reset, a per-call step,
    an open-loop rollout (which stores observations in its own output and leaves `obs` behind), a masked reset after
    such a rollout.  check_launch holds the first action to the reference on the observation a per-call replay reads."""
    eng = make_engine("halfcheetah", 7, N, device, 31)
    pol = make_policy(eng, (32,), "relu", 32)
    lo, hi = -1.0, 1.0
    gen = torch.Generator(device=device).manual_seed(5)

    def rand(*shape):
        return torch.rand(shape, device=device, generator=gen) * (hi - lo) + lo

    eng.reset()
    check_launch(eng, pol, 3)                       # directly after reset
    eng.step(rand(N, eng.sys.n_act))
    check_launch(eng, pol, 3, summary=False)        # after a step
    roll = eng.rollout(rand(4, N, eng.sys.n_act))
    stale = eng.obs.clone()
    assert not torch.equal(stale, roll["obs"][3])   # `rollout` left `obs` behind ...
    eng.snapshot()                                  # (... which a snapshot brings up to date)
    assert torch.equal(eng.obs, roll["obs"][3])
    check_launch(eng, pol, 3, summary=False)
    roll = eng.rollout(rand(4, N, eng.sys.n_act))   # rollout, then the launch with nothing in between
    want = roll["obs"][3].clone()
    st = engine_state(eng)
    out = eng.rollout_policy(pol, 1)
    x = np.concatenate([eng.ctx_table.cpu().numpy()[pol.ctx_rows][:, st["ctx_idx"].cpu().numpy().astype(np.int64)].T,
                        want.cpu().numpy()], axis=1).astype(np.float32)
    check_actions(pol, x[None], out["action"].cpu().numpy())
    roll = eng.rollout(rand(2, N, eng.sys.n_act))   # rollout, masked reset, launch
    mask = torch.zeros(N, dtype=torch.uint8, device=device)
    mask[::3] = 1
    eng.reset(mask)
    keep = (mask == 0)
    assert torch.equal(eng.obs[keep], roll["obs"][1][keep])
    check_launch(eng, pol, 3, summary=False)
    roll = eng.rollout(rand(2, N, eng.sys.n_act))   # a caller who overwrites the rollout's output hands the row over
    want = roll["obs"][1].clone()
    roll["obs"].mul_(0.5)
    eng.set_current_obs(want)
    assert torch.equal(eng.obs, want)
    check_launch(eng, pol, 3, summary=False)


def test_goal_wrapper_and_env_front_end(device):
    """the goal wrapper runs shared code (its success column is a per-step record, skipped in summary mode), and
    CARLBraxEnv.rollout_policy forwards to the engine"""
    from carl_amd.envs import CARLBraxAnt

    contexts = {k: {"target_distance": d, "target_direction": c, "target_radius": 0.3}
                for k, (d, c) in enumerate([(0.05, 112), (0.4, 334), (1.0, 1), (2.0, 32)])}
    env = CARLBraxAnt(batch_size=64, contexts=contexts, obs_context_features=["target_distance", "target_direction"],
                      device=device)
    env.reset(seed=3)
    eng = env.env
    assert eng.sys.goal_mode == 1
    rng = np.random.default_rng(3)
    pol = BraxMLPPolicy.for_env(env, BP.make_layers(rng, 2 + eng.D, (16,), eng.sys.n_act), "relu")
    assert pol.context_names == ["target_direction", "target_distance"]  # FlattenObservation sorts a Dict's keys
    snap = eng.snapshot()
    out = env.rollout_policy(pol, 5)
    after = engine_state(eng)
    goal_after = eng.goal_pos.clone()
    eng.restore(snap)
    ref = eng.rollout(out["action"], eng.alloc_rollout(5))
    for k in RECORDS + ("success",):
        assert torch.equal(out[k], ref[k]), k
    assert_same_state(after, engine_state(eng))
    assert torch.equal(goal_after, eng.goal_pos)
    eng.restore(snap)
    canary = eng.success.clone()
    env.rollout_policy(pol, 5, mode="summary")
    assert_same_state(after, engine_state(eng))
    assert torch.equal(goal_after, eng.goal_pos) and torch.equal(eng.success, canary)

    env = CARLBraxAnt(batch_size=64, obs_context_features=["gravity", "friction"], device=device)
    env.reset(seed=4)
    pol = BraxMLPPolicy.from_sequential(env, torch.nn.Sequential(torch.nn.Linear(29, 16), torch.nn.Tanh(),
                                                                 torch.nn.Linear(16, 8)))
    assert pol.context_names == ["friction", "gravity"] and pol.activation == "tanh"
    out = env.rollout_policy(pol, 4)
    assert tuple(out["action"].shape) == (4, 64, 8) and bool(torch.isfinite(out["action"]).all())
    with pytest.raises(NotImplementedError):
        env.env.evaluate_policy(pol, 1, 1)
