"""The episodes mode of the Brax closed-loop rollout (include/carl_amd.h: carl_brax_evaluate_policy;
BraxVecEngine.evaluate_episodes) on the GPU: exactly K whole episodes per env in one launch, each env frozen at the step
that ends its K-th episode (or stopped by max_steps), the wavefront out of the step loop once none of its envs is live.

Every launch is held to the transitions-mode rollout_policy from the same snapshot (brax_episodes_cases.py): the records
bit for bit against its first K episodes per env, the engine state of every env against a rollout_policy of as many steps
as the env took.  Shapes follow tests/test_gpu_brax_policy.py: 77 envs, TimeLimit 5, a round-robin selector over 5
contexts with gravity and friction as policy inputs, half the ground models touched down.  The stop steps are spread by
construction (brax_episodes_cases.spread_start: envs start at `elapsed` 3 or 0), and each test asserts the spread it
relies on."""
import faulthandler

import numpy as np
import pytest
import torch

import brax_episodes_cases as BE
import brax_policy_cases as BP
from carl_amd import _lib
from carl_amd.brax_policy import BraxMLPPolicy

pytestmark = pytest.mark.gpu

N, T = BE.N, BE.MAX_STEPS


def same_bits(a, b):
    if a.is_floating_point():
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a, b)


def assert_spread(eng, res, stop, K, T_, capped):
    """two distinct stop steps inside one wavefront, an env frozen before max_steps; `capped`: an env stopped by max_steps"""
    per = BE.envs_per_wavefront(eng)
    assert any(len(set(stop[g: g + per].tolist())) >= 2 for g in range(0, stop.size, per))
    ep = res["episodes"].cpu().numpy()
    assert ((ep == K) & (stop < T_)).any()
    if capped:
        assert ((ep < K) & (stop == T_)).any()


@pytest.mark.parametrize("model,width", BP.instance_cases(), ids=str)
def test_every_kernel_instance(device, model, width):
    """case 1: every instantiated (class, width), K = 2 and K = 3 from one snapshot"""
    case = BP.instance_cases().index((model, width))
    seed = 9000 + 100 * list(BP.MODELS).index(model) + width
    eng = BE.make_engine(model, width, N, device, seed)
    widths, act = BP.NETWORKS[case % len(BP.NETWORKS)]
    pol = BE.make_policy(eng, widths, act, seed + 1)
    snap = BE.spread_start(eng, seed + 2)
    ref = BE.reference(eng, pol, snap, T)
    res2, stop2 = BE.check_launch(eng, pol, snap, ref, 2, T)
    assert_spread(eng, res2, stop2, 2, T, capped=False)
    res3, stop3 = BE.check_launch(eng, pol, snap, ref, 3, T)
    ep3 = res3["episodes"].cpu().numpy()
    # an env stopped by max_steps, mid-episode: the starts at `elapsed` 0 -- unless the model ends every episode long before
    # the TimeLimit (the inverted double pendulum falls within three steps, so three episodes fit into 12 steps for every
    # env): then the same K from the same snapshot under a max_steps that cuts them, held to the first rows of `ref`
    if not ((ep3 < 3) & (stop3 == T)).any():
        cut = T // 2
        res_cut, stop_cut = BE.check_launch(eng, pol, snap, ref, 3, cut)
        assert ((res_cut["episodes"].cpu().numpy() < 3) & (stop_cut == cut)).any()
    print(f"{model}/{width} {act}{list(widths)}: stop steps K=2 {sorted(set(stop2.tolist()))} K=3 {sorted(set(stop3.tolist()))}")


def test_two_weight_sets_inside_one_wavefront(device):
    """case 2: Ant at 9 lanes per env is 7 envs per wavefront; 512 envs in sets of 256: wavefront 36 holds envs of both"""
    n, steps = 512, 8
    eng = BE.make_engine("ant", 9, n, device, 41)
    assert (256 // 7) * 7 < 256 < (256 // 7 + 1) * 7
    pol = BraxMLPPolicy.stack([BE.make_policy(eng, (64, 64), "relu", 400 + k) for k in range(2)], 256)
    snap = BE.spread_start(eng, 42)
    ref = BE.reference(eng, pol, snap, steps)
    res, stop = BE.check_launch(eng, pol, snap, ref, 1, steps)
    assert_spread(eng, res, stop, 1, steps, capped=False)
    straddle = stop[252:259]
    assert len(set(straddle.tolist())) >= 2  # the wavefront of both sets has envs frozen at different steps
    # the sets differ: with the sets swapped the first actions of every env differ, so the launch used each env's own
    swapped = BraxMLPPolicy.stack([BE.make_policy(eng, (64, 64), "relu", 401 - k) for k in range(2)], 256)
    eng.restore(snap)
    other = eng.rollout_policy(swapped, 1)
    assert (other["action"][0] != ref[0]["action"][0]).any(dim=1).all()


def _hand_over_count(steps):
    """the smallest Ant env count at 16 lanes per env whose launch of `steps` steps has a wait_head fragment"""
    s = BP.build_model("ant")[0]
    s.lanes_per_env = 16

    def shape_of(n):
        b = _lib.Batch()
        b.n_lanes, b.flags = n, _lib.FLAG_AUTORESET
        code, sh = BP.launch_shape(b, s, _lib.Policy(), steps)
        assert code == 0 and sh.lanes_per_env == 16
        return sh

    g = 1
    while g < 1 << 13:
        sh = shape_of(4 * (g - 1) + 1)
        if sh.grid * sh.waves_per_workgroup < g:
            break
        g += 1
    n = 4 * (g - 1) + 1
    sh = shape_of(n)
    wait = [f for f in BP.fragments(sh, n, steps) if f[5]]
    assert wait, "no wait_head fragment"
    return n, sh, wait


@pytest.mark.parametrize("K", [1, 3])
def test_fragment_hand_over(device, K):
    """case 3: a group cut between two wavefronts.  K = 1: every env is frozen by step 5, head fragments leave early and
    tail fragments find nothing live; K = 3: live envs cross the hand-over.  Runs once under its own time limit: a launch
    that does not finish is a finding about the release path (the next wavefront spins on the head's flag)."""
    n, sh, wait = _hand_over_count(T)
    assert any(f[3] >= 5 for f in wait) and any(f[3] < 12 for f in wait)
    eng = BE.make_engine("ant", 16, n, device, 51)
    pol = BE.make_policy(eng, (64, 64), "tanh", 52)
    snap = BE.spread_start(eng, 53)
    ref = BE.reference(eng, pol, snap, T)
    torch.cuda.synchronize()
    faulthandler.dump_traceback_later(120, exit=True)  # (a hung launch ends the process: nothing more runs on the GPU)
    try:
        eng.restore(snap)
        res = eng.evaluate_episodes(pol, K, T)
        torch.cuda.synchronize()
    finally:
        faulthandler.cancel_dump_traceback_later()
    after = BE.full_state(eng)
    stop = BE.check_records(res, snap, ref, K, T)
    BE.check_state(eng, pol, snap, after, stop)
    split = sorted({f[2] for f in wait})  # the groups that were handed over
    if K == 1:
        # every env is frozen by step 5, so the tails that start at step 5 or later (asserted above to exist) find nothing
        # live.  That such a tail skips its body cannot be seen from outside: it rests on reading run()'s control flow; what
        # is seen here is that the launch ends and that what those tails leave behind is right
        assert stop.max() <= 5
    else:
        live_across = [f for f in wait if (stop[4 * f[2]: 4 * f[2] + 4] > f[3]).any()]
        assert live_across, "no live env crossed a hand-over"
    print(f"hand-over from {n} envs: {sh.grid} x {sh.waves_per_workgroup} wavefronts, {len(wait)} tail fragments, "
          f"{len(split)} split groups, K = {K}")


@pytest.mark.parametrize("model,width,mode", [("hopper", 4, "redraw"), ("ant", 9, "first_state")], ids=str)
def test_auto_reset_modes_caller_buffers_and_no_steps(device, model, width, mode):
    """case 4: both auto-reset modes; outputs into caller buffers with canaries round them; max_steps = 0"""
    eng = BE.make_engine(model, width, N, device, 61, autoreset_mode=mode)
    if mode == "first_state":
        eng.reset()  # (the first_state copy is taken by an explicit reset)
    pol = BE.make_policy(eng, (32,), "relu", 62)
    snap = BE.spread_start(eng, 63)
    ref = BE.reference(eng, pol, snap, T)
    K, pad = 2, 16
    full, view = {}, {}
    for k, dt, rows in BE.RESULT:
        size = K * N if rows else N
        fill = float("inf") if dt == torch.float32 else 77
        full[k] = torch.full((size + 2 * pad,), fill, dtype=dt, device=device)
        view[k] = full[k][pad: pad + size].view((K, N) if rows else (N,))
    eng.restore(snap)
    res = eng.evaluate_episodes(pol, K, T, out=view)
    assert res is view
    after = BE.full_state(eng)
    stop = BE.check_records(res, snap, ref, K, T)
    BE.check_state(eng, pol, snap, after, stop)
    assert_spread(eng, res, stop, K, T, capped=False)
    for k, v in full.items():
        edge = torch.cat([v[:pad], v[-pad:]])
        assert bool((torch.isinf(edge) if v.is_floating_point() else edge == 77).all()), k
    # max_steps = 0: every output filled, the state left alone
    eng.restore(snap)
    before = BE.full_state(eng)
    for v in full.values():
        v.fill_(1)
    res0 = eng.evaluate_episodes(pol, K, 0, out=view)
    assert int(res0["episodes"].abs().sum()) == 0 and int(res0["steps"].abs().sum()) == 0
    assert bool(torch.isnan(res0["return"]).all()) and int(res0["length"].abs().sum()) == 0
    assert bool((res0["context_id"] == -1).all()) and int(res0["terminated"].sum()) == 0
    now = BE.full_state(eng)
    for k, a in before.items():
        assert same_bits(a, now[k]), k
    plain = BE.make_engine(model, width, N, device, 61, auto_reset=False)
    with pytest.raises(ValueError, match="auto_reset"):
        plain.evaluate_episodes(pol, K, T)


def test_goal_wrapper(device):
    """case 4, the goal wrapper: goal_pos after the launch equals the per-stop-step replays', `success` is untouched.  The
    envs of the context whose target lies inside its radius succeed at their first step and freeze there (K = 1); the
    others run to max_steps."""
    from carl_amd.envs import CARLBraxAnt

    contexts = {k: {"target_distance": d, "target_direction": c, "target_radius": 0.3}
                for k, (d, c) in enumerate([(0.05, 112), (0.4, 334), (1.0, 1), (2.0, 32)])}
    env = CARLBraxAnt(batch_size=64, contexts=contexts, obs_context_features=["target_distance", "target_direction"],
                      device=device)
    env.reset(seed=3)
    eng = env.env
    assert eng.sys.goal_mode == 1 and eng.goal_pos is not None
    rng = np.random.default_rng(3)
    pol = BraxMLPPolicy.for_env(env, BP.make_layers(rng, 2 + eng.D, (16,), eng.sys.n_act), "relu")
    snap = eng.snapshot()
    steps = 5
    ref = BE.reference(eng, pol, snap, steps)
    eng.restore(snap)
    canary = eng.success.clone()
    res = eng.evaluate_episodes(pol, 1, steps)
    after = BE.full_state(eng)
    assert "goal_pos" in after
    stop = BE.check_records(res, snap, ref, 1, steps)
    assert torch.equal(eng.success, canary)
    BE.check_state(eng, pol, snap, after, stop)
    ep = res["episodes"].cpu().numpy()
    assert ((ep == 1) & (stop < steps)).any() and ((ep == 0) & (stop == steps)).any()
    assert bool(res["terminated"][0][torch.as_tensor(ep == 1, device=device)].all())  # reached goals terminate


def test_front_ends(device):
    """case 5: CARLBraxEnv.evaluate_episodes resets and forwards; episode_stats takes the result as it is; evaluate_policy
    is still refused"""
    from carl_amd.envs import CARLBraxHopper
    from carl_amd.policy import episode_stats

    env = CARLBraxHopper(batch_size=64, obs_context_features=["gravity", "friction"], device=device)
    env.reset(seed=4)
    eng = env.env
    pol = BraxMLPPolicy.from_sequential(env, torch.nn.Sequential(torch.nn.Linear(2 + eng.D, 16), torch.nn.Tanh(),
                                                                 torch.nn.Linear(16, eng.sys.n_act)))
    K, steps = 2, 300
    res = env.evaluate_episodes(pol, K, steps, seed=9)
    env.reset(seed=9)  # the same by hand: reset(seed), then the engine's launch
    want = eng.evaluate_episodes(pol, K, steps)
    for k, _, _ in BE.RESULT:
        assert same_bits(res[k], want[k]), k
    ep = res["episodes"].cpu().numpy()
    assert ep.max() >= 1  # a random policy drops a Hopper well within 300 steps
    st = episode_stats(res)
    valid = np.arange(K)[:, None] < ep[None, :]
    r = res["return"].cpu().numpy().astype(np.float64)[valid]
    assert st["count"] == valid.sum() and st["mean_return"] == r.mean() and st["std_return"] == r.std()
    cid = res["context_id"].cpu().numpy()[valid]
    np.testing.assert_array_equal(st["context_count"], np.bincount(cid, minlength=int(cid.max()) + 1))
    ln = res["length"].cpu().numpy().astype(np.float64)[valid]
    np.testing.assert_array_equal(st["context_mean_length"][cid[0]], ln[cid == cid[0]].mean())
    with pytest.raises(NotImplementedError, match="evaluate_episodes"):
        eng.evaluate_policy(pol, 1, 1)
    with pytest.raises(TypeError, match="BraxMLPPolicy"):
        eng.evaluate_episodes(object(), 1, 1)
    with pytest.raises(ValueError, match="evaluate_episodes output 'steps'"):
        bad = eng.alloc_policy_episodes(K)
        bad["steps"] = bad["steps"].to(torch.int64)
        eng.evaluate_episodes(pol, K, steps, out=bad)
