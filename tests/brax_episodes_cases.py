"""Toolkit of the tests of the episodes mode of the Brax closed-loop rollout (test_gpu_brax_episodes.py, test_gpu_brax_es.py
on the GPU, test_brax_episodes_abi.py on the host): engines and policies built as tests/test_gpu_brax_policy.py builds
them (a small restatement: test files are not imported), the start state that spreads the envs' stop steps by
construction, and the two references every launch is held to --

  * records: policy_cases.host_records of a transitions-mode rollout_policy of max_steps steps from the same snapshot,
    bit for bit, the context ids against the ctx_idx a per-call replay of its actions reads before each step;
  * engine state: for every distinct stop step s, rollout_policy of s steps from the same snapshot, compared on exactly
    the envs that stopped at s -- every env stops at some step, so none is left unchecked.

A plain module: importing it allocates nothing and touches no device."""
import numpy as np
import torch

import brax_policy_cases as BP
from brax_kernel_cases import touch_down
from policy_cases import host_records

N, MAX_STEPS, TIME_LIMIT, N_CTX = 77, 12, 5, 5
STATE = ("state", "elapsed", "ctx_idx", "episode", "n_calls", "ep_return", "episodes_done", "ctx_obs", "last_return",
         "last_length")
RESULT = (("episodes", torch.int32, False), ("steps", torch.int32, False), ("return", torch.float32, True),
          ("length", torch.int32, True), ("context_id", torch.int32, True), ("terminated", torch.uint8, True))


def make_engine(model, width, n, device, seed, **kw):
    """tests/test_gpu_brax_policy.py's engine: round-robin selector over 5 contexts, gravity and friction visible,
    TimeLimit 5, half the ground models' envs touched down"""
    from carl_amd.brax_engine import BraxVecEngine
    from oracle import oracle as O

    s, names, default = BP.build_model(model)
    s.lanes_per_env = width
    rng = np.random.default_rng(seed)
    rows = BP.context_rows(rng, N_CTX, default, names)
    kw.setdefault("max_episode_steps", TIME_LIMIT)
    eng = BraxVecEngine(s, len(names), rows, n, device, selector=O.SEL_ROUND_ROBIN, seed=seed,
                        ctx_obs_rows=[names.index("gravity"), names.index("friction")], **kw)
    assert width in eng.lane_widths()
    eng.reset()
    if model in BP.GROUND:
        eng.set_state64(touch_down(eng.sys, eng.state64().cpu().numpy()))
    return eng


def make_policy(eng, widths, act, seed):
    from carl_amd.brax_policy import BraxMLPPolicy

    rng = np.random.default_rng(seed)
    n_in = 2 + eng.D
    shift, scale, clip = BP.transform(rng, n_in)
    shift[0] += -10.0  # gravity ~ -10: centred like a normalised input
    return BraxMLPPolicy.for_env(eng, BP.make_layers(rng, n_in, widths, eng.sys.n_act), act, shift, scale, clip)


def spread_start(eng, seed):
    """3 open-loop steps, then a masked reset of every third env: the envs start the launch at `elapsed` 3 or 0, so under
    TimeLimit 5 their episodes end at steps 2, 7, 12 or 5, 10 -- envs of one wavefront stop at different steps"""
    gen = torch.Generator(device=eng.device).manual_seed(seed)
    eng.rollout(torch.rand((3, eng.n, eng.sys.n_act), device=eng.device, generator=gen) * 2.0 - 1.0)
    mask = torch.zeros(eng.n, dtype=torch.uint8, device=eng.device)
    mask[::3] = 1
    eng.reset(mask)
    el = eng.elapsed.cpu().numpy()
    assert (el[::3] == 0).all() and (el == 3).any()
    return eng.snapshot()


def full_state(eng):
    st = {k: getattr(eng, k).clone() for k in STATE}
    st["obs"] = eng.obs.clone()
    if eng.goal_pos is not None:
        st["goal_pos"] = eng.goal_pos.clone()
    return st


def _of_envs(t, sel, n):
    """the elements of the envs `sel` of a per-env tensor, whichever axis counts the envs ([n, ...] or [..., n])"""
    return t[sel] if t.shape[0] == n else t[..., sel]


def reference(eng, pol, snap, steps):
    """the transitions launch of `steps` steps from `snap` and the ctx_idx [steps, n] a per-call replay of its actions
    reads before each step.  Leaves the engine wherever the replay ends."""
    eng.restore(snap)
    out = eng.rollout_policy(pol, steps)
    eng.restore(snap)
    ctx = []
    for t in range(steps):
        ctx.append(eng.ctx_idx.cpu().numpy().astype(np.int64))
        eng.step(out["action"][t].contiguous())
    return out, np.stack(ctx)


def check_records(res, snap, ref, K, T):
    """an evaluate_episodes result against the first K episodes of the transitions launch ref = (out, ctx); -> stop steps"""
    out, ctx = ref
    count, stop, ret, length, term, at_step = host_records(snap, out, K, T)
    n = count.size
    assert {k for k, _, _ in RESULT} <= set(res)
    for k, dt, rows in RESULT:
        assert res[k].dtype == dt and tuple(res[k].shape) == ((K, n) if rows else (n,)), k
    np.testing.assert_array_equal(res["episodes"].cpu().numpy(), count)
    np.testing.assert_array_equal(res["steps"].cpu().numpy(), stop)
    np.testing.assert_array_equal(res["return"].cpu().numpy().view(np.int32), ret.view(np.int32))  # (NaN fill: one pattern)
    np.testing.assert_array_equal(res["length"].cpu().numpy(), length)
    np.testing.assert_array_equal(res["terminated"].cpu().numpy(), term)
    want_ctx = np.where(at_step >= 0, ctx[np.maximum(at_step, 0), np.arange(n)[None, :]], -1)
    np.testing.assert_array_equal(res["context_id"].cpu().numpy(), want_ctx)
    # the unused slots' fill values, spelled out (host_records initialises to the same)
    unused = np.arange(K)[:, None] >= count[None, :]
    assert np.isnan(res["return"].cpu().numpy()[unused]).all() and (res["length"].cpu().numpy()[unused] == 0).all()
    assert (res["context_id"].cpu().numpy()[unused] == -1).all() and (res["terminated"].cpu().numpy()[unused] == 0).all()
    return stop


def check_state(eng, pol, snap, after, stop, extra=()):
    """`after` (full_state after the episodes launch) against rollout_policy of s steps from `snap` for every distinct stop
    step s, on the envs that stopped at s.  extra: further engine attributes that must equal their value in `snap`."""
    n = stop.size
    steps = sorted(set(stop.tolist()))
    assert len(steps) <= MAX_STEPS
    checked = np.zeros(n, bool)
    for s in steps:
        eng.restore(snap)
        if s > 0:
            eng.rollout_policy(pol, s)
        now = full_state(eng)
        sel = torch.as_tensor(stop == s, device=eng.device)
        for k, a in after.items():
            x, y = _of_envs(a, sel, n), _of_envs(now[k], sel, n)
            if x.is_floating_point():
                x, y = x.view(torch.int32), y.view(torch.int32)
            assert torch.equal(x, y), (k, s)
        checked |= stop == s
    assert checked.all()  # no env is left unchecked
    for k in extra:
        assert torch.equal(getattr(eng, k), snap[k]), k


def check_launch(eng, pol, snap, ref, K, T):
    """one evaluate_episodes launch from `snap` against both references; -> (result, stop steps)"""
    eng.restore(snap)
    res = eng.evaluate_episodes(pol, K, T)
    after = full_state(eng)
    stop = check_records(res, snap, ref, K, T)
    check_state(eng, pol, snap, after, stop)
    return res, stop


def envs_per_wavefront(eng):
    return 64 // int(eng.sys.lanes_per_env)
