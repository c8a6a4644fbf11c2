"""Every reachable classic-control kernel instance against the float64 oracle (oracle/carl_oracle.c), per lane.

carl_amd.hip can launch 125 functions of five templates: 60 `rollout_staged_kernel`, 24 `rollout_kernel` (direct
stores), 24 `step_kernel`, 12 `reset_kernel`, 5 `rollout_staged_pair_kernel`; 14 of them (int64 actions for the two Box
families: 6 staged, 4 direct, 4 per-call) are refused by the argument check and never launched.  tests/
classic_kernel_cases.py names a configuration for each of the other 111 and tests/test_classic_kernel_table.py holds
that table against the source and the library's launch rule on the host; here every case runs:

a. the route: `carl_rollout_plan_io`, asked on the live engine with the launch's own buffers, names the case's instance;
b. the launch, from a reset, with episodes ending inside the window (small TimeLimit; CartPole's longer windows also
   terminate), T in {1, 5, 9, 21, 37} (never a multiple of the 8-step chunk, nor of the pair kernel's 4), a ragged last
   workgroup and n % 16 != 0 through the row pitch -- full size (65 547 / 32 779 lanes) where the lean instance needs it.
   A sentinel row behind the last step stays untouched, padding columns included; rows of a wider array (the `wide`
   layout) keep the columns behind their lanes.  (The padding columns of the engine's own padded rows are the
   launch's to write: they receive the records of the padding lanes, carl_amd.h: carl_rollout_pitch.)
c. the oracle: every (t, lane) re-stepped by `O.transitions` (float64) from the state the previous output row
   determines, in the context the lane held at that step, terminal observations where the instance writes them
   (tests/test_gpu_parity.py: restep_rollout_with_oracle, one call per case: one cap of 8 threshold-edge flags);
   the reset itself bit-exact against the oracle engine;
d. the per-call path: outputs, state, counters and the finished-episode log (as a multiset) equal the same number of
   `step()` calls on a twin engine bit for bit; the cases of a group (int32 / int64 / uint8, float32 / float16 /
   bfloat16, staged / direct by flag / direct by shape) equal each other bit for bit.

Per-call instances are compared per lane with the oracle on random transitions at lane counts on both sides of
`pick_block`'s block size; reset instances bit-exactly in all three modes (whole batch, mask, indexed); the pair
instances equal two separate launches bit for bit and are re-stepped by the oracle.

Tolerances.  The five float64-parity families: |d| <= 1e-5 (1 + |x|), flags exact but for rows within the helper's
margin of a threshold (<= 8 per case).  AcrobotFast (float32 RK4, opt-in): the oracle's own float32 variant deviates
from its float64 variant by at most 2.32e-6 under the same `rel_err` over exactly this matrix's AcrobotFast inputs
(measured on the CPU: test_classic_kernel_table.py::test_acrobot_fast_bar_comes_from_the_float32_oracle_on_the_matrix_
inputs); three times that is 7.0e-6, below the recorded 5e-5 of test_acrobot_fp32_mode_is_close_on_typical_states, so
the bar is max(5e-5, 3 x 2.32e-6) = 5e-5 -- for the rollouts' free-running states as for the typical states of the
per-call cases.
"""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import classic_kernel_cases as K
import test_gpu_parity as P
from carl_amd import _lib
from oracle import oracle as O

pytestmark = pytest.mark.gpu

TORCH_DTYPE = {"i32": torch.int32, "i64": torch.int64, "u8": torch.uint8, "f32": torch.float32, "f16": torch.float16,
               "bf16": torch.bfloat16}
OUTPUTS = ("obs", "reward", "terminated", "truncated")
COUNTERS = ("state", "elapsed", "ctx_idx", "episode", "n_calls", "ep_return", "last_return", "last_length",
            "episodes_done", "ctx_obs")
SENTINEL = {"obs": -7.0, "reward": -7.0, "terminated": 9, "truncated": 9, "final_obs": -7.0}


def _engine(case, table, device, **over):
    from carl_amd.engine import VecEngine

    kw = dict(K.engine_kwargs(case), auto_reset=case.auto_reset, max_episode_steps=case.max_steps,
              fin_capacity=(1 << 16) if case.fin else 0, acrobot_fp32=case.fp32)
    kw.update(over)
    return VecEngine(case.family, table, case.n, device, **kw)


def _oracle_engine(case, table, precision="f32"):
    return O.Engine(case.family, table, case.n, autoreset=case.auto_reset, max_steps=case.max_steps, precision=precision,
                    **K.engine_kwargs(case))


def _buffers(case, eng, T):
    """-> (output dict of [T + 1, n, ...] arrays or views, the whole arrays behind them), everything a sentinel"""
    n, D, dev = case.n, eng.D, eng.device
    keys = OUTPUTS + (("final_obs",) if case.final_obs else ())
    if case.layout == "padded" or case.direct:
        out = eng.alloc_rollout(T + 1, final_obs=case.final_obs)
        full = {k: (v._base if v._base is not None else v) for k, v in out.items()}
    else:
        pitch = K.WIDE_PITCH if case.layout == "wide" else n
        full = {k: torch.empty((T + 1, pitch) + ((D,) if "obs" in k else ()),
                               dtype=torch.uint8 if k in ("terminated", "truncated") else torch.float32, device=dev) for k in keys}
        out = {k: v[:, :n] for k, v in full.items()}
    for k, v in full.items():
        v.fill_(SENTINEL[k])
    return out, full


def _run(case, device, table, acts_np):
    """reset + the case's launch -> (engine, outputs [T + 1, ...], reset state [n, S])"""
    T = case.T
    eng = _engine(case, table, device)
    if case.direct:
        eng.b.flags |= _lib.FLAG_ROLLOUT_DIRECT
    eng.reset()
    s0 = eng.state.t().cpu().numpy()
    acts = torch.as_tensor(acts_np, device=device).to(TORCH_DTYPE[case.dtype])
    out, full = _buffers(case, eng, T)
    r = eng._prepare_rollout(acts, out)
    assert r.dt == K.DTYPE_CODE[case.dtype] and r.io.row_pitch == case.row_pitch()
    # (a) the route, asked with the very structs of the launch
    assert K.instance_of(case, K.plan_of(eng.b, r.io)) == case.instance, case
    with warnings.catch_warnings():
        warnings.simplefilter("ignore" if case.layout == "dense" else "error", RuntimeWarning)  # (the direct-shape warning)
        eng._launch_rollout(r)
    torch.cuda.synchronize()
    # (b) the sentinel row behind the last step, padding columns included; columns that are not the launch's
    for k, v in full.items():
        assert bool((v[T] == SENTINEL[k]).all()), (case, k, "row T")
        if case.layout == "wide":
            assert bool((v[:T, case.n:] == SENTINEL[k]).all()), (case, k, "columns behind the lanes")
    return eng, out, s0


def _restep(case, table, s0, ctx_hist, acts_np, out, monkeypatch):
    """(c): every (t, lane) of the output re-stepped by the float64 oracle"""
    outs = {k: out[k][: case.T] for k in OUTPUTS + (("final_obs",) if case.final_obs else ())}
    rows, s_prev, a, flat, kept = K.flatten_rollout(case, s0, table[ctx_hist], acts_np, outs)
    if case.fp32:
        monkeypatch.setattr(P, "TOL", K.ACROBOT_FAST_BAR)
    done = int(((flat["terminated"] | flat["truncated"]) != 0).sum())
    assert P.restep_rollout_with_oracle(case.family, rows, s_prev, a, flat) >= kept - (0 if case.final_obs else done) - 8


@pytest.mark.parametrize("case", K.ROLLOUT_CASES, ids=str)
def test_rollout_instance_matches_oracle_and_repeated_step(device, case, monkeypatch):
    table, acts_np = K.table_and_actions(case)
    T, n = case.T, case.n
    e1, out, s0 = _run(case, device, table, acts_np)

    # the reset the rollout started from: bit-exact against the oracle engine (AcrobotFast: the float32 Acrobot's)
    ora = _oracle_engine(case, table)
    ora.reset()
    np.testing.assert_array_equal(s0, ora.state)

    # (d) the same steps one launch each, on a twin engine with every optional output on
    e2 = _engine(case, table, device)
    e2.reset()
    np.testing.assert_array_equal(e2.ctx_idx.cpu().numpy(), ora.ctx_idx)
    a32 = torch.as_tensor(acts_np, device=device)
    ctx_hist, n_done = [], 0
    for t in range(T):
        ctx_hist.append(e2.ctx_idx.cpu().numpy().copy())
        obs, rew, term, trunc = e2.step(a32[t])
        assert torch.equal(out["obs"][t], obs) and torch.equal(out["reward"][t], rew), (case, t)
        assert torch.equal(out["terminated"][t], term) and torch.equal(out["truncated"][t], trunc), (case, t)
        d = (term | trunc).bool()
        n_done += int(d.sum())
        if case.final_obs:
            assert torch.equal(out["final_obs"][t][d], e2.final_obs[d]), (case, t)
    for name in COUNTERS:
        assert torch.equal(getattr(e1, name), getattr(e2, name)), (case, name)
    assert n_done >= n  # episodes ended inside the window
    if case.fin:
        l1, r1, n1, d1 = e1.drain_finished()
        l2, r2, n2, d2 = e2.drain_finished()
        assert d1 == 0 and d2 == 0 and l1.numel() == n_done == int(e1.episodes_done.sum())
        assert sorted(zip(l1.tolist(), r1.tolist(), n1.tolist())) == sorted(zip(l2.tolist(), r2.tolist(), n2.tolist()))
    ctx_hist = np.stack(ctx_hist)
    if case.selector == K.STATIC:
        assert (ctx_hist == ctx_hist[0]).all()
    else:
        assert T <= case.max_steps or (ctx_hist[-1] != ctx_hist[0]).any()  # lanes did move
    if case.selector == K.RR and case.auto_reset:  # the k-th reset of a lane moves it k strides on
        done = (out["terminated"][:T] | out["truncated"][:T]).cpu().numpy() != 0
        before = np.concatenate([np.zeros((1, n), np.int64), np.cumsum(done, axis=0)[:-1]])
        np.testing.assert_array_equal(ctx_hist, (ctx_hist[0] + 3 * before) % case.n_ctx)

    # (c) the oracle
    _restep(case, table, s0, ctx_hist, acts_np, out, monkeypatch)


@pytest.mark.parametrize("group", sorted(K.groups()), ids=str)
def test_flavours_and_routes_of_a_group_agree_bit_for_bit(device, group):
    """int32 / int64 / uint8, float32 / float16 / bfloat16 (fed the same values), staged / direct by flag / direct by
    shape: the same transitions and the same engine state"""
    cases = K.groups()[group]
    ref = None
    for case in cases:
        table, acts_np = K.table_and_actions(case)
        eng, out, _ = _run(case, device, table, acts_np)
        cur = {k: out[k][: case.T] for k in out}
        cur.update({k: getattr(eng, k) for k in COUNTERS})
        if ref is None:
            ref = (case, cur)
            continue
        assert sorted(cur) == sorted(ref[1])
        for k, v in cur.items():
            if k == "final_obs":
                d = (cur["terminated"] | cur["truncated"]).bool()
                assert torch.equal(v[d], ref[1][k][d]), (ref[0], case, k)
            else:
                assert torch.equal(v, ref[1][k]), (ref[0], case, k)


# ---------------------------------------------------------------- per-call step
@pytest.mark.parametrize("case", K.STEP_CASES, ids=str)
def test_step_instance_matches_oracle(device, case):
    from carl_amd.engine import VecEngine

    table, idx, s, a = K.step_inputs(case)
    n = case.n
    eng = VecEngine(case.family, table, n, device, selector=K.STATIC, auto_reset=False, ctx_idx0=idx, acrobot_fp32=case.fp32)
    io = _lib.StepIO()
    io.action_dtype = K.DTYPE_CODE[case.dtype]
    plan = K.plan_of(eng.b, io)
    assert K.instance_of(case, plan) == case.instance and plan.step_block == K.STEP_BLOCK[case.label.split("-")[2]]
    eng.reset()
    eng.state.copy_(torch.as_tensor(np.ascontiguousarray(s.T)))
    act = torch.as_tensor(a, device=device).to(TORCH_DTYPE[case.dtype])
    obs, rew, term, trunc = eng.step(act)
    torch.cuda.synchronize()
    assert eng._io.action_dtype == K.DTYPE_CODE[case.dtype]
    s2, obs, rew, term = eng.state.t().cpu().numpy(), obs.cpu().numpy(), rew.cpu().numpy(), term.cpu().numpy()
    rows = table[idx]
    w_s2, w_obs, w_rew, w_term = O.transitions(case.family, rows, s.astype(np.float64), a, precision="f64")
    tol = K.ACROBOT_FAST_BAR if case.fp32 else P.TOL
    e = [float(P.rel_err(s2, w_s2).max()), float(P.rel_err(obs, w_obs).max()), float(P.rel_err(rew, w_rew).max())]
    print(f"{case}: worst rel_err state {e[0]:.2e} obs {e[1]:.2e} reward {e[2]:.2e} (bar {tol:.0e})")
    assert max(e) <= tol, (case, e)
    diff = term != w_term
    assert (P.flag_margin(case.family, rows, np.asarray(w_s2))[diff] < 1e-6).all()
    assert diff.sum() <= max(2, 1e-4 * n)
    assert not trunc.any()


# ---------------------------------------------------------------- reset
@pytest.mark.parametrize("case", K.RESET_CASES, ids=str)
def test_reset_instance_is_bit_exact_in_all_three_modes(device, case):
    from carl_amd.engine import VecEngine

    n = case.n
    rng = np.random.default_rng(case.seed)
    table = P.random_table(case.family, rng, case.n_ctx)
    if case.family == O.ACROBOT:
        table[:, 10:14] = np.float32([-0.2, 0.3, -0.5, 0.4])
    for sel in (K.RR, K.RANDOM):
        kw = dict(selector=sel, selector_stride=3, seed=1234567891011 + sel, lane_offset=10_000_000_000)
        eng = VecEngine(case.family, table, n, device, acrobot_fp32=case.fp32, **kw)
        assert K.instance_of(case, K.plan_of(eng.b, _lib.StepIO())) == case.instance
        # AcrobotFast draws what the float64 Acrobot draws: the same reset state bit for bit
        twin = VecEngine(case.family, table, n, device, **kw) if case.fp32 else None
        ora = O.Engine(case.family, table, n, precision="f32", **kw)

        def check(obs, want):
            np.testing.assert_array_equal(eng.state.t().cpu().numpy(), ora.state)
            np.testing.assert_array_equal(eng.ctx_idx.cpu().numpy(), ora.ctx_idx)
            np.testing.assert_array_equal(eng.n_calls.cpu().numpy(), ora.n_calls)
            np.testing.assert_array_equal(eng.elapsed.cpu().numpy(), ora.elapsed)
            np.testing.assert_array_equal(eng.episode.cpu().numpy().view(np.uint32), ora.episode)
            np.testing.assert_array_equal(eng.ctx_obs.cpu().numpy(), table[ora.ctx_idx].T.astype(np.float32))
            assert P.rel_err(obs.cpu().numpy(), want).max() <= P.TOL
            if twin is not None:
                assert torch.equal(eng.state, twin.state) and torch.equal(eng.ctx_idx, twin.ctx_idx)

        for _ in range(2):  # whole batch
            obs = eng.reset()
            if twin is not None:
                twin.reset()
            check(obs, ora.reset())
        mask = (rng.random(n) < 0.3).astype(np.uint8)  # mask
        obs = eng.reset(torch.as_tensor(mask))
        if twin is not None:
            twin.reset(torch.as_tensor(mask))
        check(obs, ora.reset(mask))
        lanes = np.sort(rng.choice(n, n // 5, replace=False)).astype(np.int32)  # indexed: a list longer than its count
        idx = torch.as_tensor(np.concatenate([lanes, np.full(7, n - 1, np.int32)]), device=device)
        count = torch.tensor([lanes.size], dtype=torch.int32, device=device)
        obs = eng.reset_indexed(idx, count)
        if twin is not None:
            twin.reset_indexed(idx, count)
        m = np.zeros(n, np.uint8)
        m[lanes] = 1
        check(obs, ora.reset(m))


# ---------------------------------------------------------------- pair
@pytest.mark.parametrize("fam_b,auto_b,instance", K.PAIR_CASES, ids=lambda v: str(v) if not isinstance(v, tuple) else "")
def test_pair_instance_equals_two_launches_and_matches_oracle(device, fam_b, auto_b, instance, monkeypatch):
    parts = K.pair_parts(fam_b, auto_b)
    T = K.PAIR_T
    engs, twins, preps, outs, inputs = [], [], [], [], []
    for case in parts:
        table, acts_np = K.table_and_actions(case)
        e, w = _engine(case, table, device), _engine(case, table, device)
        e.reset()
        w.reset()
        out, full = _buffers(case, e, T)
        preps.append(e._prepare_rollout(torch.as_tensor(acts_np, device=device), out))
        engs.append(e), twins.append(w), outs.append((out, full)), inputs.append((table, acts_np))
    plans = [K.plan_of(e.b, r.io) for e, r in zip(engs, preps)]
    assert K.pair_instance_of(plans[0], plans[1], fam_b) == instance
    with torch.cuda.device(device):
        _lib.check(engs[0].lib.carl_rollout_pair(engs[0]._b_ref, C.byref(preps[0].io), engs[1]._b_ref, C.byref(preps[1].io), T,
                                                 engs[0]._stream()))
    torch.cuda.synchronize()
    for case, e, w, (out, full), (table, acts_np) in zip(parts, engs, twins, outs, inputs):
        for k, v in full.items():
            assert bool((v[T] == SENTINEL[k]).all()), (case, k)
        s0 = w.state.t().cpu().numpy()
        ctx0 = w.ctx_idx.cpu().numpy().copy()
        want = w.rollout(torch.as_tensor(acts_np, device=device))
        for k in OUTPUTS:
            assert torch.equal(out[k][:T], want[k]), (case, k)
        for name in COUNTERS:
            assert torch.equal(getattr(e, name), getattr(w, name)), (case, name)
        assert int((out["terminated"][:T] | out["truncated"][:T]).sum()) >= case.n
        _restep(case, table, s0, np.tile(ctx0, (T, 1)), acts_np, out, monkeypatch)
