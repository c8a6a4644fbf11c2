"""carl_ppo_input_stats / carl_brax_ppo_input_stats on the GPU, through ``ppo_input_stats`` and ``carl_amd.PPO``'s
``normalize_inputs``: the slabs of real rollout buffers (CartPole with two context inputs in pitched rows, Pendulum, Brax
Hopper, Brax Ant with two context inputs; round robin with stride 2 under a TimeLimit of 3, so the context moves inside
the buffer) against ppo_norm_ref.py's exact sums at the derived float64 bound, the slab layout, the bits of two calls, and
the existing merge behind them: InputStats' mean / variance, the actor's and the critic's sections, a non-zero shift from
a previous merge, and a constant observation column.

Lane counts 1, 63, 65, 257, 300: a partial wavefront, a partial workgroup, more than one workgroup, more than one pass
per thread; T in {1, 2, 9}: T = 1 reads obs0 only.

Every slab is also held, bit for bit, to ppo_norm_ref.input_slabs_ref -- the same float64 additions in the kernel's order
(check_slabs) -- and REGIMES runs synthetic buffers at the shapes where the launch changes: the grid capped at 256
workgroups (more than 65 536 samples), a second round of a thread's 8-pass load window, every thread of the workgroup
active (n_in = 2 and n_in = 32).  Three documented edges have inputs of their own: context ids outside the table, row
T - 1 of obs (and rows behind it), a partial tensor longer than the slab count."""
import math

import numpy as np
import pytest
import torch

import brax_policy_cases as BPC
import brax_sampling_cases as BSC
import policy_cases as PC
import ppo_norm_ref as NR
from carl_amd import PPO, _lib
from carl_amd.brax_policy import BraxMLPPolicy
from carl_amd.policy import InputStats, MLPPolicy

pytestmark = pytest.mark.gpu

LANES = [1, 63, 65, 257, 300]
STEPS = [1, 2, 9]
KINDS = [("cartpole", 2), ("pendulum", 0), ("hopper", 0), ("ant", 2)]
CASES = [(kind, n_ctx, n, STEPS[(i + j) % 3]) for i, (kind, n_ctx) in enumerate(KINDS) for j, n in enumerate(LANES)]
# real buffers with the grid capped: 90 000 and 175 000 samples, a second round of the load window on some workgroups
CASES += [("cartpole", 2, 300, 300), ("pendulum", 0, 700, 250)]
CLASSIC = {"cartpole": _lib.CARTPOLE, "pendulum": _lib.PENDULUM, "mountaincar": _lib.MOUNTAINCAR}


def classic(kind, n_ctx, N):
    """an engine of N lanes over 7 contexts with an actor and a critic of n_ctx context inputs: the row the table varies
    first, then the table's rows from 0 on, again from 0 when they run out (28 of them give CartPole n_in = 32)"""
    fam = CLASSIC[kind]
    eng = PC.make_engine(fam, N, _lib.SEL_ROUND_ROBIN, n_contexts=7, seed=5, max_episode_steps=3, selector_stride=2)
    rng = np.random.default_rng(11)
    # the context inputs: the one row policy_cases.context_table varies (a wrong id moves the sums past the bound), then
    # row 0, which is the same number in every context
    varied = list(PC.FAMILIES[fam].get_context_features()).index(PC.VARIED[fam])
    assert varied != 0
    rows = ([varied] + [k % eng.F for k in range(n_ctx)])[:n_ctx]
    n_in = n_ctx + eng.D
    shift, scale = rng.normal(0, 0.5, n_in), rng.uniform(0.5, 1.5, n_in)
    box = not eng.info.action_is_discrete
    actor = MLPPolicy.for_env(eng, PC.rand_layers(rng, [n_in, 8, PC.n_outputs(eng)]), "tanh", shift, scale, 5.0,
                              context_features=rows, log_std=-0.5 if box else None)
    critic = MLPPolicy.for_env(eng, PC.rand_layers(rng, [n_in, 8, 1]), "tanh", shift, scale, 5.0, context_features=rows,
                               head="value")
    return eng, actor, critic


def brax(kind, n_ctx, N):
    eng = BSC.make_engine(kind, max(BPC.model_widths(kind)), N, "cuda", seed=5, max_episode_steps=3, selector_stride=2)
    rng = np.random.default_rng(12)
    rows = list(eng.ctx_obs_rows)[:n_ctx]
    n_in = n_ctx + eng.D
    shift, scale, clip = BPC.transform(rng, n_in)
    actor = BraxMLPPolicy.for_env(eng, BPC.make_layers(rng, n_in, (8,), eng.sys.n_act), "tanh", shift, scale, clip,
                                  context_features=rows, log_std=np.full(eng.sys.n_act, -0.5, np.float32))
    critic = BraxMLPPolicy.for_env(eng, BPC.make_layers(rng, n_in, (8,), 1), "tanh", shift, scale, clip,
                                   context_features=rows, head="value")
    return eng, actor, critic


def host_inputs(eng, actor, buf, T):
    """the gathered inputs of every sample of a buffer, from compact host copies (pitch = N)"""
    table = eng.ctx_table.cpu().numpy()
    return NR.gathered_inputs(actor, table, buf["context_id"][:T].cpu().numpy(), buf["obs0"].cpu().numpy(),
                              buf["obs"][:T].cpu().numpy(), eng.n, eng.n)


def check_slabs(label, res, x, shift, n_in, T, N):
    """the slab layout, each input's sums within n * 2^-53 * sum |terms| of the exact ones, and every slab bit for bit
    the ordered restatement's: each term d, d * d is an exact float64 (a contracted multiply-add rounds once, as the
    separate add does), so the order the header states decides every bit"""
    part = res["input_partial"].cpu().numpy()
    slabs = _lib.load().carl_ppo_input_stats_slabs(N, T)
    assert part.shape == (slabs, 2, NR.MAX_IN) and part.dtype == np.float64
    assert res["steps"].dtype == torch.int32 and res["steps"].cpu().tolist() == [T] * N
    assert (part[:, :, n_in:].view(np.uint64) == 0).all(), "entries at and beyond n_in are +0.0"
    assert np.isfinite(part).all()
    S1, S2, A1, A2 = NR.input_sums_ref(x, shift)
    n = T * N
    want = NR.input_slabs_ref(x, shift)
    differ = part.view(np.uint64) != want.view(np.uint64)
    print(f"{label}: {int(differ.sum())} of {slabs} x 2 x {n_in} slab entries differ from the ordered restatement"
          + (f", first at (slab, sum, input) {tuple(np.argwhere(differ)[0])}" if differ.any() else ""))
    within = True
    for q, (S, A) in enumerate(((S1, A1), (S2, A2))):
        got = np.array([math.fsum(part[:, q, i]) for i in range(n_in)])
        err, bound = np.abs(got - S), NR.sums_bound(n, A)
        print(f"{label} S{q + 1}: worst |err| {err.max():.3e}, worst |err| / bound "
              f"{np.max(err / np.maximum(bound, 1e-300)):.3e} (n = {n})")
        within = within and bool(np.all(err <= bound))
    assert within, "the whole buffer's sums are outside n * 2^-53 * sum |terms|"
    assert not differ.any(), "a slab differs from the ordered restatement"
    return part


@pytest.mark.parametrize("kind,n_ctx,N,T", CASES, ids=[f"{k}-ctx{c}-n{n}-T{t}" for k, c, n, t in CASES])
def test_input_sums_of_a_rollout_buffer_and_their_merge(kind, n_ctx, N, T):
    eng, actor, critic = (classic if kind in ("cartpole", "pendulum") else brax)(kind, n_ctx, N)
    n_in = actor.n_in
    assert n_in == n_ctx + eng.D
    ppo = PPO(eng, actor, critic, n_steps=T, n_epochs=1, normalize_inputs=True, seed=3)
    buf = ppo.collect()
    if kind == "cartpole" and T > 1:
        assert buf["obs"].stride(0) != N * eng.D  # pitched rows
    if T >= 9 and N >= 63:
        cid = buf["context_id"].cpu().numpy()
        assert (cid != cid[0]).any(), "the context moves inside the buffer"
    if T > 9:  # the large shapes: the grid is capped and a thread's load window goes round a second time
        G, _, _, passes, _ = NR.input_plan(T * N, n_in)
        assert G == 256 == _lib.load().carl_ppo_input_stats_slabs(N, T) and 8 < passes.max() <= 16 and passes.min() == 8
    x = host_inputs(eng, actor, buf, T)
    if n_ctx and N >= 63:  # the first context input takes several values over the buffer: the ids reach the sums
        assert len(np.unique(x[:, 0])) > 1, "the varied context row is among the inputs"
    # two calls: the same bits; the sums at the bound, under the template's shift
    first = eng.ppo_input_stats(ppo.actor(), buf, buf["obs0"], buf["context_id"])
    again = eng.ppo_input_stats(ppo.actor(), buf, buf["obs0"], buf["context_id"])
    part = check_slabs(f"{kind} n={N} T={T}", first, x, actor.shift, n_in, T, N)
    np.testing.assert_array_equal(part.view(np.uint64), again["input_partial"].cpu().numpy().view(np.uint64))
    # the next collect() merges the pending sums once (no update came between): the existing merge, in its order
    S1, S2 = NR.slabs_in_order(part, n_in)
    state, sh, sc = NR.merge_ref(S1, S2, T * N, actor.shift, None, ppo.norm_eps, ppo.input_stats.min_std)
    buf2 = ppo.collect()
    st = ppo.input_stats
    assert int(st.count.cpu()) == T * N
    np.testing.assert_allclose(st.mean.cpu().numpy(), state[1], rtol=1e-12, atol=0)
    np.testing.assert_allclose((st.var * st.count.double()).cpu().numpy(), state[2], rtol=1e-12, atol=1e-300)
    # ... and NumPy's statistics of the same inputs (d = fp32(x - shift): one rounding at the larger of |x|, |shift|)
    x64 = x.astype(np.float64)
    tol = 2.0 ** -23 * (np.abs(x64).max(axis=0) + np.abs(actor.shift.astype(np.float64)))
    assert np.all(np.abs(st.mean.cpu().numpy() - x64.mean(axis=0)) <= tol)
    assert np.all(np.abs(st.var.cpu().numpy() - x64.var(axis=0)) <= 4 * tol * x64.std(axis=0) + tol * tol)
    # the transform the device holds: the actor's section is the merge's, the critic's is the actor's bit for bit
    got_a, got_c = ppo.actor(), ppo.critic()
    NR.check_merged_transform(f"{kind} n={N} T={T}", got_a.shift, got_a.scale, state, sh, sc, ppo.norm_eps,
                              ppo.input_stats.min_std)
    a0, c0 = actor.weight_floats, critic.weight_floats
    np.testing.assert_array_equal(ppo.actor_params[0, a0: a0 + 2 * n_in + 1].cpu().numpy().view(np.uint32),
                                  ppo.critic_params[0, c0: c0 + 2 * n_in + 1].cpu().numpy().view(np.uint32))
    assert got_a.clip == actor.clip and got_c.clip == actor.clip
    np.testing.assert_array_equal(ppo.actor_params[0, :a0].cpu().numpy(), actor.params[0, :a0])  # (no update ran)
    # the second buffer's sums run under the merged, non-zero shift
    assert np.any(got_a.shift != actor.shift) and np.all(got_a.shift[np.abs(x64).max(axis=0) > 0] != 0)
    x2 = host_inputs(eng, actor, buf2, T)
    second = eng.ppo_input_stats(got_a, buf2, buf2["obs0"], buf2["context_id"])
    check_slabs(f"{kind} n={N} T={T}, merged shift", second, x2, got_a.shift, n_in, T, N)
    np.testing.assert_array_equal(buf2["obs0"].cpu().numpy(), buf["obs"][T - 1].cpu().numpy())


HUGE_ID = 2 ** 31 - 1


def synthetic(eng, N, T, seed, pitched, obs_rows=None):
    """a random buffer on the device -> (obs [obs_rows or T, N, D], obs0 [N, D], context_id [T, N]); pitched: rows of a
    16-aligned pitch whose padding columns hold NaN observations and the id 2^31 - 1, which nothing may read"""
    P = (N + 15) // 16 * 16 if pitched else N
    assert P > N or not pitched
    gen = torch.Generator(device="cuda").manual_seed(seed)
    obs = torch.randn((obs_rows or T, P, eng.D), device="cuda", generator=gen)
    cid = torch.randint(0, int(eng.b.n_contexts), (T, P), device="cuda", generator=gen, dtype=torch.int32)
    obs[:, N:] = float("nan")
    cid[:, N:] = HUGE_ID
    obs0 = torch.randn((N, eng.D), device="cuda", generator=gen)
    return obs[:, :N], obs0, cid[:, :N]


def gathered(eng, actor, obs, obs0, cid):
    N = eng.n
    return NR.gathered_inputs(actor, eng.ctx_table.cpu().numpy(), cid.cpu().numpy(), obs0.cpu().numpy(),
                              obs[: cid.shape[0]].cpu().numpy(), N, N)


# kind, context inputs, N, T, pitched rows -> n_in, slabs, samples per pass, passes, the workgroups that run one pass more
# than the others, the passes those run, the samples of the last pass (test_ppo_norm_reference.py holds the plan itself)
REGIMES = {
    # capped; workgroups 0 .. 94 run a 9th pass: a second round of the 8-pass window with one live slot
    "cartpole-capped-second-round": (("cartpole", 2, 300, 300, True), (6, 256, 42, 2143, 95, 9, 36)),
    "pendulum-capped-second-round": (("pendulum", 0, 700, 250, True), (3, 256, 85, 2059, 11, 9, 70)),
    # the cap engages at 259 tiles; 6 - 7 passes: capped, one round
    "cartpole-capped-one-round": (("cartpole", 2, 257, 257, True), (6, 256, 42, 1573, 37, 7, 25)),
    "hopper-capped": (("hopper", 0, 257, 257, False), (11, 256, 23, 2872, 56, 12, 16)),
    # every thread of the workgroup is active: 128 samples x 2 inputs, and 8 samples x 32 inputs (the packing limit:
    # CartPole's context rows listed until 28 of them stand before its 4 observations; 64 threads reduce; four rounds)
    "mountaincar-two-inputs": (("mountaincar", 0, 300, 9, True), (2, 11, 128, 22, 11, 2, 12)),
    "cartpole-32-inputs": (("cartpole", 28, 300, 9, True), (32, 11, 8, 338, 8, 31, 4)),
}


@pytest.mark.parametrize("name", list(REGIMES))
def test_slabs_of_a_synthetic_buffer_in_every_launch_regime(name):
    (kind, n_ctx, N, T, pitched), (n_in, slabs, spt, n_pass, extra, longest, last) = REGIMES[name]
    eng, actor, critic = (classic if kind in CLASSIC else brax)(kind, n_ctx, N)
    assert actor.n_in == n_in == n_ctx + eng.D and len(actor.ctx_rows) == n_ctx
    # the regime itself: the launch's slab count and the plan's passes per workgroup
    n = N * T
    G, got_spt, got_pass, passes, _ = NR.input_plan(n, n_in)
    assert G == slabs == _lib.load().carl_ppo_input_stats_slabs(N, T)
    assert (got_spt, got_pass) == (spt, n_pass) and n - (n_pass - 1) * spt == last
    assert passes.tolist() == [longest] * extra + [longest - 1] * (G - extra)
    assert (slabs == 256) == (n > 65536)
    assert spt * n_in == 256 or n_in not in (2, 32)  # (2 and 32: no idle thread)
    obs, obs0, cid = synthetic(eng, N, T, 40 + n_in, pitched)
    if pitched:
        assert obs.stride(0) != N * eng.D and cid.stride(0) != N
    first = eng.ppo_input_stats(actor, {"obs": obs}, obs0, cid)
    again = eng.ppo_input_stats(actor, {"obs": obs}, obs0, cid)
    x = gathered(eng, actor, obs, obs0, cid)
    if n_ctx:
        assert len(np.unique(x[:, 0])) > 1, "the varied context row is among the inputs"
    part = check_slabs(name, first, x, actor.shift, n_in, T, N)  # finite: no padding column was read
    np.testing.assert_array_equal(part.view(np.uint64), again["input_partial"].cpu().numpy().view(np.uint64))


def test_context_ids_outside_the_table_are_clamped():
    """-1, n_contexts and 2^31 - 1 at scattered samples, the first and the last among them: the sums are those of the ids
    clipped to [0, n_contexts - 1], slab by slab"""
    N, T = 300, 9
    eng, actor, critic = classic("cartpole", 2, N)
    C = int(eng.b.n_contexts)
    obs, obs0, cid = synthetic(eng, N, T, 7, True)
    bad = np.array([-1, C, HUGE_ID], np.int32)
    rng = np.random.default_rng(8)
    where = np.unique(np.concatenate([[0, N - 1, N, T * N - 1], rng.choice(T * N, 200, replace=False)]))
    ids = cid.cpu().numpy().copy()
    ids.reshape(-1)[where] = bad[np.arange(where.size) % 3]
    assert ids[0, 0] == -1 and ids[T - 1, N - 1] in bad
    cid.copy_(torch.as_tensor(ids))
    varied = eng.ctx_table.cpu().numpy()[actor.ctx_rows[0]]
    assert varied[0] != varied[C - 1] and len(np.unique(varied)) == C  # clamping to the wrong end, or wrapping, moves x
    x = gathered(eng, actor, obs, obs0, cid)
    low, high = ids.reshape(-1) < 0, ids.reshape(-1) >= C
    assert low.sum() > 50 and high.sum() > 100
    assert (x[low, 0] == varied[0]).all() and (x[high, 0] == varied[C - 1]).all()
    res = eng.ppo_input_stats(actor, {"obs": obs}, obs0, cid)
    check_slabs("ids outside the table", res, x, actor.shift, actor.n_in, T, N)


def test_the_last_row_of_obs_and_rows_behind_it_are_not_counted():
    N, T = 300, 9
    eng, actor, critic = classic("cartpole", 2, N)
    obs, obs0, cid = synthetic(eng, N, T, 9, True, obs_rows=T + 3)
    x = gathered(eng, actor, obs, obs0, cid)
    clean = check_slabs("clean rows", eng.ppo_input_stats(actor, {"obs": obs[:T]}, obs0, cid), x, actor.shift,
                        actor.n_in, T, N)
    obs[T - 1:] = float("nan")
    for label, rows in (("row T - 1 is NaN", obs[:T]), ("rows T - 1 .. T + 2 are NaN", obs)):
        assert rows.stride(0) == obs.stride(0) and torch.isnan(rows[T - 1]).all()
        part = eng.ppo_input_stats(actor, {"obs": rows}, obs0, cid)["input_partial"].cpu().numpy()
        assert np.isfinite(part).all(), label
        np.testing.assert_array_equal(part.view(np.uint64), clean.view(np.uint64), err_msg=label)


def test_a_partial_tensor_longer_than_the_slab_count_keeps_its_tail():
    N, T = 300, 9
    eng, actor, critic = classic("cartpole", 2, N)
    obs, obs0, cid = synthetic(eng, N, T, 10, True)
    slabs = _lib.load().carl_ppo_input_stats_slabs(N, T)
    canary = -7.25
    big = torch.full((slabs + 4, 2, NR.MAX_IN), canary, dtype=torch.float64, device="cuda")
    out = {"input_partial": big}
    res = eng.ppo_input_stats(actor, {"obs": obs}, obs0, cid, out=out)
    assert res is out and tuple(res["input_partial"].shape) == (slabs, 2, NR.MAX_IN)
    assert res["input_partial"].data_ptr() == big.data_ptr()
    assert (big[slabs:].cpu().numpy() == canary).all(), "the rows behind the slabs are untouched"
    x = gathered(eng, actor, obs, obs0, cid)
    part = check_slabs("oversized partial", res, x, actor.shift, actor.n_in, T, N)
    assert (part[:, :, : actor.n_in] != canary).all()
    np.testing.assert_array_equal(big[:slabs].cpu().numpy().view(np.uint64), part.view(np.uint64))


def test_a_constant_observation_column_gets_scale_zero():
    """a synthetic CartPole buffer in pitched rows whose observation entry 2 is the same fp32 value everywhere: the float64
    sums leave its variance below the merge's floor"""
    N, T = 300, 9
    eng, actor, critic = classic("cartpole", 2, N)
    P = (N + 15) // 16 * 16
    gen = torch.Generator(device="cuda").manual_seed(4)
    obs = torch.randn((T, P, eng.D), device="cuda", generator=gen)[:, :N]
    obs0 = torch.randn((N, eng.D), device="cuda", generator=gen)
    obs[:, :, 2] = 0.7
    obs0[:, 2] = 0.7
    cid = torch.randint(0, 7, (T, P), device="cuda", generator=gen, dtype=torch.int32)[:, :N]
    res = eng.ppo_input_stats(actor, {"obs": obs}, obs0, cid)
    x = NR.gathered_inputs(actor, eng.ctx_table.cpu().numpy(), cid.cpu().numpy(), obs0.cpu().numpy(), obs.cpu().numpy(), N, N)
    check_slabs("constant column", res, x, actor.shift, actor.n_in, T, N)
    block = torch.as_tensor(actor.params).to(eng.device).contiguous().clone()
    stats = InputStats(actor, eng.device)
    stats.update(res, block, policy=actor)
    got = MLPPolicy.unpack(actor, block.cpu().numpy()[0])
    col = 2 + 2  # behind the two context inputs
    assert len(np.unique(x[:, 0])) > 1  # the varied context row: the random ids reach the sums
    assert got.scale[col] == 0
    # (the mean is shift + fp32(0.7 - shift): one rounding of d at the larger magnitude, one of the fp32 mean)
    assert abs(float(got.shift[col]) - float(np.float32(0.7))) <= 2.0 ** -23 * (0.7 + abs(float(actor.shift[col])))
    moving = [i for i in range(actor.n_in) if x[:, i].max() > x[:, i].min()]
    still = [i for i in range(actor.n_in) if i not in moving]  # (context row 0 does not vary over this table either)
    assert moving == [0, 2, 3, 5] and np.all(got.scale[moving] > 0) and np.all(got.scale[still] == 0)
    assert float(stats.var[col].cpu()) <= (2.0 ** -18 * 0.7) ** 2


def test_flags_off_adds_no_keys_and_no_state():
    eng, actor, critic = classic("cartpole", 2, 65)
    ppo = PPO(eng, actor, critic, n_steps=2, n_epochs=1)
    buf = ppo.collect()
    assert "reward_normalized" not in buf and ppo.input_stats is None and ppo.return_stats is None
    ppo.update()
    np.testing.assert_array_equal(ppo.actor().shift.view(np.uint32), actor.shift.view(np.uint32))
    np.testing.assert_array_equal(ppo.actor().scale.view(np.uint32), actor.scale.view(np.uint32))
