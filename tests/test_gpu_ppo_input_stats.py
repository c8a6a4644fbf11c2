"""carl_ppo_input_stats / carl_brax_ppo_input_stats on the GPU, through ``ppo_input_stats`` and ``carl_amd.PPO``'s
``normalize_inputs``: the slabs of real rollout buffers (CartPole with two context inputs in pitched rows, Pendulum, Brax
Hopper, Brax Ant with two context inputs; round robin with stride 2 under a TimeLimit of 3, so the context moves inside
the buffer) against ppo_norm_ref.py's exact sums at the derived float64 bound, the slab layout, the bits of two calls, and
the existing merge behind them: InputStats' mean / variance, the actor's and the critic's sections, a non-zero shift from
a previous merge, and a constant observation column.

Lane counts 1, 63, 65, 257, 300: a partial wavefront, a partial workgroup, more than one workgroup, more than one pass
per thread; T in {1, 2, 9}: T = 1 reads obs0 only."""
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


def classic(kind, n_ctx, N):
    fam = {"cartpole": _lib.CARTPOLE, "pendulum": _lib.PENDULUM}[kind]
    eng = PC.make_engine(fam, N, _lib.SEL_ROUND_ROBIN, n_contexts=7, seed=5, max_episode_steps=3, selector_stride=2)
    rng = np.random.default_rng(11)
    # the context inputs: the one row policy_cases.context_table varies (a wrong id moves the sums past the bound), then
    # row 0, which is the same number in every context
    varied = list(PC.FAMILIES[fam].get_context_features()).index(PC.VARIED[fam])
    assert varied != 0
    rows = [varied, 0][:n_ctx]
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
    """the slab layout, and each input's sums within n * 2^-53 * sum |terms| of the exact ones"""
    part = res["input_partial"].cpu().numpy()
    slabs = _lib.load().carl_ppo_input_stats_slabs(N, T)
    assert part.shape == (slabs, 2, NR.MAX_IN) and part.dtype == np.float64
    assert res["steps"].dtype == torch.int32 and res["steps"].cpu().tolist() == [T] * N
    assert (part[:, :, n_in:].view(np.uint64) == 0).all(), "entries at and beyond n_in are +0.0"
    S1, S2, A1, A2 = NR.input_sums_ref(x, shift)
    n = T * N
    for q, (S, A) in enumerate(((S1, A1), (S2, A2))):
        got = np.array([math.fsum(part[:, q, i]) for i in range(n_in)])
        err, bound = np.abs(got - S), NR.sums_bound(n, A)
        print(f"{label} S{q + 1}: worst |err| {err.max():.3e}, worst |err| / bound "
              f"{np.max(err / np.maximum(bound, 1e-300)):.3e} (n = {n})")
        assert np.all(err <= bound)
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
    if T == 9 and N >= 63:
        cid = buf["context_id"].cpu().numpy()
        assert (cid != cid[0]).any(), "the context moves inside the buffer"
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
