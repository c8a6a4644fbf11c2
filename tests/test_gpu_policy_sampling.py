"""Sampled closed-loop rollout on the device (carl_rollout_policy_sampled / carl_evaluate_policy_sampled) by its
properties, against the host reference of its rule (sampling_ref.py, include/carl_amd.h: carl_policy_sampling_t) and
torch.distributions -- what test_gpu_policy_sampled_kernels.py's per-instance bounds do not show:

1. the random-word convention bit for bit (zero heads: equal logits make every operation of the categorical rule exact;
   mu = 0, log_std = 0 gives a = z);  2. teacher-forced actions against a float64 sample of oracle.policy_forward's
   outputs;  3. log_prob against torch.distributions;  4. the modes agree bit for bit (replay, summary, episodes,
   launch splits);  5. a point-mass categorical is the deterministic launch, and sample_seed moves only actions;
   6. statistics;  7. full size."""
import numpy as np
import pytest
import torch

import sampling_ref as SR
from carl_amd import _lib
from carl_amd.policy import MLPPolicy
from oracle import oracle as O
from policy_cases import SELECTORS, make_engine, n_outputs, words, zero_head_policy
from policy_checks import assert_replays, assert_same_state, assert_summary_reduces, engine_state, teacher

pytestmark = pytest.mark.gpu

SEED = 0x5EED5EED12345


def torch_policy(eng, widths, seed, gain=0.5):
    torch.manual_seed(seed)
    mods, prev = [], len(eng.ctx_obs_rows) + eng.D
    for w in widths:
        mods += [torch.nn.Linear(prev, w), torch.nn.Tanh()]
        prev = w
    mods.append(torch.nn.Linear(prev, n_outputs(eng)))
    seq = torch.nn.Sequential(*mods).double()
    with torch.no_grad():
        for m in seq:
            if isinstance(m, torch.nn.Linear):
                m.weight.mul_(gain)
    return seq


# ---------------------------------------------------------------- 1. the random-word convention, bit for bit
@pytest.mark.parametrize("sel", list(SELECTORS))
@pytest.mark.parametrize("family", [_lib.CARTPOLE, _lib.ACROBOT])
def test_equal_logits_take_the_documented_words(family, sel):
    n, T = 512, 200 if family == _lib.CARTPOLE else 600
    eng = make_engine(family, n, SELECTORS[sel], n_contexts=16, seed=3)
    pol = zero_head_policy(eng, widths=(8,))
    snap = eng.snapshot()
    out = eng.rollout_policy(pol, T, deterministic=False, sample_seed=SEED, log_prob=True)
    acts = out["action"][:T]
    done = (out["terminated"] | out["truncated"]).cpu().numpy()
    assert done.any(), "the launch must cross auto-resets"
    _, e, el = teacher(eng, pol, snap, acts)
    w = words(eng, e, el, SEED)
    na = int(eng.info.n_actions)
    want = SR.categorical_equal_logits(SR.u_categorical(w[0]), na)
    np.testing.assert_array_equal(acts.cpu().numpy(), want)
    np.testing.assert_allclose(out["log_prob"][:T].cpu().numpy(), np.full((T, n), -np.log(na)), rtol=2.5e-7, atol=0)


def test_gaussian_z_follows_the_documented_words():
    n, T = 512, 300
    eng = make_engine(_lib.PENDULUM, n, _lib.SEL_RANDOM, n_contexts=16, seed=4)
    pol = zero_head_policy(eng, log_std=0.0)
    snap = eng.snapshot()
    out = eng.rollout_policy(pol, T, deterministic=False, sample_seed=SEED, log_prob=True)
    acts = out["action"][:T]
    _, e, el = teacher(eng, pol, snap, acts)
    w = words(eng, e, el, SEED)
    z = SR.z_gaussian64(w[0], w[1])
    a = acts.cpu().numpy().astype(np.float64)
    bound = 2e-6 * np.maximum(1.0, np.abs(z))  # logf / cospif / sqrtf: a few ulp each
    assert np.all(np.abs(a - z) <= bound), np.abs(a - z).max()
    lp = out["log_prob"][:T].cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(lp, -z * z / 2 - 0.5 * np.log(2 * np.pi), atol=1e-5, rtol=1e-5)


# ---------------------------------------------------------------- 2 + 3. teacher forced, log_prob against torch
@pytest.mark.parametrize("family", [_lib.CARTPOLE, _lib.ACROBOT, _lib.MOUNTAINCAR, _lib.PENDULUM, _lib.MOUNTAINCAR_CONT])
@pytest.mark.parametrize("widths", [(), (32,), (64, 64)], ids=["linear", "1x32", "2x64"])
def test_teacher_forced_actions_and_log_probs(family, widths):
    n, T = 1024, 64
    eng = make_engine(family, n, _lib.SEL_ROUND_ROBIN, n_contexts=32, seed=6)
    seq = torch_policy(eng, widths, seed=len(widths) + family)
    box = not eng.info.action_is_discrete
    pol = MLPPolicy.from_sequential(eng, seq, log_std=-0.5 if box else None)
    snap = eng.snapshot()
    out = eng.rollout_policy(pol, T, deterministic=False, sample_seed=SEED + family, log_prob=True)
    acts = out["action"][:T]
    x, e, el = teacher(eng, pol, snap, acts)
    w = words(eng, e, el, SEED + family)
    r = O.policy_forward(pol.params, pol.n_in, pol.widths, pol.n_out, pol.activation, x.reshape(-1, pol.n_in))
    a = acts.cpu().numpy().reshape(-1)
    with torch.no_grad():
        y_t = seq(torch.as_tensor(x.reshape(-1, pol.n_in), dtype=torch.float64))
    if box:
        z = SR.z_gaussian64(w[0], w[1]).reshape(-1)
        sigma = np.exp(np.float64(np.float32(-0.5)))
        want = r.y64[:, 0] + sigma * z
        bound = r.bound[:, 0] + sigma * 2e-6 * np.maximum(1, np.abs(z)) + np.abs(want) * 2.0 ** -23
        assert np.all(np.abs(a - want) <= bound), np.abs(a - want).max()
        dist = torch.distributions.Normal(y_t[:, 0], torch.tensor(sigma, dtype=torch.float64))
    else:
        u = SR.u_categorical(w[0]).reshape(-1).astype(np.float64)
        want, margin = SR.categorical64(r.y64, u)
        # t = u S against the prefix sums in fp32: relative error of exp(y - m), the sums and the product, plus the
        # forward pass's own bound on y (twice: y_k and m)
        tol = 2 * r.bound.max(axis=1) + 16 * 2.0 ** -24 * (1 + np.abs(r.y64).max(axis=1))
        clear = margin > tol
        print(f"\n{_lib.family_info(family).n_actions} actions, {widths}: {int((~clear).sum())} of {a.size} lane-steps "
              "exempted near a prefix-sum boundary")
        assert (~clear).mean() < 1e-3
        np.testing.assert_array_equal(a[clear], want[clear])
        dist = torch.distributions.Categorical(logits=y_t)
    lp_t = dist.log_prob(torch.as_tensor(a, dtype=torch.float64 if box else torch.int64)).numpy()
    lp = out["log_prob"][:T].cpu().numpy().reshape(-1).astype(np.float64)
    np.testing.assert_allclose(lp, lp_t, atol=1e-5, rtol=1e-5)


# ---------------------------------------------------------------- 4. the modes agree, bit for bit
@pytest.mark.parametrize("family", [_lib.CARTPOLE, _lib.ACROBOT, _lib.PENDULUM])
def test_modes_and_launch_splits_agree(family):
    # T: past the first episode ends (Pendulum truncates at 200 steps, Acrobot at 500)
    n, T = 1024, {_lib.CARTPOLE: 64, _lib.PENDULUM: 256, _lib.ACROBOT: 512}[family]
    eng = make_engine(family, n, _lib.SEL_RANDOM, n_contexts=32, seed=8)
    box = not eng.info.action_is_discrete
    pol = MLPPolicy.from_sequential(eng, torch_policy(eng, (32,), seed=9, gain=1.0), log_std=0.3 if box else None)
    kw = dict(deterministic=False, sample_seed=SEED)
    snap = eng.snapshot()
    out = eng.rollout_policy(pol, T, log_prob=True, **kw)
    after = engine_state(eng)
    # replay through rollout()
    eng.restore(snap)
    assert_replays(eng, out, T, after)
    # summary = the exact reduction, same state
    eng.restore(snap)
    s = eng.rollout_policy(pol, T, mode="summary", **kw)
    count = assert_summary_reduces(eng, s, snap, out, T, after)
    assert count.sum() > 0
    # four launches of 16 = one of 64 (actions, log-probs, records, state)
    eng.restore(snap)
    parts = [eng.rollout_policy(pol, T // 4, log_prob=True, **kw) for _ in range(4)]
    for k in ("action", "log_prob", "obs", "reward", "terminated", "truncated"):
        whole = out[k][:T]
        cat = torch.cat([p[k][: T // 4] for p in parts])
        if whole.dtype == torch.float32:
            whole, cat = whole.view(torch.int32), cat.view(torch.int32)
        assert torch.equal(whole, cat), k
    assert_same_state(after, engine_state(eng))
    # episodes mode: each lane's first K episodes of the transitions
    K = 2
    eng.restore(snap)
    ep = eng.evaluate_policy(pol, K, T, **kw)
    rew = out["reward"][:T].cpu().numpy()
    done = (out["terminated"] | out["truncated"])[:T].cpu().numpy().astype(bool)
    got_n = ep["episodes"].cpu().numpy()
    np.testing.assert_array_equal(got_n, np.minimum(done.sum(0), K))
    ep_ret = snap["ep_return"].cpu().numpy().astype(np.float32).copy()
    seen = np.zeros(n, np.int64)
    want_ret = np.full((K, n), np.nan, np.float32)
    for t in range(T):
        ep_ret = (ep_ret + rew[t]).astype(np.float32)
        for lane in np.nonzero(done[t] & (seen < K))[0]:
            want_ret[seen[lane], lane] = ep_ret[lane]
            seen[lane] += 1
        ep_ret = np.where(done[t], np.float32(0), ep_ret)
    np.testing.assert_array_equal(ep["return"].cpu().numpy(), want_ret)


# ---------------------------------------------------------------- 5. point mass, and what sample_seed moves
@pytest.mark.parametrize("family", [_lib.CARTPOLE, _lib.ACROBOT])
def test_point_mass_is_the_deterministic_launch(family):
    n, T = 1024, 128
    eng = make_engine(family, n, _lib.SEL_RANDOM, n_contexts=32, seed=10)
    na = int(eng.info.n_actions)
    pol = zero_head_policy(eng, head_bias=[0.0] + [-200.0] * (na - 1), widths=(16,))
    snap = eng.snapshot()
    det = eng.rollout_policy(pol, T)
    det_state = engine_state(eng)
    eng.restore(snap)
    smp = eng.rollout_policy(pol, T, deterministic=False, sample_seed=SEED, log_prob=True)
    assert_same_state(det_state, engine_state(eng))
    for k in ("action", "obs", "reward", "terminated", "truncated"):
        assert torch.equal(det[k][:T], smp[k][:T]), k
    assert not torch.any(smp["log_prob"][:T] != 0)


def test_sample_seed_moves_actions_only():
    """a constant-action Box policy (a clipped huge mean): the trajectory is the same for any sample_seed -- resets,
    contexts and all -- while the recorded raw actions differ"""
    n, T = 1024, 300
    eng = make_engine(_lib.PENDULUM, n, _lib.SEL_RANDOM, n_contexts=32, seed=12)
    pol = zero_head_policy(eng, head_bias=[1e4], log_std=0.0)
    snap = eng.snapshot()
    a = eng.rollout_policy(pol, T, deterministic=False, sample_seed=1)
    sa = engine_state(eng)
    eng.restore(snap)
    b = eng.rollout_policy(pol, T, deterministic=False, sample_seed=2)
    assert_same_state(sa, engine_state(eng))
    assert (sa["n_calls"] > snap["n_calls"]).any(), "the launch must reset lanes"
    for k in ("obs", "reward", "terminated", "truncated"):
        assert torch.equal(a[k][:T], b[k][:T]), k
    assert (a["action"][:T] != b["action"][:T]).float().mean() > 0.99
    # and for a discrete family: different actions, the same context draws at the resets
    eng = make_engine(_lib.CARTPOLE, n, _lib.SEL_RANDOM, n_contexts=32, seed=13)
    pol = zero_head_policy(eng)
    snap = eng.snapshot()
    a = eng.rollout_policy(pol, 64, deterministic=False, sample_seed=1)
    eng.restore(snap)
    b = eng.rollout_policy(pol, 64, deterministic=False, sample_seed=2)
    assert (a["action"][:64] != b["action"][:64]).float().mean() > 0.3


# ---------------------------------------------------------------- 6. statistics
def test_categorical_frequencies_and_gaussian_moments():
    n, T = 65536, 256
    eng = make_engine(_lib.ACROBOT, n, _lib.SEL_STATIC, n_contexts=8, seed=14)
    bias = np.array([0.4, -0.3, 0.1])
    pol = zero_head_policy(eng, head_bias=bias)
    s = eng.rollout_policy(pol, T, deterministic=False, sample_seed=SEED)
    counts = torch.bincount(s["action"][:T].reshape(-1).long(), minlength=3).cpu().numpy().astype(np.float64)
    p = np.exp(bias - bias.max()) / np.exp(bias - bias.max()).sum()
    chi2 = ((counts - counts.sum() * p) ** 2 / (counts.sum() * p)).sum()
    pval = np.exp(-chi2 / 2)  # chi-square survival function, 2 degrees of freedom
    assert pval > 1e-4, (chi2, counts / counts.sum(), p)
    eng = make_engine(_lib.PENDULUM, n, _lib.SEL_STATIC, n_contexts=8, seed=15)
    pol = zero_head_policy(eng, log_std=0.0)
    z = eng.rollout_policy(pol, T, deterministic=False, sample_seed=SEED)["action"][:T].double()
    N = z.numel()
    assert abs(float(z.mean())) < 5 / np.sqrt(N)
    assert abs(float(z.var()) - 1) < 5 * np.sqrt(2 / N)


# ---------------------------------------------------------------- 7. full size
@pytest.mark.parametrize("family", [_lib.CARTPOLE, _lib.PENDULUM])
def test_full_size_both_modes(family):
    n, T = 65536, 1000
    eng = make_engine(family, n, _lib.SEL_RANDOM, n_contexts=4096, seed=21)
    box = family == _lib.PENDULUM
    pol = MLPPolicy.from_sequential(eng, torch_policy(eng, (64, 64), seed=21, gain=1.0), log_std=-1.0 if box else None)
    snap = eng.snapshot()
    out = eng.rollout_policy(pol, T, deterministic=False, sample_seed=SEED, log_prob=True)
    after = engine_state(eng)
    assert torch.isfinite(out["log_prob"][:T]).all()
    assert float(out["log_prob"][:T].max()) <= (1.0 if box else 0.0)
    eng.restore(snap)
    s = eng.rollout_policy(pol, T, mode="summary", deterministic=False, sample_seed=SEED)
    assert_same_state(after, engine_state(eng))
    assert int(s["episodes"].sum()) == int((out["terminated"] | out["truncated"])[:T].sum())
    eng.restore(snap)
    ref = eng.rollout(out["action"][:T])
    lanes = torch.as_tensor(np.random.default_rng(0).choice(n, 2048, replace=False), device=eng.device)
    for k in ("obs", "reward", "terminated", "truncated"):
        assert torch.equal(out[k][:T][:, lanes], ref[k][:, lanes]), k
    assert_same_state(after, engine_state(eng))
