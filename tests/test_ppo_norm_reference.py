"""The NumPy references of PPO's running normalisation (ppo_norm_ref.py) against independent statements of the same
quantities: np.mean / np.var of the gathered inputs, a 2-lane, 3-step case walked by hand, and a step-by-step
VecNormalize-style loop (SB3's RunningMeanStd.update_from_moments) for the returns; the ordered restatement of the input
slabs (input_plan / input_slabs_ref) against the counts of the GPU tests' launch regimes, a thread-by-thread walk of the
kernel's loops and the exact sums.  CPU-only."""
import math

import numpy as np
import pytest

import ppo_norm_ref as NR
import ppo_ref as R

CASES = [c for c in R.grad_cases() if c[6] is None or c[6] <= 600][:6]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_input_sums_and_merge_give_numpy_mean_and_variance(case):
    c = R.make_case(case)
    actor, N, P, T = c["actor"], c["N"], c["P"], c["T"]
    x = NR.gathered_inputs(actor, c["table"], c["context_id"], c["obs0"], c["obs"], N, P)
    assert x.shape == (T * N, actor.n_in) and x.dtype == np.float32
    # the gather, restated sample by sample for a few of them
    for m in (0, N - 1, N, T * N - 1):
        t, lane = divmod(m, N)
        ctx = [c["table"][r, c["context_id"][t, lane]] for r in actor.ctx_rows]
        o = c["obs0"][lane] if t == 0 else c["obs"][t - 1, lane]
        np.testing.assert_array_equal(x[m], np.concatenate([np.asarray(ctx, np.float32), o]))
    S1, S2, A1, A2 = NR.input_sums_ref(x, actor.shift)
    state, shift, scale = NR.merge_ref(S1, S2, T * N, actor.shift)
    x64 = x.astype(np.float64)
    # d = fp32(x - shift) carries one rounding of 2^-24 relative to max(|x|, |shift|): the mean inherits it
    tol = 2.0 ** -23 * (np.abs(x64).max(axis=0) + np.abs(actor.shift.astype(np.float64)))
    assert np.all(np.abs(state[1] - x64.mean(axis=0)) <= tol)
    var = state[2] / state[0]
    sd = x64.std(axis=0)
    assert np.all(np.abs(var - x64.var(axis=0)) <= 4 * tol * sd + tol * tol)
    assert state[0] == T * N
    const = sd == 0
    np.testing.assert_array_equal(scale[const], 0.0)
    np.testing.assert_allclose(scale[~const], 1.0 / np.sqrt(x64.var(axis=0)[~const] + 1e-8), rtol=1e-4)
    # a second batch merged by Chan's rule is the statistics of both
    state2, _, _ = NR.merge_ref(S1, S2, T * N, actor.shift, state)
    np.testing.assert_allclose(state2[1], x64.mean(axis=0), atol=tol.max())
    np.testing.assert_allclose(state2[2] / state2[0], x64.var(axis=0), rtol=1e-5, atol=1e-12)


def test_input_sums_of_a_hand_walked_buffer():
    """2 lanes, 3 steps, one context input and a 2-entry observation; pitch 4"""
    from carl_amd import _lib
    from carl_amd.policy import MLPPolicy
    import policy_cases as PC

    eng = PC.fake_engine(_lib.MOUNTAINCAR)
    actor = MLPPolicy.for_env(eng, [(np.zeros((3, 3)), None)], "identity", input_shift=[0.5, 0.25, -1.0],
                              context_features=[0])
    F = eng.F
    table = np.zeros((F, 3), np.float32)
    table[0] = [2.0, 3.0, 5.0]
    cid = np.array([[0, 2, 9, 9], [1, 1, 9, 9], [2, 0, 9, 9]], np.int32)  # (9: padding columns, never read)
    obs0 = np.array([[1.0, 10.0], [2.0, 20.0]], np.float32)
    obs = np.full((3, 4, 2), 99.0, np.float32)
    obs[0, :2] = [[3.0, 30.0], [4.0, 40.0]]
    obs[1, :2] = [[5.0, 50.0], [6.0, 60.0]]
    obs[2, :2] = [[7.0, 70.0], [8.0, 80.0]]  # the next collection's obs0: not counted
    x = NR.gathered_inputs(actor, table, cid, obs0, obs, 2, 4)
    want = np.array([[2, 1, 10], [5, 2, 20], [3, 3, 30], [3, 4, 40], [5, 5, 50], [2, 6, 60]], np.float32)
    np.testing.assert_array_equal(x, want)
    S1, S2, A1, A2 = NR.input_sums_ref(x, actor.shift)
    d = want.astype(np.float64) - np.array([0.5, 0.25, -1.0])
    np.testing.assert_array_equal(S1, d.sum(axis=0))        # (small dyadic numbers: every sum exact)
    np.testing.assert_array_equal(S2, (d * d).sum(axis=0))
    np.testing.assert_array_equal(A1, np.abs(d).sum(axis=0))
    assert S1.tolist() == [17.0, 19.5, 216.0]


# (n samples, n_in) of test_gpu_ppo_input_stats.py's regime cases -> (slabs, spt, passes, workgroups that run one pass
# more than the others, the passes those run, samples of the last pass)
PLAN_SHAPES = {(300 * 300, 6): (256, 42, 2143, 95, 9, 36), (700 * 250, 3): (256, 85, 2059, 11, 9, 70),
               (257 * 257, 6): (256, 42, 1573, 37, 7, 25), (257 * 257, 11): (256, 23, 2872, 56, 12, 16),
               (300 * 9, 2): (11, 128, 22, 11, 2, 12), (300 * 9, 32): (11, 8, 338, 8, 31, 4)}


@pytest.mark.parametrize("n,n_in", list(PLAN_SHAPES), ids=[f"n{n}-in{k}" for n, k in PLAN_SHAPES])
def test_input_plan_counts_every_sample_once(n, n_in):
    G, spt, n_pass, extra, longest, last = PLAN_SHAPES[(n, n_in)]
    got_G, got_spt, got_pass, passes, idx = NR.input_plan(n, n_in)
    assert (got_G, got_spt, got_pass) == (G, spt, n_pass)
    assert G == min(-(-n // 256), 256) and spt == 256 // n_in and n_pass == -(-n // spt)
    # the passes go round the grid: the first `extra` workgroups run `longest`, the others one fewer (extra == G: all)
    assert passes.shape == (G,) and passes.sum() == n_pass
    assert passes.tolist() == [longest] * extra + [longest - 1] * (G - extra)
    assert idx.shape == (G, longest, spt)
    live = idx[idx >= 0]
    np.testing.assert_array_equal(np.sort(live), np.arange(n))  # every sample exactly once
    assert n - (n_pass - 1) * spt == last
    # a thread's samples ascend (its chain is in pass order) and a pass is spt consecutive samples
    for w in (0, extra - 1, G - 1):
        rows = idx[w, : passes[w]]
        assert (rows[:, 0] == (w + G * np.arange(passes[w])) * spt).all()
        assert (idx[w, passes[w]:] == -1).all()
    tail = idx[(n_pass - 1) % G, (n_pass - 1) // G]
    assert tail[:last].tolist() == list(range(n - last, n)) and (tail[last:] == -1).all()


def walked_slabs(x, shift):
    """ppo_input_stats_kernel read line by line, one Python float per accumulator: the round loop of 8 passes per thread
    with its stride of 8 * G, the guards of a slot past the end, the LDS array and the 64 reducing threads"""
    n, n_in = x.shape
    G, ahead = min(-(-n // 256), 256), 8
    spt = 256 // n_in
    n_pass = -(-n // spt)
    d = (x - np.asarray(shift, np.float32)[None, :]).astype(np.float32).astype(np.float64)
    part = np.full((G, 2, 32), np.nan)
    for w in range(G):
        red = np.zeros((2, 256))
        for tid in range(256):
            i, so = tid % n_in, tid // n_in
            s1 = s2 = 0.0
            if so < spt:
                for p0 in range(w, n_pass, ahead * G):
                    for k in range(ahead):
                        p = p0 + k * G
                        m = p * spt + so
                        if p < n_pass and m < n:
                            s1 += float(d[m, i])
                            s2 += float(d[m, i]) * float(d[m, i])
            red[0, tid], red[1, tid] = s1, s2
        for q in range(2):
            for j in range(32):
                s = 0.0
                if j < n_in:
                    for k in range(spt):
                        s += red[q, k * n_in + j]
                part[w, q, j] = s
    return part


@pytest.mark.parametrize("n,n_in", [(300 * 9, 32), (300 * 9, 2), (257 * 80, 6), (1, 5), (257, 3)])
def test_input_slabs_restatement_equals_the_kernel_walked_thread_by_thread(n, n_in):
    """the vectorised restatement against a literal walk of the kernel's loops, bit for bit; 2 700 x 32 runs four rounds
    of the ahead loop per thread, 20 560 x 6 two passes, the others one"""
    rng = np.random.default_rng(n + n_in)
    x = rng.normal(0.3, 2.0, (n, n_in)).astype(np.float32)
    x[rng.random((n, n_in)) < 0.01] = -0.0
    shift = rng.normal(0, 0.5, n_in).astype(np.float32)
    shift[0] = 0.0  # (x = -0.0 under a zero shift: d = -0.0)
    got = NR.input_slabs_ref(x, shift)
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got.view(np.uint64), walked_slabs(x, shift).view(np.uint64))


@pytest.mark.parametrize("n,n_in", list(PLAN_SHAPES), ids=[f"n{n}-in{k}" for n, k in PLAN_SHAPES])
def test_input_slabs_restatement_meets_the_exact_sums(n, n_in):
    rng = np.random.default_rng(n_in)
    x = rng.normal(0.3, 2.0, (n, n_in)).astype(np.float32)
    shift = rng.normal(0, 0.5, n_in).astype(np.float32)
    part = NR.input_slabs_ref(x, shift)
    G = PLAN_SHAPES[(n, n_in)][0]
    assert part.shape == (G, 2, NR.MAX_IN) and (part[:, :, n_in:].view(np.uint64) == 0).all()
    S1, S2, A1, A2 = NR.input_sums_ref(x, shift)
    for q, (S, A) in enumerate(((S1, A1), (S2, A2))):
        got = np.array([math.fsum(part[:, q, i]) for i in range(n_in)])
        assert np.all(np.abs(got - S) <= NR.sums_bound(n, A))
    # a sample moved to another slab, or counted twice: per slab, the plan's samples added exactly
    _, _, _, _, idx = NR.input_plan(n, n_in)
    d = (x - shift[None, :]).astype(np.float32).astype(np.float64)
    for w in (0, G - 1):
        m = idx[w][idx[w] >= 0]
        for i in range(n_in):
            exact, mag = math.fsum(d[m, i]), math.fsum(np.abs(d[m, i]))
            assert abs(part[w, 0, i] - exact) <= m.size * NR.U64 * mag


def vecnormalize_loop(reward, done, gamma, eps, chunks):
    """SB3's VecNormalize return bookkeeping, one step at a time: ret = ret * gamma + reward; the batch of returns goes to
    a RunningMeanStd (update_from_moments, started empty) per chunk of steps; ret[done] = 0 afterwards"""
    T, N = reward.shape
    ret = np.zeros(N, np.float32)
    mean, var, count = 0.0, 0.0, 0
    scales, t = [], 0
    for n_steps in chunks:
        rows = []
        for _ in range(n_steps):
            for lane in range(N):
                ret[lane] = np.float32(np.float32(np.float32(gamma) * ret[lane]) + reward[t, lane])
            rows.append(ret.copy())
            ret[done[t]] = 0.0
            t += 1
        batch = np.concatenate(rows).astype(np.float64)
        b_mean, b_var, b_count = batch.mean(), batch.var(), batch.size
        if count == 0:
            mean, var, count = b_mean, b_var, b_count
        else:
            delta, tot = b_mean - mean, count + b_count
            m2 = var * count + b_var * b_count + delta * delta * count * b_count / tot
            mean, var, count = mean + delta * b_count / tot, m2 / tot, tot
        scales.append(1.0 / np.sqrt(var + eps))
    return ret, mean, var, count, scales


def test_return_walk_and_merge_follow_vecnormalize():
    rng = np.random.default_rng(3)
    T, N, gamma, eps = 9, 5, 0.97, 1e-8
    reward = rng.normal(0.5, 2.0, (T, N)).astype(np.float32)
    te = rng.random((T, N)) < 0.2
    tr = (rng.random((T, N)) < 0.15) & ~te
    te[T - 1, 0] = True  # a done at the last step zeroes ret
    want_ret, mean, var, count, scales = vecnormalize_loop(reward, te | tr, gamma, eps, (4, 5))
    ret, state, got = np.zeros(N, np.float32), None, []
    for lo, hi in ((0, 4), (4, 9)):
        rows, ret, S1, S2, A1 = NR.return_walk_ref(reward[lo:hi], te[lo:hi].astype(np.uint8), tr[lo:hi].astype(np.uint8), ret, gamma)
        state, scale = NR.return_merge_ref(S1, S2, rows.size, state, eps)
        got.append(scale)
    np.testing.assert_array_equal(ret.view(np.uint32), want_ret.view(np.uint32))
    assert ret[0] == 0.0
    # two calls over 4 + 5 steps leave the return of one call over 9
    _, ret9, _, _, _ = NR.return_walk_ref(reward, te.astype(np.uint8), tr.astype(np.uint8), np.zeros(N, np.float32), gamma)
    np.testing.assert_array_equal(ret9.view(np.uint32), ret.view(np.uint32))
    assert state[0] == count == T * N
    assert state[1] == pytest.approx(mean, rel=1e-12, abs=1e-12) and state[2] / state[0] == pytest.approx(var, rel=1e-10)
    np.testing.assert_allclose(got, scales, rtol=1e-6)


def test_normalized_reward_and_gae_restatements():
    r = np.array([[1.0, -30.0], [0.25, 7.0]], np.float32)
    rn = NR.normalized_reward_ref(r, np.float32(0.5), 10.0)
    np.testing.assert_array_equal(rn, np.array([[0.5, -10.0], [0.125, 3.5]], np.float32))
    v = np.array([[1.0, 2.0], [3.0, 4.0]], np.float32)
    z = np.zeros((2, 2), np.uint8)
    tr = np.array([[0, 0], [0, 1]], np.uint8)
    bv = np.array([[0, 0], [0, 6.0]], np.float32)
    adv, ret = NR.gae_ref(r, v, bv, np.array([5.0, 9.0], np.float32), z, tr, 0.5, 1.0)
    # lane 0: delta1 = .5 * 5 + .25 - 3 = -.25; delta0 = .5 * 3 + 1 - 1 = 1.5; A0 = 1.5 + .5 * -.25
    assert adv[1, 0] == -0.25 and adv[0, 0] == 1.375
    # lane 1: truncated at t = 1: bootstraps from boot_value 6, and the recurrence is cut
    assert adv[1, 1] == 0.5 * 6 + 7 - 4 and adv[0, 1] == (0.5 * 4 - 30 - 2) + 0.5 * adv[1, 1]
    np.testing.assert_array_equal(ret, adv + v)
