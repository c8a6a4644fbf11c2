"""carl_ppo_return_stats and carl_ppo_return_merge on the GPU, through ``ppo_return_stats`` / ``ppo_return_merge``: the
persistent return and the per-step values bit for bit against the float32 restatement (ppo_norm_ref.return_walk_ref), the
slab sums at the derived float64 bound (n * 2^-53 * sum |terms|), a walk split into two calls, a done at the last step,
T = 1, lane counts around the wavefront and the workgroup, pitched and dense rows; each slab against the exact sums of its
own 256 lanes at the same bound over that slab's samples (513 lanes x 17 steps: three slabs, the last of one lane, two full
rounds of the 8-row load window and one row more); the merge against the same operations
in NumPy float64 (rtol 1e-12 for mean and M2, as test_gpu_policy_stats_merge.py holds carl_policy_stats_merge) over three
successive merges."""
import math

import numpy as np
import pytest
import torch

import policy_cases as PC
import ppo_norm_ref as NR
from carl_amd import _lib

pytestmark = pytest.mark.gpu

GAMMA = 0.97


@pytest.fixture(scope="module")
def engines():
    return {n: PC.make_engine(_lib.CARTPOLE, n, n_contexts=4) for n in (1, 63, 65, 257, 513)}


def columns(N, T, seed, pitched):
    """reward / terminated / truncated [T, N] on the device (rows of pitch 16-aligned or dense) and on the host"""
    rng = np.random.default_rng(seed)
    reward = rng.normal(0.3, 2.0, (T, N)).astype(np.float32)
    te = (rng.random((T, N)) < 0.2).astype(np.uint8)
    tr = ((rng.random((T, N)) < 0.15) & (te == 0)).astype(np.uint8)
    te[T - 1, 0] = 1  # a done at the last step
    P = (N + 15) // 16 * 16 if pitched else N

    def dev(a):
        t = torch.full((T, P), 77, dtype=torch.as_tensor(a).dtype, device="cuda")[:, :N]
        t.copy_(torch.as_tensor(a))
        return t

    return (reward, te, tr), (dev(reward), dev(te), dev(tr))


@pytest.mark.parametrize("N,T,pitched", [(1, 1, False), (63, 9, True), (65, 9, False), (257, 9, True), (257, 1, True),
                                         (63, 2, False), (513, 17, True)])
def test_return_walk_bits_and_sums(engines, N, T, pitched):
    eng = engines[N]
    (reward, te, tr), (d_reward, d_te, d_tr) = columns(N, T, 100 + N + T, pitched)
    ret0 = np.random.default_rng(N).normal(0, 3.0, N).astype(np.float32)
    ret = torch.as_tensor(ret0).cuda()
    res = eng.ppo_return_stats(d_reward, d_te, d_tr, ret, GAMMA, ret_rows=True)
    rows, ret_ref, S1, S2, A1 = NR.return_walk_ref(reward, te, tr, ret0, GAMMA)
    np.testing.assert_array_equal(res["ret_rows"].cpu().numpy().view(np.uint32), rows.view(np.uint32))
    np.testing.assert_array_equal(ret.cpu().numpy().view(np.uint32), ret_ref.view(np.uint32))
    assert ret_ref[0] == 0.0 and ret.cpu()[0] == 0.0
    part = res["return_partial"].cpu().numpy()
    assert part.shape == (_lib.load().carl_ppo_return_stats_slabs(N), 2) == ((N + 255) // 256, 2)
    n = T * N
    for q, (S, A) in enumerate(((S1, A1), (S2, S2))):
        got = math.fsum(part[:, q])
        print(f"n={N} T={T} S{q + 1}: |err| {abs(got - S):.3e}, bound {n * NR.U64 * A:.3e}")
        assert abs(got - S) <= n * NR.U64 * A
    # slab by slab: workgroup w adds the returns of lanes [256 w, 256 w + 256) in a fixed tree -- any order of n_w terms
    # stays within n_w * 2^-53 * sum |terms| of their exact sum
    r64 = rows.astype(np.float64)
    for w in range(part.shape[0]):
        mine = r64[:, 256 * w: 256 * w + 256].reshape(-1)
        n_w = mine.size
        assert n_w == T * min(256, N - 256 * w)
        for q, terms in enumerate((mine, mine * mine)):  # (the float64 product of two floats is exact)
            err, bound = abs(part[w, q] - math.fsum(terms)), n_w * NR.U64 * math.fsum(np.abs(terms))
            print(f"n={N} T={T} slab {w} S{q + 1}: |err| {err:.3e}, bound {bound:.3e} (n_w = {n_w})")
            assert err <= bound
    # the same call from the same state: the same bits (and no per-step rows asked for)
    ret_b = torch.as_tensor(ret0).cuda()
    again = eng.ppo_return_stats(d_reward, d_te, d_tr, ret_b, GAMMA)
    assert "ret_rows" not in again
    np.testing.assert_array_equal(again["return_partial"].cpu().numpy().view(np.uint64), part.view(np.uint64))
    np.testing.assert_array_equal(ret_b.cpu().numpy().view(np.uint32), ret_ref.view(np.uint32))


@pytest.mark.parametrize("N", [63, 257])
def test_two_calls_continue_one_walk(engines, N):
    eng = engines[N]
    (reward, te, tr), (d_reward, d_te, d_tr) = columns(N, 9, 7, True)
    whole = torch.zeros(N, device="cuda")
    full = eng.ppo_return_stats(d_reward, d_te, d_tr, whole, GAMMA, ret_rows=True)
    split = torch.zeros(N, device="cuda")
    a = eng.ppo_return_stats(d_reward[:4], d_te[:4], d_tr[:4], split, GAMMA, ret_rows=True)
    b = eng.ppo_return_stats(d_reward[4:], d_te[4:], d_tr[4:], split, GAMMA, ret_rows=True)
    np.testing.assert_array_equal(split.cpu().numpy().view(np.uint32), whole.cpu().numpy().view(np.uint32))
    rows = torch.cat([a["ret_rows"], b["ret_rows"]]).cpu().numpy()
    np.testing.assert_array_equal(rows.view(np.uint32), full["ret_rows"].cpu().numpy().view(np.uint32))
    _, ret_ref, _, _, _ = NR.return_walk_ref(reward, te, tr, np.zeros(N, np.float32), GAMMA)
    np.testing.assert_array_equal(whole.cpu().numpy().view(np.uint32), ret_ref.view(np.uint32))


def test_return_merge_against_the_same_operations(engines):
    eng = engines[257]
    run = {"count": torch.zeros(1, dtype=torch.int64, device="cuda"), "mean": torch.zeros(1, dtype=torch.float64, device="cuda"),
           "m2": torch.zeros(1, dtype=torch.float64, device="cuda")}
    scale = torch.full((1,), 5.0, device="cuda")
    ret = torch.zeros(257, device="cuda")
    state = None
    for k, T in enumerate((9, 1, 4)):
        _, (d_reward, d_te, d_tr) = columns(257, T, 40 + k, k % 2 == 0)
        part = eng.ppo_return_stats(d_reward, d_te, d_tr, ret, GAMMA)["return_partial"]
        out = eng.ppo_return_merge(part, T * 257, run, 1e-8, scale)
        assert out is scale
        p = part.cpu().numpy()
        S1 = S2 = 0.0
        for w in range(p.shape[0]):  # the slabs in order
            S1, S2 = S1 + p[w, 0], S2 + p[w, 1]
        state, want = NR.return_merge_ref(S1, S2, T * 257, state, 1e-8)
        assert int(run["count"].cpu()) == state[0]
        np.testing.assert_allclose(run["mean"].cpu().numpy()[0], state[1], rtol=1e-12, atol=0)
        np.testing.assert_allclose(run["m2"].cpu().numpy()[0], state[2], rtol=1e-12, atol=0)
        np.testing.assert_allclose(scale.cpu().numpy()[0], want, rtol=2.0 ** -22, atol=0)
    assert state[0] == 14 * 257
    # n_b == 0: nothing is enqueued, nothing moves
    before = scale.clone()
    eng.ppo_return_merge(part, 0, run, 1e-8, scale)
    assert int(run["count"].cpu()) == state[0] and torch.equal(scale, before)
