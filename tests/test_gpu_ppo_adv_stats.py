"""carl_ppo_adv_stats on the GPU (LaneEngine.ppo_adv_stats): every row of an epoch's advantage statistics against
ppo_step_ref.adv_stats_ref, whose sums are exact (math.fsum).

The bar: each output within 1 fp32 ulp of the reference.  Rounding the float64 result to fp32 alone is half an ulp.  The
device's float64 chains differ from the exact sums by at most n * 2^-53 * sum |d| (n additions, each rounded once; the
squares d * d of differences of fp32 values this close are exact), i.e. relative n * 2^-53 <= 4099 * 1.1e-16 < 5e-13 of
the sums' magnitude, and mean, var and 1 / (sqrt(var) + eps) are a handful of float64 operations on them: below 1e-9 of an
fp32 ulp (2^-24 = 6e-8 relative) at these inputs, the shifted ones included, since the shift by the first sample removes the
1e4 before anything is squared.  So 1 ulp leaves the half ulp of the final rounding and nothing else.

Outputs have canaries behind them; two calls on fresh buffers give equal bits."""
import numpy as np
import pytest
import torch

import policy_cases as PC
import ppo_step_ref as SR
from carl_amd import _lib

pytestmark = pytest.mark.gpu

CANARY = 7.25
SHAPES = [(1, 1), (2, 1), (2, 2), (255, 256), (257, 256), (1000, 300), (4099, 1024)]
N, P, T = 300, 304, 9  # the pitched storage: 300 lanes at pitch 304


@pytest.fixture(scope="module")
def eng():
    return PC.make_engine(_lib.CARTPOLE, 256, n_contexts=4)


def values(kind, n, rng):
    if kind == "normal":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "shifted":
        return (1e4 + 1e-2 * rng.standard_normal(n)).astype(np.float32)
    return np.full(n, np.float32(1e4 + 0.37))  # constant


def run(eng, advantage, idx, batch, eps=1e-8):
    """two calls, each into a fresh canaried buffer -> the rows (equal bits twice, canaries intact)"""
    rows = -(-len(idx) // batch)
    dev_idx = torch.tensor(np.asarray(idx, np.int32), device="cuda")
    got = []
    for _ in range(2):
        big = torch.full((rows + 8, 2), CANARY, dtype=torch.float32, device="cuda")
        res = eng.ppo_adv_stats(advantage, dev_idx, batch, eps, out=big[:rows])
        torch.cuda.synchronize()
        assert res.data_ptr() == big.data_ptr() and (big[rows:] == CANARY).all()
        got.append(big[:rows].cpu().numpy())
    np.testing.assert_array_equal(got[0].view(np.uint32), got[1].view(np.uint32))
    assert tuple(eng.ppo_adv_stats(advantage, dev_idx, batch, eps).shape) == (rows, 2)  # allocated when no out is given
    return got[0]


def within_one_ulp(got, want):
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)) / SR.ulp32(want)
    print(f"largest error {err.max():.3f} ulp over {got.shape[0]} rows")
    assert np.all(err <= 1.0), (got, want)


@pytest.mark.parametrize("kind", ["normal", "shifted", "constant"])
@pytest.mark.parametrize("n_total,batch", SHAPES)
def test_dense_storage(eng, n_total, batch, kind):
    rng = np.random.default_rng(n_total * 7 + batch)
    storage = values(kind, 5000, rng)
    idx = rng.permutation(5000)[:n_total]
    got = run(eng, torch.tensor(storage, device="cuda"), idx, batch)
    want = SR.adv_stats_ref(storage, idx, batch)
    within_one_ulp(got, want)
    for k, s in enumerate(range(0, n_total, batch)):
        n = min(batch, n_total - s)
        if n == 1:  # the identity, +0.0
            assert got[k].view(np.uint32).tolist() == [0, np.float32(1.0).view(np.uint32)]
        elif kind == "constant":  # the mean exact, var == 0 exactly
            assert got[k, 0] == storage[0] and got[k, 1] == np.float32(1.0 / 1e-8)


@pytest.mark.parametrize("kind", ["normal", "shifted", "constant"])
@pytest.mark.parametrize("n_total,batch", [s for s in SHAPES if s[0] <= N * T])
def test_pitched_storage_with_nan_padding(eng, n_total, batch, kind):
    rng = np.random.default_rng(n_total * 11 + batch)
    full = np.full((T, P), np.nan, np.float32)
    full[:, :N] = values(kind, T * N, rng).reshape(T, N)
    perm = rng.permutation(T * N)[:n_total]
    idx = perm // N * P + perm % N
    dev = torch.tensor(full, device="cuda")
    got = run(eng, dev[:, :N], idx, batch)
    assert np.isfinite(got).all()  # the padding is never read
    within_one_ulp(got, SR.adv_stats_ref(full.reshape(-1)[: (T - 1) * P + N], idx, batch))


@pytest.mark.parametrize("where", [0, 1, 299, 300, 999])
@pytest.mark.parametrize("bad", [-1, 5000, 2 ** 31 - 1])
def test_an_index_outside_the_storage_counts_as_zero(eng, where, bad):
    rng = np.random.default_rng(where)
    storage = values("normal", 5000, rng)
    idx = rng.permutation(5000)[:1000]
    idx[where] = bad
    got = run(eng, torch.tensor(storage, device="cuda"), idx, 300)
    assert np.isfinite(got).all()
    within_one_ulp(got, SR.adv_stats_ref(storage, idx, 300))


def test_eps_and_a_whole_buffer_in_one_row(eng):
    rng = np.random.default_rng(5)
    storage = values("normal", 4099, rng)
    idx = rng.permutation(4099)
    for eps in (0.0, 1e-3):
        within_one_ulp(run(eng, torch.tensor(storage, device="cuda"), idx, 4099, eps), SR.adv_stats_ref(storage, idx, 4099, eps))
