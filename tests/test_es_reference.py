"""Evolution strategies, host side: the reference of the noise rule (es_ref.py) against oracle.philox4x32_10, and its
shaping and summation rules against their definitions.  CPU-only: nothing here loads a device."""
import numpy as np
import torch

import es_ref as ER
import sampling_ref as SR
from oracle import oracle as O


def test_counter_words_match_the_oracle():
    """(j >> 1, i, generation, 0x40000000) under key seed: j = 0 and 1 share a block and take different halves, j = 2
    takes the next block; pair, generation and the seed's high word each reach the block"""
    cases = [(0, 0, 0, 0), (0, 1, 0, 0), (0, 2, 0, 0), (5, 3, 0, 1), (0, 0, 7, 1), (9, 4417, 2**32 - 1, 0xDEADBEEF),
             (3, 11, 2, 0x123456789ABCDEF0), (70000, 6401, 12, 0xFFFFFFFF00000001)]
    for i, j, gen, seed in cases:
        got = ER.words(seed, np.array([i]), np.array([j]), gen)
        want = O.philox4x32_10([j >> 1, i, gen, 0x40000000], [seed & 0xFFFFFFFF, seed >> 32])
        np.testing.assert_array_equal(np.array([int(v[0]) for v in got], np.uint32), want)
    seed = 0x123456789ABCDEF0
    w0, w1, w2 = (ER.words(seed, np.array([2]), np.array([j]), 5) for j in (0, 1, 2))
    assert all(int(a[0]) == int(b[0]) for a, b in zip(w0, w1))
    assert any(int(a[0]) != int(b[0]) for a, b in zip(w0, w2))
    z = ER.z64(seed, 5, 3, 3)
    assert z[2, 0] == SR.z_gaussian64(w0[0], w0[1])[0] and z[2, 1] == SR.z_gaussian64(w1[2], w1[3])[0]
    assert z[2, 2] == SR.z_gaussian64(w2[0], w2[1])[0]
    assert ER.z64(seed ^ (1 << 40), 5, 3, 3)[2, 0] != z[2, 0]  # (the high word is part of the key)
    assert ER.z64(seed, 6, 3, 3)[2, 0] != z[2, 0] and z[1, 0] != z[2, 0]
    big = ER.z64(1, 0, 64, 512)
    assert np.abs(big).max() <= 5.8 and abs(big.mean()) < 0.02 and abs(big.std() - 1) < 0.02


def test_centered_ranks():
    f = np.array([3.0, 1.0, 2.0, 1.0, 5.0, 2.0], np.float32)  # ties: the earlier index ranks lower (a stable order)
    u = np.array([4, 0, 2, 1, 5, 3], np.float32) / np.float32(5) - np.float32(0.5)
    np.testing.assert_array_equal(ER.centered_rank_weights(f), u[0::2] - u[1::2])
    np.testing.assert_array_equal(ER.centered_rank_weights(np.array([1.0, 2.0])), np.array([-1.0], np.float32))
    np.testing.assert_array_equal(ER.centered_rank_weights(np.array([2.0, 2.0])), np.array([-1.0], np.float32))
    g = np.array([0.5, -np.inf, -np.inf, 0.25], np.float32)  # a set without a finished episode ranks lowest
    u = np.array([3, 0, 1, 2], np.float32) / np.float32(3) - np.float32(0.5)
    np.testing.assert_array_equal(ER.centered_rank_weights(g), u[0::2] - u[1::2])
    np.testing.assert_array_equal(ER.difference_weights(f), np.array([2.0, 1.0, 3.0], np.float32))


def test_driver_shaping_is_the_reference_rule():
    """carl_amd.es's torch rules on the CPU against es_ref's NumPy rules: same bits (ties, P = 2, -inf)"""
    from carl_amd import es as ES

    rng = np.random.default_rng(0)
    cases = [np.array([3.0, 1.0, 2.0, 1.0, 5.0, 2.0], np.float32), np.array([1.0, 2.0], np.float32),
             np.array([0.5, -np.inf, -np.inf, 0.25], np.float32), rng.normal(size=256).astype(np.float32),
             rng.integers(0, 5, 64).astype(np.float32)]
    for f in cases:
        got = ES.centered_rank_weights(torch.from_numpy(f)).numpy()
        np.testing.assert_array_equal(got.view(np.uint32), ER.centered_rank_weights(f).view(np.uint32))
        got = ES.difference_weights(torch.from_numpy(f)).numpy()
        np.testing.assert_array_equal(got.view(np.uint32), ER.difference_weights(f).view(np.uint32))


def test_set_fitness_rule():
    """mean over a set's lanes of each lane's mean finished-episode return; a lane without one is left out, a set
    without any gets -inf; slots at or beyond a lane's episode count (NaN) are never read into the result"""
    from carl_amd import es as ES

    nan = float("nan")
    ret = torch.tensor([[1.0, 2.0, nan, 7.0, nan, nan], [3.0, nan, nan, nan, nan, nan]])
    ep = torch.tensor([2, 1, 0, 1, 0, 0], dtype=torch.int32)
    got = ES.set_fitness({"return": ret, "episodes": ep}, 3)
    assert got.tolist() == [2.0, 7.0, float("-inf")] and got.dtype == torch.float32


def test_gradient_ref_order():
    rng = np.random.default_rng(1)
    w = rng.normal(size=11).astype(np.float32)
    z = rng.normal(size=(11, 7)).astype(np.float32)
    plain = np.zeros(7, np.float32)
    for i in range(11):
        plain = plain + w[i] * z[i]
    np.testing.assert_array_equal(ER.gradient_ref(w, z, 11), plain)  # one slice: the plain sequential sum
    np.testing.assert_array_equal(ER.gradient_ref(w, z, 64), plain)
    a = np.zeros(7, np.float32)
    for lo, hi in ((0, 4), (4, 8), (8, 11)):  # a ragged last slice
        p = np.zeros(7, np.float32)
        for i in range(lo, hi):
            p = p + w[i] * z[i]
        a = a + p
    got = ER.gradient_ref(w, z, 4)
    np.testing.assert_array_equal(got, a)
    assert got.dtype == np.float32 and not np.array_equal(got, plain)  # (the order is part of the result)
    np.testing.assert_allclose(got, (w[:, None].astype(np.float64) * z).sum(0), rtol=0, atol=1e-5)


def test_perturb_ref_mirrors_and_keeps_the_tail():
    rng = np.random.default_rng(2)
    c = rng.normal(size=12).astype(np.float32)
    c[9], c[10] = np.inf, np.float32(np.nan)
    z = rng.normal(size=(3, 7)).astype(np.float32)
    out = ER.perturb_ref(c, z, 0.1)
    assert out.shape == (6, 12) and out.dtype == np.float32
    d = np.float32(0.1) * z
    np.testing.assert_array_equal(out[0::2, :7], c[:7] + d)
    np.testing.assert_array_equal(out[1::2, :7], c[:7] - d)
    np.testing.assert_array_equal(out[:, 7:].view(np.uint32), np.tile(c[7:].view(np.uint32), (6, 1)))
