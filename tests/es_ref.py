"""Host reference of evolution strategies on the device (include/carl_amd.h: carl_es_t), written from the header and
shared by test_es_reference.py, test_gpu_es_kernels.py and test_gpu_es_population.py: the counter of a (pair, parameter,
generation), the float64 z (sampling_ref's Philox and Gaussian rule, not a copy), the perturbation and the gradient in
NumPy float32 in the header's order, and the shaping rules.  A plain module: importing it touches no device."""
import numpy as np

import sampling_ref as SR

SUB_ES = 0x40000000
_M = 0xFFFFFFFF


def counter(pair, param, generation):
    """the four counter words of parameter `param` of pair `pair`: (param >> 1, pair, generation, 0x40000000)"""
    return (np.asarray(param, np.uint64) >> np.uint64(1), np.asarray(pair, np.uint64),
            np.uint64(int(generation) & _M), np.uint64(SUB_ES))


def words(seed, pair, param, generation):
    """the Philox block (four uint32 arrays) that parameter `param` of pair `pair` draws from: key `seed`"""
    return SR.philox(*counter(pair, param, generation), int(seed) & _M, (int(seed) >> 32) & _M)


def z64(seed, generation, n_pairs, n_noisy):
    """float64 z [n_pairs, n_noisy]: even parameters use (w.x, w.y), odd ones (w.z, w.w)"""
    i, j = np.meshgrid(np.arange(n_pairs), np.arange(n_noisy), indexing="ij")
    w = words(seed, i, j, generation)
    odd = (j & 1).astype(bool)
    return SR.z_gaussian64(np.where(odd, w[2], w[0]), np.where(odd, w[3], w[1]))


def perturb_ref(center, noise, sigma):
    """params [2 * n_pairs, set_floats] float32 from center [set_floats] and noise [n_pairs, n_noisy] float32: set 2i =
    center + d, set 2i + 1 = center - d, d = sigma * z rounded to float32 on its own; the tail keeps the centre's bits"""
    center = np.asarray(center, np.float32)
    noise = np.asarray(noise, np.float32)
    n_pairs, n_noisy = noise.shape
    out = np.empty((2 * n_pairs, center.size), np.float32)
    out.view(np.uint32)[:] = center.view(np.uint32)[None, :]
    with np.errstate(all="ignore"):
        d = (np.float32(sigma) * noise).astype(np.float32)
        out[0::2, :n_noisy] = (center[None, :n_noisy] + d).astype(np.float32)
        out[1::2, :n_noisy] = (center[None, :n_noisy] - d).astype(np.float32)
    return out


def gradient_ref(weight, noise, slice_pairs):
    """grad [n_noisy] float32 = sum_i weight[i] * noise[i] in the header's order: slices of `slice_pairs` consecutive
    pairs, each summed sequentially from +0 with the product and the sum rounded separately, then the slice sums added
    sequentially from +0"""
    weight = np.asarray(weight, np.float32)
    noise = np.asarray(noise, np.float32)
    n_pairs, n_noisy = noise.shape
    total = np.zeros(n_noisy, np.float32)
    with np.errstate(all="ignore"):
        for s0 in range(0, n_pairs, slice_pairs):
            p = np.zeros(n_noisy, np.float32)
            for i in range(s0, min(s0 + slice_pairs, n_pairs)):
                p = (p + (weight[i] * noise[i]).astype(np.float32)).astype(np.float32)
            total = (total + p).astype(np.float32)
    return total


def centered_rank_weights(fitness):
    """[P] -> [P / 2]: stable ascending ranks, u = rank / (P - 1) - 0.5 in float32, weight[i] = u[2i] - u[2i + 1]"""
    f = np.asarray(fitness, np.float32)
    P = f.size
    order = np.argsort(f, kind="stable")
    rank = np.empty(P, np.int64)
    rank[order] = np.arange(P)
    u = (rank.astype(np.float32) / np.float32(P - 1)).astype(np.float32) - np.float32(0.5)
    return (u[0::2] - u[1::2]).astype(np.float32)


def difference_weights(fitness):
    f = np.asarray(fitness, np.float32)
    with np.errstate(all="ignore"):
        return (f[0::2] - f[1::2]).astype(np.float32)
