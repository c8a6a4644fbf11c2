"""Host reference of the sampled closed-loop rollout's rule (include/carl_amd.h: carl_policy_sampling_t), shared by
test_policy_sampling.py and test_gpu_policy_sampling.py: a vectorised Philox4x32-10 (checked against
oracle.philox4x32_10), the counter of a lane-step, the categorical rule as an fp32 mirror and in float64, and the
Gaussian z in float64."""
import numpy as np

_M = 0xFFFFFFFF
SUB_SAMPLE = 0x80000000


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over arrays of counters (uint32 values), keys broadcast -> four uint32 arrays"""
    c = [np.asarray(v, np.uint64) & _M for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0 & _M), np.uint64(k1 & _M)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & np.uint64(_M), (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & np.uint64(_M)]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & np.uint64(_M), (k1 + np.uint64(0xBB67AE85)) & np.uint64(_M)
    return [v.astype(np.uint32) for v in c]


def sample_words(seed, glane, episode_index, elapsed):
    """the lane-step's Philox block: key sample_seed, counter (glane lo, glane hi, e, 0x80000000 | elapsed)"""
    glane = np.asarray(glane, np.uint64)
    return philox(glane & np.uint64(_M), glane >> np.uint64(32), np.asarray(episode_index, np.uint64) & np.uint64(_M),
                  np.uint64(SUB_SAMPLE) | np.asarray(elapsed, np.uint64), seed & _M, (seed >> 32) & _M)


def u_categorical(wx):
    return (np.asarray(wx, np.uint32) >> 8).astype(np.float32) * np.float32(2.0 ** -24)


def z_gaussian64(wx, wy):
    """float64 z of the Box rule"""
    u1 = ((np.asarray(wx, np.uint32) >> 8).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (np.asarray(wy, np.uint32) >> 8).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def categorical_equal_logits(u, n_actions):
    """the fp32 rule for equal logits: e_k = 1, S = n, c_k = k + 1 (all exact), t = u * S rounded once"""
    t = np.asarray(u, np.float32) * np.float32(n_actions)
    a = np.full(t.shape, n_actions - 1, np.int32)
    for k in range(n_actions - 2, -1, -1):
        a = np.where(t < np.float32(k + 1), k, a)
    return a


def categorical64(y, u):
    """float64 rule on logits y [N, n]: (action, margin) with margin = min_k |u S - c_k| / S, the distance of t from the
    nearest prefix-sum boundary relative to S"""
    y = np.asarray(y, np.float64)
    e = np.exp(y - y.max(axis=1, keepdims=True))
    c = np.cumsum(e, axis=1)
    S = c[:, -1:]
    t = np.asarray(u, np.float64)[:, None] * S
    a = np.where((t < c).any(axis=1), np.argmax(t < c, axis=1), y.shape[1] - 1)
    margin = np.abs(t - c)[:, :-1].min(axis=1) / S[:, 0] if y.shape[1] > 1 else np.full(len(y), np.inf)
    return a.astype(np.int32), margin
