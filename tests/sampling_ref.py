"""Host reference of the sampled closed-loop rollout's rule (include/carl_amd.h: carl_policy_sampling_t), shared by
test_policy_sampling.py, test_gpu_policy_sampling.py and the policy toolkit: a vectorised Philox4x32-10 (checked
against oracle.philox4x32_10), the counter of a lane-step, the categorical rule as an fp32 mirror and in float64, the
Gaussian z in float64, and both log-probabilities in float64 with the bounds a device's fp32 evaluation must meet
(policy_checks.check_rule derives them)."""
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


def sample_words(seed, lane, episode_index, elapsed, lane_offset=0):
    """the lane-step's Philox block: key sample_seed, counter (glane lo, glane hi, e, 0x80000000 | elapsed), with the
    global lane glane = lane_offset + lane"""
    glane = np.uint64(lane_offset) + np.asarray(lane, np.uint64)
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


ULP = 2.0 ** -24  # half an fp32 ulp of 1: the relative error of one rounding


def categorical_tolerance(y64, bound):
    """margin below which the fp32 rule may pick another action than the float64 one: t = u S against the prefix sums
    in fp32 (relative error of exp(y - m), the sums and the product), plus the forward pass's own bound on y (twice: y_k
    and m).  Only logits within 20 of the maximum count: exp(-20) < 2^-24 / 30, so a logit further down moves no prefix
    sum by more than a fraction of the ulp terms, whatever its own error"""
    y64 = np.asarray(y64, np.float64)
    live = y64 >= y64.max(axis=1, keepdims=True) - 20
    B = np.where(live, np.asarray(bound), 0).max(axis=1)
    return 2 * B + 16 * ULP * (1 + np.where(live, np.abs(y64), 0).max(axis=1))


def categorical_log_prob64(y, a):
    """log softmax(y)[a] in float64: y_a - m - log sum_k exp(y_k - m)"""
    y = np.asarray(y, np.float64)
    m = y.max(axis=1)
    return y[np.arange(len(y)), a] - m - np.log(np.exp(y - m[:, None]).sum(axis=1))


def categorical_log_prob_bound(y64, bound, a):
    """|(y_a - m) - logf(S)| computed in fp32 from outputs y within `bound` of y64: 2 B (y_a - m) + 2 B (S: each
    exp(y_k - m) is off by at most 2 B relative, and log turns a relative error of S into an absolute one) + the
    roundings of y_a - m, of every y_k - m inside exp, of the n - 1 sums, expf, logf and the last subtraction, a few
    ulps each of |y_a - m|, 1 and |log_prob|"""
    y64 = np.asarray(y64, np.float64)
    B = np.asarray(bound).max(axis=1)
    gap = y64.max(axis=1) - y64[np.arange(len(y64)), a]
    lp = categorical_log_prob64(y64, a)
    return 4 * B + 8 * ULP * (y64.shape[1] + 2 + gap + np.abs(lp))


def gaussian_log_prob64(z, log_std):
    """-z^2 / 2 - log_std - ln(2 pi) / 2 in float64 (log_std: the fp32 value the device reads)"""
    return -np.asarray(z, np.float64) ** 2 / 2 - np.asarray(log_std, np.float64) - 0.5 * np.log(2 * np.pi)


def gaussian_z_bound(z):
    """the device's z = sqrtf(-2 logf(u1)) cospif(2 u2) against z_gaussian64: logf / sqrtf / cospif and the products,
    a few ulps each, relative to max(1, |z|)"""
    return 2e-6 * np.maximum(1.0, np.abs(z))


def gaussian_log_prob_bound(z, log_std):
    """|fma(-z/2, z, lp0) - log_prob64| with lp0 = -log_std - ln(2 pi)/2 rounded to fp32: |z| dz (dz =
    gaussian_z_bound) + the roundings of lp0, of the constant and of the fma"""
    z = np.asarray(z, np.float64)
    lp0 = np.abs(np.asarray(log_std, np.float64)) + 1.0
    return np.abs(z) * gaussian_z_bound(z) + 4 * ULP * (lp0 + np.abs(gaussian_log_prob64(z, log_std)) + 1)
