"""Host reference of PPO's running normalisation (include/carl_amd.h: carl_ppo_input_stats, carl_ppo_return_stats,
carl_ppo_return_merge), shared by test_ppo_norm_reference.py, test_gpu_ppo_input_stats.py, test_gpu_ppo_return_stats.py and
test_gpu_ppo_normalized.py.  The gather of a sample's inputs is ppo_ref.py's (brax_ppo_ref.py uses the same one), imported,
not restated.  A plain module: importing it touches no device.

The sums' bound.  The device adds float64 terms that are exact (d_i is one fp32 subtraction, the contract's own; d_i and
d_i * d_i widen to float64 exactly) in chains of at most n additions, n the number of samples, so with u = 2^-53
    |S - exact| <= n * u * sum |terms|
to first order (recursive summation; the second-order term is below n^2 u^2 / 2, nothing at these sizes).  ``exact`` here
is math.fsum of the same terms: correctly rounded."""
import math

import numpy as np

import brax_ppo_ref as BR  # noqa: F401  (its gather is ppo_ref's: R.sample_inputs takes a BraxMLPPolicy as it is)
import ppo_ref as R

U64 = 2.0 ** -53
MAX_IN = 32


# ---------------------------------------------------------------- the input sums
def gathered_inputs(actor, ctx_table_fc, context_id, obs0, obs, n_lanes, pitch):
    """raw inputs x [T * n_lanes, n_in] float32 of EVERY sample (t, lane), t-major, as carl_ppo_grad's gather forms them:
    arrays [T, pitch(, D)] (obs with at least one row); row T - 1 of obs is not read"""
    T = context_id.shape[0]
    flat = (np.arange(T)[:, None] * pitch + np.arange(n_lanes)[None, :]).reshape(-1)
    cid = np.clip(context_id, 0, ctx_table_fc.shape[1] - 1)
    return R.sample_inputs(actor, ctx_table_fc, cid, obs0, obs, flat, pitch)


def input_sums_ref(x, shift):
    """-> (S1, S2, A1, A2) float64 [n_in]: the exact (correctly rounded) sums of d = fp32(x - shift) and of d * d over the
    samples x [n, n_in] float32, and the sums of their magnitudes (the bound's right-hand side)"""
    d = (x.astype(np.float32) - np.asarray(shift, np.float32)[None, :]).astype(np.float32).astype(np.float64)
    n_in = d.shape[1]
    S1 = np.array([math.fsum(d[:, i]) for i in range(n_in)])
    S2 = np.array([math.fsum(d[:, i] * d[:, i]) for i in range(n_in)])  # (the float64 product of two floats is exact)
    A1 = np.array([math.fsum(np.abs(d[:, i])) for i in range(n_in)])
    return S1, S2, A1, S2.copy()


def sums_bound(n, A):
    return n * U64 * np.asarray(A, np.float64)


THREADS, MAX_WORKGROUPS = 256, 256  # ppo_device.hip.h: kPpoThreads, kPpoMaxWorkgroups


def input_plan(n, n_in):
    """ppo_input_stats_kernel's launch shape for n samples of n_in inputs, and which sample each thread chains when ->
    (G slabs, spt samples per pass, n_pass, passes [G]: the passes workgroup w runs, idx [G, max(passes), spt] int64: the
    sample that thread (so, any i) of workgroup w takes in its r-th pass, p = w + r * G, or -1 where p >= n_pass or the
    sample p * spt + so is past the end)"""
    G = min(-(-n // THREADS), MAX_WORKGROUPS)
    spt = THREADS // n_in
    n_pass = -(-n // spt)
    w = np.arange(G, dtype=np.int64)
    passes = (n_pass - w + G - 1) // G  # (G <= ceil(n / 256) <= n_pass: every workgroup has at least one)
    p = w[:, None] + G * np.arange(passes.max(), dtype=np.int64)[None, :]
    m = p[:, :, None] * spt + np.arange(spt, dtype=np.int64)[None, None, :]
    return G, spt, n_pass, passes, np.where((p[:, :, None] < n_pass) & (m < n), m, -1)


def input_slabs_ref(x, shift):
    """the slabs [G][2][32] float64 of carl_ppo_input_stats over the samples x [n, n_in] float32 (t-major), every addition
    in the kernel's order: thread (so, i) of workgroup w chains d = fp32(x - shift) widened, s1 += d, s2 += d * d, over
    its passes in pass order (samples past the end are skipped); slot i is then the sum over so = 0 .. spt - 1 in that
    order from +0.0; entries at and beyond n_in are +0.0.  Every term is an exact float64, so the order decides each bit."""
    n, n_in = x.shape
    d = (x.astype(np.float32) - np.asarray(shift, np.float32)[None, :]).astype(np.float32).astype(np.float64)
    terms = np.stack([d, d * d])  # [2, n, n_in]  (the float64 product of two floats is exact)
    G, spt, _, _, idx = input_plan(n, n_in)
    acc = np.zeros((2, G, spt, n_in))
    for r in range(idx.shape[1]):
        live = idx[:, r, :] >= 0
        np.add(acc, terms[:, np.where(live, idx[:, r, :], 0)], out=acc, where=live[None, :, :, None])
    part = np.zeros((G, 2, MAX_IN))
    for so in range(spt):
        part[:, :, :n_in] += acc[:, :, so, :].transpose(1, 0, 2)
    return part


def merge_ref(S1, S2, n_b, shift, state=None, eps=1e-8, min_std=1e-6):
    """carl_policy_stats_merge's rule in float64 for sums S1, S2 [n_in] over n_b samples centred on shift ->
    (state' = (count, mean, m2), shift' float32, scale' float32)"""
    mean_b = np.asarray(shift, np.float32).astype(np.float64) + S1 / n_b
    m2_b = np.maximum(S2 - S1 * S1 / n_b, 0.0)
    if state is None or state[0] == 0:
        count, mean, m2 = n_b, mean_b, m2_b
    else:
        c0, mean0, m20 = state
        count = c0 + n_b
        delta = mean_b - mean0
        mean = mean0 + delta * (n_b / count)
        m2 = (m20 + m2_b) + delta * delta * (c0 * n_b / count)
    var = m2 / count
    floor = np.maximum(min_std * min_std, (2.0 ** -18 * np.abs(mean)) ** 2)
    with np.errstate(divide="ignore"):
        scale = np.where(var <= floor, 0.0, 1.0 / np.sqrt(var + eps))
    return (count, mean, m2), mean.astype(np.float32), scale.astype(np.float32)


def settled32(v64, r32):
    """whether the float64 values v64 are further than 4e-12 relative from the boundary at which their fp32 rounding r32
    would change (test_gpu_policy_stats_merge.py's rule: bit for bit where settled)"""
    r32 = np.asarray(r32, np.float32)
    margin = 0.5 * np.spacing(np.abs(r32)).astype(np.float64) - np.abs(v64 - r32.astype(np.float64))
    return margin > 4e-12 * np.abs(v64)


def slabs_in_order(part, n_in):
    """(S1, S2) [n_in] of device slabs [slab][2][32], added in slab order as the merge adds them"""
    s = np.zeros((2, n_in))
    for w in range(part.shape[0]):
        s = s + part[w, :, :n_in]
    return s[0], s[1]


def check_merged_transform(label, got_shift, got_scale, state, sh, sc, eps, min_std):
    """the device's fp32 shift / scale against merge_ref's of the device's own slabs: bit for bit where the reference's
    float64 value is settled (and the variance is off the constant rule's floor), within one ulp elsewhere"""
    var = state[2] / state[0]
    floor = np.maximum(min_std ** 2, (2.0 ** -18 * np.abs(state[1])) ** 2)
    with np.errstate(divide="ignore"):
        s64 = np.where(sc == 0, 0.0, 1.0 / np.sqrt(var + eps))
    off_floor = np.abs(var - floor) > 4e-12 * floor
    every = np.ones(len(sh), bool)
    for name, got, want, v64, ok in (("shift", got_shift, sh, state[1], every), ("scale", got_scale, sc, s64, off_floor)):
        sure = ok & settled32(v64, want)
        print(f"{label}: {name} bit for bit on {int(sure.sum())} of {len(sh)} inputs")
        np.testing.assert_array_equal(got[sure].view(np.uint32), want[sure].view(np.uint32))
        np.testing.assert_allclose(got[ok], want[ok], rtol=2.0 ** -23, atol=0)


# ---------------------------------------------------------------- the return walk and its merge
def return_walk_ref(reward, terminated, truncated, ret0, gamma):
    """carl_ppo_return_stats in NumPy float32: reward / flags [T, N], ret0 [N] -> (ret_rows [T, N] float32, ret [N] float32
    after the walk, S1, S2 exact float64 sums of the rows and of their squares, A1 = sum |rows|)"""
    f32 = np.float32
    T, N = reward.shape
    ret = np.asarray(ret0, f32).copy()
    rows = np.empty((T, N), f32)
    g = f32(gamma)
    for t in range(T):
        ret = (g * ret).astype(f32) + reward[t].astype(f32)   # two roundings: the product, then the sum
        ret = ret.astype(f32)
        rows[t] = ret
        done = (terminated[t] != 0) | (truncated[t] != 0)
        ret = np.where(done, f32(0), ret)
    r64 = rows.astype(np.float64).reshape(-1)
    return rows, ret, math.fsum(r64), math.fsum(r64 * r64), math.fsum(np.abs(r64))


def return_merge_ref(S1, S2, n_b, state=None, eps=1e-8):
    """carl_ppo_return_merge's rule in float64 -> (state' = (count, mean, m2), scale float32)"""
    S1, S2, n = np.float64(S1), np.float64(S2), np.float64(n_b)
    mean_b = S1 / n
    m2_b = max(S2 - S1 * S1 / n, 0.0)
    if state is None or state[0] == 0:
        count, mean, m2 = int(n_b), mean_b, m2_b
    else:
        c0, mean0, m20 = state
        count = int(c0 + n_b)
        nn = np.float64(count)
        delta = mean_b - mean0
        mean = mean0 + delta * (n / nn)
        m2 = (m20 + m2_b) + delta * delta * (np.float64(c0) * n / nn)
    scale = np.float32(1.0 / np.sqrt(m2 / np.float64(count) + eps))
    return (count, np.float64(mean), np.float64(m2)), scale


def normalized_reward_ref(reward, scale, clip):
    """clamp(fp32(reward * scale), -clip, clip) in float32, as PPO.collect forms it"""
    return np.clip((reward.astype(np.float32) * np.float32(scale)).astype(np.float32), np.float32(-clip), np.float32(clip))


def gae_ref(reward, value, boot_value, last_value, terminated, truncated, gamma, lam):
    """carl_gae's rule in float64 from the float32 columns [T, N] -> (advantage, return) float64"""
    T, N = reward.shape
    r, v, bv = (a.astype(np.float64) for a in (reward, value, boot_value))
    adv = np.zeros((T, N))
    A = np.zeros(N)
    for t in range(T - 1, -1, -1):
        te, tr = terminated[t] != 0, truncated[t] != 0
        done = te | tr
        nxt = last_value.astype(np.float64) if t == T - 1 else v[t + 1]
        vn = np.where(done, np.where(tr & ~te, bv[t], 0.0), nxt)
        delta = gamma * vn + r[t] - v[t]
        A = delta + gamma * lam * np.where(done, 0.0, A)
        adv[t] = A
    return adv, adv + v
