"""Host reference of the input statistics (include/carl_amd.h: carl_evaluate_policy_stats, carl_policy_stats_merge), in
float64 NumPy: the sums a launch gathers, the merge with its constant rule, and the offsets of the transform section;
and the merge of integer data in exact rational arithmetic with the error bound the header's operation list implies.
A plain module: importing it touches no device."""
from fractions import Fraction

import numpy as np

MAX_IN = 32
REL_FLOOR = 2.0 ** -18  # the header's relative term of the constant rule


def input_sums(x, steps, shift):
    """x [T, n, n_in]: every lane-step's raw fp32 inputs; steps [n]: the live steps of each lane (its first ones);
    shift [n_in] or [n, n_in] fp32 (each lane's weight set's).  d = fp32(x - shift) of the live lane-steps, then in
    float64: (sum d, sum d^2, sum |d|) [n_in] each -- the last two are the scales of the device sums' error bound."""
    x = np.asarray(x, np.float32)
    T, n, n_in = x.shape
    d = (x - np.broadcast_to(np.asarray(shift, np.float32), (n, n_in))[None]).astype(np.float32).astype(np.float64)
    live = np.arange(T)[:, None] < np.asarray(steps)[None, :]
    d = np.where(live[:, :, None], d, 0.0)
    d = np.ascontiguousarray(d.reshape(T * n, n_in).T)  # [n_in, T n]: NumPy sums a contiguous row pairwise
    return d.sum(axis=1), (d * d).sum(axis=1), np.abs(d).sum(axis=1)


def fresh(n_in):
    return {"count": 0, "mean": np.zeros(n_in), "m2": np.zeros(n_in)}


def merge(state, partial, n_b, shift, eps=1e-8, min_std=1e-6):
    """carl_policy_stats_merge in the header's order.  state: {"count", "mean" [n_in], "m2" [n_in]}; partial
    [n_workgroups, 2, >= n_in] float64; n_b: the launch's lane-steps; shift [n_in]: the fp32 shift the launch ran under.
    Returns (the new state, shift32, scale32), or (state, None, None) unchanged when n_b == 0."""
    n_in = state["mean"].size
    if n_b == 0:
        return state, None, None
    partial = np.asarray(partial, np.float64)
    s1, s2 = np.zeros(n_in), np.zeros(n_in)
    for w in range(partial.shape[0]):  # workgroup order
        s1 = s1 + partial[w, 0, :n_in]
        s2 = s2 + partial[w, 1, :n_in]
    nb = float(n_b)
    mean_b = np.asarray(shift, np.float32).astype(np.float64) + s1 / nb
    m2_b = np.maximum(s2 - s1 * s1 / nb, 0.0)
    n_a = int(state["count"])
    n = n_a + int(n_b)
    if n_a == 0:
        mean, m2 = mean_b, m2_b
    else:
        delta = mean_b - state["mean"]
        mean = state["mean"] + delta * (nb / float(n))
        m2 = (state["m2"] + m2_b) + delta * delta * (float(n_a) * nb / float(n))
    new = {"count": n, "mean": mean, "m2": m2}
    return new, *transform(new, eps, min_std)


def transform(state, eps=1e-8, min_std=1e-6):
    """(shift32, scale32) of a state: scale = 0 where var <= max(min_std^2, (2^-18 |mean|)^2), else 1 / sqrt(var + eps)"""
    var = state["m2"] / float(state["count"])
    floor = np.maximum(min_std * min_std, (REL_FLOOR * np.abs(state["mean"])) ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(var <= floor, 0.0, 1.0 / np.sqrt(var + eps))
    return state["mean"].astype(np.float32), scale.astype(np.float32)


def settled(state, eps, min_std, rtol):
    """True where a merge that is within `rtol` of `state`'s float64 mean and M2 must write the same fp32 shift and
    scale as transform(state): every float64 within rtol of the mean rounds to one fp32, the variance is not within
    4 rtol of the floor (the floor moves by 2 rtol with the mean), and the scale -- which moves by half the variance's
    relative change -- rounds to one fp32 over +-rtol.  [n_in] bool."""
    mean, var = state["mean"], state["m2"] / float(state["count"])
    floor = np.maximum(min_std * min_std, (REL_FLOOR * np.abs(mean)) ** 2)
    ok = (mean * (1 - rtol)).astype(np.float32) == (mean * (1 + rtol)).astype(np.float32)
    ok &= np.abs(var - floor) > 4 * rtol * np.maximum(var, floor)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        scale = np.where(var <= floor, 0.0, 1.0 / np.sqrt(var + eps))
        ok &= (scale * (1 - rtol)).astype(np.float32) == (scale * (1 + rtol)).astype(np.float32)
    return ok


# ---------------------------------------------------------------- the merge in exact arithmetic, and its error bound
# test_gpu_policy_stats_merge.py's docstring derives the bound; exact_merge carries it beside the exact statistics.
U64 = Fraction(1, 2 ** 53) * (1 + Fraction(1, 2 ** 20))  # one float64 rounding; the factor covers the higher orders
MIN_SHARE = Fraction(1, 2 ** 20)  # (what that factor assumes: neither side of a Chan update is a smaller share than this)


def exact_fresh(n_in):
    zero = [Fraction(0)] * n_in
    return {"count": 0, "mean": list(zero), "m2": list(zero), "e_mean": list(zero), "e_m2": list(zero)}


def exact_merge(ex, partial, n_b, shift):
    """carl_policy_stats_merge of integer-valued slabs under an integer shift in exact rational arithmetic -> the new
    {"count", "mean", "m2"} (Fractions: the pooled mean and sum of squared deviations of everything merged so far) with
    "e_mean" / "e_m2", the bounds on |float64 result - exact| of an implementation that follows the header's operation
    list, given that its running state was within ex's bounds.  The slab entries must be integers whose absolute sum
    stays below 2^53: every partial sum of the workgroup-order loop is then exact."""
    n_in, n_a = len(ex["mean"]), ex["count"]
    partial = np.asarray(partial, np.float64)[:, :, :n_in]
    assert n_b > 0 and np.all(partial == np.rint(partial)) and np.abs(partial).sum(axis=0).max() < 2.0 ** 53
    n = n_a + n_b
    assert n_a == 0 or min(n_a, n_b) >= MIN_SHARE * n
    u = U64
    new = {"count": n, "mean": [], "m2": [], "e_mean": [], "e_m2": []}
    for i in range(n_in):
        s1, s2 = (sum(int(v) for v in partial[:, k, i]) for k in (0, 1))
        s = Fraction(float(np.float32(shift[i])))
        mu_b, m_b = s + Fraction(s1, n_b), s2 - Fraction(s1 * s1, n_b)
        assert m_b >= 0
        e_b = u * (Fraction(abs(s1), n_b) + abs(mu_b))       # S1 / n_b, then shift + .
        g_b = u * (2 * Fraction(s1 * s1, n_b) + m_b)         # S1 * S1, / n_b, then S2 - . (the clamp only helps)
        if n_a == 0:
            mu, m, e_mu, e_m = mu_b, m_b, e_b, g_b
        else:
            mu_a, m_a, e_a, f_a = ex["mean"][i], ex["m2"][i], ex["e_mean"][i], ex["e_m2"][i]
            delta, f = mu_b - mu_a, Fraction(n_a * n_b, n)
            t = delta * delta * f
            mu, m = mu_a + delta * Fraction(n_b, n), m_a + m_b + t
            e_mu = Fraction(n_a, n) * e_a + Fraction(n_b, n) * (e_b + 3 * u * abs(delta)) + u * abs(mu)
            e_d = e_b + e_a + u * abs(delta)
            e_m = f_a + g_b + u * (2 * (m_a + m_b) + 5 * t) + f * e_d * (2 * abs(delta) + e_d)
        for k, v in zip(("mean", "m2", "e_mean", "e_m2"), (mu, m, e_mu, e_m)):
            new[k].append(v)
    return new


def exact_ratio(ex, mean, m2):
    """the largest |got - exact| / bound over the inputs, of a float64 mean / M2 against exact_merge's state: (mean's,
    M2's); a zero bound admits a zero error only (ratio 0, else inf)"""
    def ratio(got, want, bound):
        worst = 0.0
        for g, w, b in zip(got, want, bound):
            err = abs(Fraction(float(g)) - w)
            worst = max(worst, float(err / b) if b > 0 else (0.0 if err == 0 else float("inf")))
        return worst
    return ratio(mean, ex["mean"], ex["e_mean"]), ratio(m2, ex["m2"], ex["e_m2"])


EXACT_SLABS, EXACT_LANES, EXACT_N_IN = (1, 2, 257), (1, 255, 257, 1000), (1, 12, 32)


def exact_cases(n_cases=120, seed=2024):
    """n_cases runs of one to three successive merges of integer data: [(n_in, [(partial [W][2][MAX_IN], steps [n_lanes]
    int32, shift [n_in] float32), ...], (count, sum x, sum x^2) as Python integers)].  Each input has a location of
    its own up to +-4000 and a spread from 0 (constant) to 60; a launch's shift is 0 (nothing centred: S2 cancels
    against S1^2 / n_b), the location, or the rounded mean of what came before.  Slab columns at and beyond n_in hold
    NaN."""
    rng = np.random.default_rng(seed)
    cases = []
    for c in range(n_cases):
        n_in, n_merges = EXACT_N_IN[c % 3], 1 + (c // 3) % 3
        loc = rng.integers(-4000, 4001, n_in)
        spread = rng.choice([0, 1, 7, 60], n_in)
        tot_n, tot_x, tot_xx = 0, [0] * n_in, [0] * n_in
        launches = []
        for k in range(n_merges):
            W, n_lanes = EXACT_SLABS[(c // 9 + k) % 3], EXACT_LANES[(c + k) % 4]
            mode = rng.integers(0, 3, n_in)
            prev = np.array([round(tot_x[i] / tot_n) if tot_n else 0 for i in range(n_in)])
            shift = np.where(mode == 0, 0, np.where(mode == 1, loc, prev)).astype(np.int64)
            drift = rng.integers(-3, 4, n_in) * spread  # the launches' means differ: Chan's delta is not 0
            partial = np.full((W, 2, MAX_IN), np.nan)
            cnt = rng.integers(1, 13, W)  # lane-steps of each slab
            n_b = int(cnt.sum())
            x = loc + drift + rng.integers(-1, 2, (n_b, n_in)) * rng.integers(0, 2, (n_b, n_in)) * spread \
                + rng.integers(-spread, spread + 1, (n_b, n_in))
            d = x - shift  # (int64: |d| < 2^14, a slab's sum of squares < 2^32)
            first = np.concatenate([[0], np.cumsum(cnt)[:-1]])
            partial[:, 0, :n_in], partial[:, 1, :n_in] = np.add.reduceat(d, first), np.add.reduceat(d * d, first)
            for i in range(n_in):
                tot_x[i] += int(x[:, i].sum())
                tot_xx[i] += int((x[:, i] * x[:, i]).sum())
            tot_n += n_b
            steps = np.full(n_lanes, n_b // n_lanes, np.int32)
            steps[: n_b % n_lanes] += 1
            launches.append((partial, steps, shift.astype(np.float32)))
        cases.append((n_in, launches, (tot_n, tot_x, tot_xx)))
    return cases


def transform_offsets(n_in, widths, n_out):
    """(offset of shift, of scale, of clip, set_floats) in a packed weight set: every layer's W[out][in] and b[out]
    first, then shift[n_in] | scale[n_in] | clip, zero padding to a multiple of 4 floats"""
    off, prev = 0, n_in
    for w in [*widths, n_out]:
        off += w * prev + w
        prev = w
    return off, off + n_in, off + 2 * n_in, (off + 2 * n_in + 1 + 3) // 4 * 4
