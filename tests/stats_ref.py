"""Host reference of the input statistics (include/carl_amd.h: carl_evaluate_policy_stats, carl_policy_stats_merge), in
float64 NumPy: the sums a launch gathers, the merge with its constant rule, and the offsets of the transform section.
A plain module: importing it touches no device."""
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


def transform_offsets(n_in, widths, n_out):
    """(offset of shift, of scale, of clip, set_floats) in a packed weight set: every layer's W[out][in] and b[out]
    first, then shift[n_in] | scale[n_in] | clip, zero padding to a multiple of 4 floats"""
    off, prev = 0, n_in
    for w in [*widths, n_out]:
        off += w * prev + w
        prev = w
    return off, off + n_in, off + 2 * n_in, (off + 2 * n_in + 1 + 3) // 4 * 4
