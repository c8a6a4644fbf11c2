"""NumPy restatements of PPO's minibatch step (include/carl_amd.h: carl_ppo_adv_stats, carl_adam_step).  A plain module:
importing it allocates nothing and touches no device.

adv_stats_ref: the header's contract with both sums exact (math.fsum): what the device's float64 chains are held to.
adam_ref: the header's float64 expressions in the header's order, one NumPy operation per rounding, so that a device run
with the same coefficient gives the same bits.  It takes the clip coefficient as an input; norm_ref / coef_ref give the
reference norm (fsum) and coefficient."""
import math

import numpy as np


def ulp32(x):
    """the spacing of float32 at |x| (of the smallest normal below it)"""
    return np.spacing(np.maximum(np.abs(np.asarray(x, np.float32)), np.float32(2.0 ** -126))).astype(np.float64)


def adv_stats_ref(storage, idx, batch_size, eps=1e-8):
    """-> float32 [ceil(len(idx) / batch_size), 2].  storage: float32 [n]; an index outside it counts as d = 0."""
    storage = np.asarray(storage, np.float32).reshape(-1)
    idx = np.asarray(idx, np.int64)
    rows = []
    for s in range(0, len(idx), batch_size):
        j = idx[s: s + batch_size]
        n = len(j)
        if n == 1:
            rows.append((0.0, 1.0))
            continue
        ok = (j >= 0) & (j < len(storage))
        a = storage[np.where(ok, j, 0)].astype(np.float64)
        c = a[0] if ok[0] else 0.0
        d = np.where(ok, a - c, 0.0)  # (exact: two floats of neighbouring magnitude)
        S1, S2 = math.fsum(d), math.fsum(d * d)
        mean = c + S1 / n
        var = max(0.0, (S2 - S1 * S1 / n) / (n - 1))
        rows.append((mean, 1.0 / (math.sqrt(var) + eps)))
    return np.array(rows, np.float64).astype(np.float32)


def norm_ref(grads):
    """sqrt of the exact sum of squares of every entry of every gradient"""
    return math.sqrt(math.fsum(np.concatenate([np.asarray(g, np.float32).reshape(-1).astype(np.float64) ** 2 for g in grads])))


def coef_ref(norm, max_grad_norm):
    return 1.0 if max_grad_norm is None or math.isinf(max_grad_norm) else min(1.0, max_grad_norm / (norm + 1e-6))


def adam_state(params):
    return {"m": [np.zeros(np.size(p), np.float32) for p in params], "v": [np.zeros(np.size(p), np.float32) for p in params],
            "step": 0, "beta_pow": np.ones(2, np.float64)}


def adam_ref(params, grads, state, coef, lr, betas=(0.9, 0.999), eps=1e-5):
    """One step, in place: params / state["m"] / state["v"]: lists of float32 arrays; state["step"], state["beta_pow"]"""
    b1, b2 = np.float64(betas[0]), np.float64(betas[1])
    coef, lr, eps = np.float64(coef), np.float64(lr), np.float64(eps)
    state["step"] += 1
    state["beta_pow"][0] = state["beta_pow"][0] * b1
    state["beta_pow"][1] = state["beta_pow"][1] * b2
    bc1, bc2 = 1.0 - state["beta_pow"][0], 1.0 - state["beta_pow"][1]
    step_size, sqrt_bc2 = lr / bc1, np.sqrt(bc2)
    omb1, omb2 = 1.0 - b1, 1.0 - b2
    with np.errstate(invalid="ignore", over="ignore"):
        for p, g, m, v in zip(params, grads, state["m"], state["v"]):
            gd = np.asarray(g, np.float32).reshape(-1).astype(np.float64) * coef
            m[:] = (b1 * m.astype(np.float64) + omb1 * gd).astype(np.float32)
            v[:] = (b2 * v.astype(np.float64) + (omb2 * gd) * gd).astype(np.float32)
            pf = p.reshape(-1)  # (a view: the parameters are contiguous)
            pf[:] = (pf.astype(np.float64) - (step_size * m.astype(np.float64)) / (np.sqrt(v.astype(np.float64)) / sqrt_bc2 + eps)
                     ).astype(np.float32)
