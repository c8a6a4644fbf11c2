"""Shared by test_policy_value.py, test_gpu_policy_value.py and test_gpu_gae.py: critics for the policy_cases engines, the
value check against oracle.policy_forward, and the host restatement of the GAE rule (include/carl_amd.h: carl_gae).  A
plain module like policy_cases.py: importing it touches no device."""
import numpy as np

from carl_amd.policy import MLPPolicy
from oracle import oracle as O

U = 2.0 ** -24  # unit roundoff of float32


def make_critic(eng, actor, widths, act, rng):
    """a random value network over the actor's inputs, its shift / scale / clip the actor's (one weight set)"""
    dims = [actor.n_in, *widths, 1]
    layers = [(rng.normal(0, 1.5 / np.sqrt(i), (o, i)), rng.normal(0, 0.3, o)) for i, o in zip(dims[:-1], dims[1:])]
    clip = None if np.isinf(actor.clip) else float(actor.clip)
    return MLPPolicy.for_env(eng, layers, act, input_shift=actor.shift, input_scale=actor.scale, input_clip=clip,
                             context_features=actor.ctx_rows, head="value")


def check_values(crit, x, v, sets=None, where=None):
    """device values v [...] against the exact host reference of the critic's packed block on raw inputs x [..., n_in]:
    identity / relu bit for bit (+0 == -0), tanh within the reference's own bound.  where: a mask of the entries to check"""
    x = np.asarray(x, np.float32).reshape(-1, crit.n_in)
    v = np.asarray(v, np.float32).reshape(-1)
    sets = None if sets is None else np.asarray(sets).reshape(-1)
    if where is not None:
        m = np.asarray(where).reshape(-1)
        x, v, sets = x[m], v[m], None if sets is None else sets[m]
    if v.size == 0:
        return
    r = O.policy_forward(crit.params, crit.n_in, crit.widths, 1, crit.activation, x, sets)
    if crit.activation != "tanh":
        np.testing.assert_array_equal(v, r.y32[:, 0])
    else:
        err = np.abs(v.astype(np.float64) - r.y64[:, 0])
        assert np.all(err <= r.bound[:, 0] * (1 + 1e-9)), (err.max(), r.bound[:, 0][np.argmax(err - r.bound[:, 0])])


def gae_ref(reward, value, terminated, truncated, last_value, gamma, lam, boot_value=None):
    """carl_gae's rule in fp32, operation for operation (oracle.fmaf: correctly rounded fma) -> (advantage, ret) [T, N]"""
    f = np.float32
    T, N = reward.shape
    g = f(gamma)
    gl = f(f(gamma) * f(lam))
    adv, ret = np.empty((T, N), f), np.empty((T, N), f)
    A = np.zeros(N, f)
    v_next = np.asarray(last_value, f)
    zero = np.zeros(N, f)
    for t in range(T - 1, -1, -1):
        te, tr = terminated[t].astype(bool), truncated[t].astype(bool)
        done = te | tr
        vn = np.where(done, zero, v_next)
        if boot_value is not None:
            vn = np.where(tr & ~te, boot_value[t], vn)
        delta = (O.fmaf(g, vn, reward[t]) - value[t]).astype(f)
        A = O.fmaf(gl, np.where(done, zero, A), delta)
        adv[t], ret[t] = A, (A + value[t]).astype(f)
        v_next = value[t]
    return adv, ret


def gae_sb3_f64(reward, value, terminated, truncated, last_value, gamma, lam, boot_value=None):
    """SB3's RolloutBuffer.compute_returns_and_advantage in float64 (gamma and gamma * lambda as fp32 rounds them, so
    the difference to gae_ref is rounding of the recurrence alone), the timeout bootstrap folded into the reward as
    SB3's collect_rollouts does -> (advantage, ret, bound on |fp32 advantage - this|, bound for ret).
    Bound: one step of the fp32 rule rounds three times (the fma of delta, its subtraction, the fma of A), each by at
    most U times the magnitude of its own result, all of which M_t = |r| + g |vn| + |v| + gl |A_{t+1}| bounds; the
    error carried from t + 1 is multiplied by gl (0 across a done step).  So E_t = gl E_{t+1} + 3 U M_t, with 4 in
    place of 3 for the second-order terms; ret adds one rounding of |A| + |v|."""
    g = float(np.float32(gamma))
    gl = float(np.float32(np.float32(gamma) * np.float32(lam)))
    T, N = reward.shape
    r64, v64 = reward.astype(np.float64), value.astype(np.float64)
    adv, E = np.empty((T, N)), np.empty((T, N))
    A, e = np.zeros(N), np.zeros(N)
    v_next = np.asarray(last_value, np.float64)
    for t in range(T - 1, -1, -1):
        te, tr = terminated[t].astype(bool), truncated[t].astype(bool)
        nonterminal = 1.0 - (te | tr)
        rew = r64[t].copy()
        if boot_value is not None:
            cut = tr & ~te
            rew[cut] += g * boot_value[t].astype(np.float64)[cut]
        delta = rew + g * v_next * nonterminal - v64[t]
        M = np.abs(rew) + g * np.abs(v_next) * nonterminal + np.abs(v64[t]) + gl * np.abs(A) * nonterminal
        if boot_value is not None:
            M += g * np.abs(boot_value[t].astype(np.float64)) * cut
        A = delta + gl * nonterminal * A
        e = gl * nonterminal * e + 4 * U * M
        adv[t], E[t] = A, e
        v_next = v64[t]
    return adv, adv + v64, E, E + 2 * U * (np.abs(adv) + np.abs(v64) + E)


def random_gae_inputs(rng, T, N, p_te=0.1, p_tr=0.1):
    f = np.float32
    return dict(reward=rng.normal(0, 1, (T, N)).astype(f), value=rng.normal(0, 3, (T, N)).astype(f),
                terminated=(rng.random((T, N)) < p_te).astype(np.uint8), truncated=(rng.random((T, N)) < p_tr).astype(np.uint8),
                last_value=rng.normal(0, 3, N).astype(f), boot_value=rng.normal(0, 3, (T, N)).astype(f))
