"""Host reference and shared cases of the sampled Brax closed-loop rollout (include/carl_amd.h:
carl_brax_rollout_policy_sampled), for test_brax_policy_sampled_abi.py on the host and test_gpu_brax_policy_sampled.py on
the GPU: the counter and word selection of an actuator's draw, the float64 draws, the bounds a device's fp32 evaluation of
the rule must meet, the engines and policies of the GPU cases, and the pooled statistics of the independence check.  A
plain module: importing it allocates nothing and touches no device."""
import numpy as np

import brax_policy_cases as BP
import sampling_ref as SR
from brax_kernel_cases import touch_down
from oracle import oracle as O

SUB_BRAX_SAMPLE = 0x40000000  # | block << 28 | elapsed
_M = np.uint64(0xFFFFFFFF)
SEED = 0x5A3D1E5EED0F
N_CTX = 5


# ---------------------------------------------------------------- the rule
def counter(genv, episode_index, elapsed, actuator):
    """the four counter words of the Philox block actuator j = `actuator` of an env-step draws from:
    (genv lo, genv hi, e, 0x40000000 | (j >> 1) << 28 | elapsed), arrays broadcast"""
    genv = np.asarray(genv, np.uint64)
    block = np.asarray(actuator, np.uint64) >> np.uint64(1)
    tag = np.uint64(SUB_BRAX_SAMPLE) | (block << np.uint64(28)) | np.asarray(elapsed, np.uint64)
    return genv & _M, genv >> np.uint64(32), np.asarray(episode_index, np.uint64) & _M, tag


def actuator_words(seed, genv, episode_index, elapsed, actuator):
    """(wa, wb) of actuator j: (w.x, w.y) of its block for even j, (w.z, w.w) for odd j"""
    w = SR.philox(*counter(genv, episode_index, elapsed, actuator), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    odd = (np.asarray(actuator) & 1).astype(bool)
    return np.where(odd, w[2], w[0]), np.where(odd, w[3], w[1])


def draws64(seed, genv, episode_index, elapsed, n_act):
    """float64 z of every actuator of the env-steps (genv, e, elapsed), arrays of one shape S -> [*S, n_act]"""
    j = np.arange(n_act)
    wa, wb = actuator_words(seed, np.asarray(genv)[..., None], np.asarray(episode_index)[..., None],
                            np.asarray(elapsed)[..., None], j)
    return SR.z_gaussian64(wa, wb)


def check_rule(pol, x, genv, episode_index, elapsed, sets, seed, action, log_prob=None):
    """The device's actions [M, n_act] (and log-probabilities [M], or None) of M env-steps against the rule in float64.
    x [M, n_in]: the inputs the policy saw; genv / episode_index / elapsed [M]: the env-step's counter fields; sets [M]:
    its weight set.  -> (z64, mu64, worst action |err| / bound, worst log_prob |err| / bound).

    Where the bounds come from (u = sampling_ref.ULP = 2^-24, one fp32 rounding's relative error):
      action   the device computes a = fl(s z + mu) in ONE fma, from its own s = expf(log_std), z and mu.
               |mu - mu64| <= bound_j, the forward pass's derived bound (oracle.policy_forward);
               |z - z64| <= gaussian_z_bound(z64), the bound of logf / sqrtf / cospif and the two products that the classic
               Gaussian rule is held to (sampling_ref);
               s = expf(ls) is within 1 ulp of exp(ls) (the accurate expf: 2 u relative), so |s z - exp(ls) z64| <=
               exp(ls) (dz + 2 u |z64|) to first order -- the test allows 4 u |z64|, twice that;
               the fma rounds once: u |a|, allowed 2 u |a|.
      log_prob lp_j = fl(fma(-z / 2, z, lp0_j)), lp0_j = fl(-ls_j - fl(ln(2 pi) / 2)): gaussian_log_prob_bound(z64_j, ls_j)
               (|z| dz and the roundings of lp0, the constant and the fma), as for the classic rule; the n_act values are
               summed in fp32 in actuator order: n_act - 1 additions, each rounding a partial sum that is at most
               sum_j |lp_j| (first order) -- (n_act - 1) u sum_j |lp64_j|, allowed twice."""
    M = x.shape[0]
    _, mu64, bound = BP.reference_actions(pol, x, sets)
    ls = np.asarray(pol.log_std, np.float32)[sets].astype(np.float64)  # [M, n_act]
    z = draws64(seed, genv, episode_index, elapsed, pol.n_out)
    a = np.asarray(action, np.float32).reshape(M, pol.n_out)
    assert np.isfinite(a).all()
    sigma = np.exp(ls)
    want = mu64 + sigma * z
    lim = bound + sigma * (SR.gaussian_z_bound(z) + 4 * SR.ULP * np.abs(z)) + 2 * SR.ULP * np.abs(a.astype(np.float64))
    err = np.abs(a.astype(np.float64) - want)
    k = np.unravel_index(np.argmax(err - lim), err.shape)
    assert np.all(err <= lim), ("action", k, err[k], lim[k])
    worst_a = float((err / np.maximum(lim, 1e-300)).max())
    worst_lp = 0.0
    if log_prob is not None:
        lp64 = SR.gaussian_log_prob64(z, ls)
        lp_lim = SR.gaussian_log_prob_bound(z, ls).sum(axis=1) + 2 * SR.ULP * (pol.n_out - 1) * np.abs(lp64).sum(axis=1)
        lp = np.asarray(log_prob, np.float32).reshape(M)
        assert np.isfinite(lp).all()
        lp_err = np.abs(lp.astype(np.float64) - lp64.sum(axis=1))
        k = int(np.argmax(lp_err - lp_lim))
        assert np.all(lp_err <= lp_lim), ("log_prob", k, lp_err[k], lp_lim[k])
        worst_lp = float((lp_err / lp_lim).max())
    return z, mu64, worst_a, worst_lp


# ---------------------------------------------------------------- the independence check's statistics
def pooled_stats(z):
    """z [T, n, n_act] -> (mean, variance about 0 mean estimate, sample correlation between actuators 2k and 2k + 1 pooled
    over k, sample correlation between neighbouring envs), and the 5-sigma bounds of each for independent N(0, 1) draws"""
    M = z.size
    mean, var = float(z.mean()), float(z.var())
    corr = lambda a, b: float(np.corrcoef(a.reshape(-1), b.reshape(-1))[0, 1])  # noqa: E731
    n_pair = z.shape[2] // 2 * 2
    pair = corr(z[:, :, 0:n_pair:2], z[:, :, 1:n_pair:2]) if n_pair else 0.0
    env = corr(z[:, :-1], z[:, 1:])
    return (mean, var, pair, env), (5 / np.sqrt(M), 5 * np.sqrt(2 / M), 5 / np.sqrt(M / 8), 5 / np.sqrt(M / 8))


def assert_independent(z):
    (mean, var, pair, env), (b_mean, b_var, b_pair, b_env) = pooled_stats(z)
    assert abs(mean) < b_mean, (mean, b_mean)
    assert abs(var - 1) < b_var, (var, b_var)
    assert abs(pair) < b_pair, (pair, b_pair)
    assert abs(env) < b_env, (env, b_env)
    return mean, var, pair, env


# ---------------------------------------------------------------- engines and policies of the GPU cases
def make_engine(model, width, n, device, seed, max_episode_steps=3, **kw):
    """`model` at `width` lanes per env: n envs over N_CTX contexts under a round-robin selector, gravity and friction
    visible, reset, and on the ground models half the envs 5 mm deep in the ground (the contact path from step one)"""
    from carl_amd.brax_engine import BraxVecEngine

    s, names, default = BP.build_model(model)
    s.lanes_per_env = width
    rows = BP.context_rows(np.random.default_rng(seed), N_CTX, default, names)
    eng = BraxVecEngine(s, len(names), rows, n, device, selector=O.SEL_ROUND_ROBIN, seed=seed,
                        max_episode_steps=max_episode_steps,
                        ctx_obs_rows=[names.index("gravity"), names.index("friction")], **kw)
    assert width in eng.lane_widths()
    eng.reset()
    if model in BP.GROUND:
        eng.set_state64(touch_down(eng.sys, eng.state64().cpu().numpy()))
    return eng


def make_policy(eng, widths, act, seed, log_std=None):
    from carl_amd.brax_policy import BraxMLPPolicy

    rng = np.random.default_rng(seed)
    n_in = 2 + eng.D
    shift, scale, clip = BP.transform(rng, n_in)
    shift[0] += -10.0  # gravity ~ -10: centred like a normalised input
    return BraxMLPPolicy.for_env(eng, BP.make_layers(rng, n_in, widths, eng.sys.n_act), act, shift, scale, clip,
                                 log_std=log_std)


def two_set_policy(eng, widths, act, seed):
    """two weight sets of 256 envs with different log_std rows: per actuator values between -1.5 and 0.5"""
    from carl_amd.brax_policy import BraxMLPPolicy

    rng = np.random.default_rng(seed + 17)
    pols = [make_policy(eng, widths, act, seed + k, rng.uniform(-1.5, 0.5, eng.sys.n_act).astype(np.float32))
            for k in range(2)]
    return BraxMLPPolicy.stack(pols, 256)
