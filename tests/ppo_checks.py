"""What the PPO update's GPU tests of the classic-control and of the Brax families check in the same way, written once
(test_gpu_ppo_grad.py, test_gpu_brax_ppo_grad.py: two calls on canaried buffers, the Gaussian log-probability bound, the
+0.0 entries of a gradient, the statistics block; test_gpu_ppo.py, test_gpu_brax_ppo.py: the host replica under Adam with
its error bound, the recorded minibatch order, the device parameters against the replica; test_gpu_ppo_grad_edges.py and the
CPU tests of its helpers in test_ppo_reference.py / test_brax_ppo_reference.py: guarded uploads, the zero-signal tile
identities, the helpers' own checks).  A plain module: importing it allocates nothing and touches no device."""
import numpy as np
import pytest
import torch

import ppo_ref as R
import sampling_ref as SR

CANARY = 7.25
LR, B1, B2, EPS = 3e-4, 0.9, 0.999, 1e-5
CLIP, VF, ENT, MAX_NORM = 0.2, 0.5, 0.01, 0.5


# ---------------------------------------------------------------- one gradient call (carl_ppo_grad / carl_brax_ppo_grad)
def run_twice(sizes, need, launch, dev="cuda"):
    """launch(out, workspace) twice, each time on fresh float32 buffers filled with CANARY: out[k] the first sizes[k]
    floats of a buffer 16 longer, workspace the first `need` of one 16 longer.  -> [(outputs as NumPy arrays, what lies
    behind each output and the workspace)] * 2"""
    results = []
    for _ in range(2):
        big = {k: torch.full((n + 16,), CANARY, dtype=torch.float32, device=dev) for k, n in sizes.items()}
        ws = torch.full((need + 16,), CANARY, dtype=torch.float32, device=dev)
        launch({k: big[k][:n] for k, n in sizes.items()}, ws[:need])
        torch.cuda.synchronize()
        results.append(({k: big[k][:n].cpu().numpy() for k, n in sizes.items()},
                        {**{k: big[k][n:].cpu().numpy() for k, n in sizes.items()}, "workspace": ws[need:].cpu().numpy()}))
    return results


def check_canaries_and_bits(results):
    """a canary behind every output and the workspace, and the same bits twice -> the first call's outputs"""
    (got, tail), (again, tail2) = results
    for t in (tail, tail2):
        for k, v in t.items():
            assert (v == CANARY).all(), k
    for k in got:
        np.testing.assert_array_equal(got[k].view(np.uint32), again[k].view(np.uint32), err_msg=k)
    return got


def gaussian_log_prob_reference(y64, ybound, log_std, action):
    """(lp64 [M], bound [M]) of the joint Gaussian log-probability of actions [M, n_out] under means y64 [M, n_out] known
    within ybound.  Per output z = (a - mu) * exp(-log_std) in fp32: the forward bound on mu and the roundings of the
    subtraction, of expf and of the product; then fma(-z / 2, z, lp0) as the rollout's log-probability
    (sampling_ref.gaussian_log_prob_bound); summed over the outputs"""
    ls = np.asarray(log_std, np.float32).reshape(-1).astype(np.float64)
    a = np.asarray(action, np.float32).reshape(-1, len(ls))
    lp64, bound = np.zeros(len(a)), np.zeros(len(a))
    for j in range(len(ls)):
        mu = y64[:, j]
        z = (a[:, j].astype(np.float64) - mu) * np.exp(-ls[j])
        dz = (ybound[:, j] + 4 * SR.ULP * (np.abs(a[:, j]) + np.abs(mu))) * np.exp(-ls[j]) + 4 * SR.ULP * np.abs(z)
        lpj = SR.gaussian_log_prob64(z, ls[j])
        lp64 += lpj
        bound += np.abs(z) * dz + dz * dz + 4 * SR.ULP * (abs(ls[j]) + 2 + np.abs(lpj))
    return lp64, bound


def check_log_prob(got, lp64, bound, ref_log_prob):
    """new_log_prob within the forward bound of lp64, and lp64 the gradient reference's own log-probability"""
    err = np.abs(got.astype(np.float64) - lp64)
    assert np.all(err <= bound * (1 + 1e-9)), (err.max(), bound[np.argmax(err - bound)])
    np.testing.assert_allclose(lp64, ref_log_prob, rtol=0, atol=1e-9 * (1 + np.abs(lp64).max()))
    return err


def check_transform_entries(got, actor, critic):
    """the shift | scale | clip entries and the padding of both gradients: +0.0 bits"""
    for name, pol in (("actor", actor), ("critic", critic)):
        assert not got["grad_" + name][pol.weight_floats:].view(np.uint32).any(), name


def check_statistics(stats, ref_stats, M):
    """means of per-sample fp32 terms, each within a few 1e-6 relative of its float64 value (the log-probability bound,
    through exp), accumulated in float64"""
    s = stats.astype(np.float64)
    assert s[5] == M
    np.testing.assert_allclose(s[:4], ref_stats[:4], rtol=2e-5, atol=2e-5)
    assert s[4] == pytest.approx(ref_stats[4], abs=0.5 / M + 1e-6)  # ratios are 0.01 away from 1 +- clip: the same count


# ---------------------------------------------------------------- the edges (test_gpu_ppo_grad_edges.py, part D's CPU tests)
GRADS = ("grad_actor", "grad_critic", "grad_log_std")
MIN_NORMAL, SUBNORMAL_STEP = 2.0 ** -126, 2.0 ** -149


def guarded(a, band, fill, dev="cuda"):
    """the NumPy array `a` on the device as a view into a larger allocation: `band` elements filled with `fill` on both
    sides of it"""
    a = np.ascontiguousarray(a)
    big = torch.full((a.size + 2 * band,), fill, dtype=torch.as_tensor(a[:0]).dtype, device=dev)
    view = big[band: band + a.size]
    view.copy_(torch.as_tensor(a.reshape(-1)))
    return view.view(a.shape)


def grad_units(got, ref, names=GRADS):
    """largest |g - g_64| / (2^-24 S) over the named gradients a reference dict has (ppo_ref.grad_error_units)"""
    k = 0.0
    for name in names:
        if name in got:
            g64, S = np.atleast_1d(ref[name]), np.atleast_1d(ref["S_" + name[5:]])
            k = max(k, R.grad_error_units(np.atleast_1d(got[name]), g64, S).max(initial=0.0))
    return k


def check_tile_identities(runs, nA, nB, M, weight_floats):
    """The second pass of the tile loop, isolated by zero-signal samples.  runs: {"small_A", "small_B", "big_A", "big_B",
    "big_AB"} -> {gradient name: float32 array}; weight_floats: {gradient name: its leading entries that are weights}.

    A workgroup's slab entry is an fp32 accumulator: the tile sums of its tiles added in order.  A zero-signal sample adds
    +-0 to every block sum, so in big_A the entry is the fp32 value `a` that the one workgroup of small_A has, and the
    outputs are rn32(a / M) and rn32(a / |A|) with the division in float64: M big_A and |A| small_A agree within
    3 * 2^-24 |A| |small_A| (two fp32 roundings and the float64 terms); likewise B with `b`.  In big_AB the entry is
    rn32(a + b): that rounding, the final one and the two small runs' roundings each cost 2^-24 of a magnitude of at most
    |a| + |b| -- 3 units where they align, and the bound is 4 * 2^-24 (|A| |small_A| + |B| |small_B|) to leave room for
    the float64 terms.  An entry below 2^-126 is rounded to a multiple of 2^-149 instead: one such step, times its run's
    sample count, is added where that happens.  At least half the weight entries of each gradient must be non-zero in
    small_A and in small_B.  -> the largest error / bound"""
    worst = 0.0
    f64 = lambda v: np.atleast_1d(v).astype(np.float64)  # noqa: E731
    floor = lambda v, n: n * SUBNORMAL_STEP * (np.abs(v) < MIN_NORMAL)  # noqa: E731
    for name in GRADS:
        if name not in runs["small_A"]:
            continue
        a, b = f64(runs["small_A"][name]), f64(runs["small_B"][name])
        for small, n, label in ((a, nA, "A"), (b, nB, "B")):
            nz = np.count_nonzero(small[: weight_floats[name]])
            assert 2 * nz >= weight_floats[name], (name, label, nz)
            big = f64(runs["big_" + label][name])
            err = np.abs(M * big - n * small)
            bound = 3 * R.U * n * np.abs(small) + floor(small, n) + floor(big, M)
            assert np.all(err <= bound), (name, label, float(np.max(err - bound)))
            worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
        big = f64(runs["big_AB"][name])
        err = np.abs(M * big - (nA * a + nB * b))
        bound = 4 * R.U * (nA * np.abs(a) + nB * np.abs(b)) + floor(a, nA) + floor(b, nB) + floor(big, M)
        assert np.all(err <= bound), (name, "AB", float(np.max(err - bound)))
        worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
    return worst


def gradients_of(ref, box):
    """a reference dict's gradients as the device's outputs are shaped (grad_log_std an array, absent for a discrete head)"""
    return {k: np.atleast_1d(ref[k]) for k in GRADS if box or k != "grad_log_std"}


def check_tile_loop_helpers(mod, spec):
    """On the CPU, what test_gpu_ppo_grad_edges.py's part A does on the device, with the float32 restatement in the
    device's summation order (``tile_order=True``) in the device's place: ppo_ref.tile_loop_runs' five runs per workgroup,
    the small runs within K of the float64 reference, the identities within their bounds -- and the identities must refuse
    a big_AB whose second tile counts twice.  mod: ppo_ref or brax_ppo_ref"""
    case = mod.make_case(spec)
    box = not getattr(case["actor"], "discrete", False)
    M = case["flat"].size
    assert M == R.M_TILES and len(set(case["flat"].tolist())) == M

    def restatement(pos, columns):
        return mod.case_reference(case, np.float32, pos, columns, adv_norm=None, ent_coef=0.0, tile_order=True)

    for w in R.TILE_LOOP_WORKGROUPS:
        runs, A, B = R.tile_loop_runs(case, w, restatement)
        assert (A.size, B.size) == ((R.TILE, R.TILE) if w < 3 else (R.TILE, 7)) and A[0] == w * R.TILE
        assert B[0] == (w + R.WORKGROUPS_CAP) * R.TILE and B[-1] < M
        g = {k: gradients_of(v, box) for k, v in runs.items()}
        wf = {"grad_actor": case["actor"].weight_floats, "grad_critic": case["critic"].weight_floats,
              "grad_log_std": g["small_A"]["grad_log_std"].size if box else 0}
        for label, pos in (("small_A", A), ("small_B", B)):
            k = grad_units(g[label], mod.case_reference(case, pos=pos, adv_norm=None, ent_coef=0.0))
            assert k <= mod.K, (label, k)
        worst = check_tile_identities(g, A.size, B.size, M, wf)
        print(f"{case['id']}, workgroup {w}: largest identity error / bound {worst:.3f}")
        twice = {n: ((A.size * g["small_A"][n].astype(np.float64) + 2 * B.size * g["small_B"][n]) / M).astype(np.float32)
                 for n in g["big_AB"]}
        with pytest.raises(AssertionError):
            check_tile_identities({**g, "big_AB": twice}, A.size, B.size, M, wf)


def check_skipped_helpers(mod, spec):
    """On the CPU: ppo_ref.with_bad_entries replaces exactly the entries the header's rule skips, and
    ppo_ref.rescaled(reference over the valid samples) is the float64 evaluation of all M samples with the skipped samples'
    terms zero -- made so by ppo_ref.zero_signal (ent_coef = 0, no advantage normalisation), which zeroes their gradient,
    policy-loss and value-loss terms (the entropy, approx_kl and clip-fraction terms of a sample do not depend on its
    advantage or return: those three means are compared with sums over the valid samples)"""
    case = mod.make_case(spec)
    T, pitch, N = case["T"], case["P"], case["N"]
    idx, valid = R.with_bad_entries(case["flat"], T, pitch, N)
    M, pos = idx.size, np.flatnonzero(valid)
    i64 = idx.astype(np.int64)
    skipped = (i64 < 0) | (i64 >= T * pitch) | (i64 % pitch >= N)
    np.testing.assert_array_equal(skipped, ~valid)
    np.testing.assert_array_equal(idx[valid], case["flat"][valid])
    assert set(R.bad_positions(M)) == set(np.flatnonzero(~valid)) and np.abs(i64[~valid] - T * pitch // 2).max() <= T * pitch
    assert len(set(i64[~valid].tolist())) == (3 if pitch == N else 6)
    kw = dict(adv_norm=None, ent_coef=0.0)
    sub = mod.case_reference(case, pos=pos, **kw)
    got = R.rescaled(sub, pos.size, M)
    v64 = mod.case_reference(case, **kw)["new_value"]
    full = mod.case_reference(case, columns=R.zero_signal(case, pos, v64), **kw)
    for k in ("grad_actor", "grad_critic", "grad_log_std", "S_actor", "S_critic", "S_log_std"):
        np.testing.assert_allclose(got[k], full[k], rtol=1e-11, atol=1e-14, err_msg=k)
        assert np.any(np.asarray(full[k]) != 0) or (k.endswith("log_std") and getattr(case["actor"], "discrete", False))
    np.testing.assert_allclose(got["stats"][:2], full["stats"][:2], rtol=1e-11, atol=1e-14)
    r = sub["ratio"]
    means = [sub["entropy"].sum() / M, ((r - 1) - np.log(r)).sum() / M, (np.abs(r - 1) > np.float64(np.float32(R.CLIP))).sum() / M]
    np.testing.assert_allclose(got["stats"][2:5], means, rtol=1e-11, atol=1e-14)
    assert got["stats"][5] == M and sub["stats"][5] == pos.size


# ---------------------------------------------------------------- a PPO run against a host replica
class AdamReplica:
    """The host side of one PPO run: packed float32 parameters under torch's CPU Adam, and next to them a bound on how far
    the device's parameters may be from them.  A test's subclass turns a minibatch into the reference gradients `g` and
    their tolerances `dg` and hands them to apply().

    The bound.  The device's gradient entry differs from the reference's by at most dg = K 2^-24 S (ppo_ref.py,
    brax_ppo_ref.py).  The clip multiplies by coef = min(1, max_norm / (|g| + 1e-6)), whose relative error is at most
    |dg|_2 / |g|_2.  Adam keeps m = b1 m + (1 - b1) g and v = b2 v + (1 - b2) g^2, so their errors obey
    em = b1 em + (1 - b1) dg and ev = b2 ev + (1 - b2) (2 |g| dg + dg^2); with the bias corrections the step is
    lr * mh / (sqrt(vh) + eps), whose error is at most lr * (emh / D + |mh| ds / (D_ref D)), ds = min(sqrt(evh),
    evh / sqrt(vh)) the error of sqrt(vh) and D = max(D_ref - ds, eps) the smallest denominator the device can have; never
    more than lr * 2 / sqrt(1 - b2) (|step| <= lr / sqrt(1 - b2) on both sides).  The per-step errors add up over the
    steps.  The parameters' own difference changes later gradients too, a second-order effect: the total is doubled for
    it, and 4 roundings of the parameter are added."""

    def __init__(self, params):
        self.params = [torch.tensor(np.array(p, copy=True)) for p in params]
        self.opt = torch.optim.Adam(self.params, lr=LR, eps=EPS)
        self.em = [np.zeros(p.numel()) for p in self.params]
        self.ev = [np.zeros(p.numel()) for p in self.params]
        self.err = [np.zeros(p.numel()) for p in self.params]
        self.steps = 0

    def apply(self, g, dg):
        total = np.sqrt(sum((v ** 2).sum() for v in g))
        coef = min(1.0, MAX_NORM / (total + 1e-6))
        rel = np.sqrt(sum((v ** 2).sum() for v in dg)) / total
        self.steps += 1
        k = self.steps
        for i, p in enumerate(self.params):
            p.grad = torch.tensor((g[i] * coef).astype(np.float32))
            gi, dgi = np.abs(g[i]) * coef, coef * dg[i] + np.abs(g[i]) * coef * rel
            self.em[i] = B1 * self.em[i] + (1 - B1) * dgi
            self.ev[i] = B2 * self.ev[i] + (1 - B2) * (2 * gi * dgi + dgi ** 2)
        self.opt.step()
        for i, p in enumerate(self.params):
            st = self.opt.state[p]
            mh = np.abs(st["exp_avg"].numpy().astype(np.float64)) / (1 - B1 ** k)
            vh = st["exp_avg_sq"].numpy().astype(np.float64) / (1 - B2 ** k)
            emh, evh = self.em[i] / (1 - B1 ** k), self.ev[i] / (1 - B2 ** k)
            with np.errstate(divide="ignore", invalid="ignore"):
                ds = np.minimum(np.sqrt(evh), np.where(vh > 0, evh / np.sqrt(vh), np.inf))
            d_ref = np.sqrt(vh) + EPS
            d_min = np.maximum(d_ref - ds, EPS)
            du = emh / d_min + mh * ds / (d_ref * d_min)
            self.err[i] += LR * np.minimum(du, 2 / np.sqrt(1 - B2))

    def bound(self, i):
        return 2 * self.err[i] + 4 * R.U * np.abs(self.params[i].numpy().astype(np.float64))


def record(ppo, eng):
    """-> (order, start): order gets every epoch's minibatches (int64 flat indices) as update() draws them; start gets
    ctx_idx / episode right before each rollout launch (the first collect() resets the engine)"""
    order, draw = [], ppo.minibatches

    def recording():
        mbs = draw()
        order.append([m.cpu().numpy().astype(np.int64) for m in mbs])
        return mbs

    ppo.minibatches = recording
    start, roll = {}, eng.rollout_policy

    def recording_rollout(*a, **kw):
        start["ctx"], start["ep"] = eng.ctx_idx.cpu().numpy(), eng.episode.cpu().numpy()
        return roll(*a, **kw)

    eng.rollout_policy = recording_rollout
    return order, start


def check_against_replica(label, dev, rep, ppo, actor, critic):
    """the device tensors `dev` within the replica's bounds; the transform section and the padding keep their bits"""
    for i, d in enumerate(dev):
        diff = np.abs(d.cpu().numpy().astype(np.float64) - rep.params[i].numpy().astype(np.float64))
        bound = rep.bound(i)
        print(f"{label}, tensor {i}: largest difference {diff.max():.3e}, bound there "
              f"{bound[np.argmax(diff)]:.3e}, largest difference / bound {np.max(diff / np.maximum(bound, 1e-300)):.3e}")
        assert np.all(diff <= bound)
    for d, pol in ((ppo.actor_params[0], actor), (ppo.critic_params[0], critic)):
        np.testing.assert_array_equal(d.cpu().numpy()[pol.weight_floats:].view(np.uint32),
                                      pol.params[0][pol.weight_floats:].view(np.uint32))
