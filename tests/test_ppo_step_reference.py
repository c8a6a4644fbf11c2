"""ppo_step_ref.py, the host restatement of carl_ppo_adv_stats and carl_adam_step, against torch on the CPU.  CPU-only.

Adam.  The restatement keeps m, v and p in float32 as torch does but computes every step in float64; torch.optim.Adam
computes in float32.  With u = 2^-24 the two states drift apart by roundings alone, bounded per element and step by
  em <- b1 em + 4 u (|m| + |g|)        torch's lerp rounds g - m, the product and the sum; the restatement rounds once
  ev <- b2 ev + 4 u (v + g^2)          torch's mul and addcmul round three times; the restatement once
and the update lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps) differs by at most
  du = emh / D + mh ds / (D_ref D) + 5 u mh / D
emh = em / bc1, mh = |m| / bc1, evh = ev / bc2, vh = v / bc2, ds = min(sqrt(evh), evh / sqrt(vh)) the error of sqrt(vh),
D_ref = sqrt(vh) + eps, D = max(D_ref - ds, eps) (1 - 3 u) the smallest denominator torch can have, 5 u for torch's fp32
sqrt, division by sqrt(bc2), addition of eps, division and product with the step size.  Both sides round p once per step:
2 u |p|.  The per-step terms add up over the steps (ppo_checks.AdamReplica propagates a gradient error the same way).  The
running products of the betas differ from pow() by a few 2^-53 relative: 1e-12 of the update is added for them."""
import numpy as np
import pytest
import torch

import ppo_step_ref as SR

U = 2.0 ** -24
LR, EPS, B1, B2, STEPS = 3e-4, 1e-5, 0.9, 0.999, 20


@pytest.mark.parametrize("coef", [1.0, 0.5])
def test_adam_restatement_against_torch(coef):
    rng = np.random.default_rng(3)
    sizes = (1, 5, 1025)
    p0 = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    zero = [np.zeros(n, bool) for n in sizes]
    zero[1][[1, 3]] = True
    zero[2][::7] = True
    p0[2][0], p0[2][7] = -0.0, np.inf  # zero-gradient entries: a negative zero and an infinite (clip) entry
    ref = [p.copy() for p in p0]
    st = SR.adam_state(ref)
    tp = [torch.tensor(p.copy()) for p in p0]
    opt = torch.optim.Adam(tp, lr=LR, eps=EPS, betas=(B1, B2))
    em, ev, err = ([np.zeros(n) for n in sizes] for _ in range(3))
    worst = 0.0
    for k in range(1, STEPS + 1):
        g = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 1, n)).astype(np.float32) for n in sizes]
        for gi, z in zip(g, zero):
            gi[z] = 0.0
        SR.adam_ref(ref, g, st, coef, LR, (B1, B2), EPS)
        for t, gi in zip(tp, g):
            t.grad = torch.tensor(gi * np.float32(coef))  # (0.5: exact)
        opt.step()
        assert st["step"] == k
        np.testing.assert_allclose(st["beta_pow"], [B1 ** k, B2 ** k], rtol=1e-14)
        bc1, bc2 = 1 - B1 ** k, 1 - B2 ** k
        for i in range(len(sizes)):
            m, v = st["m"][i].astype(np.float64), st["v"][i].astype(np.float64)
            gd = np.abs(g[i].astype(np.float64)) * coef
            em[i] = B1 * em[i] + 4 * U * (np.abs(m) + gd)
            ev[i] = B2 * ev[i] + 4 * U * (v + gd * gd)
            emh, mh, evh, vh = em[i] / bc1, np.abs(m) / bc1, ev[i] / bc2, v / bc2
            with np.errstate(divide="ignore", invalid="ignore"):
                ds = np.minimum(np.sqrt(evh), np.where(vh > 0, evh / np.sqrt(vh), np.inf))
            d_ref = np.sqrt(vh) + EPS
            d = np.maximum(d_ref - ds, EPS) * (1 - 3 * U)
            du = emh / d + mh * ds / (d_ref * d) + (5 * U + 1e-12) * mh / d
            finite = np.isfinite(ref[i])
            err[i] += LR * du + 2 * U * np.where(finite, np.abs(ref[i]), 0.0)
            got = tp[i].detach().numpy()
            z = zero[i]
            # zero-gradient entries: bit-equal to torch and to the start
            for a, b in ((ref[i], got), (ref[i], p0[i]), (st["m"][i], opt.state[tp[i]]["exp_avg"].numpy()),
                         (st["v"][i], opt.state[tp[i]]["exp_avg_sq"].numpy())):
                np.testing.assert_array_equal(a[z].view(np.uint32), b[z].view(np.uint32))
            assert not st["m"][i][z].view(np.uint32).any() and not st["v"][i][z].view(np.uint32).any()
            diff = np.abs(ref[i][~z].astype(np.float64) - got[~z].astype(np.float64))
            assert np.all(diff <= err[i][~z]), (k, i, np.max(diff / err[i][~z]))
            if diff.size:
                worst = max(worst, float(np.max(diff / err[i][~z])))
    assert all(not np.array_equal(r[~z], p[~z]) for r, p, z in zip(ref, p0, zero) if (~z).any())  # they moved
    print(f"coef {coef}: largest difference / bound over {STEPS} steps {worst:.3f}")


def test_adam_restatement_takes_the_coefficient_and_a_clip_reference():
    g = [np.array([3.0, 0.0], np.float32), np.array([4.0], np.float32)]
    assert SR.norm_ref(g) == 5.0
    assert SR.coef_ref(5.0, None) == 1.0 and SR.coef_ref(5.0, float("inf")) == 1.0 and SR.coef_ref(0.0, 0.5) == 1.0
    assert SR.coef_ref(5.0, 0.5) == 0.5 / (5.0 + 1e-6)
    p, st = [np.ones(2, np.float32), np.ones(1, np.float32)], None
    st = SR.adam_state(p)
    SR.adam_ref(p, g, st, 0.1, LR)
    # the first step moves by lr * sign(g) up to eps: m / bc1 = gd, sqrt(v / bc2) = |gd|
    np.testing.assert_allclose(p[0], [1 - LR, 1.0], rtol=1e-4)
    np.testing.assert_allclose(st["m"][1], [0.1 * 0.4], rtol=1e-6)
    assert p[0][1] == 1.0 and st["m"][0][1] == 0 and st["v"][0][1] == 0


@pytest.mark.parametrize("n_total,batch", [(2, 2), (255, 256), (257, 256), (1000, 300), (4099, 1024)])
def test_adv_stats_restatement_against_torch(n_total, batch):
    rng = np.random.default_rng(n_total)
    storage = (1e4 + 1e-2 * rng.standard_normal(5000)).astype(np.float32) if n_total == 1000 else rng.standard_normal(5000).astype(np.float32)
    idx = rng.permutation(5000)[:n_total]
    got = SR.adv_stats_ref(storage, idx, batch)
    assert got.dtype == np.float32 and got.shape == (-(-n_total // batch), 2)
    for k, s in enumerate(range(0, n_total, batch)):
        a = torch.tensor(storage[idx[s: s + batch]]).double()
        if a.numel() == 1:
            assert got[k].tolist() == [0.0, 1.0]
            continue
        want = np.array([a.mean().item(), 1.0 / (a.std().item() + 1e-8)])
        assert np.all(np.abs(got[k].astype(np.float64) - want) <= SR.ulp32(want)), (k, got[k], want)


def test_adv_stats_rules():
    # n == 1: the identity, with the sign of zero
    one = SR.adv_stats_ref(np.array([3.5, -2.0], np.float32), [1, 0], 1)
    assert one.tolist() == [[0.0, 1.0], [0.0, 1.0]] and not np.signbit(one[:, 0]).any()
    # a constant column: the mean exact, var == 0 exactly, the scale fp32(1 / eps)
    const = np.full(300, np.float32(1e4 + 0.37))
    got = SR.adv_stats_ref(const, np.arange(300), 128, eps=1e-8)
    assert (got[:, 0] == const[0]).all() and (got[:, 1] == np.float32(1.0 / 1e-8)).all()
    # an index outside the storage counts as d = 0 (results stay finite), a last shorter minibatch is a row
    out = SR.adv_stats_ref(np.array([1.0, 2.0, 4.0], np.float32), [0, 1, 7, 2, -1], 3)
    assert out.shape == (2, 2) and np.isfinite(out).all()
    d = np.array([0.0, 1.0, 0.0])
    np.testing.assert_allclose(out[0], [1.0 + d.sum() / 3, 1.0 / (np.sqrt((d @ d - d.sum() ** 2 / 3) / 2) + 1e-8)], rtol=1e-6)
