"""carl_adam_step on the GPU (LaneEngine.adam_step): five consecutive steps over each tensor set, after every step
  - norm_out[0] within n * 2^-52 relative of the exact (fsum) norm: n additions of exact squares, each rounded once
    (n * 2^-53 of the sum), halved by the square root and one more rounding for it;
  - norm_out[1] the bits of min(1, max_grad_norm / (norm_out[0] + 1e-6)) -- the header's expression on the device's own
    norm -- and so within 1 fp32 ulp (in fact n * 2^-52 relative) of the coefficient of the exact norm;
  - with the device's own norm_out[1] fed to ppo_step_ref.adam_ref: m, v, p, step and beta_pow bit-equal to it.
Every buffer has canaries behind it; two runs from equal fresh buffers give equal bits.  Entries whose gradient is +0.0
(with m = v = 0) keep the bits of p, m and v beside moving neighbours, a -0.0 and an infinite parameter among them."""
import numpy as np
import pytest
import torch

import policy_cases as PC
import ppo_step_ref as SR
from carl_amd import _lib

pytestmark = pytest.mark.gpu

CANARY, STEPS = 7.25, 5
LR, B1, B2, EPS = 3e-4, 0.9, 0.999, 1e-5
SETS = [(1,), (63, 65), (1023, 1025, 1), (5000, 4097, 8), (64, 64, 64, 3)]
CLIPS = {"active": 10.0, "inactive": 0.1, "off": None}  # the gradient norm over max_grad_norm


@pytest.fixture(scope="module")
def eng():
    return PC.make_engine(_lib.CARTPOLE, 256, n_contexts=4)


def canaried(arr, dtype):
    """-> (the whole buffer, its first len(arr) elements holding arr)"""
    big = torch.full((arr.size + 16,), CANARY if dtype.is_floating_point else 7, dtype=dtype, device="cuda")
    big[: arr.size] = torch.tensor(arr, device="cuda")
    return big, big[: arr.size]


def device_run(eng, p0, grads, max_norm, step0=0, beta_pow0=(1.0, 1.0), betas=(B1, B2)):
    """STEPS steps from fresh canaried buffers -> per step a dict of NumPy copies of p, m, v, step, beta_pow, norm"""
    f32, f64 = torch.float32, torch.float64
    bufs = {"p": [canaried(p, f32) for p in p0], "m": [canaried(np.zeros_like(p), f32) for p in p0],
            "v": [canaried(np.zeros_like(p), f32) for p in p0], "step": canaried(np.array([step0], np.int64), torch.int64),
            "beta_pow": canaried(np.array(beta_pow0, np.float64), f64), "norm": canaried(np.zeros(2), f64)}
    state = {"m": [b[1] for b in bufs["m"]], "v": [b[1] for b in bufs["v"]], "step": bufs["step"][1], "beta_pow": bufs["beta_pow"][1]}
    params = [b[1] for b in bufs["p"]]
    out = []
    for g in grads:
        dg = [canaried(x, f32) for x in g]
        eng.adam_step(params, [b[1] for b in dg], state, LR, betas, EPS, max_norm, norm_out=bufs["norm"][1])
        torch.cuda.synchronize()
        for big, view in dg + bufs["p"] + bufs["m"] + bufs["v"] + [bufs["step"], bufs["beta_pow"], bufs["norm"]]:
            assert (big[view.numel():] == (CANARY if big.is_floating_point() else 7)).all()
        for (big, view), x in zip(dg, g):  # the gradients are read only
            np.testing.assert_array_equal(view.cpu().numpy().view(np.uint32), x.view(np.uint32))
        out.append({"p": [t.cpu().numpy() for t in params], "m": [t.cpu().numpy() for t in state["m"]],
                    "v": [t.cpu().numpy() for t in state["v"]], "step": int(state["step"].cpu()),
                    "beta_pow": state["beta_pow"].cpu().numpy(), "norm": bufs["norm"][1].cpu().numpy()})
    return out


def same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    view = np.uint32 if a.dtype == np.float32 else np.uint64
    np.testing.assert_array_equal(a.view(view), b.view(view), err_msg=what)


def check_run(eng, p0, grads, max_norm, zero=None, step0=0, beta_pow0=(1.0, 1.0)):
    """two device runs with equal bits; every step against the references -> the first run's snapshots"""
    runs = [device_run(eng, p0, grads, max_norm, step0, beta_pow0) for _ in range(2)]
    for a, b in zip(*runs):
        for k in ("p", "m", "v"):
            for x, y in zip(a[k], b[k]):
                same_bits(x, y, k)
        same_bits(a["beta_pow"], b["beta_pow"], "beta_pow")
        same_bits(a["norm"], b["norm"], "norm")
        assert a["step"] == b["step"]
    ref = [p.copy() for p in p0]
    st = SR.adam_state(ref)
    st["step"], st["beta_pow"] = step0, np.array(beta_pow0, np.float64)
    n = sum(p.size for p in p0)
    for k, (g, got) in enumerate(zip(grads, runs[0])):
        norm, coef = got["norm"]
        exact = SR.norm_ref(g)
        assert abs(norm - exact) <= n * 2.0 ** -52 * exact, (norm, exact)
        want = SR.coef_ref(norm, max_norm)
        assert coef == want, (coef, want)
        c_exact = SR.coef_ref(exact, max_norm)
        assert abs(coef - c_exact) <= (n + 1) * 2.0 ** -52 * c_exact <= np.spacing(np.float32(c_exact))
        SR.adam_ref(ref, g, st, coef, LR, (B1, B2), EPS)
        for i in range(len(p0)):
            same_bits(got["p"][i], ref[i], f"step {k}, p[{i}]")
            same_bits(got["m"][i], st["m"][i], f"step {k}, m[{i}]")
            same_bits(got["v"][i], st["v"][i], f"step {k}, v[{i}]")
            if zero is not None:
                z = zero[i]
                same_bits(got["p"][i][z], p0[i][z], "a zero-gradient parameter")
                assert not got["m"][i][z].view(np.uint32).any() and not got["v"][i][z].view(np.uint32).any()
        assert got["step"] == st["step"] == step0 + k + 1
        same_bits(got["beta_pow"], st["beta_pow"], f"step {k}, beta_pow")
    return runs[0]


def make_case(sizes, seed, ratio):
    """(p0, grads of STEPS steps, max_grad_norm, zero masks): every third entry has a +0.0 gradient throughout, a -0.0 and
    a +inf parameter among them where the tensor has room"""
    rng = np.random.default_rng(seed)
    p0 = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    zero = [np.arange(n) % 3 == 2 for n in sizes]
    for p, z in zip(p0, zero):
        spots = np.flatnonzero(z)
        if len(spots) >= 2:
            p[spots[0]], p[spots[1]] = -0.0, np.inf
    grads = []
    for _ in range(STEPS):
        g = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 0, n)).astype(np.float32) for n in sizes]
        for x, z in zip(g, zero):
            x[z] = 0.0
        grads.append(g)
    max_norm = None if ratio is None else SR.norm_ref(grads[0]) / ratio
    return p0, grads, max_norm, zero


@pytest.mark.parametrize("clip", list(CLIPS))
@pytest.mark.parametrize("sizes", SETS, ids=["-".join(map(str, s)) for s in SETS])
def test_five_steps_against_the_restatement(eng, sizes, clip):
    p0, grads, max_norm, zero = make_case(sizes, len(sizes) * 100 + sizes[0], CLIPS[clip])
    snaps = check_run(eng, p0, grads, max_norm, zero)
    coef = snaps[0]["norm"][1]
    if clip == "active":
        assert coef == pytest.approx(0.1, rel=1e-4)
    else:
        assert coef == 1.0
    moving = [~z for z in zero]
    if any(m.any() for m in moving):
        assert any(not np.array_equal(s[m], p[m]) for s, p, m in zip(snaps[-1]["p"], p0, moving))


def test_all_zero_gradients_move_nothing(eng):
    p0, grads, _, _ = make_case((63, 65), 4, None)
    grads = [[np.zeros_like(x) for x in g] for g in grads]
    p0[0][:3] = [-0.0, np.inf, -np.inf]
    snaps = check_run(eng, p0, grads, 0.5, [np.ones(63, bool), np.ones(65, bool)])
    assert all(s["norm"].tolist() == [0.0, 1.0] for s in snaps) and snaps[-1]["step"] == STEPS


@pytest.mark.parametrize("steps_before", [1000, 10 ** 6])
def test_a_long_run_s_state(eng, steps_before):
    p0, grads, max_norm, zero = make_case((1023, 1025, 1), 8, 10.0)
    snaps = check_run(eng, p0, grads, max_norm, zero, step0=steps_before, beta_pow0=(B1 ** steps_before, B2 ** steps_before))
    assert snaps[-1]["step"] == steps_before + STEPS
