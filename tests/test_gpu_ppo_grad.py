"""carl_ppo_grad on the GPU against ppo_ref.py's float64 reference, over ppo_ref.grad_cases(): four families (D = 4, 2,
6, 3; 2 / 3 actions and Box) x five networks (linear .. 2 x (64, 64)), with and without context inputs, the three
activations, M in {1, TS - 1, TS, TS + 1, 2 TS + 3} as permuted index subsets and every sample (idx NULL), one M just past
workgroups_cap x TS (some workgroup runs a second tile), 272 lanes (dense rows) and 260 (rows of carl_rollout_pitch).
Per case: new_log_prob / new_value against the forward references of the closed-loop tests at their tolerances; every
gradient entry within K * 2^-24 * S of the reference (ppo_ref.py: K = 8 K0, K0 measured on the CPU); the shift | scale |
clip entries and the padding exactly +0.0; two calls bit-identical; a canary behind every output."""
import numpy as np
import pytest
import torch

import ppo_ref as R
import sampling_ref as SR
import value_cases as VC
from carl_amd import _lib
from carl_amd.engine import VecEngine
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CANARY = 7.25
OUTPUTS = ("grad_actor", "grad_critic", "grad_log_std", "stats", "new_log_prob", "new_value")


def run(case):
    """the case on the GPU, twice -> (outputs as NumPy arrays, second call's outputs, what lies behind each output)"""
    dev = "cuda"
    N, P, T = case["N"], case["P"], case["T"]
    eng = VecEngine(case["family"], case["table"].T.astype(np.float64), N, dev)
    up = lambda a: torch.as_tensor(a).to(dev)  # noqa: E731
    buf = {k: up(case[src])[:, :N] for k, src in (("action", "action"), ("log_prob", "log_prob"), ("advantage", "advantage"),
                                                  ("return", "ret"), ("obs", "obs"))}
    cid = up(case["context_id"])[:, :N]
    M = case["flat"].size
    sizes = {"grad_actor": case["actor"].set_floats, "grad_critic": case["critic"].set_floats, "grad_log_std": 1, "stats": 6,
             "new_log_prob": M, "new_value": M}
    if case["actor"].discrete:
        del sizes["grad_log_std"]
    need = eng.ppo_workspace(case["actor"], case["critic"], M).numel()
    results = []
    for _ in range(2):
        big = {k: torch.full((n + 16,), CANARY, dtype=torch.float32, device=dev) for k, n in sizes.items()}
        ws = torch.full((need + 16,), CANARY, dtype=torch.float32, device=dev)
        out = {k: big[k][:n] for k, n in sizes.items()}
        eng.ppo_grad(case["actor"], case["critic"], buf, up(case["obs0"]), cid, idx=None if case["every"] else up(case["flat"]),
                     adv_norm=None if case["adv_norm"] is None else up(case["adv_norm"]), clip_range=R.CLIP, vf_coef=R.VF,
                     ent_coef=R.ENT, forward=True, out=out, workspace=ws[:need])
        results.append(({k: out[k].cpu().numpy() for k in sizes},
                        {**{k: big[k][n:].cpu().numpy() for k, n in sizes.items()}, "workspace": ws[need:].cpu().numpy()}))
    return results


@pytest.mark.parametrize("spec", R.grad_cases(), ids=[c[0] for c in R.grad_cases()])
def test_ppo_grad_against_the_reference(spec):
    lib = _lib.load()
    assert lib.carl_ppo_tile() == R.TILE and lib.carl_ppo_grad_workgroups(1 << 30) == R.WORKGROUPS_CAP
    case = R.make_case(spec)
    ref = R.case_reference(case)
    R.assert_conditioned(case, ref)
    actor, critic, x = case["actor"], case["critic"], case["x"]
    M = case["flat"].size
    (got, tail), (again, tail2) = run(case)
    # a canary behind every output, and the same bits twice
    for t in (tail, tail2):
        for k, v in t.items():
            assert (v == CANARY).all(), k
    for k in got:
        np.testing.assert_array_equal(got[k].view(np.uint32), again[k].view(np.uint32), err_msg=k)

    # ---- the forward pass, at the tolerances of the closed-loop tests
    VC.check_values(critic, x, got["new_value"])
    fwd = O.policy_forward(actor.params, actor.n_in, actor.widths, actor.n_out, actor.activation, x)
    a = case["action"].reshape(-1)[case["flat"]]
    if actor.discrete:
        lp64 = SR.categorical_log_prob64(fwd.y64, a)
        bound = SR.categorical_log_prob_bound(fwd.y64, fwd.bound, a)
    else:
        # z = (a - mu) * exp(-log_std) in fp32: the forward bound on mu and the roundings of the subtraction, of expf and
        # of the product; then fma(-z / 2, z, lp0) as the rollout's log-probability (sampling_ref.gaussian_log_prob_bound)
        ls = float(actor.log_std[0])
        mu = fwd.y64[:, 0]
        z = (a.astype(np.float64) - mu) * np.exp(-ls)
        dz = (fwd.bound[:, 0] + 4 * SR.ULP * (np.abs(a) + np.abs(mu))) * np.exp(-ls) + 4 * SR.ULP * np.abs(z)
        lp64 = SR.gaussian_log_prob64(z, ls)
        bound = np.abs(z) * dz + dz * dz + 4 * SR.ULP * (abs(ls) + 2 + np.abs(lp64))
    err = np.abs(got["new_log_prob"].astype(np.float64) - lp64)
    assert np.all(err <= bound * (1 + 1e-9)), (err.max(), bound[np.argmax(err - bound)])
    np.testing.assert_allclose(lp64, ref["new_log_prob"], rtol=0, atol=1e-9 * (1 + np.abs(lp64).max()))

    # ---- the gradients
    worst = 0.0
    for name, pol in (("actor", actor), ("critic", critic)):
        g = got["grad_" + name]
        assert not g[pol.weight_floats:].view(np.uint32).any(), name  # shift | scale | clip | padding: +0.0 bits
        units = R.grad_error_units(g, ref["grad_" + name], ref["S_" + name])
        worst = max(worst, units.max())
    if not actor.discrete:
        worst = max(worst, abs(float(got["grad_log_std"][0]) - float(ref["grad_log_std"])) / (R.U * ref["S_log_std"]))
    print(f"{case['id']}: M = {M}, largest gradient error {worst:.2f} x 2^-24 S (K = {R.K:.0f})")
    assert worst <= R.K

    # ---- the statistics: means of per-sample fp32 terms, each within a few 1e-6 relative of its float64 value (the
    # log-probability bound above, through exp), accumulated in float64
    s = got["stats"].astype(np.float64)
    assert s[5] == M
    np.testing.assert_allclose(s[:4], ref["stats"][:4], rtol=2e-5, atol=2e-5)
    assert s[4] == pytest.approx(ref["stats"][4], abs=0.5 / M + 1e-6)  # ratios are 0.01 away from 1 +- clip: the same count
