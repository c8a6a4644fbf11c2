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

import ppo_checks as PK
import ppo_ref as R
import sampling_ref as SR
import value_cases as VC
from carl_amd import _lib
from carl_amd.engine import VecEngine
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def run(case):
    """the case on the GPU, twice (ppo_checks.run_twice)"""
    dev = "cuda"
    N = case["N"]
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

    def launch(out, ws):
        eng.ppo_grad(case["actor"], case["critic"], buf, up(case["obs0"]), cid, idx=None if case["every"] else up(case["flat"]),
                     adv_norm=None if case["adv_norm"] is None else up(case["adv_norm"]), clip_range=R.CLIP, vf_coef=R.VF,
                     ent_coef=R.ENT, forward=True, out=out, workspace=ws)

    return PK.run_twice(sizes, need, launch, dev)


@pytest.mark.parametrize("spec", R.grad_cases(), ids=[c[0] for c in R.grad_cases()])
def test_ppo_grad_against_the_reference(spec):
    lib = _lib.load()
    assert lib.carl_ppo_tile() == R.TILE and lib.carl_ppo_grad_workgroups(1 << 30) == R.WORKGROUPS_CAP
    case = R.make_case(spec)
    ref = R.case_reference(case)
    R.assert_conditioned(case, ref)
    actor, critic, x = case["actor"], case["critic"], case["x"]
    M = case["flat"].size
    got = PK.check_canaries_and_bits(run(case))

    # ---- the forward pass, at the tolerances of the closed-loop tests
    VC.check_values(critic, x, got["new_value"])
    fwd = O.policy_forward(actor.params, actor.n_in, actor.widths, actor.n_out, actor.activation, x)
    a = case["action"].reshape(-1)[case["flat"]]
    if actor.discrete:
        lp64 = SR.categorical_log_prob64(fwd.y64, a)
        bound = SR.categorical_log_prob_bound(fwd.y64, fwd.bound, a)
    else:
        lp64, bound = PK.gaussian_log_prob_reference(fwd.y64[:, :1], fwd.bound[:, :1], actor.log_std[:1], a)
    PK.check_log_prob(got["new_log_prob"], lp64, bound, ref["new_log_prob"])

    # ---- the gradients
    PK.check_transform_entries(got, actor, critic)
    worst = 0.0
    for name in ("actor", "critic"):
        worst = max(worst, R.grad_error_units(got["grad_" + name], ref["grad_" + name], ref["S_" + name]).max())
    if not actor.discrete:
        worst = max(worst, abs(float(got["grad_log_std"][0]) - float(ref["grad_log_std"])) / (R.U * ref["S_log_std"]))
    print(f"{case['id']}: M = {M}, largest gradient error {worst:.2f} x 2^-24 S (K = {R.K:.0f})")
    assert worst <= R.K

    PK.check_statistics(got["stats"], ref["stats"], M)
