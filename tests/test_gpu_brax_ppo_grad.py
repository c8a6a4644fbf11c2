"""carl_brax_ppo_grad on the GPU against brax_ppo_ref.py's float64 reference, over brax_ppo_ref.grad_cases(): 1, 2, 3 and
8 actuators, 4 .. 32 inputs (32: Ant's 27 observations with five context inputs), five networks (linear .. 2 x (64, 64)),
the three activations, with and without context inputs and advantage normalisation, M in {1, TS - 1, TS, TS + 1, 2 TS + 3}
as permuted index subsets and every sample (idx NULL), one M just past workgroups_cap x TS (some workgroup runs a second
tile), a distinct log_std per actuator.  The synthetic shapes go through the C entry point directly (it reads obs_dim and
n_act of the model table, nothing else); the engine's method is held by the end-to-end test below.  Per case: new_value
within value_cases.check_values; new_log_prob within ppo_checks.py's Gaussian bound, summed over the actuators; every
gradient entry within K * 2^-24 * S (brax_ppo_ref.py: K = 8 K0, K0 measured on the CPU); the shift | scale | clip entries
and the padding exactly +0.0; two calls bit-identical; a canary behind every output and the workspace; the statistics as
in the classic test.

End to end: one valued launch of a real model, the trace, then ppo_grad(forward=True) over every sample with the unchanged
parameters must reproduce the launch's own value and log_prob columns within those forward bounds, no env-step exempted:
the trace, the obs0 / obs[t - 1] gather and the forward pass against what the rollout kernel itself computed."""
import ctypes as C

import numpy as np
import pytest
import torch

import brax_policy_cases as BPC
import brax_ppo_ref as BR
import brax_sampling_cases as BSC
import ppo_checks as PK
import value_cases as VC
from carl_amd import _lib
from carl_amd.brax_policy import BraxMLPPolicy

pytestmark = pytest.mark.gpu


def log_prob_reference(actor, x, action):
    """(lp64 [M], bound [M]) of the joint Gaussian log-probability of actions [M, n_act] on raw inputs x
    (ppo_checks.gaussian_log_prob_reference on the host reference's means)"""
    _, y64, ybound = BPC.reference_actions(actor, x)
    return PK.gaussian_log_prob_reference(y64, ybound, actor.log_std, action)


def run(case):
    """the case on the GPU, twice (ppo_checks.run_twice)"""
    dev = "cuda"
    lib = _lib.load()
    actor, critic = case["actor"], case["critic"]
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    t = {k: up(case[k]) for k in ("obs0", "obs", "context_id", "action", "log_prob", "advantage", "ret")}
    t["ctx_table"] = up(case["table"])
    t["idx"] = None if case["every"] else up(case["flat"])
    t["adv_norm"] = None if case["adv_norm"] is None else up(case["adv_norm"])
    pa, pc, ls = up(actor.params), up(critic.params), up(actor.log_std)
    pol, crit = actor.struct(case["N"], pa.data_ptr()), critic.struct(case["N"], pc.data_ptr())
    M = case["flat"].size
    sizes = {"grad_actor": actor.set_floats, "grad_critic": critic.set_floats, "grad_log_std": actor.n_out, "stats": 6,
             "new_log_prob": M, "new_value": M}
    need = int(lib.carl_brax_ppo_workspace_floats(C.byref(pol), C.byref(crit), M))
    assert need > 0
    sys_t = BR.fake_sys(case["shape"])
    pb = BR.ppo_batch(case, {k: (None if v is None else v.data_ptr()) for k, v in t.items()})

    def launch(out, ws):
        po = _lib.PpoOut(*(out[k].data_ptr() for k in ("grad_actor", "grad_critic", "grad_log_std", "stats", "new_log_prob",
                                                        "new_value")), ws.data_ptr(), need)
        _lib.check(lib.carl_brax_ppo_grad(C.byref(pb), C.byref(sys_t), C.byref(pol), C.byref(crit), ls.data_ptr(),
                                          C.byref(po), torch.cuda.current_stream().cuda_stream))

    return PK.run_twice(sizes, need, launch, dev)


@pytest.mark.parametrize("spec", BR.grad_cases(), ids=[c[0] for c in BR.grad_cases()])
def test_brax_ppo_grad_against_the_reference(spec):
    lib = _lib.load()
    assert lib.carl_brax_ppo_tile() == BR.TILE and lib.carl_brax_ppo_grad_workgroups(1 << 30) == BR.WORKGROUPS_CAP
    case = BR.make_case(spec)
    ref = BR.case_reference(case)
    BR.assert_conditioned(case, ref)
    actor, critic, x = case["actor"], case["critic"], case["x"]
    M = case["flat"].size
    got = PK.check_canaries_and_bits(run(case))

    # ---- the forward pass, at the tolerances of the closed-loop tests
    VC.check_values(critic, x, got["new_value"])
    a = case["action"].reshape(-1, actor.n_out)[case["flat"]]
    lp64, bound = log_prob_reference(actor, x, a)
    err = PK.check_log_prob(got["new_log_prob"], lp64, bound, ref["new_log_prob"])
    print(f"{case['id']}: largest log-prob error / bound {np.max(err / bound):.3f}")

    # ---- the gradients
    PK.check_transform_entries(got, actor, critic)
    worst = BR.case_k(got, ref)
    print(f"{case['id']}: M = {M}, largest gradient error {worst:.2f} x 2^-24 S (K = {BR.K:.0f})")
    assert worst <= BR.K

    PK.check_statistics(got["stats"], ref["stats"], M)


# ---------------------------------------------------------------- end to end: the launch's own columns
E2E = [("ant", "widest"), ("ant", "narrowest"), ("hopper", "widest")]


@pytest.mark.parametrize("model,which", E2E, ids=[f"{m}-{w}" for m, w in E2E])
def test_forward_reproduces_the_valued_launch(model, which):
    dev = "cuda"
    N, T = 300, 8
    widths = BPC.model_widths(model)
    eng = BSC.make_engine(model, max(widths) if which == "widest" else min(widths), N, dev, seed=5, max_episode_steps=3,
                          selector_stride=2)  # a TimeLimit of 3: every env is truncated twice; the context moves each time
    rng = np.random.default_rng(11)
    n_in = 2 + eng.D
    actor = BSC.make_policy(eng, (64, 64), "tanh", 21, (-0.7 + 0.1 * np.arange(eng.sys.n_act)).astype(np.float32))
    critic = BraxMLPPolicy.for_env(eng, BPC.make_layers(rng, n_in, (32,), 1), "tanh", actor.shift, actor.scale, actor.clip,
                                   head="value")
    obs0 = eng.obs.clone()
    ctx0, ep0 = eng.ctx_idx.clone(), eng.episode.clone()
    buf = eng.rollout_policy(actor, T, deterministic=False, sample_seed=3, value_net=critic, gae=(0.99, 0.95))
    assert int(buf["truncated"][:T].sum()) >= 2 * N
    cid = eng.context_trace(ctx0, ep0, buf["terminated"][:T], buf["truncated"][:T])
    cid_h = cid.cpu().numpy()
    assert (cid_h[0] != cid_h[-1]).any()  # the selector moved
    g = eng.ppo_grad(actor, critic, buf, obs0, cid, forward=True)
    v, lp = g["new_value"].cpu().numpy().reshape(T, N), g["new_log_prob"].cpu().numpy().reshape(T, N)
    v0, lp0 = buf["value"][:T].cpu().numpy(), buf["log_prob"][:T].cpu().numpy()
    eq_v = bool((v.view(np.uint32) == v0.view(np.uint32)).all())
    eq_lp = bool((lp.view(np.uint32) == lp0.view(np.uint32)).all())
    print(f"{model}-{which}: value bit-equal {eq_v} (max |dv| {np.abs(v - v0).max():.3g}), log_prob bit-equal {eq_lp} "
          f"(max |dlp| {np.abs(lp - lp0).max():.3g})")
    # both sides within the host reference's bounds of the same float64 numbers, every env-step
    obs = buf["obs"][:T].cpu().numpy()
    x_obs = np.concatenate([obs0.cpu().numpy()[None], obs[:-1]])
    table = eng.ctx_table.cpu().numpy()  # [F, stride]
    ctx = np.stack([table[r][cid_h] for r in actor.ctx_rows], axis=2)
    x = np.concatenate([ctx, x_obs], axis=2).reshape(T * N, n_in).astype(np.float32)
    VC.check_values(critic, x, v)
    VC.check_values(critic, x, v0)
    lp64, bound = log_prob_reference(actor, x, buf["action"][:T].cpu().numpy())
    for col in (lp, lp0):
        err = np.abs(col.reshape(-1).astype(np.float64) - lp64)
        assert np.all(err <= bound * (1 + 1e-9)), (err.max(), bound[np.argmax(err - bound)])
