"""carl_amd.PPO on the GPU: after every update the device parameters against a host replica -- ppo_ref.py's float64
gradients of the same minibatches in the same order, the same global-norm clip, torch's CPU Adam -- within the gradient
tolerance of test_gpu_ppo_grad.py propagated through Adam's step; the rollout buffer's context ids and first observation;
the refusals for engines out of scope.  No learning-curve threshold here: tools/ppo_update_time.py records one."""
import numpy as np
import pytest
import torch

import policy_cases as PC
import ppo_checks as PK
import ppo_ref as R
import value_cases as VC
from carl_amd import PPO, _lib
from carl_amd.policy import MLPPolicy
from ppo_checks import CLIP, ENT, LR, MAX_NORM, VF

pytestmark = pytest.mark.gpu


class Replica(PK.AdamReplica):
    """ppo_checks.AdamReplica on ppo_ref.py's gradients: the actor, the critic and, for a Box family, log_std [1]"""

    def __init__(self, actor, critic):
        self.templates = (actor, critic)
        self.box = not actor.discrete
        super().__init__([actor.params[0], critic.params[0]] + ([actor.log_std] if self.box else []))

    def policies(self):
        ls = float(self.params[2][0]) if self.box else None
        return (MLPPolicy.unpack(self.templates[0], self.params[0].numpy(), ls),
                MLPPolicy.unpack(self.templates[1], self.params[1].numpy()))

    def step(self, table, buf, flat, P):
        actor, critic = self.policies()
        x = R.sample_inputs(actor, table, buf["context_id"], buf["obs0"], buf["obs"], flat, P)
        pick = lambda a: a.reshape(-1)[flat]  # noqa: E731
        adv = torch.tensor(pick(buf["advantage"]))
        norm = np.array([adv.mean().item(), (1.0 / (adv.std() + 1e-8)).item()], np.float32)
        ref = R.ppo_grad_ref(actor, critic, x, pick(buf["action"]), pick(buf["log_prob"]), pick(buf["advantage"]),
                             pick(buf["return"]), norm, CLIP, VF, ENT)
        g = [ref["grad_actor"], ref["grad_critic"]] + ([np.array([ref["grad_log_std"]])] if self.box else [])
        dg = [R.K * R.U * ref["S_actor"], R.K * R.U * ref["S_critic"]] + ([np.array([R.K * R.U * ref["S_log_std"]])] if self.box else [])
        self.apply(g, dg)


def host(buf, T):
    keys = ("obs", "action", "log_prob", "advantage", "return", "context_id", "terminated", "truncated")
    out = {}
    for k in keys:
        t = buf[k][:T]
        P = t.stride(0) // (t.shape[2] if t.dim() == 3 else 1) if T > 1 else t.shape[1]
        full = torch.as_strided(t, (T, P) + tuple(t.shape[2:]), t.stride())  # the padded rows, as the flat indices address them
        out[k] = full.cpu().numpy()
    out["obs0"] = buf["obs0"].cpu().numpy()
    return out, P


@pytest.mark.parametrize("family", [_lib.CARTPOLE, _lib.PENDULUM], ids=["cartpole", "pendulum"])
def test_ppo_updates_match_the_host_replica(family):
    N, T = 256, 32
    eng = PC.make_engine(family, N, _lib.SEL_ROUND_ROBIN, n_contexts=7, seed=5, max_episode_steps=20)
    rng = np.random.default_rng(2)
    box = not eng.info.action_is_discrete
    actor = PC.make_policy(eng, (8, 8), "tanh", rng, ctx="all", clip=5.0, log_std=-0.5 if box else None)
    critic = VC.make_critic(eng, actor, (8,), "tanh", rng)
    ppo = PPO(eng, actor, critic, n_steps=T, n_epochs=2, batch_size=2048, lr=LR, clip_range=CLIP, vf_coef=VF, ent_coef=ENT,
              max_grad_norm=MAX_NORM, seed=9)
    order, start = PK.record(ppo, eng)
    rep = Replica(actor, critic)
    table = eng.ctx_table.cpu().numpy()
    for it in range(2):
        buf = ppo.collect()
        ctx0, ep0 = start["ctx"], start["ep"]
        hb, P = host(buf, T)
        # the buffer: the context walk, and the observation step 0 was chosen from
        walk = R.context_walk(ctx0, ep0, hb["terminated"][:, :N], hb["truncated"][:, :N], _lib.SEL_ROUND_ROBIN, 1, 7, 5, 0, True)
        np.testing.assert_array_equal(hb["context_id"][:, :N], walk)
        assert (walk != walk[0]).any()
        if it:
            np.testing.assert_array_equal(hb["obs0"], prev_last)
        prev_last = hb["obs"][T - 1, :N].copy()
        order.clear()
        res = ppo.update()
        assert res["stats"].shape == (2 * 4, 6) and res["stats"].is_cuda
        assert sorted(np.concatenate(order[0]) % P + np.concatenate(order[0]) // P * N) == list(range(T * N))  # a permutation
        for epoch in order:
            for flat in epoch:
                rep.step(table, hb, flat, P)
        dev = [ppo.actor_params[0], ppo.critic_params[0]] + ([ppo.log_std] if box else [])
        PK.check_against_replica(f"iteration {it}", dev, rep, ppo, actor, critic)
    # the parameters moved, and come back as host policies
    assert not np.array_equal(ppo.actor().params, actor.params) and ppo.critic().head == "value"
    info = ppo.learn(1)
    assert len(info) == 1 and info[0]["mean_reward"].is_cuda


def test_ppo_refuses_engines_out_of_scope():
    from carl_amd.brax_engine import BraxVecEngine
    from carl_amd.mixed import MixedVecEngine

    eng = PC.make_engine(_lib.CARTPOLE, 256, n_contexts=4)
    rng = np.random.default_rng(0)
    actor = PC.make_policy(eng, (4,), "tanh", rng)
    critic = VC.make_critic(eng, actor, (4,), "tanh", rng)
    with pytest.raises(TypeError, match="classic-control families only"):
        PPO(object.__new__(BraxVecEngine), actor, critic)
    with pytest.raises(TypeError, match="out of scope"):
        PPO(object.__new__(MixedVecEngine), actor, critic)
    with pytest.raises(ValueError, match="head='value'"):
        PPO(eng, actor, actor)
    with pytest.raises(ValueError, match="batch_size"):
        PPO(eng, actor, critic, n_steps=4, batch_size=4 * 256 + 1)
    with pytest.raises(ValueError, match="auto_reset"):
        PPO(PC.make_engine(_lib.CARTPOLE, 256, n_contexts=4, auto_reset=False), actor, critic)
    with pytest.raises(RuntimeError, match="collect"):
        PPO(eng, actor, critic).update()


def test_learn_does_not_synchronise_with_the_host():
    probe = torch.zeros(1, device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            supported = False
        except RuntimeError:
            supported = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not supported:
        pytest.skip("this torch build does not report synchronising calls under set_sync_debug_mode('error') on ROCm")
    for family in (_lib.CARTPOLE, _lib.PENDULUM):
        eng = PC.make_engine(family, 272, n_contexts=7, max_episode_steps=20)
        rng = np.random.default_rng(1)
        actor = PC.make_policy(eng, (8,), "tanh", rng, clip=5.0, log_std=None if eng.info.action_is_discrete else 0.0)
        critic = VC.make_critic(eng, actor, (8,), "relu", rng)
        ppo = PPO(eng, actor, critic, n_steps=8, n_epochs=2, batch_size=1000)  # (a last, shorter minibatch per epoch)
        ppo.learn(1)  # warm-up: first uploads, code objects, Adam's state
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            info = ppo.learn(2)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert len(info) == 2 and bool(torch.isfinite(info[1]["stats"]).all())
