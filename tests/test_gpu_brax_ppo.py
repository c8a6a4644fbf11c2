"""carl_amd.PPO on a Brax model on the GPU (inverted pendulum: 1 actuator; Reacher: 2): after every update the device
parameters against a host replica -- brax_ppo_ref.py's float64 gradients of the same minibatches in the same order, the
same global-norm clip, torch's CPU Adam -- within the gradient tolerance of test_gpu_brax_ppo_grad.py propagated through
Adam's step (ppo_checks.AdamReplica, which test_gpu_ppo.py shares, here with a log_std vector); the rollout buffer's
context ids and first observation; the transform entries and padding of the packed tensors unchanged bit for bit; the
refusals of the first-state auto-reset, of auto_reset=False and of the engines out of scope."""
import numpy as np
import pytest
import torch

import brax_policy_cases as BPC
import brax_ppo_ref as BR
import brax_sampling_cases as BSC
import ppo_checks as PK
import ppo_ref as R
from carl_amd import PPO, _lib
from carl_amd.brax_policy import BraxMLPPolicy
from ppo_checks import CLIP, ENT, LR, MAX_NORM, VF

pytestmark = pytest.mark.gpu


class Replica(PK.AdamReplica):
    """ppo_checks.AdamReplica on brax_ppo_ref.py's gradients: the actor, the critic and log_std [n_act]"""

    def __init__(self, actor, critic):
        self.templates = (actor, critic)
        super().__init__([actor.params[0], critic.params[0], actor.log_std[0]])

    def policies(self):
        a, c = self.templates
        qa, qc = BraxMLPPolicy.unpack(a, self.params[0].numpy()), BraxMLPPolicy.unpack(c, self.params[1].numpy())
        actor = BraxMLPPolicy(a._info, a.ctx_rows, qa.layers, a.activation, qa.shift, qa.scale, qa.clip,
                              log_std=self.params[2].numpy())
        return actor, qc

    def step(self, table, buf, flat, N):
        actor, critic = self.policies()
        x = R.sample_inputs(actor, table, buf["context_id"], buf["obs0"], buf["obs"], flat, N)
        pick = lambda a: a.reshape(-1)[flat]  # noqa: E731
        adv = torch.tensor(pick(buf["advantage"]))
        norm = np.array([adv.mean().item(), (1.0 / (adv.std() + 1e-8)).item()], np.float32)
        ref = BR.brax_ppo_grad_ref(actor, critic, x, buf["action"].reshape(-1, actor.n_out)[flat], pick(buf["log_prob"]),
                                   pick(buf["advantage"]), pick(buf["return"]), norm, CLIP, VF, ENT)
        g = [ref["grad_actor"], ref["grad_critic"], ref["grad_log_std"]]
        dg = [BR.K * BR.U * ref["S_actor"], BR.K * BR.U * ref["S_critic"], BR.K * BR.U * ref["S_log_std"]]
        self.apply(g, dg)


def networks(eng, seed):
    rng = np.random.default_rng(seed)
    n_act = eng.sys.n_act
    actor = BSC.make_policy(eng, (8, 8), "tanh", seed, (-0.5 + 0.3 * np.arange(n_act)).astype(np.float32))
    critic = BraxMLPPolicy.for_env(eng, BPC.make_layers(rng, 2 + eng.D, (8,), 1), "tanh", actor.shift, actor.scale, actor.clip,
                                   head="value")
    return actor, critic


@pytest.mark.parametrize("model", ["inverted_pendulum", "reacher"])
def test_ppo_updates_match_the_host_replica(model):
    N, T = 64, 8
    eng = BSC.make_engine(model, max(BPC.model_widths(model)), N, "cuda", seed=5, max_episode_steps=3)
    actor, critic = networks(eng, 2)
    ppo = PPO(eng, actor, critic, n_steps=T, n_epochs=2, batch_size=128, lr=LR, clip_range=CLIP, vf_coef=VF, ent_coef=ENT,
              max_grad_norm=MAX_NORM, seed=9)
    assert ppo.brax and tuple(ppo.log_std.shape) == (1, eng.sys.n_act)
    order, start = PK.record(ppo, eng)
    rep = Replica(actor, critic)
    table = eng.ctx_table.cpu().numpy()
    for it in range(2):
        buf = ppo.collect()
        hb = {k: buf[k][:T].cpu().numpy() for k in ("obs", "action", "log_prob", "advantage", "return", "context_id",
                                                     "terminated", "truncated")}
        hb["obs0"] = buf["obs0"].cpu().numpy()
        walk = BR.context_walk(start["ctx"], start["ep"].view(np.uint32), hb["terminated"], hb["truncated"],
                               _lib.SEL_ROUND_ROBIN, 1, BSC.N_CTX, 5, 0, True)
        np.testing.assert_array_equal(hb["context_id"], walk)
        assert (walk != walk[0]).any()
        if it:
            np.testing.assert_array_equal(hb["obs0"], prev_last)
        prev_last = hb["obs"][T - 1].copy()
        order.clear()
        res = ppo.update()
        assert res["stats"].shape == (2 * 4, 6) and res["stats"].is_cuda
        assert sorted(np.concatenate(order[0])) == list(range(T * N))  # a permutation of the dense buffer
        for epoch in order:
            for flat in epoch:
                rep.step(table, hb, flat, N)
        dev = [ppo.actor_params[0], ppo.critic_params[0], ppo.log_std[0]]
        PK.check_against_replica(f"{model}, iteration {it}", dev, rep, ppo, actor, critic)
    got = ppo.actor()
    assert isinstance(got, BraxMLPPolicy) and not np.array_equal(got.params, actor.params)
    np.testing.assert_array_equal(got.log_std, ppo.log_std.cpu().numpy())
    assert not np.array_equal(got.log_std, actor.log_std) and ppo.critic().head == "value"
    info = ppo.learn(1)
    assert len(info) == 1 and info[0]["mean_reward"].is_cuda


def test_ppo_refusals_on_a_brax_engine():
    from carl_amd.mixed import MixedVecEngine

    W = max(BPC.model_widths("inverted_pendulum"))
    eng = BSC.make_engine("inverted_pendulum", W, 64, "cuda", seed=1)
    actor, critic = networks(eng, 0)
    with pytest.raises(ValueError, match="first_state"):
        PPO(BSC.make_engine("inverted_pendulum", W, 64, "cuda", seed=1, autoreset_mode="first_state"), actor, critic)
    with pytest.raises(ValueError, match="auto_reset"):
        PPO(BSC.make_engine("inverted_pendulum", W, 64, "cuda", seed=1, auto_reset=False), actor, critic)
    with pytest.raises(ValueError, match="MixedVecEngine"):
        PPO(object.__new__(MixedVecEngine), actor, critic)
    with pytest.raises(ValueError, match="head='value'"):
        PPO(eng, actor, actor)
    with pytest.raises(ValueError, match="batch_size"):
        PPO(eng, actor, critic, n_steps=4, batch_size=4 * 64 + 1)
    with pytest.raises(RuntimeError, match="collect"):
        PPO(eng, actor, critic).update()
