"""carl_amd.PPO on a Brax model on the GPU (inverted pendulum: 1 actuator; Reacher: 2): after every update the device
parameters against a host replica -- brax_ppo_ref.py's float64 gradients of the same minibatches in the same order, the
same global-norm clip, torch's CPU Adam -- within the gradient tolerance of test_gpu_brax_ppo_grad.py propagated through
Adam's step (the bound test_gpu_ppo.py derives, restated in Replica below for a log_std vector); the rollout buffer's
context ids and first observation; the transform entries and padding of the packed tensors unchanged bit for bit; the
refusals of the first-state auto-reset, of auto_reset=False and of the engines out of scope."""
import numpy as np
import pytest
import torch

import brax_policy_cases as BPC
import brax_ppo_ref as BR
import brax_sampling_cases as BSC
import ppo_ref as R
from carl_amd import PPO, _lib
from carl_amd.brax_policy import BraxMLPPolicy

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 3e-4, 0.9, 0.999, 1e-5
CLIP, VF, ENT, MAX_NORM = 0.2, 0.5, 0.01, 0.5


class Replica:
    """The host side of one PPO run: packed float32 parameters (actor, critic, log_std [n_act]) under torch's CPU Adam,
    and next to them a bound on how far the device's parameters may be from them.

    The bound is test_gpu_ppo.py's.  The device's gradient entry differs from the reference's by at most dg = K 2^-24 S
    (brax_ppo_ref.py).  The clip multiplies by coef = min(1, max_norm / (|g| + 1e-6)), whose relative error is at most
    |dg|_2 / |g|_2.  Adam keeps m = b1 m + (1 - b1) g and v = b2 v + (1 - b2) g^2, so their errors obey
    em = b1 em + (1 - b1) dg and ev = b2 ev + (1 - b2) (2 |g| dg + dg^2); with the bias corrections the step is
    lr * mh / (sqrt(vh) + eps), whose error is at most lr * (emh / D + |mh| ds / (D_ref D)), ds = min(sqrt(evh),
    evh / sqrt(vh)) the error of sqrt(vh) and D = max(D_ref - ds, eps) the smallest denominator the device can have; never
    more than lr * 2 / sqrt(1 - b2).  The per-step errors add up over the steps; the total is doubled for the second-order
    effect of the parameters' own difference on later gradients, and 4 roundings of the parameter are added."""

    def __init__(self, actor, critic):
        self.templates = (actor, critic)
        self.params = [torch.tensor(actor.params[0].copy()), torch.tensor(critic.params[0].copy()),
                       torch.tensor(actor.log_std[0].copy())]
        self.opt = torch.optim.Adam(self.params, lr=LR, eps=EPS)
        self.em = [np.zeros(p.numel()) for p in self.params]
        self.ev = [np.zeros(p.numel()) for p in self.params]
        self.err = [np.zeros(p.numel()) for p in self.params]
        self.steps = 0

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
        return 2 * self.err[i] + 4 * BR.U * np.abs(self.params[i].numpy().astype(np.float64))


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
    order, draw = [], ppo.minibatches

    def recording():
        mbs = draw()
        order.append([m.cpu().numpy().astype(np.int64) for m in mbs])
        return mbs

    ppo.minibatches = recording
    start, roll = {}, eng.rollout_policy

    def recording_rollout(*a, **kw):  # ctx_idx / episode right before the launch (the first collect() resets the engine)
        start["ctx"], start["ep"] = eng.ctx_idx.cpu().numpy(), eng.episode.cpu().numpy().view(np.uint32)
        return roll(*a, **kw)

    eng.rollout_policy = recording_rollout
    rep = Replica(actor, critic)
    table = eng.ctx_table.cpu().numpy()
    for it in range(2):
        buf = ppo.collect()
        hb = {k: buf[k][:T].cpu().numpy() for k in ("obs", "action", "log_prob", "advantage", "return", "context_id",
                                                     "terminated", "truncated")}
        hb["obs0"] = buf["obs0"].cpu().numpy()
        walk = BR.context_walk(start["ctx"], start["ep"], hb["terminated"], hb["truncated"], _lib.SEL_ROUND_ROBIN, 1,
                               BSC.N_CTX, 5, 0, True)
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
        for i, d in enumerate(dev):
            diff = np.abs(d.cpu().numpy().astype(np.float64) - rep.params[i].numpy().astype(np.float64))
            bound = rep.bound(i)
            print(f"{model}, iteration {it}, tensor {i}: largest difference {diff.max():.3e}, bound there "
                  f"{bound[np.argmax(diff)]:.3e}, largest difference / bound {np.max(diff / np.maximum(bound, 1e-300)):.3e}")
            assert np.all(diff <= bound)
        for d, pol in ((ppo.actor_params[0], actor), (ppo.critic_params[0], critic)):
            np.testing.assert_array_equal(d.cpu().numpy()[pol.weight_floats:].view(np.uint32),
                                          pol.params[0][pol.weight_floats:].view(np.uint32))
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
