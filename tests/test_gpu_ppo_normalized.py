"""carl_amd.PPO with normalize_inputs and normalize_reward on the GPU: CartPole, Pendulum and Brax Hopper at 300 lanes,
T = 8, two iterations, against a host replica -- ppo_checks.AdamReplica on the float64 reference gradients (ppo_ref.py,
brax_ppo_ref.py) plus ppo_norm_ref.py's restatements of the return walk, its merge, the scaled rewards, GAE and the input
merge.  Per iteration:
  - the return walk: the persistent return bit for bit, the running statistics and the scale against the same operations;
    ``reward_normalized`` bit for bit from the device's scale; the advantages within a bound derived below; ``reward`` raw;
  - the update of iteration k runs under the transform collection k ran: every ``ppo_grad`` call of ``update()`` sees the
    section ``collect()`` ran, ``ppo_grad(forward=True)`` under it reproduces the buffer's values (value_cases.check_values
    holds both to the exact reference), and the section changes exactly once per iteration, after the last minibatch;
  - the merged section against ppo_norm_ref.merge_ref of the device's own slabs, the critic's equal to the actor's;
  - the weights within the replica's bounds.
The advantages' bound: carl_gae adds T = 8 terms per chain in fp32, each of magnitude at most M = max(|r| + |v| + |v'|) +
max |A|, one rounding per operation and four operations per step (gamma and lambda are dyadic, so the device's fp32
coefficients are the reference's): |A_dev - A_64| <= 4 T 2^-24 M."""
import numpy as np
import pytest
import torch

import brax_policy_cases as BPC
import brax_ppo_ref as BR
import brax_sampling_cases as BSC
import policy_cases as PC
import ppo_checks as PK
import ppo_norm_ref as NR
import ppo_ref as R
import value_cases as VC
from carl_amd import PPO, _lib
from carl_amd.brax_policy import BraxMLPPolicy
from carl_amd.policy import MLPPolicy
from ppo_checks import CLIP, ENT, LR, MAX_NORM, VF

pytestmark = pytest.mark.gpu

N, T, GAMMA, LAM, CLIP_REWARD, EPS = 300, 8, 0.96875, 0.875, 2.0, 1e-8  # (gamma, lambda and their product exact in fp32)


class Replica(PK.AdamReplica):
    """ppo_checks.AdamReplica on the reference gradients of either engine; the packed tensors carry the transform, which
    the test overwrites with the device's after each merge"""

    def __init__(self, actor, critic, brax):
        self.templates, self.brax, self.box = (actor, critic), brax, brax or not actor.discrete
        ls = actor.log_std[0] if brax else actor.log_std
        super().__init__([actor.params[0], critic.params[0]] + ([ls] if self.box else []))

    def policies(self):
        a, c = self.templates
        if self.brax:
            qa, qc = BraxMLPPolicy.unpack(a, self.params[0].numpy()), BraxMLPPolicy.unpack(c, self.params[1].numpy())
            return BraxMLPPolicy(a._info, a.ctx_rows, qa.layers, a.activation, qa.shift, qa.scale, qa.clip,
                                 log_std=self.params[2].numpy()), qc
        ls = float(self.params[2][0]) if self.box else None
        return MLPPolicy.unpack(a, self.params[0].numpy(), ls), MLPPolicy.unpack(c, self.params[1].numpy())

    def step(self, table, buf, flat, P):
        actor, critic = self.policies()
        x = R.sample_inputs(actor, table, buf["context_id"], buf["obs0"], buf["obs"], flat, P)
        pick = lambda a: a.reshape(-1)[flat]  # noqa: E731
        adv = torch.tensor(pick(buf["advantage"]))
        norm = np.array([adv.mean().item(), (1.0 / (adv.std() + 1e-8)).item()], np.float32)
        if self.brax:
            ref = BR.brax_ppo_grad_ref(actor, critic, x, buf["action"].reshape(-1, actor.n_out)[flat], pick(buf["log_prob"]),
                                       pick(buf["advantage"]), pick(buf["return"]), norm, CLIP, VF, ENT)
            K, g_ls, s_ls = BR.K * BR.U, ref["grad_log_std"], ref["S_log_std"]
        else:
            ref = R.ppo_grad_ref(actor, critic, x, pick(buf["action"]), pick(buf["log_prob"]), pick(buf["advantage"]),
                                 pick(buf["return"]), norm, CLIP, VF, ENT)
            K, g_ls, s_ls = R.K * R.U, np.array([ref["grad_log_std"]]), np.array([ref["S_log_std"]])
        g = [ref["grad_actor"], ref["grad_critic"]] + ([g_ls] if self.box else [])
        dg = [K * ref["S_actor"], K * ref["S_critic"]] + ([K * s_ls] if self.box else [])
        self.apply(g, dg)


def setup(kind):
    rng = np.random.default_rng(2)
    if kind == "hopper":
        eng = BSC.make_engine(kind, max(BPC.model_widths(kind)), N, "cuda", seed=5, max_episode_steps=3, selector_stride=2)
        n_act = eng.sys.n_act
        actor = BSC.make_policy(eng, (8, 8), "tanh", 2, (-0.5 + 0.3 * np.arange(n_act)).astype(np.float32))
        critic = BraxMLPPolicy.for_env(eng, BPC.make_layers(rng, 2 + eng.D, (8,), 1), "tanh", actor.shift, actor.scale,
                                       actor.clip, head="value")
        return eng, actor, critic, True
    fam = {"cartpole": _lib.CARTPOLE, "pendulum": _lib.PENDULUM}[kind]
    eng = PC.make_engine(fam, N, _lib.SEL_ROUND_ROBIN, n_contexts=7, seed=5, max_episode_steps=3, selector_stride=2)
    box = not eng.info.action_is_discrete
    actor = PC.make_policy(eng, (8, 8), "tanh", rng, ctx="all", clip=5.0, log_std=-0.5 if box else None)
    critic = VC.make_critic(eng, actor, (8,), "tanh", rng)
    return eng, actor, critic, False


def host(buf, brax):
    """the buffer's columns as the flat indices address them (the padded rows of a classic buffer) -> (arrays, pitch)"""
    out, P = {}, N
    for k in ("obs", "action", "log_prob", "advantage", "return", "context_id", "terminated", "truncated", "reward",
              "reward_normalized", "value", "boot_value"):
        t = buf[k][:T]
        if not brax:
            P = t.stride(0) // (t.shape[2] if t.dim() == 3 else 1)
            t = torch.as_strided(t, (T, P) + tuple(t.shape[2:]), t.stride())
        out[k] = t.cpu().numpy()
    out["obs0"], out["last_value"] = buf["obs0"].cpu().numpy(), buf["last_value"].cpu().numpy()
    return out, P


def section(ppo, which):
    params = ppo.actor_params if which == 0 else ppo.critic_params
    w = ppo._templates[which].weight_floats
    return params[0, w: w + 2 * ppo._templates[which].n_in + 1].cpu().numpy().view(np.uint32).copy()


@pytest.mark.parametrize("kind", ["cartpole", "pendulum", "hopper"])
def test_normalized_ppo_matches_the_host_replica(kind):
    eng, actor, critic, brax = setup(kind)
    n_in = actor.n_in
    ppo = PPO(eng, actor, critic, n_steps=T, n_epochs=2, batch_size=600, lr=LR, gamma=GAMMA, lam=LAM, clip_range=CLIP,
              vf_coef=VF, ent_coef=ENT, max_grad_norm=MAX_NORM, seed=9, normalize_inputs=True, normalize_reward=True,
              clip_reward=CLIP_REWARD, norm_eps=EPS)
    order, _ = PK.record(ppo, eng)
    rep = Replica(actor, critic, brax)
    table = eng.ctx_table.cpu().numpy()
    seen, grad = [], eng.ppo_grad

    def recording_grad(*a, **kw):  # the section every ppo_grad of update() runs under
        seen.append(section(ppo, 0))
        return grad(*a, **kw)

    eng.ppo_grad = recording_grad
    ret_ref, ret_state, in_state, dev_state = np.zeros(N, np.float32), None, None, None
    for it in range(2):
        before = section(ppo, 0)
        buf = ppo.collect()
        ran = section(ppo, 0)
        np.testing.assert_array_equal(ran, before)  # an update came between: collect() merges nothing
        hb, P = host(buf, brax)
        lanes = slice(0, N)
        # ---- rewards: the walk, its merge, the scale, the scaled rewards, the advantages
        rew, te, tr = hb["reward"][:, lanes], hb["terminated"][:, lanes], hb["truncated"][:, lanes]
        rows, ret_ref, S1, S2, _ = NR.return_walk_ref(rew, te, tr, ret_ref, GAMMA)
        ret_state, scale_ref = NR.return_merge_ref(S1, S2, T * N, ret_state, EPS)
        rs = ppo.return_stats
        np.testing.assert_array_equal(rs["ret"].cpu().numpy().view(np.uint32), ret_ref.view(np.uint32))
        assert int(rs["count"].cpu()) == ret_state[0] == (it + 1) * T * N
        # (the device adds its slabs in another order than fsum: mean and M2 to the sums' bound, far inside 1e-9)
        np.testing.assert_allclose(rs["mean"].cpu().numpy()[0], ret_state[1], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(rs["m2"].cpu().numpy()[0], ret_state[2], rtol=1e-9, atol=1e-12)
        scale = rs["scale"].cpu().numpy()[0]
        np.testing.assert_allclose(scale, scale_ref, rtol=2.0 ** -22)
        rn = NR.normalized_reward_ref(rew, scale, CLIP_REWARD)
        np.testing.assert_array_equal(hb["reward_normalized"][:, lanes].view(np.uint32), rn.view(np.uint32))
        assert np.abs(rn).max() <= CLIP_REWARD and "reward_normalized" in buf
        np.testing.assert_array_equal(buf["reward"][:T].cpu().numpy(), rew)  # raw
        adv64, ret64 = NR.gae_ref(rn, hb["value"][:, lanes], hb["boot_value"][:, lanes], hb["last_value"], te, tr, GAMMA, LAM)
        M = (np.abs(rn) + 2 * max(np.abs(hb["value"][:, lanes]).max(), np.abs(hb["last_value"]).max(),
                                  np.abs(hb["boot_value"][:, lanes]).max())).max() + np.abs(adv64).max()
        tol = 4 * T * 2.0 ** -24 * M
        err_a = np.abs(hb["advantage"][:, lanes] - adv64).max()
        err_r = np.abs(hb["return"][:, lanes] - ret64).max()
        print(f"{kind} iteration {it}: scale {scale:.6g}, advantage |err| {err_a:.3e}, return |err| {err_r:.3e}, bound {tol:.3e}")
        assert err_a <= tol and err_r <= tol + 2.0 ** -24 * np.abs(ret64).max()
        # ---- the buffer was computed under the section the collection ran: forward under it gives the buffer's values
        a_k, c_k = ppo.actor(), ppo.critic()
        g = eng.ppo_grad(a_k, c_k, buf, buf["obs0"], buf["context_id"], forward=True)
        seen.clear()
        x = NR.gathered_inputs(a_k, table, hb["context_id"], hb["obs0"], hb["obs"], N, P)
        VC.check_values(c_k, x, g["new_value"].cpu().numpy())
        VC.check_values(c_k, x, hb["value"][:, lanes])
        # ---- the input sums of this collection, merged by the reference from the template's / the previous shift
        S1i, S2i, _, _ = NR.input_sums_ref(x, a_k.shift)
        in_state, sh, sc = NR.merge_ref(S1i, S2i, T * N, a_k.shift, in_state, EPS, ppo.input_stats.min_std)
        # ... and by the same operations from the device's own slabs (the launch's bits: two calls give the same), in order
        slabs = eng.ppo_input_stats(a_k, buf, buf["obs0"], buf["context_id"])["input_partial"].cpu().numpy()
        dev_state, sh_d, sc_d = NR.merge_ref(*NR.slabs_in_order(slabs, n_in), T * N, a_k.shift, dev_state, EPS,
                                             ppo.input_stats.min_std)
        # ---- the update: every minibatch under the collection's section, the merge after the last one, once
        order.clear()
        ppo.update()
        assert len(seen) == 2 * 4
        for s in seen:
            np.testing.assert_array_equal(s, ran)
        after = section(ppo, 0)
        assert not np.array_equal(after, ran)
        np.testing.assert_array_equal(section(ppo, 1), after)  # the critic's section is the actor's
        assert int(ppo.input_stats.count.cpu()) == (it + 1) * T * N
        got = ppo.actor()
        scale_tol = 2.0 ** -22 + 1e-6  # (the reference sums are fsum's, the device's are its chains': far inside 1e-6)
        np.testing.assert_allclose(got.shift, sh, rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(got.scale, sc, rtol=scale_tol, atol=0)
        assert got.clip == actor.clip
        np.testing.assert_allclose(ppo.input_stats.mean.cpu().numpy(), in_state[1], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(ppo.input_stats.mean.cpu().numpy(), dev_state[1], rtol=1e-12, atol=0)
        NR.check_merged_transform(f"{kind} iteration {it}", got.shift, got.scale, dev_state, sh_d, sc_d, EPS,
                                  ppo.input_stats.min_std)
        # ---- the weights, against the replica stepping the same minibatches in the same order
        for epoch in order:
            for flat in epoch:
                rep.step(table, hb, flat, P)
        dev = [ppo.actor_params[0], ppo.critic_params[0]] + ([ppo.log_std[0] if brax else ppo.log_std] if rep.box else [])
        for i, (d, pol) in enumerate(zip(dev, (actor, critic, None))):
            w = d.numel() if pol is None else pol.weight_floats
            diff = np.abs(d.cpu().numpy().astype(np.float64) - rep.params[i].numpy().astype(np.float64))[:w]
            bound = rep.bound(i)[:w]
            print(f"{kind} iteration {it}, tensor {i}: largest difference / bound {np.max(diff / np.maximum(bound, 1e-300)):.3e}")
            assert np.all(diff <= bound)
        # the replica's next iteration runs under the device's merged transform (checked above), bit for bit
        with torch.no_grad():
            for i, pol in enumerate((actor, critic)):
                w = pol.weight_floats
                rep.params[i][w: w + 2 * n_in] = torch.tensor(after.view(np.float32)[: 2 * n_in])
                # (the padding and the clip keep their bits on the device)
                np.testing.assert_array_equal(dev[i].cpu().numpy()[w + 2 * n_in:].view(np.uint32),
                                              pol.params[0][w + 2 * n_in:].view(np.uint32))
    info = ppo.learn(1)
    assert info[0]["mean_reward"].is_cuda and bool(torch.isfinite(info[0]["stats"]).all())


def test_a_collection_without_an_update_is_merged_once_by_the_next():
    eng, actor, critic, _ = setup("cartpole")
    ppo = PPO(eng, actor, critic, n_steps=T, normalize_inputs=True)
    first = section(ppo, 0)
    ppo.collect()
    np.testing.assert_array_equal(section(ppo, 0), first)
    buf = ppo.collect()  # merges the first collection's sums, then runs under them
    second = section(ppo, 0)
    assert not np.array_equal(second, first) and int(ppo.input_stats.count.cpu()) == T * N
    np.testing.assert_array_equal(section(ppo, 1), second)
    ppo.update()   # merges the second collection's, after its minibatches
    assert int(ppo.input_stats.count.cpu()) == 2 * T * N and not np.array_equal(section(ppo, 0), second)
    third = section(ppo, 0)
    with pytest.raises(RuntimeError, match="updated on once"):  # the buffer was computed under the section before the merge
        ppo.update()
    np.testing.assert_array_equal(section(ppo, 0), third)
    assert int(ppo.input_stats.count.cpu()) == 2 * T * N and "reward_normalized" not in buf


def test_with_both_flags_off_collect_adds_no_keys():
    eng, actor, critic, _ = setup("pendulum")
    plain = PPO(eng, actor, critic, n_steps=T, seed=4)
    keys = set(plain.collect())
    eng2, actor2, critic2, _ = setup("pendulum")
    both = PPO(eng2, actor2, critic2, n_steps=T, seed=4, normalize_inputs=True, normalize_reward=True)
    assert set(both.collect()) - keys == {"reward_normalized"}
    assert plain.input_stats is None and plain.return_stats is None
    # the same engine state, seed and (so far unchanged) transform: the launch's own columns are the same bits
    for k in ("obs", "action", "reward", "log_prob", "value", "context_id"):
        np.testing.assert_array_equal(plain._buf[k][:T].cpu().numpy(), both._buf[k][:T].cpu().numpy())
