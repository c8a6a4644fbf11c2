"""carl_amd.PPO(fused_step=True) on the GPU: the runs of test_gpu_ppo.py, test_gpu_brax_ppo.py and
test_gpu_ppo_normalized.py with the advantage statistics of an epoch in one launch (carl_ppo_adv_stats) and clip + Adam in
one launch per minibatch (carl_adam_step), after every update against a host replica.

The replica is ppo_checks.AdamReplica, its apply() and its bound as they are.  Its optimiser is ppo_step_ref.adam_ref -- the
restatement the device is bit-equal to (test_gpu_adam_step.py) -- behind an object with torch's ``step()`` and ``state``;
its advantage normalisation is the device's own ``adv_norm`` row AFTER that row has passed the 1-ulp check against the
exact reference (test_gpu_ppo_adv_stats.py's bar), so ppo_ref.py's / brax_ppo_ref.py's gradient tolerance applies unchanged.
The transform sections and the padding of the packed tensors keep their bits (ppo_checks.check_against_replica)."""
import numpy as np
import pytest
import torch

import brax_policy_cases as BPC
import brax_ppo_ref as BR
import brax_sampling_cases as BSC
import policy_cases as PC
import ppo_checks as PK
import ppo_ref as R
import ppo_step_ref as SR
import value_cases as VC
from carl_amd import PPO, _lib
from carl_amd.brax_policy import BraxMLPPolicy
from carl_amd.policy import MLPPolicy
from ppo_checks import B1, B2, CLIP, ENT, EPS, LR, MAX_NORM, VF

pytestmark = pytest.mark.gpu


class RefAdam:
    """ppo_step_ref.adam_ref over the replica's tensors with torch.optim.Adam's ``step()`` and ``state``; the gradients
    arrive clipped (AdamReplica.apply), so the coefficient is 1"""

    def __init__(self, params):
        self.params = params
        self.arrays = [p.numpy().reshape(-1) for p in params]  # (views: the tensors move with them)
        self.st = SR.adam_state(self.arrays)
        self.state = {p: {"exp_avg": torch.from_numpy(m), "exp_avg_sq": torch.from_numpy(v)}
                      for p, m, v in zip(params, self.st["m"], self.st["v"])}

    def step(self):
        SR.adam_ref(self.arrays, [p.grad.numpy() for p in self.params], self.st, 1.0, LR, (B1, B2), EPS)


class Replica(PK.AdamReplica):
    """ppo_checks.AdamReplica on the reference gradients of either engine, under RefAdam and the device's adv_norm rows"""

    def __init__(self, actor, critic, brax):
        self.templates, self.brax, self.box = (actor, critic), brax, brax or not actor.discrete
        ls = actor.log_std[0] if brax else actor.log_std
        super().__init__([actor.params[0], critic.params[0]] + ([ls] if self.box else []))
        self.opt = RefAdam(self.params)

    def policies(self):
        a, c = self.templates
        if self.brax:
            qa, qc = BraxMLPPolicy.unpack(a, self.params[0].numpy()), BraxMLPPolicy.unpack(c, self.params[1].numpy())
            return BraxMLPPolicy(a._info, a.ctx_rows, qa.layers, a.activation, qa.shift, qa.scale, qa.clip,
                                 log_std=self.params[2].numpy()), qc
        ls = float(self.params[2][0]) if self.box else None
        return MLPPolicy.unpack(a, self.params[0].numpy(), ls), MLPPolicy.unpack(c, self.params[1].numpy())

    def step(self, table, buf, flat, P, norm):
        actor, critic = self.policies()
        x = R.sample_inputs(actor, table, buf["context_id"], buf["obs0"], buf["obs"], flat, P)
        pick = lambda a: a.reshape(-1)[flat]  # noqa: E731
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


def host(buf, T, brax):
    """the buffer's columns as the flat indices address them (the padded rows of a classic buffer) -> (arrays, pitch)"""
    out, P = {}, None
    for k in ("obs", "action", "log_prob", "advantage", "return", "context_id"):
        t = buf[k][:T]
        P = t.shape[1]
        if not brax and T > 1:
            P = t.stride(0) // (t.shape[2] if t.dim() == 3 else 1)
            t = torch.as_strided(t, (T, P) + tuple(t.shape[2:]), t.stride())
        out[k] = t.cpu().numpy()
    out["obs0"] = buf["obs0"].cpu().numpy()
    return out, P


def classic(family, N, **opts):
    eng = PC.make_engine(family, N, _lib.SEL_ROUND_ROBIN, n_contexts=7, seed=5, **{"max_episode_steps": 20, **opts})
    rng = np.random.default_rng(2)
    box = not eng.info.action_is_discrete
    actor = PC.make_policy(eng, (8, 8), "tanh", rng, ctx="all", clip=5.0, log_std=-0.5 if box else None)
    return eng, actor, VC.make_critic(eng, actor, (8,), "tanh", rng), False


def brax(model, N, **opts):
    eng = BSC.make_engine(model, max(BPC.model_widths(model)), N, "cuda", seed=5, **{"max_episode_steps": 3, **opts})
    rng = np.random.default_rng(2)
    actor = BSC.make_policy(eng, (8, 8), "tanh", 2, (-0.5 + 0.3 * np.arange(eng.sys.n_act)).astype(np.float32))
    critic = BraxMLPPolicy.for_env(eng, BPC.make_layers(rng, 2 + eng.D, (8,), 1), "tanh", actor.shift, actor.scale, actor.clip,
                                   head="value")
    return eng, actor, critic, True


def device_tensors(ppo, rep, is_brax):
    return [ppo.actor_params[0], ppo.critic_params[0]] + ([ppo.log_std[0] if is_brax else ppo.log_std] if rep.box else [])


def update_and_replay(ppo, rep, order, table, hb, P, N, T, batch, n_epochs):
    """one fused update(); its results' shapes; every adv_norm row within 1 ulp of the exact reference; the clip
    coefficient the header's expression on the device's norm; the replica stepped through the same minibatches"""
    order.clear()
    res = ppo.update()
    per_epoch = -(-T * N // batch)
    n_mb = n_epochs * per_epoch
    assert set(res) == {"stats", "adv_norm", "grad_norm"} and all(v.is_cuda for v in res.values())
    assert res["stats"].shape == (n_mb, 6) and res["adv_norm"].shape == (n_mb, 2) and res["grad_norm"].shape == (n_mb, 2)
    assert res["adv_norm"].dtype == torch.float32 and res["grad_norm"].dtype == torch.float64
    assert len(order) == n_epochs and all(len(e) == per_epoch for e in order)  # the wrapper saw every epoch
    assert sorted(np.concatenate(order[0]) % P + np.concatenate(order[0]) // P * N) == list(range(T * N))  # a permutation
    rows, gn, stats = res["adv_norm"].cpu().numpy(), res["grad_norm"].cpu().numpy(), res["stats"].cpu().numpy()
    assert np.isfinite(stats).all() and [int(v) for v in stats[:per_epoch, 5]] == [len(f) for f in order[0]]
    k = 0
    for epoch in order:
        want = SR.adv_stats_ref(hb["advantage"].reshape(-1), np.concatenate(epoch), batch)
        got = rows[k: k + per_epoch]
        assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= SR.ulp32(want)), (got, want)
        for flat in epoch:
            assert gn[k, 1] == SR.coef_ref(gn[k, 0], ppo.max_grad_norm)
            rep.step(table, hb, flat, P, rows[k])
            k += 1
    assert int(ppo.adam_state["step"].cpu()) == rep.steps
    return res


RUNS = {
    "cartpole": (lambda: classic(_lib.CARTPOLE, 256), 32, 2048),
    "pendulum": (lambda: classic(_lib.PENDULUM, 256), 32, 2048),
    "inverted_pendulum": (lambda: brax("inverted_pendulum", 64), 8, 128),
    "reacher": (lambda: brax("reacher", 64), 8, 128),
    "cartpole-short-last-minibatch": (lambda: classic(_lib.CARTPOLE, 272), 8, 1000),
}


@pytest.mark.parametrize("run", list(RUNS))
def test_fused_updates_match_the_host_replica(run):
    make, T, batch = RUNS[run]
    eng, actor, critic, is_brax = make()
    N = eng.n
    ppo = PPO(eng, actor, critic, n_steps=T, n_epochs=2, batch_size=batch, lr=LR, clip_range=CLIP, vf_coef=VF, ent_coef=ENT,
              max_grad_norm=MAX_NORM, seed=9, fused_step=True)
    assert ppo.optimizer is None and set(ppo.adam_state) == {"m", "v", "step", "beta_pow"}
    order, _ = PK.record(ppo, eng)
    rep = Replica(actor, critic, is_brax)
    table = eng.ctx_table.cpu().numpy()
    for it in range(2):
        buf = ppo.collect()
        hb, P = host(buf, T, is_brax)
        update_and_replay(ppo, rep, order, table, hb, P, N, T, batch, 2)
        PK.check_against_replica(f"{run}, iteration {it}", device_tensors(ppo, rep, is_brax), rep, ppo, actor, critic)
    assert not np.array_equal(ppo.actor().params, actor.params) and ppo.critic().head == "value"  # they moved
    info = ppo.learn(1)
    assert len(info) == 1 and info[0]["mean_reward"].is_cuda and info[0]["grad_norm"].is_cuda


def test_fused_step_is_off_by_default():
    eng, actor, critic, _ = classic(_lib.CARTPOLE, 256)
    ppo = PPO(eng, actor, critic, n_steps=4)
    assert isinstance(ppo.optimizer, torch.optim.Adam) and ppo.adam_state is None and not ppo.fused_step
    ppo.collect()
    assert set(ppo.update()) == {"stats"}


def test_fused_normalized_ppo_matches_the_host_replica():
    """normalize_inputs and normalize_reward with fused_step, 300 lanes, T = 8, as test_gpu_ppo_normalized.py runs them:
    every minibatch under the section the collection ran, the merge once after the last one, the weights within the
    replica's bounds; the replica's next iteration runs under the device's merged section"""
    N, T, batch = 300, 8, 600
    eng, actor, critic, _ = classic(_lib.CARTPOLE, N, max_episode_steps=3, selector_stride=2)
    n_in = actor.n_in
    ppo = PPO(eng, actor, critic, n_steps=T, n_epochs=2, batch_size=batch, lr=LR, gamma=0.96875, lam=0.875, clip_range=CLIP,
              vf_coef=VF, ent_coef=ENT, max_grad_norm=MAX_NORM, seed=9, normalize_inputs=True, normalize_reward=True,
              clip_reward=2.0, norm_eps=1e-8, fused_step=True)
    order, _ = PK.record(ppo, eng)
    rep = Replica(actor, critic, False)
    table = eng.ctx_table.cpu().numpy()

    def section(which):
        params = ppo.actor_params if which == 0 else ppo.critic_params
        w = ppo._templates[which].weight_floats
        return params[0, w: w + 2 * n_in + 1].cpu().numpy().view(np.uint32).copy()

    seen, grad = [], eng.ppo_grad

    def recording_grad(*a, **kw):
        seen.append(section(0))
        return grad(*a, **kw)

    eng.ppo_grad = recording_grad
    for it in range(2):
        buf = ppo.collect()
        ran = section(0)
        assert "reward_normalized" in buf
        hb, P = host(buf, T, False)
        seen.clear()
        update_and_replay(ppo, rep, order, table, hb, P, N, T, batch, 2)
        assert len(seen) == 2 * 4 and all(np.array_equal(s, ran) for s in seen)
        after = section(0)
        assert not np.array_equal(after, ran) and np.array_equal(section(1), after)
        assert int(ppo.input_stats.count.cpu()) == (it + 1) * T * N
        dev = device_tensors(ppo, rep, False)
        for i, (d, pol) in enumerate(zip(dev, (actor, critic))):
            w = pol.weight_floats
            diff = np.abs(d.cpu().numpy().astype(np.float64) - rep.params[i].numpy().astype(np.float64))[:w]
            print(f"iteration {it}, tensor {i}: largest difference / bound {np.max(diff / np.maximum(rep.bound(i)[:w], 1e-300)):.3e}")
            assert np.all(diff <= rep.bound(i)[:w])
            with torch.no_grad():
                rep.params[i][w: w + 2 * n_in] = torch.tensor(after.view(np.float32)[: 2 * n_in])
            np.testing.assert_array_equal(d.cpu().numpy()[w + 2 * n_in:].view(np.uint32), pol.params[0][w + 2 * n_in:].view(np.uint32))
    with pytest.raises(RuntimeError, match="updated on once"):
        ppo.update()


def test_fused_learn_does_not_synchronise_with_the_host():
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
        ppo = PPO(eng, actor, critic, n_steps=8, n_epochs=2, batch_size=1000, fused_step=True)
        ppo.learn(1)  # warm-up: first uploads, code objects, the persistent gradient tensors
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            info = ppo.learn(2)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert len(info) == 2 and bool(torch.isfinite(info[1]["stats"]).all())


@pytest.mark.parametrize("kw", [dict(max_grad_norm=None), dict(normalize_advantage=False)], ids=["no-clip", "raw-advantages"])
def test_fused_step_without_the_clip_or_the_normalisation(kw):
    eng, actor, critic, _ = classic(_lib.PENDULUM, 256)
    ppo = PPO(eng, actor, critic, n_steps=8, n_epochs=2, batch_size=512, fused_step=True, **kw)
    ppo.lr = 1e-3  # (read at every step)
    res = ppo.learn(1)[0]
    assert bool(torch.isfinite(res["stats"]).all()) and res["stats"].shape == (8, 6)
    gn, rows = res["grad_norm"].cpu().numpy(), res["adv_norm"].cpu().numpy()
    assert np.isfinite(gn).all() and (gn[:, 0] > 0).all()
    if "max_grad_norm" in kw:
        assert (gn[:, 1] == 1.0).all()
    else:
        assert (rows == np.array([0.0, 1.0], np.float32)).all()
    assert not np.array_equal(ppo.actor().params, actor.params)
