"""carl_amd.PopulationPPO on the GPU: three learners in one launch sequence, each bit-equal to a replay of its own
minibatches through the one-set engine calls (ppo_adv_stats, ppo_grad, adam_step with adam_state) on clones of its starting
parameters.  The one-set calls are compared against exact references and a host replica in test_gpu_ppo_grad.py,
test_gpu_ppo_adv_stats.py, test_gpu_adam_step.py and test_gpu_ppo_fused.py; bit equality carries those contracts over.

The common shape (ppo_sets_cases.py): P = 3 members of 256 lanes, T = 5, n_epochs = 2, batch_size = 512 -- minibatches of
512, 512 and 256 samples per member."""
import numpy as np
import pytest
import torch

import ppo_sets_cases as S
from carl_amd import PopulationPPO, _lib
from carl_amd.policy import MLPPolicy
from ppo_sets_cases import HYPER, L, N, P, T

pytestmark = pytest.mark.gpu

BATCH, EPOCHS = 512, 2
PER_EPOCH = -(-T * L // BATCH)
FAMILIES = {"cartpole": _lib.CARTPOLE, "pendulum": _lib.PENDULUM}


def population(family, **kw):
    eng = S.make_engine(family)
    actors, critics = S.make_members(eng, (8, 8), (8,))
    cols = {name: [float(v) for v in HYPER[:, c]] for c, name in enumerate(_lib.PPO_HYPER_NAMES)}
    pop = PopulationPPO(eng, actors, critics, lanes_per_set=L, n_steps=T, n_epochs=EPOCHS, batch_size=BATCH, seed=9,
                        **{**cols, **kw})
    return eng, actors, critics, pop


def record_epochs(pop):
    """every epoch's [P, T * L] index tensor, as update() draws it"""
    epochs, draw = [], pop.minibatches

    def recording():
        mbs = draw()
        assert len(mbs) == PER_EPOCH and [tuple(m.shape) for m in mbs] == [(P, 512), (P, 512), (P, 256)]
        epochs.append(pop._epoch_idx.clone())
        return mbs

    pop.minibatches = recording
    return epochs


class MemberReplay:
    """member s as a one-learner run of the existing engine calls, on clones of its starting parameters"""

    def __init__(self, eng, actor, critic, s):
        dev = eng.device
        self.eng, self.s, self.box = eng, s, not actor.discrete
        self.actor_params = torch.as_tensor(actor.params).to(dev).contiguous().clone()
        self.critic_params = torch.as_tensor(critic.params).to(dev).contiguous().clone()
        self.log_std = torch.as_tensor(actor.log_std).to(dev).contiguous().clone()
        self.actor = MLPPolicy.on_device(actor, self.actor_params, N, self.log_std if self.box else None)
        self.critic = MLPPolicy.on_device(critic, self.critic_params, N)
        self.params = [self.actor_params, self.critic_params] + ([self.log_std] if self.box else [])
        self.state = eng.adam_state(self.params)

    def update(self, buf, epochs, hyper):
        """-> (stats [n_mb, 6], adv_norm [n_mb, 2], grad_norm [n_mb, 2]) of this member's minibatches"""
        eng, s = self.eng, self.s
        h = hyper[s]
        coef = {"clip_range": float(np.float32(h[1])), "vf_coef": float(np.float32(h[2])), "ent_coef": float(np.float32(h[3]))}
        mgn = None if np.isinf(h[4]) else float(h[4])
        stats, adv_norm, grad_norm = [], [], []
        adv = buf["advantage"][:T]
        for epoch in epochs:
            row = epoch[s].contiguous()
            rows = eng.ppo_adv_stats(adv, row, BATCH, 1e-8)
            for j in range(PER_EPOCH):
                g = eng.ppo_grad(self.actor, self.critic, buf, buf["obs0"], buf["context_id"],
                                 idx=row[j * BATCH: (j + 1) * BATCH].contiguous(), adv_norm=rows[j], **coef)
                grads = [g["grad_actor"].view_as(self.actor_params), g["grad_critic"].view_as(self.critic_params)]
                if self.box:
                    grads.append(g["grad_log_std"])
                gn = torch.zeros(2, dtype=torch.float64, device=eng.device)
                eng.adam_step(self.params, grads, self.state, float(h[0]), eps=1e-5, max_grad_norm=mgn, norm_out=gn)
                stats.append(g["stats"].clone())
                adv_norm.append(rows[j].clone())
                grad_norm.append(gn)
        return torch.stack(stats), torch.stack(adv_norm), torch.stack(grad_norm)


def check_member_state(pop, rep, s, label):
    S.assert_bits(pop.actor_params[s], rep.actor_params[0], f"{label}: actor of member {s}")
    S.assert_bits(pop.critic_params[s], rep.critic_params[0], f"{label}: critic of member {s}")
    S.assert_bits(pop.log_std[s: s + 1], rep.log_std, f"{label}: log_std of member {s}")
    for i in range(len(rep.params)):
        S.assert_bits(pop.adam_state["m"][i][s], rep.state["m"][i].reshape(-1), f"{label}: m[{i}] of member {s}")
        S.assert_bits(pop.adam_state["v"][i][s], rep.state["v"][i].reshape(-1), f"{label}: v[{i}] of member {s}")
    S.assert_bits(pop.adam_state["step"][s: s + 1], rep.state["step"], f"{label}: step of member {s}")
    S.assert_bits(pop.adam_state["beta_pow"][s], rep.state["beta_pow"], f"{label}: beta_pow of member {s}")


@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_member_is_bit_equal_to_its_one_learner_replay(family):
    eng, actors, critics, pop = population(FAMILIES[family])
    S.assert_bits(pop.hyper, HYPER, "hyper")
    with pytest.raises(RuntimeError, match=r"collect\(\) first"):
        pop.update()
    epochs = record_epochs(pop)
    replays = [MemberReplay(eng, actors[s], critics[s], s) for s in range(P)]
    n_mb = EPOCHS * PER_EPOCH
    for it in range(2):  # (the second collection runs the updated population)
        buf = pop.collect()
        pitch = int(buf["action"].stride(0))
        epochs.clear()
        res = pop.update()
        torch.cuda.synchronize()
        assert len(epochs) == EPOCHS
        assert set(res) == {"stats", "adv_norm", "grad_norm"} and all(v.is_cuda for v in res.values())
        assert tuple(res["stats"].shape) == (n_mb, P, 6) and tuple(res["adv_norm"].shape) == (n_mb, P, 2)
        assert tuple(res["grad_norm"].shape) == (n_mb, P, 2) and res["grad_norm"].dtype == torch.float64
        for epoch in epochs:  # each row: a permutation of that member's own samples
            rows = epoch.cpu().numpy().astype(np.int64)
            for s in range(P):
                t, lane = rows[s] // pitch, rows[s] % pitch
                assert ((lane >= s * L) & (lane < (s + 1) * L)).all()
                assert sorted(t * L + lane - s * L) == list(range(T * L))
        assert not np.array_equal(epochs[0].cpu().numpy(), epochs[1].cpu().numpy())
        for s in range(P):
            stats, adv_norm, grad_norm = replays[s].update(buf, epochs, HYPER)
            torch.cuda.synchronize()
            label = f"{family}, iteration {it}"
            S.assert_bits(res["stats"][:, s], stats, f"{label}: stats of member {s}")
            S.assert_bits(res["adv_norm"][:, s], adv_norm, f"{label}: adv_norm of member {s}")
            S.assert_bits(res["grad_norm"][:, s], grad_norm, f"{label}: grad_norm of member {s}")
            check_member_state(pop, replays[s], s, label)
        assert bool(torch.isfinite(res["stats"]).all())
        assert [int(v) for v in res["stats"][:PER_EPOCH, 0, 5].cpu()] == [512, 512, 256]
    assert pop.adam_state["step"].tolist() == [2 * n_mb] * P
    actor0, critic0 = pop.member(0)
    assert not np.array_equal(actor0.params, actors[0].params) and critic0.head == "value"  # they moved
    assert actor0.n_sets == 1 and np.array_equal(S.bits(actor0.params[0]), S.bits(pop.actor_params[0]))
    info = pop.learn(1)
    assert len(info) == 1 and tuple(info[0]["mean_reward"].shape) == (P,) and info[0]["mean_reward"].is_cuda


def test_update_does_not_synchronise_with_the_host():
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
    for family in FAMILIES.values():
        _, _, _, pop = population(family)
        pop.learn(1)  # warm-up: first uploads, code objects, the persistent gradient tensors
        src = torch.tensor([1, 1, 2], dtype=torch.int64, device="cuda")
        pop.collect()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            res = pop.update()
            pop.copy_members(src)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert bool(torch.isfinite(res["stats"]).all())


def test_copy_members():
    _, _, _, pop = population(_lib.PENDULUM)
    pop.learn(1)  # (the members' states differ now)

    def snapshot():
        st = pop.adam_state
        return [t.clone() for t in [pop.actor_params, pop.critic_params, pop.log_std, *st["m"], *st["v"], st["step"],
                                    st["beta_pow"], pop.hyper]]

    before = snapshot()
    pop.copy_members(torch.arange(P, dtype=torch.int64, device="cuda"))
    for a, b in zip(snapshot(), before):
        S.assert_bits(a, b, "the identity map")
    pop.copy_members(torch.tensor([1, 1, 2], dtype=torch.int64, device="cuda"))
    after = snapshot()
    assert not np.array_equal(S.bits(before[0][0]), S.bits(before[0][1]))
    for a, b in zip(after, before):
        S.assert_bits(a[0], b[1], "member 0 <- member 1")
        S.assert_bits(a[1], b[1], "member 1 stays")
        S.assert_bits(a[2], b[2], "member 2 stays")
    S.assert_bits(pop.hyper[0], HYPER[1], "member 0's hyper row")
    pop.collect()
    res = pop.update()  # (a following update runs)
    assert bool(torch.isfinite(res["stats"]).all())
    with pytest.raises(ValueError, match="'src'"):
        pop.copy_members(torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda"))


def test_raw_advantages_skip_the_statistics_launch():
    eng, _, _, pop = population(_lib.CARTPOLE, normalize_advantage=False)
    calls, launch = [], eng.ppo_adv_stats_sets

    def counting(*a, **kw):
        calls.append(1)
        return launch(*a, **kw)

    eng.ppo_adv_stats_sets = counting
    res = pop.learn(1)[0]
    assert not calls
    assert (res["adv_norm"].cpu().numpy() == np.array([0.0, 1.0], np.float32)).all()
    assert bool(torch.isfinite(res["stats"]).all()) and tuple(res["stats"].shape) == (EPOCHS * PER_EPOCH, P, 6)
    pop.set_hyper("lr", [1e-3, 2e-3, 3e-3])
    S.assert_bits(pop.hyper[:, 0], np.array([1e-3, 2e-3, 3e-3]), "set_hyper")
    with pytest.raises(ValueError, match="finite and >= 0"):
        pop.set_hyper("clip_range", [0.1, -0.2, 0.3])
