"""brax_ppo_ref.py against independent restatements, on the CPU: its joint-Gaussian loss and analytic gradients (the
per-actuator grad_log_std among them) against torch float64 autograd of SB3's PPO loss on a subset of the case table, the
conditioning of every case of the table by the reference alone, and its trace walk against hand-written examples per
selector and auto-reset mode.  CPU-only."""
import numpy as np
import pytest
import torch

import brax_ppo_ref as BR
import ppo_checks as PK
from carl_amd import _lib

CASES = BR.grad_cases()
# one case per shape, network depth and activation, and both advantage modes; the 65 537-sample case stays out (autograd
# over it proves nothing the 257-sample one does not)
AUTOGRAD = [c for c in CASES if c[0] in ("pendulum-linear-0", "pendulum-2x(64,64)-3", "reacher-1x7-6", "reacher-2x(7,3)-9",
                                         "hopper-linear-10", "hopper-2x(64,64)-13", "ant-1x7-16", "ant-1x32-17",
                                         "ant-2x(64,64)-18", "ant-2x(7,3)-19")]


def _torch_loss(case):
    """SB3's PPO loss of the case's minibatch in torch float64 on leaf tensors -> (loss, leaves, (lp, V, pl, vl, H))"""
    actor, critic = case["actor"], case["critic"]
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)  # noqa: E731
    leaves = {}

    def net(pol, x, tag):
        h = x
        for k, (W, b) in enumerate(pol.layers):
            Wt, bt = t(W).requires_grad_(), t(b).requires_grad_()
            leaves[f"{tag}W{k}"], leaves[f"{tag}b{k}"] = Wt, bt
            h = h @ Wt.T + bt
            if k < len(pol.layers) - 1:
                h = torch.tanh(h) if pol.activation == "tanh" else torch.relu(h) if pol.activation == "relu" else h
        return h

    f = case["flat"]
    pick = lambda a: a.reshape(-1)[f]  # noqa: E731
    x = torch.clamp((t(case["x"]) - t(actor.shift)) * t(actor.scale), -float(actor.clip), float(actor.clip))
    y, V = net(actor, x, "a"), net(critic, x, "c")[:, 0]
    A = t(pick(case["advantage"]))
    if case["adv_norm"] is not None:
        A = (A - float(case["adv_norm"][0])) * float(case["adv_norm"][1])
    ls = t(actor.log_std.reshape(-1)).requires_grad_()
    leaves["log_std"] = ls
    dist = torch.distributions.Normal(y, torch.exp(ls) * torch.ones_like(y))
    lp = dist.log_prob(t(case["action"].reshape(-1, actor.n_out)[f])).sum(dim=1)  # SB3's sum_independent_dims
    H = dist.entropy().sum(dim=1)
    c = float(np.float32(BR.CLIP))
    r = torch.exp(lp - t(pick(case["log_prob"])))
    pl = -torch.min(r * A, torch.clamp(r, 1 - c, 1 + c) * A).mean()
    vl = ((t(pick(case["ret"])) - V) ** 2).mean()
    loss = pl + float(np.float32(BR.ENT)) * (-H.mean()) + float(np.float32(BR.VF)) * vl
    return loss, leaves, (lp, V, pl, vl, H.mean())


def _packed(pol, leaves, tag):
    parts = []
    for k in range(len(pol.layers)):
        parts += [leaves[f"{tag}W{k}"].grad.numpy().reshape(-1), leaves[f"{tag}b{k}"].grad.numpy()]
    g = np.zeros(pol.set_floats)
    flat = np.concatenate(parts)
    g[: flat.size] = flat
    return g


@pytest.mark.parametrize("spec", AUTOGRAD, ids=[c[0] for c in AUTOGRAD])
def test_reference_matches_torch_autograd(spec):
    case = BR.make_case(spec)
    ref = BR.case_reference(case)
    loss, leaves, (lp, V, pl, vl, ent) = _torch_loss(case)
    loss.backward()
    close = lambda a, b: np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-12)  # noqa: E731
    close(ref["new_log_prob"], lp.detach().numpy())
    close(ref["new_value"], V.detach().numpy())
    close(ref["stats"][:3], [pl.item(), vl.item(), ent.item()])
    close(ref["loss"], loss.item())
    close(ref["grad_actor"], _packed(case["actor"], leaves, "a"))
    close(ref["grad_critic"], _packed(case["critic"], leaves, "c"))
    close(ref["grad_log_std"], leaves["log_std"].grad.numpy())
    assert ref["grad_log_std"].shape == (case["actor"].n_out,)
    for name, pol in (("actor", case["actor"]), ("critic", case["critic"])):
        g, S = ref["grad_" + name], ref["S_" + name]
        assert np.all(np.abs(g) <= S * (1 + 1e-12) + 1e-300)
        assert not g[pol.weight_floats:].any() and not S[pol.weight_floats:].any()
    assert np.all(np.abs(ref["grad_log_std"]) <= ref["S_log_std"] * (1 + 1e-12))


def test_the_case_table_covers_what_it_says():
    made = [BR.make_case(c) for c in CASES if c[6] is None or c[6] <= 3 * BR.TILE]
    assert {c["actor"].n_out for c in made} == {1, 2, 3, 8}
    assert {4, 13, 32} <= {c["actor"].n_in for c in made}
    assert {tuple(c["actor"].widths) for c in made} == {(), (7,), (32,), (64, 64), (7, 3)}
    assert {c["actor"].activation for c in made} == {"tanh", "relu", "identity"}
    assert {c["flat"].size for c in made} >= {1, BR.TILE - 1, BR.TILE, BR.TILE + 1, 2 * BR.TILE + 3}
    assert any(c["every"] for c in made) and any(c["adv_norm"] is None for c in made) and any(c["adv_norm"] is not None for c in made)
    assert any(c[6] == BR.WORKGROUPS_CAP * BR.TILE + 1 for c in CASES)
    for c in made:
        ls = c["actor"].log_std.reshape(-1)
        assert len(set(ls.tolist())) == ls.size and ls.min() < 0  # distinct per actuator, some negative
        assert c["critic"].log_std.shape == (1, 0)


@pytest.mark.parametrize("spec", CASES, ids=[c[0] for c in CASES])
def test_every_case_is_conditioned(spec):
    """ratios away from 1 +- clip (the clip count is exact), ReLU pre-activations away from 0: by the reference alone"""
    case = BR.make_case(spec)
    ref = BR.case_reference(case)
    BR.assert_conditioned(case, ref)
    assert ref["ratio"].min() > 0.5 and ref["ratio"].max() < 1.5
    if case["flat"].size > 16:
        assert 0 < (np.abs(ref["ratio"] - 1) > BR.CLIP).mean() < 1  # some clipped, some not


def test_k0_is_what_the_float32_restatement_gives():
    """K0's two dominating cases, re-measured: the constant in brax_ppo_ref.py is the printed figure"""
    ks = {}
    for spec in CASES:
        if spec[0] in ("hopper-2x(64,64)-13", "ant-2x(64,64)-18"):
            c = BR.make_case(spec)
            ks[spec[0]] = BR.case_k(BR.case_reference(c, np.float32), BR.case_reference(c))
    assert max(ks.values()) == pytest.approx(BR.K0, rel=1e-3) and BR.K == 8 * BR.K0


# ---------------------------------------------------------------- the trace walk, by hand
#  step            0  1  2  3  4  5
DONE = np.array([[0, 1, 0, 1, 1, 0]], bool).T  # one env; terminated at 1 and 4, truncated at 3
TE = np.array([[0, 1, 0, 0, 1, 0]], bool).T


def walk(selector, autoreset, first_state, c0=2, e0=1, stride=3, C=7, seed=9, off=0):
    return BR.context_walk([c0], [e0], TE, DONE & ~TE, selector, stride, C, seed, off, autoreset, first_state)[:, 0].tolist()


def test_round_robin_walk_by_hand():
    # the context step t's action was chosen in: it moves by the stride AFTER each done step
    assert walk(_lib.SEL_ROUND_ROBIN, True, False) == [2, 2, 5, 5, 1, 4]
    assert walk(_lib.SEL_ROUND_ROBIN, True, True) == [2] * 6    # first-state auto-reset: the context never moves
    assert walk(_lib.SEL_ROUND_ROBIN, False, False) == [2] * 6  # auto-reset off
    assert walk(_lib.SEL_ROUND_ROBIN, False, True) == [2] * 6


@pytest.mark.parametrize("selector", [_lib.SEL_STATIC, _lib.SEL_HOST])
def test_static_and_host_walks_by_hand(selector):
    for autoreset in (True, False):
        for first in (True, False):
            assert walk(selector, autoreset, first) == [2] * 6


def test_random_walk_by_hand():
    """umulhi(Philox(seed; genv lo, genv hi, episode, 1).x, C) with the episode counter advancing once per reset, genv =
    lane_offset + env; under the first-state mode neither the context nor the counter moves"""
    from oracle import oracle as O

    C_, seed, off, e0 = 7, 0x1234567890ABCDEF, (1 << 32) + 17, 0xFFFFFFFF
    want, c, e = [], 2, e0
    for t in range(6):
        want.append(c)
        if DONE[t, 0]:
            w = O.philox4x32_10((off & 0xFFFFFFFF, off >> 32, e, 1), (seed & 0xFFFFFFFF, seed >> 32))
            c = (int(w[0]) * C_) >> 32
            e = (e + 1) & 0xFFFFFFFF
    assert walk(_lib.SEL_RANDOM, True, False, e0=e0, C=C_, seed=seed, off=off) == want
    assert len(set(want)) > 1
    assert walk(_lib.SEL_RANDOM, True, True, e0=e0, C=C_, seed=seed, off=off) == [2] * 6
    assert walk(_lib.SEL_RANDOM, False, False, e0=e0, C=C_, seed=seed, off=off) == [2] * 6


# ---------------------------------------------------------------- the helpers of test_gpu_ppo_grad_edges.py
SMALL_TILE_LOOP = [c for c in BR.tile_loop_cases() if "64" not in c[3]]  # (the 64-wide restatement takes half a minute)


@pytest.mark.parametrize("spec", SMALL_TILE_LOOP, ids=[c[0] for c in SMALL_TILE_LOOP])
def test_tile_loop_identities_hold_for_the_float32_restatement(spec):
    PK.check_tile_loop_helpers(BR, spec)


@pytest.mark.parametrize("spec", BR.skipped_cases(), ids=[c[0] for c in BR.skipped_cases()])
def test_rescaled_subset_reference_is_the_evaluation_with_zero_terms(spec):
    PK.check_skipped_helpers(BR, spec)
