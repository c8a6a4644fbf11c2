"""ppo_ref.py against independent restatements, on the CPU: its loss and analytic gradients against torch float64
autograd of SB3's PPO loss (every head, activation and depth, with and without advantage normalisation), and its
selector walk against the host selectors of carl_amd/context/selection.py; and the helpers that build the cases of
test_gpu_ppo_grad_edges.py (zero-signal samples, the rescaled subset reference, the clip-edge columns) on the float32
restatement.  CPU-only."""
import numpy as np
import pytest
import torch

import ppo_checks as PK
import ppo_ref as R
from carl_amd import _lib
from carl_amd.context.selection import RoundRobinSelector, StaticSelector
from carl_amd.policy import MLPPolicy
from policy_cases import fake_engine, n_outputs

HEADS = {"categorical2": _lib.CARTPOLE, "categorical3": _lib.ACROBOT, "gaussian": _lib.PENDULUM}
DEPTHS = {0: (), 1: (6,), 2: (7, 5)}
CLIP, VF, ENT = 0.2, 0.5, 0.01


def _networks(family, widths, act, rng):
    eng = fake_engine(family)
    rows = [0, 2]
    n_in = len(rows) + eng.D
    shift, scale = rng.normal(0, 0.2, n_in), rng.uniform(0.5, 1.5, n_in)

    def layers(dims):
        return [(rng.normal(0, 1 / np.sqrt(i), (o, i)), rng.normal(0, 0.3, o)) for i, o in zip(dims[:-1], dims[1:])]

    box = not eng.info.action_is_discrete
    kw = dict(input_shift=shift, input_scale=scale, input_clip=2.0, context_features=rows)
    actor = MLPPolicy.for_env(eng, layers([n_in, *widths, n_outputs(eng)]), act, log_std=0.4 if box else None, **kw)
    critic = MLPPolicy.for_env(eng, layers([n_in, *widths, 1]), act, head="value", **kw)
    return actor, critic


def _torch_loss(actor, critic, log_std, x_raw, action, logp_old, adv, ret, norm):
    """SB3's PPO loss in torch float64 on leaf tensors -> (loss, {name: leaf})"""
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

    x = torch.clamp((t(x_raw) - t(actor.shift)) * t(actor.scale), -float(actor.clip), float(actor.clip))
    y, V = net(actor, x, "a"), net(critic, x, "c")[:, 0]
    A = t(adv)
    if norm is not None:
        A = (A - float(norm[0])) * float(norm[1])
    if actor.discrete:
        dist = torch.distributions.Categorical(logits=y)
        lp, H = dist.log_prob(torch.tensor(np.asarray(action, np.int64))), dist.entropy()
    else:
        ls = torch.tensor(float(log_std), dtype=torch.float64, requires_grad=True)
        leaves["log_std"] = ls
        dist = torch.distributions.Normal(y[:, 0], torch.exp(ls) * torch.ones_like(y[:, 0]))
        lp, H = dist.log_prob(t(action)), dist.entropy()
    c = float(np.float32(CLIP))
    r = torch.exp(lp - t(logp_old))
    pl = -torch.min(r * A, torch.clamp(r, 1 - c, 1 + c) * A).mean()
    vl = ((t(ret) - V) ** 2).mean()
    loss = pl + float(np.float32(ENT)) * (-H.mean()) + float(np.float32(VF)) * vl
    return loss, leaves, (lp, V, pl, vl, H.mean())


def _packed(pol, leaves, tag):
    parts = []
    for k in range(len(pol.layers)):
        parts += [leaves[f"{tag}W{k}"].grad.numpy().reshape(-1), leaves[f"{tag}b{k}"].grad.numpy()]
    g = np.zeros(pol.set_floats)
    flat = np.concatenate(parts)
    g[: flat.size] = flat
    return g


@pytest.mark.parametrize("use_norm", [False, True], ids=["raw", "normalised"])
@pytest.mark.parametrize("depth", sorted(DEPTHS))
@pytest.mark.parametrize("act", ["identity", "tanh", "relu"])
@pytest.mark.parametrize("head", sorted(HEADS))
def test_reference_matches_torch_autograd(head, act, depth, use_norm):
    rng = np.random.default_rng(7 + depth)
    actor, critic = _networks(HEADS[head], DEPTHS[depth], act, rng)
    M = 37
    f32 = np.float32
    x_raw = rng.normal(0, 1.5, (M, actor.n_in)).astype(f32)
    action = rng.integers(0, actor.n_out, M) if actor.discrete else rng.normal(0, 1.5, M).astype(f32)
    adv, ret = rng.normal(0.2, 1, M).astype(f32), rng.normal(0, 2, M).astype(f32)
    norm = np.array([adv.mean(), 1 / (adv.std() + 1e-8)], f32) if use_norm else None
    lp0 = R.ppo_grad_ref(actor, critic, x_raw, action, np.zeros(M, f32), adv, ret, norm, CLIP, VF, ENT)["new_log_prob"]
    # ratios on both sides of both clip boundaries, none on one
    logp_old = (lp0 - np.log(rng.choice([0.5, 0.7, 0.9, 1.0, 1.1, 1.3, 1.6], M))).astype(f32)
    ref = R.ppo_grad_ref(actor, critic, x_raw, action, logp_old, adv, ret, norm, CLIP, VF, ENT)
    assert (np.abs(ref["ratio"] - 0.8) > 1e-3).all() and (np.abs(ref["ratio"] - 1.2) > 1e-3).all()
    assert 0 < (np.abs(ref["ratio"] - 1) > CLIP).mean() < 1  # some clipped, some not
    loss, leaves, (lp, V, pl, vl, ent) = _torch_loss(actor, critic, actor.log_std[0], x_raw, action, logp_old, adv, ret, norm)
    loss.backward()
    close = lambda a, b: np.testing.assert_allclose(a, b, rtol=1e-10, atol=1e-13)  # noqa: E731
    close(ref["new_log_prob"], lp.detach().numpy())
    close(ref["new_value"], V.detach().numpy())
    close(ref["stats"][:3], [pl.item(), vl.item(), ent.item()])
    close(ref["loss"], loss.item())
    close(ref["grad_actor"], _packed(actor, leaves, "a"))
    close(ref["grad_critic"], _packed(critic, leaves, "c"))
    if not actor.discrete:
        close(ref["grad_log_std"], leaves["log_std"].grad.item())
    # S bounds each entry, and the transform section and the padding carry no gradient
    for name, pol in (("actor", actor), ("critic", critic)):
        g, S = ref["grad_" + name], ref["S_" + name]
        assert np.all(np.abs(g) <= S * (1 + 1e-12) + 1e-300)
        assert not g[pol.weight_floats:].any() and not S[pol.weight_floats:].any()


@pytest.mark.parametrize("stride", [1, 3])
def test_round_robin_walk_is_the_host_selector(stride):
    C, T = 7, 40
    rng = np.random.default_rng(stride)
    done = rng.random((T, 1)) < 0.3
    sel = RoundRobinSelector({k: {} for k in range(C)}, stride=stride)
    sel.select()  # the reset before the launch
    want = []
    for t in range(T):
        want.append(sel.context_id)
        if done[t, 0]:
            sel.select()
    te = done & (rng.random((T, 1)) < 0.5)
    got = R.context_walk([want[0]], [1], te, done & ~te, _lib.SEL_ROUND_ROBIN, stride, C, 5, 0, True)
    np.testing.assert_array_equal(got[:, 0], want)
    # without auto-reset the context never moves
    got = R.context_walk([want[0]], [1], te, done & ~te, _lib.SEL_ROUND_ROBIN, stride, C, 5, 0, False)
    assert (got == want[0]).all()


def test_static_walk_is_the_host_selector():
    sel = StaticSelector({k: {} for k in range(5)})
    sel.select()
    done = np.ones((9, 1), bool)
    got = R.context_walk([sel.context_id], [1], done, ~done, _lib.SEL_STATIC, 1, 5, 0, 0, True)
    for t in range(9):
        assert got[t, 0] == sel.context_id
        sel.select()


def test_random_walk_draws_once_per_reset_from_the_episode_counter():
    """the random rule: umulhi(Philox(seed; glane lo, glane hi, episode, 1).x, C), the episode counter advancing by one
    per reset -- each lane's sequence is that of its own (global lane, episode) pairs, whatever the other lanes do"""
    C, T, N, seed, off = 7, 30, 5, 0x1234567890ABCDEF, (1 << 32) + 17
    rng = np.random.default_rng(0)
    done = rng.random((T, N)) < 0.4
    ep0 = np.array([1, 2, 3, 0xFFFFFFFF, 9], np.uint32)
    got = R.context_walk(np.zeros(N, np.int32), ep0, done, np.zeros_like(done), _lib.SEL_RANDOM, 1, C, seed, off, True)
    from oracle import oracle as O
    for lane in range(N):
        c, e = 0, int(ep0[lane])
        for t in range(T):
            assert got[t, lane] == c
            if done[t, lane]:
                g = off + lane
                w = O.philox4x32_10((g & 0xFFFFFFFF, g >> 32, e, 1), (seed & 0xFFFFFFFF, seed >> 32))
                c = (int(w[0]) * C) >> 32
                e = (e + 1) & 0xFFFFFFFF
    assert got.min() >= 0 and got.max() < C


# ---------------------------------------------------------------- the helpers of test_gpu_ppo_grad_edges.py
SMALL_TILE_LOOP = [c for c in R.tile_loop_cases() if "64" not in c[3]]  # (the 64-wide restatement takes half a minute)


@pytest.mark.parametrize("spec", SMALL_TILE_LOOP, ids=[c[0] for c in SMALL_TILE_LOOP])
def test_tile_loop_identities_hold_for_the_float32_restatement(spec):
    PK.check_tile_loop_helpers(R, spec)


@pytest.mark.parametrize("spec", R.skipped_cases(), ids=[c[0] for c in R.skipped_cases()])
def test_rescaled_subset_reference_is_the_evaluation_with_zero_terms(spec):
    PK.check_skipped_helpers(R, spec)


@pytest.mark.parametrize("spec", R.clip_edge_cases(), ids=[c[0] for c in R.clip_edge_cases()])
def test_clip_edge_columns_give_the_reference_the_float32_ratios(spec):
    """the float32 restatement's log-probabilities in the device's place: the reference's ratios are 1 exactly where the
    column holds them and 2 and 1/2 within a few roundings where it was moved, as the float32 ratios are"""
    case = R.make_case(spec)
    flat = case["flat"]
    lp32, lp64 = R.case_reference(case, np.float32)["new_log_prob"], R.case_reference(case)["new_log_prob"]
    assert lp32.dtype == np.float32
    m = np.arange(flat.size) % 3
    for mixed in (False, True):
        dev, ref = R.clip_edge_columns(case, lp32, lp64, mixed)
        assert dev.dtype == np.float32 and ref.dtype == np.float64
        r = R.case_reference(case, columns={"log_prob": ref}, clip_range=0.0)["ratio"]
        lr32 = lp32 - dev.reshape(-1)[flat]
        if not mixed:
            assert (r == 1).all() and (lr32 == 0).all()
            continue
        assert (r[m == 0] == 1).all()
        np.testing.assert_allclose(r[m == 1], 2.0, rtol=2e-6)
        np.testing.assert_allclose(r[m == 2], 0.5, rtol=2e-6)
        r32 = np.exp(lr32)
        assert (r32[m == 0] == 1).all() and (r32[m == 1] > 1.9).all() and (r32[m == 2] < 0.6).all()
        np.testing.assert_allclose(r32, r, rtol=4 * R.U)  # (half an ulp of lr, a rounding of exp)
