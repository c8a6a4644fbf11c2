"""carl_ppo_adv_stats_sets and carl_adam_step_sets on the GPU: every member's rows bit-equal to carl_ppo_adv_stats /
carl_adam_step on that member's rows.  The one-set kernels are compared against exact references in
test_gpu_ppo_adv_stats.py and test_gpu_adam_step.py; the population kernels run their bodies, so bit equality carries
those contracts over and no tolerance appears here.  The common shape (ppo_sets_cases.py): P = 3 members of 256 lanes,
T = 5, 1 280 samples per member."""
import numpy as np
import pytest
import torch

import ppo_sets_cases as S
from carl_amd import _lib
from ppo_sets_cases import HYPER, L, N, P, T

pytestmark = pytest.mark.gpu

EPS = 1e-8


def epoch_rows(pitch, seed, dev):
    """int32 [P, T * L]: row s a permutation of member s's flat sample indices in [T, N] rows of `pitch`"""
    rng = np.random.default_rng(seed)
    rows = []
    for s in range(P):
        j = rng.permutation(T * L)
        rows.append((j // L) * pitch + s * L + j % L)
    return torch.tensor(np.stack(rows), dtype=torch.int32, device=dev)


# (n_total, batch_size): 512 + 512 + 256; four of 300 and a short one; a one-sample last minibatch for either size
@pytest.mark.parametrize("n_total,batch", [(T * L, 512), (T * L, 300), (1025, 512), (901, 300)])
def test_adv_stats_rows_are_bit_equal_to_the_one_set_call(n_total, batch):
    eng = S.make_engine(_lib.CARTPOLE)
    dev = eng.device
    pitch = N + 16  # rows of a pitch of their own
    g = torch.Generator(device="cpu")
    g.manual_seed(4)
    adv = torch.zeros((T, pitch), dtype=torch.float32)
    adv[:, :N] = torch.randn((T, N), generator=g) * 3.0 + 0.5
    adv[:, L: 2 * L] = 0.37  # member 1: a constant advantage column
    adv = adv.to(dev)[:, :N]
    idx = epoch_rows(pitch, seed=n_total + batch, dev=dev)[:, :n_total]  # (the row stride stays T * L)
    rows = -(-n_total // batch)
    got = eng.ppo_adv_stats_sets(adv, idx, batch, EPS)
    again = eng.ppo_adv_stats_sets(adv, idx, batch, EPS)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (P, rows, 2) and got.dtype == torch.float32
    S.assert_bits(again, got, "two calls")
    for s in range(P):
        want = eng.ppo_adv_stats(adv, idx[s].contiguous(), batch, EPS)
        S.assert_bits(got[s], want, f"member {s}")
    host = got.cpu().numpy()
    full = host[1, : n_total // batch]  # the constant member's full minibatches: var == 0 exactly
    assert (full[:, 0] == np.float32(0.37)).all() and (full[:, 1] == np.float32(1.0 / EPS)).all()
    if n_total % batch == 1:  # a one-sample minibatch: the identity row, with +0.0
        S.assert_bits(host[:, -1], np.tile(np.array([0.0, 1.0], np.float32), (P, 1)), "identity rows")


def test_adam_step_members_are_bit_equal_to_the_one_set_call():
    """three steps over three tensors (4 100, 130 and 1 elements per member: more than one pass of the workgroup's
    4 096-element stride, a partial one, a single element) with per-member lr and max_grad_norm: +inf, an active clip, an
    idle one"""
    eng = S.make_engine(_lib.CARTPOLE)
    dev = eng.device
    sizes = (4100, 130, 1)
    g = torch.Generator(device="cpu")
    g.manual_seed(7)
    params = [torch.randn((P, n), generator=g).to(dev) for n in sizes]
    params[0][:, :4] = -0.0  # entries whose gradient stays +0.0: the bits of -0.0 must survive
    start = [p.clone() for p in params]
    hyper = torch.tensor(HYPER, dtype=torch.float64, device=dev)
    state = eng.adam_state(params, n_sets=P)
    assert tuple(state["step"].shape) == (P,) and tuple(state["beta_pow"].shape) == (P, 2)
    ref_params = [[p[s].clone() for p in start] for s in range(P)]
    ref_state = [eng.adam_state(ref_params[s]) for s in range(P)]
    for step in range(3):
        grads = [torch.randn((P, n), generator=g).to(dev) * (10.0 ** (step - 1)) for n in sizes]
        grads[0][:, :4] = 0.0
        norm = torch.full((P, 2), -1.0, dtype=torch.float64, device=dev)
        eng.adam_step_sets(params, grads, state, hyper, norm_out=norm)
        torch.cuda.synchronize()
        coef = norm[:, 1].cpu().numpy()
        assert coef[0] == 1.0 and coef[1] < 1.0 and coef[2] == 1.0  # no clip, an active clip, an idle one
        for s in range(P):
            want_norm = torch.zeros(2, dtype=torch.float64, device=dev)
            mgn = float(HYPER[s, _lib.PPO_HYPER_MAX_GRAD_NORM])
            eng.adam_step(ref_params[s], [x[s].clone() for x in grads], ref_state[s], float(HYPER[s, _lib.PPO_HYPER_LR]),
                          max_grad_norm=None if np.isinf(mgn) else mgn, norm_out=want_norm)
            torch.cuda.synchronize()
            for i in range(len(sizes)):
                S.assert_bits(params[i][s], ref_params[s][i], f"step {step}, member {s}: param {i}")
                S.assert_bits(state["m"][i][s], ref_state[s]["m"][i], f"step {step}, member {s}: m {i}")
                S.assert_bits(state["v"][i][s], ref_state[s]["v"][i], f"step {step}, member {s}: v {i}")
            S.assert_bits(state["step"][s: s + 1], ref_state[s]["step"], f"step {step}, member {s}: step")
            S.assert_bits(state["beta_pow"][s], ref_state[s]["beta_pow"], f"step {step}, member {s}: beta_pow")
            S.assert_bits(norm[s], want_norm, f"step {step}, member {s}: norm_out")
    assert state["step"].tolist() == [3] * P
    S.assert_bits(params[0][:, :4], start[0][:, :4], "-0.0 parameters under a +0.0 gradient")
    assert (S.bits(params[0][:, :4]) == 0x80000000).all()
    assert not S.bits(state["m"][0][:, :4]).any() and not S.bits(state["v"][0][:, :4]).any()
    assert not np.array_equal(params[0][0].cpu().numpy(), params[0][1].cpu().numpy())
