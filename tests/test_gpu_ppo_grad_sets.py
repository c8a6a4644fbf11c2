"""carl_ppo_grad_sets on the GPU: every member's gradients, grad_log_std and statistics bit-equal to carl_ppo_grad with
that member's one-set networks, index row, adv_norm row and float32-rounded coefficients, on the same buffer.
ppo_net_kernel compares the surrogate and the gradients against exact references (test_gpu_ppo_grad.py, ppo_ref.py); the
population kernels run that kernel's body, so bit equality carries that contract over and no tolerance appears here.

Shapes (ppo_sets_cases.py): P = 3 members of 256 lanes, T = 5 -- 1 280 samples, 5 tiles per member; minibatches of 512 (two
tiles), 300 (a tile and a part of one) and 1 280 (every sample); CartPole (categorical) and Pendulum (Gaussian, three
different log_std); the H = 32 instance ((8, 8) with a (8,) critic), the H = 64 instance and the H = 0 instance (a linear
actor).  Members differ in weights, transform sections and all three coefficients (one ent_coef = 0, one clip_range = 0)."""
import numpy as np
import pytest
import torch

import ppo_checks as PK
import ppo_sets_cases as S
from carl_amd import _lib
from ppo_sets_cases import L, P, T

pytestmark = pytest.mark.gpu

SHAPES = {
    "cartpole-8x8": (_lib.CARTPOLE, (8, 8), (8,)),
    "pendulum-8x8": (_lib.PENDULUM, (8, 8), (8,)),
    "cartpole-64x64": (_lib.CARTPOLE, (64, 64), (64, 64)),
    "cartpole-linear": (_lib.CARTPOLE, (), (8,)),
    "pendulum-linear": (_lib.PENDULUM, (), (8,)),
}
ADV_NORM = np.array([[0.125, 1.5], [-0.25, 0.75], [0.0, 2.0]], np.float32)


def sizes_of(c):
    sizes = {"grad_actor": P * c.actor.set_floats, "grad_critic": P * c.critic.set_floats, "stats": P * 6}
    if c.box:
        sizes["grad_log_std"] = P
    return sizes


def shaped(c, out):
    """run_twice's flat canaried outputs as the [P, ...] tensors ppo_grad_sets writes"""
    res = {"grad_actor": out["grad_actor"].view(P, -1), "grad_critic": out["grad_critic"].view(P, -1),
           "stats": out["stats"].view(P, 6)}
    if c.box:
        res["grad_log_std"] = out["grad_log_std"]
    return res


def population_call(c, idx, adv_norm):
    """two calls on canaried buffers -> the first call's outputs as NumPy arrays (canaries intact, equal bits twice)"""
    eng, M = c.eng, int(idx.shape[1])
    need = int(eng.ppo_sets_workspace(c.actor, c.critic, M).numel())

    def launch(out, ws):
        eng.ppo_grad_sets(c.actor, c.critic, c.buf, c.obs0, c.context_id, idx=idx, hyper=c.hyper, adv_norm=adv_norm,
                          out=shaped(c, out), workspace=ws)

    return PK.check_canaries_and_bits(PK.run_twice(sizes_of(c), need, launch))


def member_call(c, s, idx_row, adv_row):
    """eng.ppo_grad with member s's one-set policies on the same buffer"""
    g = c.eng.ppo_grad(c.actors[s], c.critics[s], c.buf, c.obs0, c.context_id, idx=idx_row.contiguous(),
                       adv_norm=None if adv_row is None else adv_row.contiguous(), **c.coefficients(s))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in g.items()}


def check_member(c, got, s, want, label):
    sa, sc = c.actor.set_floats, c.critic.set_floats
    S.assert_bits(got["grad_actor"][s * sa: (s + 1) * sa], want["grad_actor"], f"{label}: grad_actor of member {s}")
    S.assert_bits(got["grad_critic"][s * sc: (s + 1) * sc], want["grad_critic"], f"{label}: grad_critic of member {s}")
    S.assert_bits(got["stats"][6 * s: 6 * s + 6], want["stats"], f"{label}: stats of member {s}")
    if c.box:
        S.assert_bits(got["grad_log_std"][s: s + 1], want["grad_log_std"], f"{label}: grad_log_std of member {s}")
    # the transform and padding entries: +0.0
    assert not got["grad_actor"][s * sa + c.actors[s].weight_floats: (s + 1) * sa].view(np.uint32).any()
    assert not got["grad_critic"][s * sc + c.critics[s].weight_floats: (s + 1) * sc].view(np.uint32).any()


@pytest.mark.parametrize("with_adv_norm", [True, False], ids=["adv_norm", "raw"])
@pytest.mark.parametrize("M", [512, 300, T * L])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_member_is_bit_equal_to_the_one_set_call(shape, M, with_adv_norm):
    c = S.case(*SHAPES[shape])
    # the rows of a wider tensor: a row stride that is not the row length
    idx = c.member_rows(T * L, seed=M)[:, :M] if M < T * L else c.member_rows(M, seed=M)
    adv = torch.tensor(ADV_NORM, device=c.eng.device) if with_adv_norm else None
    got = population_call(c, idx, adv)
    assert [float(v) for v in got["stats"].reshape(P, 6)[:, 5]] == [float(M)] * P
    for s in range(P):
        check_member(c, got, s, member_call(c, s, idx[s], None if adv is None else adv[s]), shape)
    members = got["grad_actor"].reshape(P, -1)
    assert not np.array_equal(members[0], members[1]) and not np.array_equal(members[1], members[2])  # three learners


@pytest.mark.parametrize("shape", ["cartpole-8x8", "pendulum-linear"])
def test_a_lane_of_another_member_contributes_zero(shape):
    """one index of member 0's lanes in member 1's row: member 1 equals the one-set call with that entry replaced by -1
    (n_samples still counts it), members 0 and 2 keep their bits"""
    c = S.case(*SHAPES[shape])
    M = 300
    idx = c.member_rows(M, seed=11)
    adv = torch.tensor(ADV_NORM, device=c.eng.device)
    clean = population_call(c, idx, adv)
    foreign = idx.clone()
    foreign[1, 7] = 2 * c.pitch + 5  # (step 2, lane 5: a sample of member 0, inside the buffer)
    got = population_call(c, foreign, adv)
    skipped = foreign[1].clone()
    skipped[7] = -1
    check_member(c, got, 1, member_call(c, 1, skipped, adv[1]), shape)
    assert got["stats"][6 + 5] == M
    sa = c.actor.set_floats
    assert not np.array_equal(got["grad_actor"][sa: 2 * sa], clean["grad_actor"][sa: 2 * sa])  # (the sample did count before)
    for s in (0, 2):
        for k in got:
            n = got[k].size // P
            S.assert_bits(got[k][s * n: (s + 1) * n], clean[k][s * n: (s + 1) * n], f"{k} of member {s}")
