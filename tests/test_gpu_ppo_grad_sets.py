"""carl_ppo_grad_sets on the GPU: every member's gradients, grad_log_std and statistics bit-equal to carl_ppo_grad with
that member's one-set networks, index row, adv_norm row and float32-rounded coefficients, on the same buffer.
ppo_net_kernel compares the surrogate and the gradients against exact references (test_gpu_ppo_grad.py, ppo_ref.py); the
population kernels run that kernel's body, so bit equality carries that contract over and no tolerance appears here.

Shapes (ppo_sets_cases.py): P = 3 members of 256 lanes, T = 5 -- 1 280 samples, 5 tiles per member; minibatches of 512 (two
tiles), 300 (a tile and a part of one) and 1 280 (every sample); CartPole (categorical) and Pendulum (Gaussian, three
different log_std); the H = 32 instance ((8, 8) with a (8,) critic), the H = 64 instance and the H = 0 instance (a linear
actor).  Members differ in weights, transform sections and all three coefficients (one ent_coef = 0, one clip_range = 0).
Two more shapes: P = 2, T = 258 with 256 x 256 + 256 + 7 samples per member (the second pass of the tile loop on the 2-D
grid), and a member's row holding another member's samples against the float64 reference over its own samples alone."""
import numpy as np
import pytest
import torch

import ppo_checks as PK
import ppo_ref as R
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
    sizes = {"grad_actor": c.P * c.actor.set_floats, "grad_critic": c.P * c.critic.set_floats, "stats": c.P * 6}
    if c.box:
        sizes["grad_log_std"] = c.P
    return sizes


def shaped(c, out):
    """run_twice's flat canaried outputs as the [P, ...] tensors ppo_grad_sets writes"""
    res = {"grad_actor": out["grad_actor"].view(c.P, -1), "grad_critic": out["grad_critic"].view(c.P, -1),
           "stats": out["stats"].view(c.P, 6)}
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


M_SECOND_PASS = 256 * 256 + 256 + 7  # a member's workgroup 0 runs a full second tile, workgroup 1 one of 7 samples


@pytest.mark.parametrize("shape", ["cartpole-8x8", "pendulum-linear"])
def test_the_second_pass_of_every_member_is_bit_equal_to_the_one_set_call(shape):
    """P = 2 members of 256 lanes, T = 258: 66 048 samples per member and a minibatch of 256 x 256 + 256 + 7 of them, so
    on the grid (256, 2) the workgroups (0, s) and (1, s) of both members run a second tile -- which the one-set kernel's
    own second pass is held to references for in test_gpu_ppo_grad_edges.py"""
    c = S.case(*SHAPES[shape], T=258, P=2)
    assert _lib.load().carl_ppo_grad_workgroups(M_SECOND_PASS) == 256 and M_SECOND_PASS > 256 * _lib.load().carl_ppo_tile()
    idx = c.member_rows(M_SECOND_PASS, seed=3)
    adv = torch.tensor(ADV_NORM[:2], device=c.eng.device)
    got = population_call(c, idx, adv)
    assert [float(v) for v in got["stats"].reshape(2, 6)[:, 5]] == [float(M_SECOND_PASS)] * 2
    for s in range(2):
        check_member(c, got, s, member_call(c, s, idx[s], adv[s]), shape)
    members = got["grad_actor"].reshape(2, -1)
    assert not np.array_equal(members[0], members[1])


@pytest.mark.parametrize("shape", ["cartpole-8x8", "pendulum-linear"])
def test_a_lane_of_another_member_is_skipped_as_the_reference_skips_it(shape):
    """a whole wavefront of member 0's samples, and one at the first position of a tile, in member 2's row: member 2's
    gradients and statistics are the float64 reference's over its own samples alone, times n_valid / M (ppo_ref.rescaled),
    at test_gpu_ppo_grad.py's bounds -- the lane window against the reference itself, not against the one-set kernel's
    handling of a bad index.  (Member 2: clip_range 0.1.  Member 1's clip_range of 0 on a buffer whose ratios are 1 within
    a rounding makes the clip decision a matter of that rounding, which no reference can follow.)"""
    c = S.case(*SHAPES[shape])
    M = 300
    idx = c.member_rows(M, seed=13)
    foreign = idx.clone()
    pos = np.concatenate([np.arange(64, 128), [256]])
    foreign[2, pos] = idx[0, pos]  # (member 0's own samples: inside the buffer, lanes [0, 256))
    adv = torch.tensor(ADV_NORM, device=c.eng.device)
    got = population_call(c, foreign, adv)
    h = c.host()
    valid = np.ones(M, bool)
    valid[pos] = False
    flat = foreign[2].cpu().numpy().astype(np.int64)[valid]
    actor, critic = c.actors[2], c.critics[2]
    pick = lambda a: a.reshape(-1)[flat]  # noqa: E731
    x = R.sample_inputs(actor, h["table"], h["context_id"], h["obs0"], h["obs"], flat, c.pitch)
    k = c.coefficients(2)
    ref = R.rescaled(R.ppo_grad_ref(actor, critic, x, pick(h["action"]), pick(h["log_prob"]), pick(h["advantage"]),
                                    pick(h["return"]), ADV_NORM[2], k["clip_range"], k["vf_coef"], k["ent_coef"]),
                     int(valid.sum()), M)
    sa, sc = c.actor.set_floats, c.critic.set_floats
    mine = {"grad_actor": got["grad_actor"][2 * sa:], "grad_critic": got["grad_critic"][2 * sc:]}
    if c.box:
        mine["grad_log_std"] = got["grad_log_std"][2:]
    worst = PK.grad_units(mine, ref)
    print(f"{shape}: {int(valid.sum())} of {M} samples valid, largest gradient error {worst:.2f} x 2^-24 S (K = {R.K:.0f})")
    assert worst <= R.K
    for v in got.values():
        assert np.isfinite(v).all()
    PK.check_statistics(got["stats"][12:], ref["stats"], M)


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
