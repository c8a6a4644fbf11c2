"""What the GPU tests of a population of PPO learners share (test_gpu_ppo_grad_sets.py, test_gpu_ppo_step_sets.py,
test_gpu_population_ppo.py): the common shape -- three members (odd, not a power of two) of 256 lanes, the lane quantum, so
768 lanes; a round-robin selector over 7 contexts, 20-step episodes; T = 5, so a member has 1 280 samples, 5 tiles (a case
may ask for another T and member count: two members and T = 258 reach a second pass of the tile loop) -- the members'
networks, one collected buffer per case and the bit comparison.  A plain module: importing it allocates nothing
and touches no device; a case's engine and buffer are built once and shared, and no test writes into them."""
import functools

import numpy as np
import torch

import policy_cases as PC
import value_cases as VC
from carl_amd import _lib
from carl_amd.policy import MLPPolicy

P, L, T = 3, 256, 5
N = P * L
LOG_STD = (-0.5, 0.0, 0.3)  # three different ones (Box families)
# members differ in every coefficient; one has ent_coef = 0, one clip_range = 0; one no clip, one an active, one an idle clip
HYPER = np.array([[1e-3, 0.2, 0.5, 0.0, np.inf],
                  [3e-4, 0.0, 0.25, 0.01, 1e-3],
                  [1e-2, 0.1, 1.0, 0.02, 1e6]], np.float64)


def make_engine(family, n=N):
    """768 lanes, round robin over 7 contexts, 20-step episodes: test_gpu_ppo_fused.py's classic() engine"""
    return PC.make_engine(family, n, _lib.SEL_ROUND_ROBIN, n_contexts=7, seed=5, max_episode_steps=20)


def make_members(eng, actor_widths, critic_widths, seed=2, n_members=P):
    """n_members actors and critics of one shape with different weights (and transform sections): one-set host policies"""
    rng = np.random.default_rng(seed)
    box = not eng.info.action_is_discrete
    actors = [PC.make_policy(eng, actor_widths, "tanh", rng, ctx="all", clip=5.0, log_std=LOG_STD[s] if box else None)
              for s in range(n_members)]
    critics = [VC.make_critic(eng, a, critic_widths, "tanh", rng) for a in actors]
    return actors, critics


class Case:
    """an engine, its members, their stacks and one collected rollout buffer of T steps (T = 258 with two members: 66 048
    samples per member, 258 tiles, so a minibatch can take the first workgroups of a member's launch through a second tile)"""

    def __init__(self, family, actor_widths, critic_widths, T=T, P=P):
        self.T, self.P = T, P
        self.eng = eng = make_engine(family, P * L)
        self.box = not eng.info.action_is_discrete
        self.actors, self.critics = make_members(eng, actor_widths, critic_widths, n_members=P)
        self.actor = MLPPolicy.stack(self.actors, L, head="policy")
        self.critic = MLPPolicy.stack(self.critics, L, head="value")
        obs0 = eng.obs.clone()
        ctx0, ep0 = eng.ctx_idx.clone(), eng.episode.clone()
        self.buf = buf = eng.rollout_policy(self.actor, T, deterministic=False, sample_seed=3, value_net=self.critic,
                                            gae=(0.99, 0.95))
        self.context_id = eng.context_trace(ctx0, ep0, buf["terminated"][:T], buf["truncated"][:T])
        self.obs0 = obs0
        self.pitch = int(buf["action"].stride(0))
        self.hyper = torch.tensor(HYPER[:P], dtype=torch.float64, device=eng.device)
        torch.cuda.synchronize()

    def member_rows(self, n, seed):
        """int32 [P, n] on the device: row s the first n of a permutation of member s's own flat sample indices"""
        rng = np.random.default_rng(seed)
        rows = []
        for s in range(self.P):
            j = rng.permutation(self.T * L)[:n]
            rows.append((j // L) * self.pitch + s * L + j % L)
        return torch.tensor(np.stack(rows), dtype=torch.int32, device=self.eng.device)

    def coefficients(self, s):
        """member s's clip_range, vf_coef, ent_coef as the float32 values the population kernels round its hyper row to"""
        return {k: float(np.float32(HYPER[s, c])) for k, c in (("clip_range", _lib.PPO_HYPER_CLIP_RANGE),
                                                                ("vf_coef", _lib.PPO_HYPER_VF_COEF),
                                                                ("ent_coef", _lib.PPO_HYPER_ENT_COEF))}


    def host(self):
        """the buffer's columns, context_id and obs0 as NumPy arrays in rows of the buffer's pitch (as the flat indices
        address them), and the context table [F, stride] -- what ppo_ref.sample_inputs / ppo_grad_ref read"""
        T, pitch = self.T, self.pitch
        out = {"obs0": self.obs0.cpu().numpy(), "table": self.eng.ctx_table.cpu().numpy()}
        for k, t in (("context_id", self.context_id), *((k, self.buf[k][:T]) for k in ("obs", "action", "log_prob", "advantage",
                                                                                       "return"))):
            out[k] = torch.as_strided(t, (T, pitch) + tuple(t.shape[2:]), t.stride()).cpu().numpy()
        return out


@functools.lru_cache(maxsize=None)
def case(family, actor_widths, critic_widths, T=T, P=P):
    return Case(family, actor_widths, critic_widths, T, P)


def bits(t):
    """a float32 / float64 / int64 tensor or array as unsigned integers, for a bit comparison"""
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_bits(got, want, what):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)
