"""A population of PPO learners on the device: P independent learners collected and updated by the launches of one
(include/carl_amd.h: carl_ppo_grad_sets, carl_ppo_adv_stats_sets, carl_adam_step_sets).

``PopulationPPO`` trains P independent copies of ``carl_amd.PPO(fused_step=True)`` -- over seeds, learning rates, clip
ranges, entropy coefficients -- on ONE classic-control engine of ``P * lanes_per_set`` lanes.  Member ``s`` owns lanes
``[s * L, (s + 1) * L)`` and has its own actor, critic and ``log_std``, its own minibatch permutation and advantage
statistics, its own gradients and Adam state and its own row of hyperparameters.  Nothing is shared between members but
the launches:

1. ``collect()``: ``PPO.collect()``'s sequence with the stacked on-device actor and critic (``MLPPolicy.on_device``: lane
   ``l`` uses weight set ``l // L``, with ``log_std [P]``) -- ``rollout_policy(deterministic=False, value_net=, gae=)``,
   then one ``context_trace`` launch.
2. ``update()``: per epoch one draw of every member's permutation (an int32 ``[P, n_steps * L]`` tensor of flat sample
   indices from one device generator) and ONE ``ppo_adv_stats_sets`` launch (skipped with ``normalize_advantage=False``);
   per minibatch ``ppo_grad_sets`` (three launches) into one persistent set of ``[P, ...]`` gradient tensors and ONE
   ``adam_step_sets`` launch.  Four launches per minibatch step for the whole population, whatever P is; nothing is read
   back.

Every kernel runs the one-learner kernel's own code once per member, so a member's parameters, Adam state, statistics,
``adv_norm`` and ``grad_norm`` rows are bit-equal to a replay of its minibatches through ``ppo_adv_stats``, ``ppo_grad`` and
``adam_step`` with its one-set networks.

The hyperparameters live on the device: ``hyper`` is a float64 ``[P, 5]`` tensor with the columns ``HYPER_COLUMNS`` = (lr,
clip_range, vf_coef, ent_coef, max_grad_norm); the kernels read member ``s``'s row (clip_range, vf_coef and ent_coef
rounded to float32 once; ``max_grad_norm = +inf``: no clip).  They cannot be validated where they live: ``set_hyper``
validates before it uploads, and a caller that writes ``hyper`` on the device (the explore half of population-based
training) keeps every value finite and ``>= 0``.  ``copy_members`` is the exploit half: member ``i`` takes member
``src[i]``'s parameters, ``log_std``, Adam state and hyper row by plain indexing on the ``[P, ...]`` tensors, with no host
synchronisation.  ``gamma`` and ``lam`` are shared.

Out of scope, and refused: the Brax families (their actor kernel is a unit of its own), ``MixedVecEngine`` pairs, the
gymnasium drop-in, running normalisation (``normalize_inputs`` / ``normalize_reward`` are not parameters), members of
different shapes, an engine whose lane count is not ``P * lanes_per_set``.
"""
from __future__ import annotations

import math
from typing import Sequence

import torch

from carl_amd import _lib
from carl_amd._tensors import is_exact
from carl_amd.brax_policy import BraxMLPPolicy
from carl_amd.policy import MLPPolicy, _engine_of
from carl_amd.ppo import _ResidentPolicy, _resident

HYPER_COLUMNS = _lib.PPO_HYPER_NAMES


def _hyper_column(name: str, values, n_sets: int) -> list:
    """``values`` (a scalar or a sequence of ``n_sets``) as ``n_sets`` validated floats of hyper column ``name``"""
    if name not in HYPER_COLUMNS:
        raise ValueError(f"PopulationPPO: hyperparameter {name!r}: one of {list(HYPER_COLUMNS)}")
    if isinstance(values, torch.Tensor):
        values = values.detach().cpu().tolist()
    if values is None or isinstance(values, (int, float)):
        values = [values] * n_sets
    values = list(values)
    if len(values) != n_sets:
        raise ValueError(f"PopulationPPO: {name} has {len(values)} values, the population has {n_sets} members (a scalar or one "
                         "value per member)")
    out = []
    for v in values:
        if v is None and name == "max_grad_norm":
            v = math.inf  # no clip
        v = float(v)
        if name == "max_grad_norm":
            if not v >= 0.0:
                raise ValueError(f"PopulationPPO: max_grad_norm {v}: >= 0, or None / inf for no clip")
        elif not 0.0 <= v < math.inf:
            raise ValueError(f"PopulationPPO: {name} {v}: finite and >= 0")
        out.append(v)
    return out


class PopulationPPO:
    """``policies`` / ``value_nets``: sequences of P one-set host-built ``MLPPolicy`` objects of one shape for ``env``
    (``head="policy"`` / ``head="value"``, each critic's shift | scale | clip its actor's): the starting parameters of the P
    members.  ``env``: a classic-control ``CARLEnv`` or ``VecEngine`` of exactly ``P * lanes_per_set`` lanes with
    ``auto_reset=True``.  ``lr``, ``clip_range``, ``vf_coef``, ``ent_coef``, ``max_grad_norm`` (None: no clip): a scalar or a
    sequence of P, validated here and kept in ``hyper`` (module docstring).  ``batch_size``: samples per member and minibatch
    (default: a quarter of a member's ``n_steps * lanes_per_set``).  ``seed``: the sample seed of the first collection (one
    more per collection) and the seed of the permutations.  State, all ``[P, ...]`` device tensors: ``actor_params``,
    ``critic_params``, ``log_std``, ``adam_state`` (``{"m", "v", "step" [P], "beta_pow" [P, 2]}``), ``hyper``."""

    def __init__(self, env, policies: Sequence[MLPPolicy], value_nets: Sequence[MLPPolicy], lanes_per_set: int = 256,
                 n_steps: int = 128, n_epochs: int = 4, batch_size: int | None = None, lr=3e-4, clip_range=0.2,
                 ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, gamma: float = 0.99, lam: float = 0.95,
                 normalize_advantage: bool = True, seed: int = 0):
        policies, value_nets = list(policies), list(value_nets)
        P = len(policies)
        if P < 1 or len(value_nets) != P:
            raise ValueError(f"PopulationPPO: {P} policies and {len(value_nets)} value_nets: one actor and one critic per member")
        for p in policies + value_nets:
            if isinstance(p, BraxMLPPolicy):
                raise ValueError("PopulationPPO: Brax policies are out of scope (a population covers the classic-control "
                                 "families only; the Brax actor kernel is a unit of its own)")
            if not isinstance(p, MLPPolicy) or p._on_device or p.n_sets != 1 or p.lanes_per_set is not None:
                raise ValueError("PopulationPPO: policies and value_nets must be one-set host-built MLPPolicy objects")
        try:
            eng, cenv = _engine_of(env)
        except TypeError:
            raise ValueError(f"PopulationPPO: {type(env).__name__} is not a classic-control CARLEnv or VecEngine (Brax engines, "
                             "MixedVecEngine pairs and the gymnasium drop-in are out of scope)") from None
        L = int(lanes_per_set)
        try:  # (MLPPolicy.stack's rule: one family, inputs, shape, activation and head; lanes_per_set a multiple of the quantum)
            actor_host = MLPPolicy.stack(policies, L, head="policy")
            critic_host = MLPPolicy.stack(value_nets, L, head="value")
        except ValueError as e:
            raise ValueError(f"PopulationPPO: the members' networks must have one shape -- {e}") from None
        for p in (actor_host, critic_host):
            if p.family != eng.family or p.obs_dim != eng.D:
                raise ValueError(f"the policy was built for family {p.family}, this engine runs family {eng.family}")
        if eng.n != P * L:
            raise ValueError(f"PopulationPPO: the engine has {eng.n} lanes, {P} members x lanes_per_set {L} need exactly {P * L}")
        if not eng.auto_reset:
            raise ValueError("PopulationPPO needs auto_reset=True (a collection runs through episode ends)")
        eng._check_value_net(actor_host, critic_host)
        self.env, self.engine, self._carl_env = env, eng, cenv
        self.n_sets, self.lanes_per_set = P, L
        self.n_steps, self.n_epochs = int(n_steps), int(n_epochs)
        if self.n_steps < 1 or self.n_epochs < 0:
            raise ValueError(f"PopulationPPO: n_steps {n_steps} < 1 or n_epochs {n_epochs} < 0")
        total = self.n_steps * L
        self.batch_size = max(1, total // 4) if batch_size is None else int(batch_size)
        if not 1 <= self.batch_size <= total:
            raise ValueError(f"batch_size {self.batch_size} outside [1, n_steps x lanes_per_set = {total}]")
        self.gamma, self.lam = float(gamma), float(lam)
        self.normalize_advantage = bool(normalize_advantage)
        self.seed, self.collections = int(seed), 0
        given = {"lr": lr, "clip_range": clip_range, "vf_coef": vf_coef, "ent_coef": ent_coef, "max_grad_norm": max_grad_norm}
        columns = [_hyper_column(name, given[name], P) for name in HYPER_COLUMNS]
        dev = eng.device
        self._templates = (policies[0], value_nets[0])
        self.box = not policies[0].discrete
        self._opt_floats = policies[0].set_floats + value_nets[0].set_floats + (1 if self.box else 0)
        most = int(_lib.load().carl_adam_step_max_floats())
        if self._opt_floats > most:
            raise ValueError(f"PopulationPPO: {self._opt_floats} parameters per member are more than "
                             f"carl_adam_step_max_floats() = {most}")
        self.hyper = torch.tensor(columns, dtype=torch.float64).t().contiguous().to(dev)        # [P, 5]
        self.actor_params = torch.as_tensor(actor_host.params).to(dev).contiguous().clone()     # [P, set_floats]
        self.critic_params = torch.as_tensor(critic_host.params).to(dev).contiguous().clone()
        self.log_std = torch.as_tensor(actor_host.log_std).to(dev).contiguous().clone()         # [P]
        self._actor = _resident(_ResidentPolicy, policies[0], self.actor_params, L, self.log_std if self.box else None)
        self._critic = _resident(_ResidentPolicy, value_nets[0], self.critic_params, L)
        # (Every member's section as built, on the host.  rollout_policy compares the critic's with the actor's; no update
        # changes a section, and copy_members moves the actor's and the critic's by one map, so equality here, checked
        # above, is equality on the device ever after.  After copy_members these copies are no longer the device's rows.)
        self._actor._host_section = actor_host.transform_section().copy()
        self._critic._host_section = critic_host.transform_section().copy()
        self._opt_params = [self.actor_params, self.critic_params] + ([self.log_std] if self.box else [])
        self.adam_state = eng.adam_state(self._opt_params, n_sets=P)
        self._grad_out = {}  # ppo_grad_sets's outputs: allocated by the first minibatch, kept
        self._epoch_idx = None  # the last epoch's permutations, [P, n_steps * L] (minibatches())
        self._gen = torch.Generator(device=dev)
        self._gen.manual_seed(self.seed)
        self._obs0 = None  # the observation the next collection's first action is chosen from
        self._buf = None
        self._ws = eng.ppo_sets_workspace(self._actor, self._critic, self.batch_size)

    # ------------------------------------------------------------------ state
    def member(self, i: int) -> tuple[MLPPolicy, MLPPolicy]:
        """Member ``i``'s actor and critic as one-set host ``MLPPolicy`` objects (device-to-host copies)."""
        i = int(i)
        if not 0 <= i < self.n_sets:
            raise IndexError(f"member {i}: the population has {self.n_sets}")
        ls = float(self.log_std[i].cpu()) if self.box else None
        return (MLPPolicy.unpack(self._templates[0], self.actor_params[i].cpu().numpy(), ls),
                MLPPolicy.unpack(self._templates[1], self.critic_params[i].cpu().numpy()))

    def set_hyper(self, name: str, values) -> None:
        """Column ``name`` of ``hyper`` (one of ``HYPER_COLUMNS``) from a scalar or a sequence of P, validated on the host,
        then uploaded."""
        col = _hyper_column(name, values, self.n_sets)
        self.hyper[:, HYPER_COLUMNS.index(name)] = torch.tensor(col, dtype=torch.float64).to(self.hyper.device)

    def copy_members(self, src: torch.Tensor) -> None:
        """Member ``i`` takes member ``src[i]``'s parameters, ``log_std``, Adam ``m`` / ``v`` / ``step`` / ``beta_pow`` and
        ``hyper`` row: the exploit step of population-based training.  ``src``: an int64 ``[P]`` device tensor with values
        in ``[0, P)`` (not checked: they live on the device).  Plain indexing on the ``[P, ...]`` tensors, no host
        synchronisation; the identity map changes no bit.  The whole packed row moves, the shift | scale | clip section
        included: a network's weights mean nothing under another member's input transform, so member ``i`` then normalises
        its inputs as ``src[i]`` does.  The actor's and the critic's rows move by the same map, so every member's critic
        section stays bit-equal to its actor's, which is all ``rollout_policy`` asks of the two; the host copies of the
        sections it compares are those of construction and are not moved (``src`` is not known on the host) -- read a
        member's current transform from ``member(i)``, not from them."""
        dev = self.engine.device
        if not is_exact(src, dev, torch.int64, (self.n_sets,), contiguous=False):
            raise ValueError(f"copy_members 'src': needs an int64 [{self.n_sets}] tensor on {dev}")
        st = self.adam_state
        for t in [*self._opt_params, *st["m"], *st["v"], st["step"], st["beta_pow"], self.hyper]:
            t.copy_(t[src])  # (the gather is a tensor of its own before the copy)

    # ------------------------------------------------------------------ one iteration
    def collect(self) -> dict:
        """One rollout buffer of the whole population: ``rollout_policy``'s dict plus ``"obs0"`` ``[N, D]`` and
        ``"context_id"`` ``[T, N]``; member ``s``'s samples are columns ``[s * L, (s + 1) * L)``."""
        eng = self.engine
        if self._obs0 is None:
            if self._carl_env is not None:
                self._carl_env.reset()  # (the env's own bookkeeping; the engine's observation buffer is read below)
            else:
                eng.reset()
            self._obs0 = eng.obs.clone()
        ctx0, ep0 = eng.ctx_idx.clone(), eng.episode.clone()
        T = self.n_steps
        buf = eng.rollout_policy(self._actor, T, deterministic=False, sample_seed=self.seed + self.collections,
                                 value_net=self._critic, gae=(self.gamma, self.lam))
        self.collections += 1
        buf["context_id"] = eng.context_trace(ctx0, ep0, buf["terminated"][:T], buf["truncated"][:T])
        buf["obs0"] = self._obs0
        self._obs0 = buf["obs"][T - 1].clone()  # (contiguous [N, D]: the next collection starts from it)
        self._buf = buf
        return buf

    def minibatches(self) -> list:
        """One epoch for every member: the int32 ``[P, b]`` views, in order, of one ``[P, n_steps * L]`` tensor of flat
        sample indices ``t * pitch + lane`` -- row ``s`` a permutation of member ``s``'s own samples, every row drawn from
        one device generator (device tensors)."""
        eng, T, P, L = self.engine, self.n_steps, self.n_sets, self.lanes_per_set
        pitch = int(self._buf["action"].stride(0)) if T > 1 else eng.n
        keys = torch.rand((P, T * L), device=eng.device, generator=self._gen)
        perm = torch.argsort(keys, dim=1)  # (per row: a uniform permutation of the member's T * L samples)
        lane0 = torch.arange(P, device=eng.device).unsqueeze(1) * L
        flat = (torch.div(perm, L, rounding_mode="floor") * pitch + lane0 + perm % L).to(torch.int32)
        self._epoch_idx = flat  # (the minibatches are views of it, in order: what ppo_adv_stats_sets reads)
        return [flat[:, s: s + self.batch_size] for s in range(0, T * L, self.batch_size)]

    def update(self) -> dict:
        """``n_epochs`` passes of every member over the last collection.  Returns ``{"stats" [n_minibatches, P, 6]: per
        minibatch and member the policy loss, value loss, mean entropy, approx_kl, clip fraction and sample count; "adv_norm"
        [n_minibatches, P, 2] float32; "grad_norm" [n_minibatches, P, 2] float64: the norm before the clip and the
        coefficient}`` on the device."""
        if self._buf is None:
            raise RuntimeError("PopulationPPO.update: collect() first")
        eng, buf, dev, P = self.engine, self._buf, self.engine.device, self.n_sets
        total = self.n_steps * self.lanes_per_set
        per_epoch = (total + self.batch_size - 1) // self.batch_size
        n_mb = self.n_epochs * per_epoch
        stats = torch.empty((n_mb, P, 6), dtype=torch.float32, device=dev)
        grad_norm = torch.empty((n_mb, P, 2), dtype=torch.float64, device=dev)
        adv_norm = torch.empty((self.n_epochs, P, per_epoch, 2), dtype=torch.float32, device=dev)  # (the launch's layout)
        if not self.normalize_advantage:
            adv_norm[..., 0], adv_norm[..., 1] = 0.0, 1.0  # (the identity; ppo_grad_sets gets no adv_norm)
        adv = buf["advantage"][: self.n_steps]
        out, k = self._grad_out, 0
        for e in range(self.n_epochs):
            mbs = self.minibatches()
            rows = adv_norm[e]
            if self.normalize_advantage:
                eng.ppo_adv_stats_sets(adv, self._epoch_idx, self.batch_size, 1e-8, out=rows)
            for j, idx in enumerate(mbs):
                out["stats"] = stats[k]
                g = eng.ppo_grad_sets(self._actor, self._critic, buf, buf["obs0"], buf["context_id"], idx=idx, hyper=self.hyper,
                                      adv_norm=rows[:, j] if self.normalize_advantage else None, out=out, workspace=self._ws)
                grads = [g["grad_actor"], g["grad_critic"]] + ([g["grad_log_std"]] if self.box else [])
                eng.adam_step_sets(self._opt_params, grads, self.adam_state, self.hyper, eps=1e-5, norm_out=grad_norm[k])
                k += 1
        return {"stats": stats, "adv_norm": adv_norm.permute(0, 2, 1, 3).reshape(n_mb, P, 2), "grad_norm": grad_norm}

    def learn(self, iterations: int) -> list:
        """``iterations`` times ``collect()`` + ``update()``; returns each iteration's ``{"stats", "adv_norm", "grad_norm",
        "mean_reward" [P]}`` (device tensors; ``mean_reward``: each member's mean per-step reward of the collection)."""
        info = []
        for _ in range(int(iterations)):
            buf = self.collect()
            res = self.update()
            rew = buf["reward"][: self.n_steps]
            res["mean_reward"] = rew.unflatten(1, (self.n_sets, self.lanes_per_set)).mean(dim=(0, 2))
            info.append(res)
        return info
