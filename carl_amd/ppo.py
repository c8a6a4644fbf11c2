"""PPO on the device: collect, trace, update (include/carl_amd.h: carl_policy_context_trace, carl_ppo_grad; for the Brax
families carl_brax_policy_context_trace, carl_brax_ppo_grad).

``PPO`` runs SB3's PPO (clipped surrogate, value loss, entropy bonus, GAE, advantage normalisation per minibatch, a
global-norm gradient clip, Adam) on a classic-control ``CARLEnv`` or ``VecEngine`` with ``MLPPolicy`` networks, or on a
``CARLBraxEnv`` or ``BraxVecEngine`` with ``BraxMLPPolicy`` networks, as a fixed sequence of launches on the engine's
stream:

1. ``collect()``: clones ``ctx_idx`` / ``episode``, keeps the observation the first action is chosen from, runs
   ``rollout_policy(deterministic=False, value_net=, gae=)`` -- one launch for the T steps of every lane with sampled
   actions, log-probabilities, values, timeout bootstrap values, one for GAE -- and one ``context_trace`` launch that
   rebuilds the context each step ran in (a moving selector changes it at every reset).
2. ``update()``: per epoch a ``torch.randperm`` on the device, sliced into minibatches; per minibatch the advantage mean
   and standard deviation by torch ops on the gathered slice, ``carl_ppo_grad`` (loss and gradients of the actor, the
   critic and ``log_std`` in three launches, no floating-point atomics), the global-norm clip and ``torch.optim.Adam``
   on the packed parameter tensors.  The gradient of a packed tensor's shift | scale | clip entries and padding is +0.0,
   so Adam leaves them untouched.

The actor, the critic and ``log_std`` live on the device as packed tensors, handed to the launches through
``MLPPolicy.on_device``; nothing here reads a result back (``rollout_policy``'s check of the critic's transform section
against the actor's compares the host templates' sections, which no update changes).  ``info`` holds device tensors.

A Brax model is a Box family whose Gaussian is the joint one over the model's actuators: ``log_std`` is ``[1, n_act]``
(one value per actuator), the action column ``[T, N, n_act]`` in dense rows; everything else is the same sequence.

Running normalisation (both off by default; with both off the sequence of launches and every result are as described
above).  ``normalize_inputs=True``: ``collect()`` launches the input sums of the buffer right after the trace
(``ppo_input_stats``: every input the policy acted on, float64); the running merge (``InputStats``) writes the new shift |
scale into ``actor_params`` AFTER the last minibatch of ``update()`` -- the buffer's ``log_prob`` and ``value`` were
computed under the transform the collection ran, and ``ppo_grad`` must see that same transform -- or at the start of the
next ``collect()`` when no update came between, once per collection; the same section is then copied device-to-device
into ``critic_params``, so the two stay bit-equal.  ``normalize_reward=True``: ``collect()`` runs the launch without
``gae=``, walks the discounted return of every lane (``ppo_return_stats``, a persistent per-lane return as in SB3's
VecNormalize), merges its sums into ``return_stats`` and computes the advantages from ``reward_normalized = clamp(reward
* scale, -clip_reward, clip_reward)``: a collection is scaled by the statistics that include it.  ``buf["reward"]``
stays raw.

The fused minibatch step (``fused_step=True``; off by default, and with it off every launch and every result are as
described above).  Per epoch ONE launch gives every minibatch's advantage mean and scale (``ppo_adv_stats``:
carl_ppo_adv_stats, float64 sums in a fixed order; skipped with ``normalize_advantage=False``); per minibatch
``carl_ppo_grad``'s three launches write into one persistent set of gradient tensors and ONE launch clips them by their
global norm and applies Adam to the packed tensors (``adam_step``: carl_adam_step, float64 arithmetic, state in
``adam_state``).  No ``torch.optim.Adam`` exists then (``optimizer`` is None); ``lr`` is read at every step, so a caller may
change it between updates.  ``update()`` also returns each minibatch's ``adv_norm`` row and ``grad_norm`` (the norm
before the clip, the coefficient).

Out of scope, and refused: ``MixedVecEngine`` pairs, the gymnasium drop-in; of the Brax families the models the closed
loop refuses (more than 8 actuators, Humanoid-size inputs beyond ``CARL_POLICY_MAX_IN``) and collection under the
first-state auto-reset (``autoreset_mode="first_state"``: an env's next episode would repeat the previous one's noise).
"""
from __future__ import annotations

import torch

from carl_amd import _lib
from carl_amd.brax_policy import BraxMLPPolicy, _brax_engine_of
from carl_amd.policy import InputStats, MLPPolicy, _engine_of


class _ResidentPolicy(MLPPolicy):
    """An ``on_device`` policy whose shift | scale | clip section is known on the host: the template's, which ``PPO`` never
    changes (its gradient is +0.0).  ``rollout_policy`` compares the critic's section with the actor's at every launch; for
    a plain ``on_device`` policy that is a device-to-host copy."""

    def transform_section(self):
        return self._host_section


class _ResidentBraxPolicy(BraxMLPPolicy):
    """``_ResidentPolicy`` for a Brax model"""

    transform_section = _ResidentPolicy.transform_section


def _resident(cls, template: MLPPolicy, params: torch.Tensor, lanes_per_set: int, log_std=None):
    """``template`` on the device as a ``cls`` (``_ResidentPolicy`` / ``_ResidentBraxPolicy``)"""
    out = cls.on_device(template, params, lanes_per_set, log_std)
    out.__class__ = cls
    out._host_section = template.transform_section().copy()
    return out


_MAX_BRAX_ACT = 8  # actuators of a sampled closed-loop launch (include/carl_amd.h: carl_brax_rollout_policy_sampled)


def _brax_engine_for_ppo(env):
    """(BraxVecEngine, CARLBraxEnv or None), with PPO's refusals of what the Brax closed loop does not cover"""
    try:
        eng, cenv = _brax_engine_of(env)
    except TypeError:
        raise ValueError(f"PPO: {type(env).__name__} is not a CARLBraxEnv or BraxVecEngine (MixedVecEngine pairs and the "
                         "gymnasium drop-in are out of scope of the PPO update)") from None
    if eng.autoreset_mode == "first_state":
        raise ValueError("PPO: autoreset_mode='first_state' (CARL_FLAG_AUTORESET_FIRST_STATE) repeats an env's sampling "
                         "noise in its next episode; PPO collects under the default auto-reset mode")
    if eng.sys.n_act > _MAX_BRAX_ACT:
        raise ValueError(f"PPO: the model has {eng.sys.n_act} actuators, the sampled closed loop holds at most {_MAX_BRAX_ACT}")
    if eng.D > _lib.POLICY_MAX_IN:
        raise ValueError(f"PPO: {eng.D} observations are more than CARL_POLICY_MAX_IN = {_lib.POLICY_MAX_IN} policy inputs "
                         "(Humanoid-size observations are out of scope)")
    return eng, cenv


class PPO:
    """``policy`` / ``value_net``: one-set host-built ``MLPPolicy`` objects for ``env`` (``head="policy"`` /
    ``head="value"``, the critic's shift | scale | clip the actor's) -- the shapes and the starting parameters; for a
    ``CARLBraxEnv`` / ``BraxVecEngine`` they are ``BraxMLPPolicy`` objects, the actor's ``log_std`` one value per actuator.
    ``n_steps``: steps per lane and collection; ``batch_size``: samples per minibatch (default: a quarter of the buffer);
    the other arguments are SB3's.  ``seed``: the sample seed of the first collection (one more per collection) and the
    seed of the minibatch permutations.  ``normalize_inputs`` / ``normalize_reward``: running normalisation of the
    policy's inputs / of the rewards (module docstring); ``clip_reward``: the bound of a scaled reward; ``norm_eps`` (> 0 with
    ``normalize_reward``; with ``normalize_inputs`` a second ``update()`` of one collection is refused): the
    epsilon under both square roots.  ``input_stats`` (an ``InputStats``) and ``return_stats`` (``{"count", "mean",
    "m2", "scale", "ret"}`` device tensors) hold the running state, None where the flag is off.  ``fused_step``: the
    advantage statistics of an epoch in one launch and clip + Adam in one launch per minibatch (module docstring);
    ``adam_state`` (``{"m", "v", "step", "beta_pow"}`` device tensors) then holds the optimiser's state and ``optimizer`` is
    None.  ``lr``: the attribute the fused step reads at every minibatch."""

    def __init__(self, env, policy: MLPPolicy, value_net: MLPPolicy, n_steps: int = 128, n_epochs: int = 4,
                 batch_size: int | None = None, lr: float = 3e-4, gamma: float = 0.99, lam: float = 0.95,
                 clip_range: float = 0.2, vf_coef: float = 0.5, ent_coef: float = 0.0, max_grad_norm: float = 0.5,
                 normalize_advantage: bool = True, seed: int = 0, normalize_inputs: bool = False,
                 normalize_reward: bool = False, clip_reward: float = 10.0, norm_eps: float = 1e-8,
                 fused_step: bool = False):
        self.brax = isinstance(policy, BraxMLPPolicy) or isinstance(value_net, BraxMLPPolicy)
        eng, cenv = _brax_engine_for_ppo(env) if self.brax else _engine_of(env)
        for p, head in ((policy, "policy"), (value_net, "value")):
            if not isinstance(p, MLPPolicy) or p._on_device or p.n_sets != 1 or p.lanes_per_set is not None:
                raise ValueError("PPO: policy and value_net must be one-set host-built MLPPolicy objects")
            if p.head != head:
                raise ValueError(f"PPO: the {'actor' if head == 'policy' else 'critic'} must have head={head!r}")
            if p.family != eng.family or p.obs_dim != eng.D:
                raise ValueError(f"the policy was built for family {p.family}, this engine runs family {eng.family}")
        if not eng.auto_reset:
            raise ValueError("PPO needs auto_reset=True (a collection runs through episode ends)")
        if self.brax:
            eng._check_policy(policy, "PPO")
        eng._check_value_net(policy, value_net)
        self.env, self.engine, self._carl_env = env, eng, cenv
        self.n_steps, self.n_epochs = int(n_steps), int(n_epochs)
        total = self.n_steps * eng.n
        self.batch_size = max(1, total // 4) if batch_size is None else int(batch_size)
        if not 1 <= self.batch_size <= total:
            raise ValueError(f"batch_size {self.batch_size} outside [1, n_steps x n_lanes = {total}]")
        self.gamma, self.lam = float(gamma), float(lam)
        self.clip_range, self.vf_coef, self.ent_coef = float(clip_range), float(vf_coef), float(ent_coef)
        self.max_grad_norm, self.normalize_advantage = max_grad_norm, bool(normalize_advantage)
        self.seed, self.collections = int(seed), 0
        self.normalize_inputs, self.normalize_reward = bool(normalize_inputs), bool(normalize_reward)
        self.clip_reward, self.norm_eps = float(clip_reward), float(norm_eps)
        if not 0.0 < self.clip_reward or self.clip_reward != self.clip_reward:
            raise ValueError(f"clip_reward {clip_reward}: > 0")
        if not 0.0 <= self.norm_eps < float("inf"):
            raise ValueError(f"norm_eps {norm_eps}: finite and >= 0")
        if self.normalize_reward and self.norm_eps == 0.0:
            raise ValueError("norm_eps 0 with normalize_reward: constant returns (all-zero rewards) would give scale = inf, "
                             "and 0 * inf is a NaN the clip does not remove; norm_eps > 0")
        self.lr, self.fused_step = float(lr), bool(fused_step)
        if self.fused_step:  # (what carl_adam_step would refuse at the first minibatch)
            if not 0.0 <= self.lr < float("inf"):
                raise ValueError(f"fused_step: lr {lr}: finite and >= 0")
            if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
                raise ValueError(f"fused_step: max_grad_norm {max_grad_norm}: >= 0, or None for no clip")
        dev = eng.device
        q = int(_lib.load().carl_policy_lane_quantum())
        lanes = max(q, (eng.n + q - 1) // q * q)
        self._templates = (policy, value_net)
        self.actor_params = torch.as_tensor(policy.params).to(dev).contiguous().clone()   # [1, set_floats]
        self.critic_params = torch.as_tensor(value_net.params).to(dev).contiguous().clone()
        self.box = not policy.discrete
        self.log_std = torch.as_tensor(policy.log_std).to(dev).contiguous().clone()        # [1]; a Brax model: [1, n_act]
        resident = _ResidentBraxPolicy if self.brax else _ResidentPolicy
        self._actor = _resident(resident, policy, self.actor_params, lanes, self.log_std if self.box else None)
        self._critic = _resident(resident, value_net, self.critic_params, lanes)
        self._opt_params = [self.actor_params, self.critic_params] + ([self.log_std] if self.box else [])
        if self.fused_step:
            if len(self._opt_params) > _lib.ADAM_MAX_TENSORS:
                raise ValueError(f"fused_step: {len(self._opt_params)} tensors, carl_adam_step takes {_lib.ADAM_MAX_TENSORS}")
            floats, most = sum(p.numel() for p in self._opt_params), int(_lib.load().carl_adam_step_max_floats())
            if floats > most:
                raise ValueError(f"fused_step: {floats} parameters are more than carl_adam_step_max_floats() = {most}")
            self.optimizer, self.adam_state = None, eng.adam_state(self._opt_params)
            self._grad_out = {}  # ppo_grad's outputs: allocated by the first minibatch, kept
        else:
            self.optimizer, self.adam_state = torch.optim.Adam(self._opt_params, lr=self.lr, eps=1e-5), None
        self._epoch_idx = None  # the last epoch's permutation as one contiguous tensor (minibatches())
        self._gen = torch.Generator(device=dev)
        self._gen.manual_seed(self.seed)
        self._obs0 = None  # the observation the next collection's first action is chosen from
        self._buf = None
        self._ws = eng.ppo_workspace(policy, value_net, self.batch_size)
        self.input_stats = InputStats(policy, dev, eps=self.norm_eps) if self.normalize_inputs else None
        self._pending_inputs = None  # the last collection's input sums, until they are merged
        self._input_out, self._return_out = {}, {}  # the slabs and the step counts: allocated by the first collection, kept
        self.return_stats = None
        if self.normalize_reward:
            z = lambda dt, n=1: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
            self.return_stats = {"count": z(torch.int64), "mean": z(torch.float64), "m2": z(torch.float64),
                                 "scale": torch.ones(1, dtype=torch.float32, device=dev), "ret": z(torch.float32, eng.n)}

    # ------------------------------------------------------------------ state
    def actor(self) -> MLPPolicy:
        """The actor as a one-set host ``MLPPolicy`` (device-to-host copies)."""
        if self.brax:  # (BraxMLPPolicy.unpack takes no log_std: through the constructor)
            t = self._templates[0]
            q = BraxMLPPolicy.unpack(t, self.actor_params.cpu().numpy()[0])
            return BraxMLPPolicy(t._info, t.ctx_rows, q.layers, t.activation, q.shift, q.scale, q.clip, t.context_names,
                                 self.log_std.cpu().numpy()[0], t.head)
        ls = float(self.log_std.cpu()[0]) if self.box else None
        return MLPPolicy.unpack(self._templates[0], self.actor_params.cpu().numpy()[0], ls)

    def critic(self) -> MLPPolicy:
        """The critic as a one-set host ``MLPPolicy`` (one device-to-host copy)."""
        unpack = BraxMLPPolicy.unpack if self.brax else MLPPolicy.unpack
        return unpack(self._templates[1], self.critic_params.cpu().numpy()[0])

    def _merge_inputs(self) -> None:
        """The pending collection's input sums into the running statistics, the new shift | scale into the actor's packed
        block and from there into the critic's (two launches, no host synchronisation); once per collection."""
        if self._pending_inputs is None:
            return
        self.input_stats.update(self._pending_inputs, self.actor_params, policy=self._actor)
        self._pending_inputs = None
        n, a0, c0 = self._actor.n_in, self._actor.weight_floats, self._critic.weight_floats
        self.critic_params[0, c0: c0 + 2 * n].copy_(self.actor_params[0, a0: a0 + 2 * n])

    # ------------------------------------------------------------------ one iteration
    def collect(self) -> dict:
        """One rollout buffer: ``rollout_policy``'s dict plus ``"obs0"`` ``[N, D]`` and ``"context_id"`` ``[T, N]``; with
        ``normalize_reward`` also ``"reward_normalized"`` ``[T, N]``, what the advantages were computed from."""
        eng = self.engine
        self._merge_inputs()  # (a collection without an update behind it)
        if self._obs0 is None:
            if self._carl_env is not None:
                self._carl_env.reset()  # (the env's own bookkeeping; the engine's observation buffer is read below)
            else:
                eng.reset()
            self._obs0 = eng.obs.clone()
        ctx0, ep0 = eng.ctx_idx.clone(), eng.episode.clone()
        T = self.n_steps
        buf = eng.rollout_policy(self._actor, self.n_steps, deterministic=False, sample_seed=self.seed + self.collections,
                                 value_net=self._critic, gae=None if self.normalize_reward else (self.gamma, self.lam))
        if self.normalize_reward:
            rs = self.return_stats
            rew, te, tr = buf["reward"][:T], buf["terminated"][:T], buf["truncated"][:T]
            part = eng.ppo_return_stats(rew, te, tr, rs["ret"], self.gamma, out=self._return_out)["return_partial"]
            eng.ppo_return_merge(part, T * eng.n, rs, self.norm_eps, rs["scale"])
            P = int(rew.stride(0)) if T > 1 else eng.n
            rn = torch.empty((T, P), dtype=torch.float32, device=eng.device)[:, : eng.n]  # (the reward rows' pitch)
            torch.mul(rew, rs["scale"], out=rn)
            rn.clamp_(-self.clip_reward, self.clip_reward)
            adv = eng.gae(rn, buf["value"][:T], te, tr, buf["last_value"], self.gamma, self.lam,
                          boot_value=buf["boot_value"][:T])
            buf["reward_normalized"], buf["advantage"], buf["return"] = rn, adv["advantage"], adv["return"]
        self.collections += 1
        buf["context_id"] = eng.context_trace(ctx0, ep0, buf["terminated"][:T], buf["truncated"][:T])
        buf["obs0"] = self._obs0
        if self.normalize_inputs:
            self._pending_inputs = eng.ppo_input_stats(self._actor, buf, buf["obs0"], buf["context_id"], out=self._input_out)
        self._obs0 = buf["obs"][T - 1].clone()  # (contiguous [N, D]: the next collection starts from it)
        self._buf = buf
        return buf

    def minibatches(self):
        """The int32 flat sample indices ``t * pitch + lane`` of one epoch's minibatches, in order (device tensors)."""
        eng, T = self.engine, self.n_steps
        P = int(self._buf["action"].stride(0)) if T > 1 and not self.brax else eng.n  # (a Brax buffer: dense rows)
        perm = torch.randperm(T * eng.n, device=eng.device, generator=self._gen)
        flat = ((perm // eng.n) * P + perm % eng.n).to(torch.int32)
        self._epoch_idx = flat  # (the minibatches are views of it, in order: what ppo_adv_stats reads)
        return [flat[s: s + self.batch_size].contiguous() for s in range(0, T * eng.n, self.batch_size)]

    def update(self) -> dict:
        """``n_epochs`` passes over the last collection.  Returns ``{"stats" [n_minibatches, 6]}``: per minibatch the
        policy loss, value loss, mean entropy, approx_kl, clip fraction and sample count, on the device."""
        if self._buf is None:
            raise RuntimeError("PPO.update: collect() first")
        if self.normalize_inputs and self._pending_inputs is None:
            raise RuntimeError("PPO.update: with normalize_inputs a collection is updated on once -- the first update() "
                               "merged its input statistics, and the buffer's log_prob and value were computed under the "
                               "transform before that merge; collect() first")
        eng, buf = self.engine, self._buf
        if self.fused_step:
            return self._update_fused()
        adv_flat = buf["advantage"]
        P = int(adv_flat.stride(0)) if self.n_steps > 1 else eng.n
        adv_storage = torch.as_strided(adv_flat, (self.n_steps * P,), (1,)) if P != eng.n else adv_flat.reshape(-1)
        stats = []
        for _ in range(self.n_epochs):
            for idx in self.minibatches():
                norm = None
                if self.normalize_advantage and idx.numel() > 1:
                    a = adv_storage[idx.long()]
                    norm = torch.stack([a.mean(), 1.0 / (a.std() + 1e-8)]).contiguous()
                g = eng.ppo_grad(self._actor, self._critic, buf, buf["obs0"], buf["context_id"], idx=idx, adv_norm=norm,
                                 clip_range=self.clip_range, vf_coef=self.vf_coef, ent_coef=self.ent_coef,
                                 workspace=self._ws)  # (sized for batch_size: a last, shorter minibatch needs no more)
                grads = [g["grad_actor"].view_as(self.actor_params), g["grad_critic"].view_as(self.critic_params)]
                if self.box:
                    grads.append(g["grad_log_std"].view_as(self.log_std))
                if self.max_grad_norm is not None:
                    total = torch.sqrt(sum((x.double() ** 2).sum() for x in grads)).float()
                    coef = torch.clamp(float(self.max_grad_norm) / (total + 1e-6), max=1.0)
                    grads = [x * coef for x in grads]
                for p, x in zip(self._opt_params, grads):
                    p.grad = x
                self.optimizer.step()
                stats.append(g["stats"])
        self._merge_inputs()  # (after the last minibatch: every ppo_grad above saw the transform the collection ran)
        return {"stats": torch.stack(stats)}

    def _update_fused(self) -> dict:
        """``update()`` with ``fused_step``: per epoch one ``ppo_adv_stats`` launch, per minibatch ``ppo_grad`` + one
        ``adam_step`` launch.  Returns ``{"stats" [n_minibatches, 6], "adv_norm" [n_minibatches, 2] float32, "grad_norm"
        [n_minibatches, 2] float64: the norm before the clip and the coefficient}`` on the device."""
        eng, buf, dev = self.engine, self._buf, self.engine.device
        total = self.n_steps * eng.n
        per_epoch = (total + self.batch_size - 1) // self.batch_size
        n_mb = self.n_epochs * per_epoch
        stats = torch.empty((n_mb, 6), dtype=torch.float32, device=dev)
        grad_norm = torch.empty((n_mb, 2), dtype=torch.float64, device=dev)
        adv_norm = torch.empty((n_mb, 2), dtype=torch.float32, device=dev)
        if not self.normalize_advantage:
            adv_norm[:, 0], adv_norm[:, 1] = 0.0, 1.0  # (the identity; ppo_grad gets no adv_norm)
        adv = buf["advantage"][: self.n_steps]
        out, k = self._grad_out, 0
        for e in range(self.n_epochs):
            mbs = self.minibatches()
            rows = adv_norm[e * per_epoch: (e + 1) * per_epoch]
            if self.normalize_advantage:
                eng.ppo_adv_stats(adv, self._epoch_idx, self.batch_size, 1e-8, out=rows)
            for j, idx in enumerate(mbs):
                out["stats"] = stats[k]
                g = eng.ppo_grad(self._actor, self._critic, buf, buf["obs0"], buf["context_id"], idx=idx,
                                 adv_norm=rows[j] if self.normalize_advantage else None, clip_range=self.clip_range,
                                 vf_coef=self.vf_coef, ent_coef=self.ent_coef, out=out, workspace=self._ws)
                grads = [g["grad_actor"], g["grad_critic"]] + ([g["grad_log_std"]] if self.box else [])
                eng.adam_step(self._opt_params, grads, self.adam_state, self.lr, eps=1e-5,
                              max_grad_norm=self.max_grad_norm, norm_out=grad_norm[k])
                k += 1
        self._merge_inputs()  # (after the last minibatch, as in update())
        return {"stats": stats, "adv_norm": adv_norm, "grad_norm": grad_norm}

    def learn(self, iterations: int) -> list:
        """``iterations`` times ``collect()`` + ``update()``; returns each iteration's ``{"stats", "mean_reward"}`` (device
        tensors; ``mean_reward``: the mean per-step reward of the collection)."""
        info = []
        for _ in range(int(iterations)):
            buf = self.collect()
            res = self.update()
            res["mean_reward"] = buf["reward"][: self.n_steps].mean()
            info.append(res)
        return info
