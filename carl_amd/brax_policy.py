"""A small fp32 MLP evaluated inside the Brax rollout kernel (include/carl_amd.h: carl_brax_rollout_policy).

``BraxMLPPolicy`` is ``carl_amd.policy.MLPPolicy`` for the Brax families: the same packed weight sets, built by the same
code, the same input vector -- ``FlattenObservation(env)``: the visible context values, then the observation -- and the
same arithmetic on the device.  What differs is where its sizes come from: a Brax engine is a model table, not one of the
built-in families, so the head width is the model's actuator count (``n_act`` Box outputs, which the env clips as it
clips an action given to ``step``) and the observation width the model's ``obs_dim``, both read from the engine.
``BraxVecEngine.rollout_policy`` / ``CARLBraxEnv.rollout_policy`` run it for T steps in one launch.

``BraxVecEngine.evaluate_episodes`` / ``CARLBraxEnv.evaluate_episodes`` run it for whole episodes -- K per env, each env
stopping at its K-th episode end -- and ``carl_amd.es.EvolutionStrategy`` takes it as its template.  With
``input_stats=True`` that launch also gathers the sums of every input every env visited; ``carl_amd.policy.InputStats``
with a ``BraxMLPPolicy`` template merges them into running statistics on the device (ARS V2's normalisation).

``rollout_policy(..., deterministic=False)`` samples each action from a diagonal Gaussian around the head's outputs
(include/carl_amd.h: carl_brax_rollout_policy_sampled): ``log_std`` holds one state-independent value per weight set and
actuator, as SB3's ``log_std`` parameter does, and ``log_prob=True`` returns each env-step's joint log-probability.

Value networks: ``head="value"`` (the constructor, ``for_env``, ``from_sequential``) builds a critic for the model -- one
output, no ``log_std`` -- packed, stacked and uploaded by the same code.  ``rollout_policy(..., deterministic=False,
value_net=critic)`` evaluates it inside the same launch on the inputs the actor sees (include/carl_amd.h:
carl_brax_rollout_policy_valued): ``"value"``, ``"last_value"`` and the timeout bootstrap ``"boot_value"`` are right
under every context selector, because the launch knows the context each env ran in at every step; ``gae=(gamma, lam)``
adds advantages and returns from one more launch.  That is a PPO collection step with no host synchronisation.  The
critic reads the actor's transformed inputs, so its ``input_shift`` / ``input_scale`` / ``input_clip`` must equal the
actor's bit for bit.

The update runs on the device too: ``carl_amd.PPO`` takes a ``CARLBraxEnv`` / ``BraxVecEngine`` with a ``BraxMLPPolicy``
actor and critic, and ``BraxVecEngine.context_trace`` / ``ppo_grad`` are its two launches (include/carl_amd.h:
carl_brax_policy_context_trace, carl_brax_ppo_grad): the context each step ran in, then the clipped-surrogate loss and the
gradients of the actor, the critic and the per-actuator ``log_std`` for one minibatch.

At most ``CARL_POLICY_MAX_IN`` = 32 inputs: Humanoid's and HumanoidStandup's 244 observations do not fit.  Still out of
scope: a sampled episodes mode (``evaluate_episodes`` and ``EvolutionStrategy`` stay deterministic; ``evaluate_policy``
stays the classic-control families'), a critic next to a deterministic actor, Humanoid-size inputs and ``MixedVecEngine``;
for PPO also more than 8 actuators, collection under the first-state auto-reset and the gymnasium drop-in.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np

from carl_amd.policy import MLPPolicy, flattened_context_rows


def _brax_engine_of(env):
    """(BraxVecEngine, CARLBraxEnv or None) of what the caller passes"""
    from carl_amd.brax_engine import BraxVecEngine

    carl_env, eng = None, env
    if not isinstance(env, BraxVecEngine) and isinstance(getattr(env, "env", None), BraxVecEngine):
        carl_env, eng = env, env.env
    if not isinstance(eng, BraxVecEngine):
        raise TypeError(f"BraxMLPPolicy: {type(env).__name__} is not a CARLBraxEnv or BraxVecEngine (the classic-control "
                        "families take carl_amd.policy.MLPPolicy)")
    return eng, carl_env


class BraxMLPPolicy(MLPPolicy):
    """One or more weight sets of one MLP shape for one Brax model (see the module docstring).  ``info``: the engine's
    info record (``BraxVecEngine.info``); the other parameters are ``MLPPolicy``'s, but ``log_std``: a float or ``[n_act]``
    values (default 0), held as float32 ``[n_sets, n_act]`` -- ``stack`` concatenates the sets' rows, ``on_device(...,
    log_std=)`` takes a ``[n_sets, n_act]`` device tensor and ``device_log_std`` uploads it.  ``head="value"``: a critic --
    the last layer has one output and ``log_std`` is an empty ``[n_sets, 0]`` array (passing one is refused)."""

    _STATS_MERGE = "carl_brax_policy_stats_merge"  # (n_out up to the model's actuators: the Brax packing rule)

    def __init__(self, info, ctx_rows: Sequence[int], layers: Sequence, activation: str = "tanh", input_shift=None,
                 input_scale=None, input_clip: float | None = None, context_names: Sequence | None = None, log_std=None,
                 head: str = "policy"):
        from carl_amd.brax_engine import _BRAX_FAMILY

        super().__init__(_BRAX_FAMILY, info.obs_dim, ctx_rows, layers, activation, input_shift, input_scale, input_clip,
                         context_names, None, head, info=info)
        self._info = info  # (unpack builds its result through this constructor)
        if head == "value":  # a critic samples nothing: no column per actuator (stack / on_device keep the empty shape)
            if log_std is not None:
                raise ValueError("log_std: a value network samples nothing")
            self.log_std = np.zeros((1, 0), np.float32)
            return
        if hasattr(log_std, "detach"):
            log_std = log_std.detach().cpu()
        ls = np.asarray(0.0 if log_std is None else log_std, np.float32).reshape(-1)
        if ls.size not in (1, self.n_out):
            raise ValueError(f"log_std: one value or one per actuator ({self.n_out}), got {ls.size}")
        # [n_sets, n_act] float32: the Gaussian's log standard deviation per weight set and actuator
        self.log_std = np.broadcast_to(ls, (self.n_out,)).copy()[None]

    @staticmethod
    def _box_outputs(info) -> int:
        return int(info.action_dim)  # one output per actuator

    @classmethod
    def for_env(cls, env, layers: Sequence, activation: str = "tanh", input_shift=None, input_scale=None,
                input_clip: float | None = None, context_features: Sequence | None = None, log_std=None,
                head: str = "policy") -> "BraxMLPPolicy":
        """A policy for ``env`` (a ``CARLBraxEnv`` or ``BraxVecEngine``) from explicit ``(W [out, in], b [out])`` arrays,
        hidden layers first, the head (``n_act`` outputs) last; ``context_features`` as ``MLPPolicy.for_env``'s;
        ``log_std``: a float or ``[n_act]`` values (default 0), for sampled launches; ``head="value"``: a critic, whose
        last layer has one output.  (``from_sequential`` passes its keywords, ``log_std=`` and ``head=`` among them,
        through to here.)"""
        eng, _ = _brax_engine_of(env)
        rows, names = flattened_context_rows(env, context_features, _brax_engine_of)
        return cls(eng.info, rows, layers, activation, input_shift, input_scale, input_clip, names, log_std, head)

    @staticmethod
    def unpack(template, packed, log_std=None) -> "BraxMLPPolicy":
        """A one-set host policy of ``template``'s model, inputs, shape and activation from one packed weight set
        ``[set_floats]`` (host floats): the inverse of the packing, bit for bit, its shift | scale | clip section included
        (``MLPPolicy.unpack`` for a Brax template; ``EvolutionStrategy.policy()`` reads the centre through it).  A
        ``log_std`` is refused: evolution strategies on the Brax families stay deterministic, and the result carries the
        default ``log_std`` (zeros)."""
        if not isinstance(template, BraxMLPPolicy):
            raise TypeError(f"BraxMLPPolicy.unpack: the template is a {type(template).__name__}, not a BraxMLPPolicy")
        if log_std is not None:
            raise NotImplementedError("BraxMLPPolicy.unpack: log_std is not unpacked (ES on the Brax families is "
                                      "deterministic); pass log_std= to the constructor, for_env or on_device")
        if template._on_device or template.n_sets != 1:
            raise ValueError("unpack(): the template must be a one-set host-built BraxMLPPolicy")
        flat = np.ascontiguousarray(np.asarray(packed, dtype=np.float32).reshape(-1))
        if flat.size != template.set_floats:
            raise ValueError(f"unpack(): {flat.size} floats, the template's weight set has {template.set_floats}")
        layers, off = [], 0
        for W, b in template.layers:
            layers.append((flat[off: off + W.size].reshape(W.shape), flat[off + W.size: off + W.size + b.size]))
            off += W.size + b.size
        n = template.n_in
        return BraxMLPPolicy(template._info, template.ctx_rows, layers, template.activation, flat[off: off + n],
                             flat[off + n: off + 2 * n], flat[off + 2 * n], template.context_names, head=template.head)
