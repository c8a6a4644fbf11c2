"""A small fp32 MLP evaluated on the device inside the fused rollout (include/carl_amd.h: carl_rollout_policy).

``MLPPolicy`` holds the weights of one policy -- or of several with the same shape (``stack``) -- in the packed layout
the kernel reads, plus the context rows its input starts with.  Its input is what ``FlattenObservation(env)`` gives a
trained agent (the reference's examples/carl_with_sb3.py): gymnasium's ``Dict`` space orders its keys, so "context"
comes before "obs", and inside the context part the feature names are sorted when ``obs_context_as_dict`` is set and
in ``obs_context_features`` order otherwise.  ``VecEngine.rollout_policy`` / ``CARLEnv.rollout_policy`` run it for T
steps; ``evaluate_policy`` runs it for K whole episodes per lane, and ``episode_stats`` reduces those per context.

Packed layout of one weight set (float32): for every layer in order -- the hidden layers, then the head -- ``W[out][in]``
row-major followed by ``b[out]``; then ``shift[n_in]``, ``scale[n_in]`` and one ``clip``; zero padding to a multiple of
four floats.  The kernel computes ``x = clip((x - shift) * scale, -clip, clip)`` (SB3's ``VecNormalize`` with
``scale = 1 / sqrt(var + eps)``), ``h = act(W h + b)`` per hidden layer and a linear head; discrete families take the
first index of the largest head output, Box families the head output itself (the env clips it as usual).

Stochastic policies: ``rollout_policy(..., deterministic=False, sample_seed=s)`` and ``evaluate_policy(...,
deterministic=False, sample_seed=s)`` sample each action on the device instead (include/carl_amd.h:
carl_policy_sampling_t) -- a categorical over the head's logits for discrete families, a diagonal Gaussian with mean
the head output and a state-independent ``log_std`` (``log_std=`` of the constructors, one value per weight set; SB3's
PPO default) for Box families.  The draws are keyed by ``sample_seed`` and by (lane, episode, step in episode), apart
from the reset and context streams; a transitions launch can also return each action's log-probability
(``log_prob=True``), what an on-policy learner (PPO, A2C) stores next to the action.

Value networks: ``head="value"`` (``for_env`` / ``from_sequential`` / ``stack``) builds a critic for the env -- one
scalar output whatever the family's action space.  ``rollout_policy(..., value_net=critic)`` evaluates it inside the
same launch on the inputs the actor sees (include/carl_amd.h: carl_rollout_policy_valued) and ``gae=(gamma, lam)`` adds
advantages and returns from one more launch (carl_gae).  The critic reads the actor's transformed inputs, so its
``input_shift`` / ``input_scale`` / ``input_clip`` must equal the actor's bit for bit.

Weight sets made on the device: ``MLPPolicy.on_device(template, params, lanes_per_set)`` wraps a caller-owned device
tensor ``[n_sets, set_floats]`` in the packed layout as a multi-set policy, with no host copy -- what an on-device
producer of weight sets (``carl_amd.es.EvolutionStrategy``) hands to ``rollout_policy`` / ``evaluate_policy``.

Input normalisation from the device: ``evaluate_policy(..., input_stats=True)`` gathers the sums of every input the
lanes visited inside the launch, and ``InputStats`` keeps their running mean and variance on the device and writes the
``shift`` / ``scale`` they imply into packed weight sets (include/carl_amd.h: carl_policy_stats_merge) -- ARS V2's state
normalisation, which ``carl_amd.es.EvolutionStrategy(normalize_inputs=True)`` runs every generation.

Out of scope: ``MixedVecEngine`` pairs, the gymnasium drop-in (``carl_amd.dropin``) and the
multi-process helpers (``carl_amd.distributed``).  The Brax families have a class and a launch of their own:
``carl_amd.brax_policy.BraxMLPPolicy`` (same packing, through this class) and ``BraxVecEngine.rollout_policy``.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np
import torch

from carl_amd import _lib
from carl_amd._tensors import is_exact

_ACTIVATIONS = {"identity": _lib.POLICY_IDENTITY, "tanh": _lib.POLICY_TANH, "relu": _lib.POLICY_RELU}


def _engine_of(env):
    """(VecEngine, CARLEnv or None) of what the caller passes; refuses the out-of-scope engines."""
    from carl_amd.engine import LaneEngine, VecEngine

    carl_env = None
    eng = env
    if not isinstance(env, LaneEngine) and isinstance(getattr(env, "env", None), LaneEngine):
        carl_env, eng = env, env.env
    if not isinstance(eng, LaneEngine):
        raise TypeError(f"MLPPolicy: {type(env).__name__} is not a classic-control CARLEnv or VecEngine (MixedVecEngine "
                        "pairs, the gymnasium drop-in and the distributed helpers are out of scope of the closed-loop rollout)")
    if not isinstance(eng, VecEngine):
        raise TypeError(f"MLPPolicy: the closed-loop rollout covers the classic-control families only, not "
                        f"{type(eng).__name__}")
    return eng, carl_env


def flattened_context_rows(env, features: Sequence | None = None, engine_of=None) -> tuple[list[int], list]:
    """Context-table rows (and their names, or rows for a bare engine) of the context part of ``FlattenObservation(env)``,
    in its order.  ``features``: a subset to use instead (names for a ``CARLEnv``, table rows for a ``VecEngine``), each of
    which must be a context value the engine makes visible; ``[]``: the policy sees the observation only.  ``engine_of``:
    what resolves (and refuses) ``env`` (default: the classic-control rule)."""
    eng, cenv = (engine_of or _engine_of)(env)
    visible = list(eng.ctx_obs_rows)
    if cenv is None:
        rows = visible if features is None else [int(f) for f in features]
        for r in rows:
            if r not in visible:
                raise ValueError(f"context row {r} is not one of the engine's visible context rows {visible}")
        return rows, list(rows)
    names = list(cenv._table.names)
    vis_names = [names[r] for r in visible]
    if features is None:
        order = sorted(vis_names) if cenv.obs_context_as_dict else vis_names  # (vis_names: obs_context_features order)
    else:
        order = [str(f) for f in features]
        for f in order:
            if f not in vis_names:
                raise ValueError(f"context feature {f!r} is not a visible context row of this env (visible: {vis_names})")
    return [names.index(f) for f in order], order


class MLPPolicy:
    """One or more weight sets of one MLP shape, for one env family (see the module docstring)."""

    _STATS_MERGE = "carl_policy_stats_merge"  # the C entry point InputStats merges this packing rule's policies through

    def __init__(self, family: int, obs_dim: int, ctx_rows: Sequence[int], layers: Sequence, activation: str = "tanh",
                 input_shift=None, input_scale=None, input_clip: float | None = None, context_names: Sequence | None = None,
                 log_std=None, head: str = "policy", info=None):
        """``info``: the family's info record (default: ``carl_family_info(family)``; a subclass for engines that are
        not built-in families passes its engine's)."""
        info = _lib.family_info(int(family)) if info is None else info
        self.family, self.obs_dim = int(family), int(obs_dim)
        self.ctx_rows = [int(r) for r in ctx_rows]
        self.context_names = list(context_names) if context_names is not None else list(self.ctx_rows)
        if activation not in _ACTIVATIONS:
            raise ValueError(f"activation {activation!r}: one of {sorted(_ACTIVATIONS)}")
        self.activation = activation
        if head not in ("policy", "value"):
            raise ValueError(f"head {head!r}: 'policy' or 'value'")
        self.head = head  # "value": a critic -- one scalar output, evaluated next to an actor (rollout_policy(value_net=))
        self.discrete = bool(info.action_is_discrete)
        self.n_in = len(self.ctx_rows) + self.obs_dim
        if len(self.ctx_rows) > _lib.POLICY_MAX_IN or self.n_in > _lib.POLICY_MAX_IN:
            raise ValueError(f"{self.n_in} inputs: at most {_lib.POLICY_MAX_IN}")
        for r in self.ctx_rows:
            if not 0 <= r < info.n_features:
                raise ValueError(f"context row {r} outside the family's table (F = {info.n_features})")
        self.layers = []
        prev = self.n_in
        for k, (W, b) in enumerate(layers):
            W = np.asarray(W, dtype=np.float32)
            b = np.zeros(W.shape[0], np.float32) if b is None else np.asarray(b, dtype=np.float32).reshape(-1)
            if W.ndim != 2 or W.shape[1] != prev or b.shape != (W.shape[0],):
                raise ValueError(f"layer {k}: W {W.shape} / b {b.shape} do not continue from {prev} inputs")
            self.layers.append((W, b))
            prev = W.shape[0]
        if not self.layers:
            raise ValueError("a policy needs at least its head layer")
        self.widths = [W.shape[0] for W, _ in self.layers[:-1]]
        if len(self.widths) > _lib.POLICY_MAX_HIDDEN or any(not 1 <= w <= _lib.POLICY_MAX_WIDTH for w in self.widths):
            raise ValueError(f"hidden widths {self.widths}: at most {_lib.POLICY_MAX_HIDDEN} layers of width <= "
                             f"{_lib.POLICY_MAX_WIDTH}")
        self.n_out = self.layers[-1][0].shape[0]
        want = 1 if head == "value" else int(info.n_actions) if self.discrete else self._box_outputs(info)
        if self.n_out != want:
            kind = "a value network has one output" if head == "value" else "n_actions" if self.discrete else "Box"
            raise ValueError(f"head width {self.n_out}: this family needs {want} ({kind})")
        self.shift = np.zeros(self.n_in, np.float32) if input_shift is None else np.asarray(input_shift, np.float32).reshape(-1)
        self.scale = np.ones(self.n_in, np.float32) if input_scale is None else np.asarray(input_scale, np.float32).reshape(-1)
        if self.shift.shape != (self.n_in,) or self.scale.shape != (self.n_in,):
            raise ValueError(f"input_shift / input_scale need {self.n_in} values")
        self.clip = np.float32(np.inf if input_clip is None else input_clip)
        self.params = self._pack()[None]  # [n_sets, set_floats]
        if log_std is not None and head == "value":
            raise ValueError("log_std: a value network samples nothing")
        if log_std is not None and self.discrete:
            raise ValueError("log_std: Box families only (a discrete policy samples from its logits)")
        ls = np.asarray(log_std.detach().cpu() if isinstance(log_std, torch.Tensor) else (0.0 if log_std is None else log_std),
                        np.float32).reshape(-1)
        if ls.size != 1:
            raise ValueError(f"log_std: one value (state-independent), got {ls.size}")
        self.log_std = ls  # [n_sets] float32: the Gaussian's log standard deviation per weight set (Box families)
        self.lanes_per_set = None  # one set: every lane
        self._on_device = False  # on_device(): params is the caller's device tensor, never copied
        self._dev = {}

    @staticmethod
    def _box_outputs(info) -> int:
        """head width of a Box family's policy"""
        return 1

    # ------------------------------------------------------------------ construction
    @classmethod
    def for_env(cls, env, layers: Sequence, activation: str = "tanh", input_shift=None, input_scale=None,
                input_clip: float | None = None, context_features: Sequence | None = None, log_std=None,
                head: str = "policy") -> "MLPPolicy":
        """A policy for ``env`` (a classic-control ``CARLEnv`` or ``VecEngine``) from explicit ``(W [out, in], b [out])``
        arrays, hidden layers first, the head last.  The input is ``FlattenObservation(env)``'s vector (module docstring);
        ``context_features`` narrows its context part (``[]``: observation only).  ``log_std`` (Box families only; a float
        or a one-element tensor, default 0): the log standard deviation of the sampled Gaussian.  ``head="value"``: a
        value network instead -- the last layer has one output whatever the family's action space."""
        eng, _ = _engine_of(env)
        rows, names = flattened_context_rows(env, context_features)
        return cls(eng.family, eng.D, rows, layers, activation, input_shift, input_scale, input_clip, names, log_std, head)

    @classmethod
    def from_sequential(cls, env, seq: torch.nn.Sequential, **kw) -> "MLPPolicy":
        """The same from a ``torch.nn.Sequential`` of ``Linear`` layers with ``Tanh`` / ``ReLU`` / ``Identity`` between
        them (one activation kind for every hidden layer; nothing after the head but ``Identity``); ``log_std=`` and
        ``head=`` as ``for_env``."""
        linears, acts = [], []
        for m in seq:
            if isinstance(m, torch.nn.Linear):
                linears.append(m)
                acts.append(None)
            elif isinstance(m, (torch.nn.Tanh, torch.nn.ReLU)):
                if not linears or acts[-1] is not None:
                    raise ValueError(f"{type(m).__name__} must follow a Linear layer (one activation per layer)")
                acts[-1] = "tanh" if isinstance(m, torch.nn.Tanh) else "relu"
            elif isinstance(m, torch.nn.Identity):
                continue
            else:
                raise TypeError(f"{type(m).__name__}: the device policy takes Linear / Tanh / ReLU / Identity only")
        if not linears:
            raise ValueError("the Sequential holds no Linear layer")
        if acts[-1] is not None:
            raise ValueError("the head (the last Linear) must be linear: no activation after it")
        kinds = {a or "identity" for a in acts[:-1]}
        if len(kinds) > 1:
            raise ValueError(f"hidden activations {sorted(kinds)}: the device policy applies one kind to every hidden layer")
        layers = [(m.weight.detach().cpu().numpy(), None if m.bias is None else m.bias.detach().cpu().numpy())
                  for m in linears]
        return cls.for_env(env, layers, activation=kinds.pop() if kinds else "tanh", **kw)

    @staticmethod
    def stack(policies: Sequence["MLPPolicy"], lanes_per_set: int, head: str | None = None) -> "MLPPolicy":
        """Several weight sets of one shape: lane ``l`` uses set ``l // lanes_per_set`` (a multiple of
        ``carl_policy_lane_quantum()``, 256 -- the lanes of one workgroup).  ``head``: what every set must be
        (``"policy"`` / ``"value"``; default: whatever the first one is)."""
        if not policies:
            raise ValueError("stack() needs at least one policy")
        p0 = policies[0]
        if any(p._on_device for p in policies):
            raise ValueError("stack(): a policy whose parameters live on the device (on_device) is not stacked on the host")
        if head is not None and any(p.head != head for p in policies):
            raise ValueError(f"stack(head={head!r}): every weight set must have that head")
        key = lambda p: (type(p), p.family, p.ctx_rows, p.obs_dim, [W.shape for W, _ in p.layers], p.activation, p.head)  # noqa: E731
        for p in policies[1:]:
            if key(p) != key(p0):
                raise ValueError("stack(): every weight set must have the same family, inputs, shape and activation")
        q = _lib.load().carl_policy_lane_quantum()
        if lanes_per_set <= 0 or lanes_per_set % q:
            raise ValueError(f"lanes_per_set {lanes_per_set} is not a positive multiple of {q}")
        out = object.__new__(type(p0))
        out.__dict__.update(p0.__dict__)
        out.params = np.concatenate([p.params for p in policies], axis=0)
        out.log_std = np.concatenate([p.log_std for p in policies])
        out.lanes_per_set = int(lanes_per_set)
        out._dev = {}
        return out

    @classmethod
    def on_device(cls, template: "MLPPolicy", params: torch.Tensor, lanes_per_set: int, log_std=None) -> "MLPPolicy":
        """A multi-set policy whose packed block is the caller's device tensor: ``params`` ``[n_sets, set_floats]``,
        contiguous float32 on a GPU, 16-byte aligned, each row one weight set in the packed layout (module docstring) --
        written by whoever owns it, at any time, in stream order; never copied, never read back except for
        ``transform_section``.  ``template``: a one-set host-built policy that gives the family, the context rows, the
        shape, the activation and the head (its own weights are not used).  Lane ``l`` uses set ``l // lanes_per_set``
        (as ``stack``).  ``log_std`` (Box families): a ``[n_sets]`` float32 tensor on the same device, or None: the
        template's value for every set."""
        if not isinstance(template, MLPPolicy) or template._on_device or template.n_sets != 1 or template.lanes_per_set is not None:
            raise ValueError("on_device(): the template must be a one-set host-built MLPPolicy")
        if not isinstance(params, torch.Tensor):
            raise ValueError("on_device(): params must be a torch tensor")
        if params.dtype != torch.float32:
            raise ValueError(f"on_device(): params must be torch.float32, got {params.dtype}")
        if params.dim() != 2 or params.shape[0] < 1 or params.shape[1] != template.set_floats:
            raise ValueError(f"on_device(): params {tuple(params.shape)} is not [n_sets, {template.set_floats}] (the "
                             "template's set_floats)")
        if not params.is_contiguous():
            raise ValueError("on_device(): params must be contiguous")
        if not params.is_cuda:
            raise ValueError(f"on_device(): params must live on a GPU, not on {params.device}")
        if params.data_ptr() % 16:
            raise ValueError("on_device(): params must start on a 16-byte boundary")
        q = _lib.load().carl_policy_lane_quantum()
        if lanes_per_set <= 0 or lanes_per_set % q:
            raise ValueError(f"lanes_per_set {lanes_per_set} is not a positive multiple of {q}")
        ls = template._device_log_std_of(log_std, params)
        out = object.__new__(type(template))
        out.__dict__.update(template.__dict__)
        out.params, out.log_std = params, ls
        out.lanes_per_set = int(lanes_per_set)
        out._on_device = True
        out._dev = {}
        return out

    def _device_log_std_of(self, log_std, params: torch.Tensor) -> torch.Tensor:
        """``on_device``'s ``log_std`` for the sets of ``params`` with this policy as the template: the caller's tensor,
        checked, or the template's values for every set.  One value per set, of shape ``log_std.shape[1:]``."""
        n_sets = int(params.shape[0])
        shape = (n_sets, *self.log_std.shape[1:])
        if log_std is None:
            row = torch.as_tensor(self.log_std[0], dtype=torch.float32, device=params.device)
            return row.expand(shape).contiguous()
        if self.discrete or self.head == "value":
            raise ValueError("log_std: Box policies only")
        ls = log_std
        if (not isinstance(ls, torch.Tensor) or ls.device != params.device or ls.dtype != torch.float32
                or tuple(ls.shape) != shape or not ls.is_contiguous()):
            raise ValueError(f"on_device(): log_std must be a contiguous float32 {list(shape)} tensor on {params.device}")
        return ls

    @staticmethod
    def unpack(template: "MLPPolicy", packed, log_std=None) -> "MLPPolicy":
        """A one-set host policy of ``template``'s family, inputs, shape, activation and head from one packed weight set
        ``[set_floats]`` (host floats; the inverse of the packing, bit for bit, its shift | scale | clip section
        included).  ``log_std``: default the template's."""
        if template._on_device or template.n_sets != 1:
            raise ValueError("unpack(): the template must be a one-set host-built MLPPolicy")
        flat = np.ascontiguousarray(np.asarray(packed, dtype=np.float32).reshape(-1))
        if flat.size != template.set_floats:
            raise ValueError(f"unpack(): {flat.size} floats, the template's weight set has {template.set_floats}")
        layers, off = [], 0
        for W, b in template.layers:
            layers.append((flat[off: off + W.size].reshape(W.shape), flat[off + W.size: off + W.size + b.size]))
            off += W.size + b.size
        n = template.n_in
        if log_std is None and not template.discrete and template.head != "value":
            log_std = float(template.log_std[0])
        return MLPPolicy(template.family, template.obs_dim, template.ctx_rows, layers, template.activation, flat[off: off + n],
                         flat[off + n: off + 2 * n], flat[off + 2 * n], template.context_names, log_std, template.head)

    @property
    def n_sets(self) -> int:
        return int(self.params.shape[0])

    @property
    def weight_floats(self) -> int:
        """Leading floats of a packed weight set that are network parameters: the sum of ``W.size + b.size`` over the
        layers (the shift | scale | clip section and the padding follow)."""
        return int(sum(W.size + b.size for W, b in self.layers))

    @property
    def set_floats(self) -> int:
        """Floats of one packed weight set (``carl_policy_set_floats`` of the shape): a multiple of 4."""
        return int(self.params.shape[1])

    def _pack(self) -> np.ndarray:
        parts = []
        for W, b in self.layers:
            parts += [W.reshape(-1), b]
        parts += [self.shift, self.scale, np.array([self.clip], np.float32)]
        flat = np.concatenate(parts).astype(np.float32)
        pad = (-flat.size) % 4
        return np.concatenate([flat, np.zeros(pad, np.float32)])

    # ------------------------------------------------------------------ C ABI
    def struct(self, n_lanes: int, params_ptr: int | None = None) -> "_lib.Policy":
        """The ``carl_policy_t`` of this policy for a batch of ``n_lanes`` (one set: every lane uses it)."""
        p = _lib.Policy()
        p.n_in, p.n_ctx = self.n_in, len(self.ctx_rows)
        for k, r in enumerate(self.ctx_rows):
            p.ctx_rows[k] = r
        p.n_hidden = len(self.widths)
        for k, w in enumerate(self.widths):
            p.width[k] = w
        p.n_out = self.n_out
        p.activation = _ACTIVATIONS[self.activation]
        p.head = _lib.POLICY_HEAD_ARGMAX if self.discrete and self.head != "value" else _lib.POLICY_HEAD_BOX
        p.n_sets = self.n_sets
        if self.lanes_per_set is None:
            q = int(_lib.load().carl_policy_lane_quantum())
            p.lanes_per_set = max(q, (int(n_lanes) + q - 1) // q * q)
        else:
            p.lanes_per_set = self.lanes_per_set
        p.params = params_ptr
        return p

    def transform_section(self) -> np.ndarray:
        """The shift | scale | clip section of every packed weight set ``[n_sets, 2 * n_in + 1]`` (a view; for an
        ``on_device`` policy a host copy of that section alone: one device-to-host copy)."""
        off = self.weight_floats
        sec = self.params[:, off: off + 2 * self.n_in + 1]
        return sec.cpu().numpy() if self._on_device else sec

    def device_params(self, device) -> torch.Tensor:
        """The packed parameters on ``device`` (uploaded once per device; an ``on_device`` policy returns its own
        tensor, and raises on another device)."""
        if self._on_device:
            return self._own("params", self.params, device)
        return self._upload("params", self.params, device)

    def device_log_std(self, device) -> torch.Tensor:
        """``log_std`` ``[n_sets]`` float32 on ``device`` (uploaded once per device)."""
        if self._on_device:
            return self._own("log_std", self.log_std, device)
        return self._upload("log_std", self.log_std, device)

    def _own(self, key: str, t: torch.Tensor, device) -> torch.Tensor:
        dev = torch.device(device)
        if dev.type != t.device.type or (dev.index is not None and dev.index != t.device.index):
            raise ValueError(f"this policy's {key} live on {t.device}, the launch runs on {dev}")
        return t

    def _upload(self, key: str, a: np.ndarray, device) -> torch.Tensor:
        dev = torch.device(device)
        t = self._dev.get((key, dev))
        if t is None:
            t = torch.as_tensor(a).to(dev).contiguous()
            self._dev[(key, dev)] = t
        return t


class InputStats:
    """Running count, mean and M2 (sum of squared deviations) of a policy's inputs, float64 on the device, merged from
    ``evaluate_policy(..., input_stats=True)`` results by one small launch each (carl_policy_stats_merge) with no host
    synchronisation.  ``template``: a policy of the shape the launches run (its context rows and layer sizes give the
    input count and the offset of the transform section; a ``BraxMLPPolicy`` template takes
    ``evaluate_episodes(..., input_stats=True)`` results and merges through carl_brax_policy_stats_merge).  ``eps``: ``scale = 1 / sqrt(var + eps)``; ``min_std``: an input
    whose variance is at most ``max(min_std^2, (2^-18 |mean|)^2)`` counts as constant and gets ``scale = 0``."""

    def __init__(self, template: MLPPolicy, device, eps: float = 1e-8, min_std: float = 1e-6):
        if not isinstance(template, MLPPolicy):
            raise TypeError("InputStats: the template must be an MLPPolicy")
        if not (0 <= eps < float("inf")) or not (0 <= min_std < float("inf")):
            raise ValueError(f"eps {eps} / min_std {min_std}: finite and >= 0")
        self.template, self.device = template, torch.device(device)
        self.n_in, self.eps, self.min_std = template.n_in, float(eps), float(min_std)
        self._count = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._mean = torch.zeros(_lib.POLICY_MAX_IN, dtype=torch.float64, device=self.device)
        self._m2 = torch.zeros(_lib.POLICY_MAX_IN, dtype=torch.float64, device=self.device)

    @property
    def count(self) -> torch.Tensor:
        """Lane-steps merged so far: an int64 ``[1]`` device tensor."""
        return self._count

    @property
    def mean(self) -> torch.Tensor:
        """``[n_in]`` float64 device tensor."""
        return self._mean[: self.n_in]

    @property
    def var(self) -> torch.Tensor:
        """``M2 / count`` (ddof 0, as VecNormalize), ``[n_in]`` float64 on the device; NaN before the first merge."""
        return self._m2[: self.n_in] / self._count.to(torch.float64)

    def update(self, result: dict, policy_or_block=None, n_write: int | None = None, policy: MLPPolicy | None = None,
               stream: int | None = None) -> None:
        """Merge one ``evaluate_policy(..., input_stats=True)`` result.  ``policy``: the policy that launch ran (default:
        ``policy_or_block`` when that is a policy) -- the merge reads the shift the launch ran under from its weight set
        0, so it must still hold it, and for a policy of several weight sets every set must have carried that same
        shift during the launch (the sums are centred on it; nothing here can check this without a synchronisation --
        ``EvolutionStrategy`` guarantees it, since the perturbation copies the centre's transform into every member).
        Merge a result once: a second ``update`` of the same result counts its lane-steps twice.  ``policy_or_block``: an ``on_device`` policy, or a float32 device tensor of packed
        weight sets (``[set_floats]`` or ``[n, set_floats]``), whose first ``n_write`` sets (default: all) receive the new
        shift and scale; None: only the running state moves.  Stream-ordered on ``stream`` (default: the current one)."""
        partial, steps = result.get("input_partial"), result["steps"]
        if partial is None:
            raise ValueError("InputStats.update: the result has no 'input_partial' (evaluate_policy(..., input_stats=True))")
        block, ran = None, policy
        if isinstance(policy_or_block, MLPPolicy):
            if not policy_or_block._on_device:
                raise ValueError("InputStats.update: a host-built policy is not written on the device (apply_to copies)")
            block, ran = policy_or_block.params, policy_or_block if ran is None else ran
        elif policy_or_block is not None:
            block = policy_or_block
        if ran is None:
            raise ValueError("InputStats.update: policy= (the policy the launch ran) is needed to read its shift")
        S = self.template.set_floats
        if (ran.n_in != self.n_in or ran.weight_floats != self.template.weight_floats or ran.set_floats != S):
            raise ValueError("InputStats.update: the policy's shape is not the template's")
        n_blocks = 0
        if block is not None:
            if not (is_exact(block, self.device, torch.float32, (S,)) or is_exact(block, self.device, torch.float32, (None, S))):
                raise ValueError(f"InputStats.update: the block must be a contiguous float32 [{S}] or [n, {S}] tensor on "
                                 f"{self.device}")
            n_blocks = block.numel() // S
            n_write = n_blocks if n_write is None else int(n_write)
            if not 0 <= n_write <= n_blocks:
                raise ValueError(f"n_write {n_write} outside [0, {n_blocks}]")
        params = ran.device_params(self.device)
        pol = ran.struct(int(steps.numel()), params.data_ptr())
        st = _lib.PolicyStats(partial.data_ptr(), int(partial.shape[0]))
        run = _lib.PolicyRunningStats(self._count.data_ptr(), self._mean.data_ptr(), self._m2.data_ptr())
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        with torch.cuda.device(self.device):
            _lib.check(getattr(_lib.load(), type(self.template)._STATS_MERGE)(
                C.byref(pol), C.byref(st), int(partial.shape[0]), steps.data_ptr(), int(steps.numel()), C.byref(run),
                self.eps, self.min_std, None if block is None else block.data_ptr(), n_write if block is not None else 0,
                stream))

    def transform(self) -> tuple[np.ndarray, np.ndarray]:
        """``(shift, scale)`` float32 ``[n_in]`` the running statistics imply, by the merge's rule, on the host (one
        device-to-host copy)."""
        host = torch.cat([self._count.to(torch.float64), self._mean, self._m2]).cpu().numpy()
        n, mean, m2 = host[0], host[1: 1 + self.n_in], host[1 + _lib.POLICY_MAX_IN: 1 + _lib.POLICY_MAX_IN + self.n_in]
        if n == 0:
            raise ValueError("InputStats: nothing merged yet")
        var = m2 / n
        floor = np.maximum(self.min_std * self.min_std, (2.0 ** -18 * np.abs(mean)) ** 2)
        with np.errstate(divide="ignore"):
            scale = np.where(var <= floor, 0.0, 1.0 / np.sqrt(var + self.eps))
        return mean.astype(np.float32), scale.astype(np.float32)

    def apply_to(self, policy: MLPPolicy) -> MLPPolicy:
        """A one-set host-built policy of ``policy``'s weights (and of its type) with the statistics' shift and scale (its
        clip is kept)."""
        if policy._on_device or policy.n_sets != 1 or policy.n_in != self.n_in:
            raise ValueError("InputStats.apply_to: a one-set host-built policy with the template's inputs")
        shift, scale = self.transform()
        flat = policy.params[0].copy()
        off = policy.weight_floats
        flat[off: off + self.n_in], flat[off + self.n_in: off + 2 * self.n_in] = shift, scale
        return type(policy).unpack(policy, flat)

    def state_dict(self) -> dict:
        """``{"count", "mean", "m2"}`` as host tensors (one copy each)."""
        return {"count": self._count.cpu().clone(), "mean": self._mean[: self.n_in].cpu().clone(),
                "m2": self._m2[: self.n_in].cpu().clone()}

    def load_state_dict(self, state: dict) -> None:
        count, mean, m2 = (torch.as_tensor(state[k]) for k in ("count", "mean", "m2"))
        if count.numel() != 1 or mean.numel() != self.n_in or m2.numel() != self.n_in:
            raise ValueError(f"InputStats.load_state_dict: count [1], mean / m2 [{self.n_in}]")
        self._count.copy_(count.reshape(1).to(torch.int64))
        self._mean.zero_()
        self._m2.zero_()
        self._mean[: self.n_in].copy_(mean.reshape(-1).to(torch.float64))
        self._m2[: self.n_in].copy_(m2.reshape(-1).to(torch.float64))


def episode_stats(result: dict, n_contexts: int | None = None) -> dict:
    """Per-context statistics of an ``evaluate_policy`` result over its finished episodes (slot k of a lane counts when
    k < ``episodes[lane]``), as float64 NumPy arrays after ONE device-to-host copy:
    ``context_count``, ``context_mean_return``, ``context_std_return`` (ddof 0, as SB3 reports it),
    ``context_mean_length`` and ``context_terminated_share``, ``[n_contexts]`` each (default: the largest context id
    + 1), NaN where a context has no episode; ``mean_return`` / ``std_return`` over all episodes (the pair SB3's
    ``evaluate_policy`` returns; NaN without any) and ``count``."""
    keys = ("return", "length", "context_id", "terminated")
    ret = torch.as_tensor(result["return"])
    K, n = (int(s) for s in ret.shape)
    parts = [torch.as_tensor(result[k]).to(torch.float64).reshape(K, n) for k in keys]
    parts.append(torch.as_tensor(result["episodes"]).to(torch.float64).reshape(1, n).to(ret.device))
    host = torch.cat(parts, dim=0).cpu().numpy()  # (every value exact in float64)
    r, ln, cid, te = (host[j * K:(j + 1) * K] for j in range(4))
    valid = np.arange(K)[:, None] < host[4 * K][None, :]
    r, ln, te, cid = r[valid], ln[valid], te[valid], cid[valid].astype(np.int64)
    C_ = (int(cid.max()) + 1 if cid.size else 0) if n_contexts is None else int(n_contexts)
    if cid.size and (cid.min() < 0 or cid.max() >= C_):
        raise ValueError(f"context ids {int(cid.min())} .. {int(cid.max())} outside [0, {C_})")
    count = np.bincount(cid, minlength=C_).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.bincount(cid, weights=r, minlength=C_) / count
        dev = r - mean[cid]
        std = np.sqrt(np.bincount(cid, weights=dev * dev, minlength=C_) / count)
        mean_len = np.bincount(cid, weights=ln, minlength=C_) / count
        term = np.bincount(cid, weights=te, minlength=C_) / count
    nan = np.float64(np.nan)
    return {"context_count": count, "context_mean_return": mean, "context_std_return": std,
            "context_mean_length": mean_len, "context_terminated_share": term,
            "mean_return": np.float64(r.mean()) if r.size else nan, "std_return": np.float64(r.std()) if r.size else nan,
            "count": np.float64(r.size)}
