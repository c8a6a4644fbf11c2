"""Evolution strategies on the device: perturb, evaluate, update (include/carl_amd.h: carl_es_t).

``EvolutionStrategy`` runs one generation of antithetic ES (Salimans et al. 2017; ``fitness_shaping="difference"`` gives
ARS's raw form, Mania et al. 2018) as a fixed sequence of launches on the engine's stream, with no host synchronisation
and no Python loop over the population:

1. ``carl_es_perturb`` writes the ``P = n_lanes // lanes_per_set`` weight sets ``centre +- sigma * z_i`` straight into the
   packed block an ``MLPPolicy.on_device`` policy points at;
2. the env resets and ``evaluate_policy`` runs every set on its ``lanes_per_set`` lanes in one launch;
3. each set's fitness is the mean over its lanes of the lane's mean finished-episode return (torch, on the device);
4. the fitnesses are shaped into one weight per pair;
5. ``carl_es_gradient`` rebuilds ``sum_i weight[i] * z_i`` by regenerating the noise from its counter -- it is never stored;
6. the centre moves.

The noise is a pure function of (seed, generation, pair, parameter), like every other random stream here, so a
generation does not depend on the GPU count or on how many launches it takes.

Input normalisation (ARS V2): with ``normalize_inputs=True`` the evaluation launch also gathers the sums of every input
every member visited (``evaluate_policy(..., input_stats=True)``), and after the centre has moved one more small launch
merges them into the running mean and variance (``self.input_stats``, ``carl_amd.policy.InputStats``) and writes the
shift and scale they imply into the centre's transform section.  The next generation's ``carl_es_perturb`` carries that
section into every member, so the statistics of generation g act from generation g + 1.  Still no host synchronisation.
``input_stats=`` takes a ready ``InputStats`` for the template's shape in the place of a fresh one -- the statistics of a
checkpoint (``InputStats.load_state_dict``), to resume a run where it stopped -- and is the one route for both families;
``normalize_inputs=True`` is the classic-control shorthand that builds one.

Choosing contexts: with a static selector and a context count that divides ``lanes_per_set``, every member of the
population is evaluated on every context once per episode slot -- the CARL question ES is asked here.

The Brax families: with a ``carl_amd.brax_policy.BraxMLPPolicy`` template on a ``CARLBraxEnv`` or ``BraxVecEngine`` the
same sequence runs over the Brax closed loop -- step 2 is ``evaluate_episodes`` (include/carl_amd.h:
carl_brax_evaluate_policy: exactly K whole episodes per env, each env stopping at its K-th episode end), the other
launches do not depend on the family.  Input normalisation runs through ``input_stats=InputStats(template, device)``:
the launch is then ``evaluate_episodes(..., input_stats=True)`` (carl_brax_evaluate_policy_stats) and the merge
carl_brax_policy_stats_merge, in the same places.  Deterministic actions only: sampling for the Brax families is separate
work.

Out of scope, and refused as ``carl_amd.policy`` refuses them: ``MixedVecEngine`` pairs, the gymnasium drop-in.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable

import torch

from carl_amd import _lib
from carl_amd._tensors import is_exact
from carl_amd.brax_policy import BraxMLPPolicy, _brax_engine_of
from carl_amd.policy import InputStats, MLPPolicy, _engine_of


def centered_rank_weights(fitness: torch.Tensor) -> torch.Tensor:
    """``[P]`` fitness -> ``[P / 2]`` pair weights: rank by a stable ascending argsort (NaN last, as torch sorts),
    ``u_k = rank_k / (P - 1) - 0.5`` in float32, ``weight[i] = u_{2i} - u_{2i+1}``."""
    P = fitness.numel()
    rank = torch.argsort(torch.argsort(fitness, stable=True), stable=True).to(torch.float32)
    u = rank / torch.full_like(rank, float(P - 1)) - 0.5
    return (u[0::2] - u[1::2]).contiguous()


def difference_weights(fitness: torch.Tensor) -> torch.Tensor:
    """``weight[i] = F_{2i} - F_{2i+1}`` (ARS's raw form)."""
    return (fitness[0::2] - fitness[1::2]).contiguous()


def set_fitness(result: dict, n_sets: int) -> torch.Tensor:
    """Fitness ``[n_sets]`` float32 of an ``evaluate_policy`` result whose lanes are ``n_sets`` equal runs: the mean over
    a set's lanes of each lane's mean finished-episode return.  A lane without a finished episode is left out; a set
    without any gets ``-inf``.  Plain torch on the tensors' device (no host synchronisation)."""
    ret, ep = result["return"], result["episodes"]
    K = ret.shape[0]
    valid = torch.arange(K, device=ret.device, dtype=ep.dtype)[:, None] < ep[None, :]
    lane_mean = torch.where(valid, ret, torch.zeros_like(ret)).sum(dim=0) / ep.to(torch.float32)
    has = (ep > 0).view(n_sets, -1)
    lane_mean = lane_mean.view(n_sets, -1)
    total = torch.where(has, lane_mean, torch.zeros_like(lane_mean)).sum(dim=1)
    count = has.sum(dim=1).to(torch.float32)
    return torch.where(count > 0, total / count, torch.full_like(total, float("-inf")))


_SHAPING = {"centered_rank": centered_rank_weights, "difference": difference_weights}


class EvolutionStrategy:
    """One ES generation per ``step`` on a classic-control ``CARLEnv`` or ``VecEngine`` with ``auto_reset`` -- or, with a
    ``BraxMLPPolicy`` template, on a ``CARLBraxEnv`` or ``BraxVecEngine`` (module docstring).

    ``policy``: a one-set ``MLPPolicy`` for ``env`` -- the shape, the inputs and the starting centre (its shift | scale |
    clip section is carried into every member unchanged).  The population is ``P = n_lanes // lanes_per_set`` weight sets,
    even and at least 2; ``n_lanes`` must be exactly ``P * lanes_per_set``.  ``sigma``: the noise scale; ``lr``: the step
    of the default update ``center[:n_noisy] += lr / (P * sigma) * grad``; ``seed``: the Philox key of the noise.
    ``fitness_shaping``: ``"centered_rank"``, ``"difference"`` or a callable ``fitness [P] -> weight [P / 2]`` (float32,
    on the device).  ``optimizer``: a factory ``lambda param: torch.optim.X([param], ...)``: it receives the noisy slice of
    the centre as a leaf tensor, and each step sets its ``.grad = -grad / (P * sigma)`` and calls ``step()`` instead of
    the default update.  ``normalize_inputs``: keep running statistics of the policy inputs and normalise the next
    generation's inputs by them (module docstring); ``stats_eps`` / ``stats_min_std``: ``InputStats``' ``eps`` / ``min_std``.
    ``input_stats``: an ``InputStats`` built for this template's shape on the engine's device, fresh or loaded from a
    checkpoint, to the same effect -- either family; giving both is an error.

    ``center``: the ``[set_floats]`` float32 device tensor of the packed centre (readable at any time; assign a tensor to
    replace its values).  ``generation``: starts at 0, one more per ``step``.  ``population``: the ``on_device`` policy
    the members are written into.  ``input_stats``: the ``InputStats`` given, or built by ``normalize_inputs=True``, else None."""

    def __init__(self, env, policy: MLPPolicy, lanes_per_set: int = 256, sigma: float = 0.1, lr: float = 0.05, seed: int = 0,
                 fitness_shaping: str | Callable = "centered_rank", optimizer: Callable | None = None,
                 normalize_inputs: bool = False, stats_eps: float = 1e-8, stats_min_std: float = 1e-6,
                 input_stats: InputStats | None = None):
        brax = isinstance(policy, BraxMLPPolicy)  # the template's type picks the closed loop: every other one the classic
        if brax and normalize_inputs:
            raise NotImplementedError("EvolutionStrategy: normalize_inputs=True builds the statistics of a classic-control "
                                      "template; for the Brax families pass input_stats=InputStats(template, device)")
        if normalize_inputs and input_stats is not None:
            raise ValueError("EvolutionStrategy: normalize_inputs=True builds an InputStats, input_stats= brings one: give "
                             "one of the two")
        eng, cenv = _brax_engine_of(env) if brax else _engine_of(env)
        if not eng.auto_reset:
            raise ValueError("EvolutionStrategy needs auto_reset=True (evaluate_policy counts whole episodes)")
        if not isinstance(policy, MLPPolicy) or policy._on_device or policy.n_sets != 1 or policy.lanes_per_set is not None:
            raise ValueError("EvolutionStrategy: the template must be a one-set host-built MLPPolicy")
        if policy.head != "policy":
            raise ValueError("EvolutionStrategy: the template must have head='policy'")
        if brax:
            if policy.obs_dim != eng.D or policy.n_out != eng.sys.n_act:
                raise ValueError(f"the policy was built for {policy.obs_dim} observations and {policy.n_out} actuators, "
                                 f"this engine's model has {eng.D} and {eng.sys.n_act}")
        elif policy.family != eng.family or policy.obs_dim != eng.D:
            raise ValueError(f"the policy was built for family {policy.family}, this engine runs family {eng.family}")
        L = int(lanes_per_set)
        q = int(_lib.load().carl_policy_lane_quantum())
        if L <= 0 or L % q:
            raise ValueError(f"lanes_per_set {L} is not a positive multiple of {q}")
        P = eng.n // L
        if eng.n != P * L:
            raise ValueError(f"{eng.n} lanes are not a whole number of sets of {L}: {eng.n - P * L} lanes beyond "
                             f"{P} x {L} would run without a population member")
        if P < 2 or P % 2:
            raise ValueError(f"a population of {P} weight sets ({eng.n} lanes / {L}): it must be even and at least 2 "
                             "(antithetic pairs)")
        if not (sigma > 0 and sigma < float("inf")):
            raise ValueError(f"sigma {sigma}: finite and positive")
        if not callable(fitness_shaping) and fitness_shaping not in _SHAPING:
            raise ValueError(f"fitness_shaping {fitness_shaping!r}: one of {sorted(_SHAPING)} or a callable")
        dev = eng.device
        if input_stats is not None:
            t = input_stats.template if isinstance(input_stats, InputStats) else None
            at = input_stats.device if t is not None else None  # ("cuda" without an index: the engine's)
            if (t is None or type(t) is not type(policy) or t.n_in != policy.n_in or t.weight_floats != policy.weight_floats
                    or t.set_floats != policy.set_floats or at.type != dev.type
                    or (at.index is not None and dev.index is not None and at.index != dev.index)):
                raise ValueError(f"input_stats: an InputStats built for a {type(policy).__name__} of this template's shape "
                                 f"({policy.n_in} inputs, {policy.set_floats} floats per weight set) on {dev}")
        self.env, self.engine, self._carl_env = env, eng, cenv
        self.template, self._brax = policy, brax
        self.lanes_per_set, self.n_sets, self.n_pairs = L, P, P // 2
        self.sigma, self.lr, self.seed = float(sigma), float(lr), int(seed) & (2**64 - 1)
        self.set_floats, self.n_noisy = policy.set_floats, policy.weight_floats
        self.generation = 0
        self._shape = fitness_shaping if callable(fitness_shaping) else _SHAPING[fitness_shaping]
        self._center = torch.as_tensor(policy.params[0]).to(dev).contiguous().clone()
        self._params = torch.empty((P, self.set_floats), dtype=torch.float32, device=dev)
        self.population = MLPPolicy.on_device(policy, self._params, L)
        self._noisy = self._center[: self.n_noisy]  # (a view: the optimizer's parameter)
        self._opt = optimizer(self._noisy) if optimizer is not None else None
        self.lib = _lib.load()
        self.input_stats = InputStats(policy, dev, stats_eps, stats_min_std) if normalize_inputs else input_stats

    # ------------------------------------------------------------------ state
    @property
    def center(self) -> torch.Tensor:
        return self._center

    @center.setter
    def center(self, value) -> None:
        v = torch.as_tensor(value)
        if v.dtype != torch.float32 or tuple(v.shape) != (self.set_floats,):
            raise ValueError(f"center: a float32 [{self.set_floats}] tensor, got {v.dtype} {tuple(v.shape)}")
        self._center.copy_(v)  # (in place: the optimizer's parameter is a view of this storage)

    def policy(self) -> MLPPolicy:
        """The centre as a one-set host ``MLPPolicy`` (one device-to-host copy)."""
        return (BraxMLPPolicy if self._brax else MLPPolicy).unpack(self.template, self._center.cpu().numpy())

    def struct(self, generation: int | None = None) -> "_lib.Es":
        """The ``carl_es_t`` of a generation (default: the next ``step``'s)."""
        es = _lib.Es()
        es.seed = self.seed
        es.generation = (self.generation if generation is None else int(generation)) & 0xFFFFFFFF
        es.n_pairs, es.set_floats, es.n_noisy, es.sigma = self.n_pairs, self.set_floats, self.n_noisy, self.sigma
        return es

    # ------------------------------------------------------------------ one generation
    def step(self, n_episodes: int = 1, max_steps: int = 500, deterministic: bool = True,
             sample_seed: int | None = None) -> dict:
        """One generation: perturb, reset, ``evaluate_policy`` (``n_episodes`` per lane, at most ``max_steps`` steps;
        sampled actions with ``deterministic=False``, keyed by ``sample_seed``, default the generation), fitness, shaping,
        gradient, update (and, with ``input_stats``, the statistics' merge into the centre).  Returns ``{"fitness" [P], "weight" [P / 2], "grad" [n_noisy], "result": evaluate_policy's
        dict}``, every value a device tensor.  No host synchronisation.  A Brax template: ``evaluate_episodes`` in place
        of ``evaluate_policy``, ``deterministic=True`` only (``sample_seed`` has nothing to key)."""
        eng = self.engine
        if self._brax and not deterministic:
            raise ValueError("EvolutionStrategy.step: deterministic=False (sampled actions) is out of scope for the Brax "
                             "families")
        es = self.struct()
        stream = eng._stream()
        with torch.cuda.device(eng.device):
            _lib.check(self.lib.carl_es_perturb(C.byref(es), self._center.data_ptr(), self._params.data_ptr(), None, stream))
        if self._brax:
            kw = dict(input_stats=True) if self.input_stats is not None else {}
            if self._carl_env is not None:
                res = self._carl_env.evaluate_episodes(self.population, n_episodes, max_steps, **kw)
            else:
                eng.reset()
                res = eng.evaluate_episodes(self.population, n_episodes, max_steps, **kw)
        else:
            seed = self.generation if sample_seed is None else int(sample_seed)
            kw = dict(deterministic=deterministic, sample_seed=seed)
            if self.input_stats is not None:
                kw["input_stats"] = True
            if self._carl_env is not None:
                res = self._carl_env.evaluate_policy(self.population, n_episodes, max_steps, **kw)
            else:
                eng.reset()
                res = eng.evaluate_policy(self.population, n_episodes, max_steps, **kw)
        fitness = set_fitness(res, self.n_sets)
        weight = self._shape(fitness)
        if not is_exact(weight, eng.device, torch.float32, (self.n_pairs,), contiguous=False):
            raise ValueError(f"fitness_shaping must return a float32 [{self.n_pairs}] tensor on {eng.device}")
        weight = weight.contiguous()
        grad = torch.empty(self.n_noisy, dtype=torch.float32, device=eng.device)
        with torch.cuda.device(eng.device):
            _lib.check(self.lib.carl_es_gradient(C.byref(es), weight.data_ptr(), grad.data_ptr(), stream))
        scale = self.n_sets * self.sigma
        if self._opt is None:
            self._noisy += grad * (self.lr / scale)
        else:
            self._noisy.grad = grad * (-1.0 / scale)
            self._opt.step()
        if self.input_stats is not None:  # the members still hold the shift this generation ran under
            self.input_stats.update(res, self._center, n_write=1, policy=self.population, stream=stream)
        self.generation += 1
        return {"fitness": fitness, "weight": weight, "grad": grad, "result": res}
