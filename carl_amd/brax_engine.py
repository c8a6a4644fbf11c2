"""Lane engine for the Brax-locomotion families: a ``LaneEngine`` over a model table
(``carl_brax_sys_t``) instead of a built-in family.  Replaces, for N lanes at once, what
``CARLBraxEnv`` builds with ``brax.envs.create(env_name, backend="spring", batch_size)`` +
``VectorGymWrapper`` (reference: carl/envs/brax/carl_brax_env.py:163-190,
carl/envs/brax/wrappers.py:93-158).  No CPU path."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from carl_amd import _lib
from carl_amd._tensors import is_exact
from carl_amd.engine import LaneEngine, _ptr


@dataclass
class _BraxInfo:
    state_dim: int
    obs_dim: int
    n_features: int
    action_dim: int
    action_is_discrete: int
    n_actions: int
    max_episode_steps: int
    action_low: float
    action_high: float


_BRAX_FAMILY = -1  # ``carl_batch_t.family`` of a Brax batch: none of the built-in families (include/carl_amd.h)


class BraxVecEngine(LaneEngine):
    # optional buffers (None: not built): BraxWalkerGoalWrapper state, the first_state auto-reset's copy, the branch record
    goal_pos = success = first_state = branch_sig = None
    # the last row of the open-loop ``rollout`` that ran since ``obs`` was last written: ``rollout`` stores observations in
    # its own ``[T, N, D]`` output, so ``obs`` is stale after it until ``_flush_obs`` (``rollout_policy`` starts from ``obs``).
    # A VIEW of the caller's output, read when the next ``rollout_policy`` / ``snapshot`` / masked ``reset`` runs: it keeps
    # that output alive until then, and what the caller does to it in between is what gets read (``rollout``'s docstring)
    _obs_pending = None
    _SNAPSHOT = LaneEngine._SNAPSHOT + ("goal_pos", "success", "first_state", "branch_sig")

    def __init__(self, sys_table: _lib.BraxSys, n_features: int, ctx_table, n_lanes: int, device="cuda", *,
                 autoreset_mode: str = "redraw", branch_record: bool = False, generic_substep: bool = False,
                 pose_float32: bool = False, **kw):
        """``autoreset_mode``: what the in-kernel auto-reset does with a done env --
        "redraw" (default): selector advance, new init-state draw, like an explicit reset;
        "first_state": put the env back to the state its last explicit ``reset()`` produced, same context,
        nothing drawn -- brax's ``AutoResetWrapper`` as the reference reaches it (wrappers.py:54-78,121-145).
        ``branch_record``: per-step hash of the physics' discrete decisions (carl_step_io_t::branch_sig).
        ``generic_substep``: planar models step with the general 3-D substep (A/B, tests).
        ``pose_float32``: OPT-IN, never a default: the substeps' pose algebra in float32 -- brax's own precision under JAX's
        default; faster, and off the float64 restatement by more than north_star's 1e-5 (include/carl_amd.h:
        CARL_FLAG_BRAX_FP32).  ``kw``: ``LaneEngine``'s keywords."""
        if autoreset_mode not in ("redraw", "first_state"):
            raise ValueError("autoreset_mode must be 'redraw' or 'first_state'")
        s = sys_table
        if pose_float32 and (s.target_link > 0 or s.push_link > 0):
            raise ValueError("pose_float32 is not built for the reach / push task models")
        info = _BraxInfo(_lib.BRAX_LINK_RECORD * s.n_links, s.obs_dim, int(n_features), s.n_act, 0, 0,
                         s.max_episode_steps, float(min(s.act_lo[: s.n_act])), float(max(s.act_hi[: s.n_act])))
        super().__init__(info, _BRAX_FAMILY, ctx_table, n_lanes, device, **kw, flags=(
            _lib.FLAG_BRAX_GENERIC if generic_substep else 0) | (_lib.FLAG_BRAX_FP32 if pose_float32 else 0) | (
            _lib.FLAG_AUTORESET_FIRST_STATE if autoreset_mode == "first_state" else 0))
        self.sys, self.autoreset_mode = s, autoreset_mode
        dev = self.device
        # Brax state is env-major in HBM ([N][L][20]: per link pose head 7 | pose tail 7 | velocities 6,
        # include/carl_amd.h ABI 8); ``self.state`` is the [20 L, N] VIEW of that storage (the classic-control
        # engine's indexing); ``state64()`` returns it as float64 [N, L, 13].
        self._state_storage = self.state.view(self.n, self.S)  # (the same zeroed memory, env-major)
        self.state = self._state_storage.t()
        if autoreset_mode == "first_state":
            self.first_state = torch.zeros((self.n, self.S), dtype=torch.float32, device=dev)
        if branch_record:
            self.branch_sig = torch.zeros((self.n, 2), dtype=torch.int32, device=dev)
        if s.goal_mode:  # BraxWalkerGoalWrapper state: integrated (x, y) + per-step success flag
            self.goal_pos = torch.zeros((2, self.n), dtype=torch.float32, device=dev)
            self.success = torch.zeros(self.n, dtype=torch.uint8, device=dev)
        self._sync_pointers()
        # device copy of the model table (the kernels stage it into LDS once per workgroup)
        self.sys_dev = torch.frombuffer(bytearray(bytes(s)), dtype=torch.uint8).to(dev)
        self._sys_ref = C.byref(s)
        # launch-shape autotuning: fastest width per launch-length class (_shape_for), a probe is running, the last timings
        self._tuned, self._tuning, self.autotune_ms = {}, False, None

    def _sync_pointers(self) -> None:
        super()._sync_pointers()
        b = self.b
        b.goal_pos, b.success, b.first_state = _ptr(self.goal_pos), _ptr(self.success), _ptr(self.first_state)
        self._io.branch_sig = _ptr(self.branch_sig)

    def _c_reset(self, mask_ptr) -> int:
        return self.lib.carl_brax_reset(C.byref(self.b), _ptr(self.sys_dev), C.byref(self.sys), mask_ptr,
                                        _ptr(self.obs), self._stream())

    def _c_step(self, io) -> int:
        return self.lib.carl_brax_step(C.byref(self.b), _ptr(self.sys_dev), C.byref(self.sys), C.byref(io),
                                       self._stream())

    def _c_step_fast(self, stream: int) -> int:
        return self.lib.carl_brax_step(self._b_ref, self.sys_dev.data_ptr(), self._sys_ref, self._io_ref, stream)

    def _c_rollout(self, io, n_steps: int) -> int:
        return self.lib.carl_brax_rollout(C.byref(self.b), _ptr(self.sys_dev), C.byref(self.sys), C.byref(io),
                                          n_steps, self._stream())

    # ------------------------------------------------------------------ state access
    def state64(self) -> torch.Tensor:
        """The envs' maximal-coordinate state as float64 ``[N, L, 13]`` (per link COM position 3, rotation 4
        (w, x, y, z), linear velocity 3, angular velocity 3): pose = head + tail of the HBM record."""
        L = self.sys.n_links
        rec = self._state_storage.to(torch.float64).reshape(self.n, L, _lib.BRAX_LINK_RECORD)
        return torch.cat([rec[:, :, :7] + rec[:, :, 7:14], rec[:, :, 14:]], dim=2)

    def state_np(self):
        """``state64()`` on the host as ``[N, 13 L]`` float64 (the oracle's layout)"""
        return self.state64().reshape(self.n, 13 * self.sys.n_links).cpu().numpy()

    def set_state64(self, state) -> None:
        """Inverse of ``state64``: ``[N, L, 13]`` (or ``[N, 13 L]``) float64 -> the HBM record (pose split into a
        float32 head and tail; velocities rounded to float32).  Planar models (Halfcheetah, Hopper, Walker2d) are
        stepped by a substep that assumes the state lies in the y = 0 plane -- what ``reset`` produces; a state
        that does not switches the engine to the general substep (``_check_planar_state``).  Direct writes to
        ``eng.state`` bypass that check: pass ``generic_substep=True`` if you write out-of-plane states yourself."""
        L = self.sys.n_links
        st = torch.as_tensor(state, dtype=torch.float64, device=self.device).reshape(self.n, L, 13)
        self._check_planar_state(st)
        # (rotations are taken as given.  The engine's own reset makes its rotations unit quaternions in float64 -- round 6 --
        # because rotation formulas that agree for unit quaternions differ by (|q|^2 - 1) x the vector otherwise; a caller
        # who wants the float64 restatement's numbers to 1e-5 on the first substep passes unit quaternions too.)
        pose = st[:, :, :7]
        head = pose.to(torch.float32)
        tail = (pose - head.to(torch.float64)).to(torch.float32)
        self._state_storage.copy_(torch.cat([head, tail, st[:, :, 7:].to(torch.float32)], dim=2).reshape(self.n, -1))

    def is_planar_model(self) -> bool:
        """True when the library steps this model with the planar substep (Halfcheetah, Hopper, Walker2d: every joint
        axis is +-y and all geometry lies in the y = 0 plane) -- unless ``generic_substep=True`` was passed."""
        return bool(self.lib.carl_brax_model_is_planar(C.byref(self.sys))) and not (self.b.flags & _lib.FLAG_BRAX_GENERIC)

    def _check_planar_state(self, st: torch.Tensor) -> None:
        """The planar substep neither reads nor updates the out-of-plane components of a state (y positions, the x / z
        quaternion components, v_y, w_x, w_z): a caller-provided state that is not planar would silently get wrong
        physics.  Such a state switches this engine to the general 3-D substep, with one warning."""
        if not self.is_planar_model():
            return
        off = torch.stack([st[:, :, 1].abs().amax(), st[:, :, 4].abs().amax(), st[:, :, 6].abs().amax(),
                           st[:, :, 8].abs().amax(), st[:, :, 10].abs().amax(), st[:, :, 12].abs().amax()]).amax()
        if float(off) > 1e-4:  # (reset's float32 kinematics leaves <= 1e-5 out of plane)
            import warnings

            self.b.flags |= _lib.FLAG_BRAX_GENERIC
            warnings.warn(f"set_state64: the state leaves the y = 0 plane of a planar model (largest out-of-plane "
                          f"component {float(off):.3g}); this engine now steps it with the general 3-D substep "
                          "(CARL_FLAG_BRAX_GENERIC)", RuntimeWarning, stacklevel=3)

    def rollout_variant(self) -> int:
        """Brax families have ONE rollout kernel (no staged / direct-store pair): nothing to warn about."""
        return _lib.ROLLOUT_STAGED

    def _row_pitch(self) -> int:
        return self.n  # dense rows: the Brax kernel writes per-env pieces, not 16-byte pieces of lane rows

    def _out_pitch(self, out: dict) -> int:
        r = out["reward"]
        if r.dim() == 2 and r.stride(0) > self.n:
            raise ValueError(f"{type(self).__name__}: dense rows only ({self.n} lanes per row); these output buffers have "
                             f"rows of {int(r.stride(0))} lanes")
        return self.n

    def alloc_rollout(self, n_steps: int, final_obs: bool = False, branch_record: bool = False,
                      action: bool = False) -> dict:
        """``action=True``: plus ``"action"`` ``[T, N, n_act]`` float32, the column ``rollout_policy`` writes."""
        out = super().alloc_rollout(n_steps, final_obs)
        if action:
            out["action"] = torch.empty((n_steps, self.n, self.sys.n_act), dtype=torch.float32, device=self.device)
        if branch_record:
            out["branch_sig"] = torch.zeros((n_steps, self.n, 2), dtype=torch.int32, device=self.device)
        if self.sys.goal_mode:
            out["success"] = torch.zeros((n_steps, self.n), dtype=torch.uint8, device=self.device)
        return out

    def _shape_for(self, n_steps: int) -> None:
        """Once ``autotune`` has been used on this engine, launches keep to the lane-group width that was fastest for THEIR
        length class: launches of >= 4 env steps run the balanced fragment schedule, shorter ones one wavefront per group
        (carl_brax.hip: launch_brax), and the best width differs (Halfcheetah x 32 768: a 2-step probe picks 8 lanes per
        env, 50-step rollouts are 30 % faster at 7).  The class not probed yet is probed on first use (state saved and
        restored; results never depend on the width)."""
        tuned = self._tuned
        if not tuned or self._tuning or torch.cuda.is_current_stream_capturing():
            return  # (never probe inside a hipGraph capture: the width in force is recorded as it is)
        long_launch = n_steps >= 4
        if long_launch not in tuned:  # only after autotune(both_classes=False)
            self._probe_widths(8 if long_launch else 2, 2)
        self.sys.lanes_per_env = tuned[long_launch]

    def step(self, action):
        self._shape_for(1)
        self._obs_pending = None  # (the step writes every lane's observation)
        return super().step(action)

    def reset(self, mask: torch.Tensor | None = None) -> torch.Tensor:
        if mask is None:
            self._obs_pending = None
        else:
            self._flush_obs()  # (a masked reset writes the masked lanes' observations only)
        return super().reset(mask)

    def snapshot(self) -> dict:
        self._flush_obs()
        return super().snapshot()

    def restore(self, snap: dict) -> None:
        super().restore(snap)
        self._obs_pending = None

    def _flush_obs(self) -> None:
        """``obs`` <- the current observation, where an open-loop ``rollout`` left it in its own output"""
        if self._obs_pending is not None:
            self.obs.copy_(self._obs_pending)
            self._obs_pending = None

    def rollout(self, actions, out: dict | None = None) -> dict:
        """``LaneEngine.rollout``.  The kernel does not write ``obs``; the engine remembers the last row of the returned
        ``"obs"`` instead and copies it into ``obs`` when it is next needed (``rollout_policy``, ``snapshot``, a masked
        ``reset``) -- a rollout loop pays no copy.  Until then that row must still hold what this call wrote: a caller who
        normalises ``out["obs"]`` in place, reuses ``out`` for another launch, or replays a ``torch.cuda.graph`` that
        captured this call (the replay does not pass through here) hands the current observation over itself, with
        ``set_current_obs``, before ``rollout_policy``."""
        T = int(actions.shape[0])
        self._shape_for(T)
        res = self._rollout_goal(actions, out) if self.sys.goal_mode else super().rollout(actions, out)
        if T > 0:
            self._obs_pending = res["obs"][T - 1]  # (a view: no copy unless a closed-loop launch follows)
        return res

    def set_current_obs(self, obs: torch.Tensor) -> None:
        """``obs`` <- ``obs`` ``[N, D]``, every env's current observation, for a caller whose last ``rollout`` output no
        longer holds it (``rollout``'s docstring); ``rollout_policy`` then starts from it."""
        self.obs.copy_(obs)
        self._obs_pending = None

    def _rollout_goal(self, actions, out: dict | None) -> dict:
        if out is None:
            out = self.alloc_rollout(int(actions.shape[0]))
        self.b.success = out["success"].data_ptr()  # [T][N] for the duration of this launch
        try:
            return super().rollout(actions, out)
        finally:
            self.b.success = self.success.data_ptr()

    # ------------------------------------------------------------------ launch-shape autotuning
    def lane_widths(self) -> list[int]:
        """Lane-group widths (lanes sharing one env) the library can launch for this model."""
        out = (C.c_int32 * 16)()
        n = self.lib.carl_brax_lane_widths(C.byref(self.sys), int(self.b.flags), out, 16)
        return [int(out[i]) for i in range(n)]

    def autotune(self, n_steps: int = 2, reps: int = 2, both_classes: bool = True) -> int:
        """Time ``carl_brax_rollout`` on THIS batch for every launchable lane-group width and keep
        the fastest (``sys.lanes_per_env``).  The width is a pure scheduling choice -- results are
        bit-identical across widths (tests/test_gpu_brax.py) -- but the best one depends on the
        batch size AND on the launch length: what matters is how evenly ceil(N / envs_per_wave) groups
        fill the resident wave slots of the chip, the instruction count per wave, and -- for batches
        larger than the chip holds at once -- how the kernel's (group, step-range) fragments divide
        (Halfcheetah x 32 768: width 4 wins a 2-step probe, width 7 is 10 % faster at 20 steps:
        ``tools/autotune_probe.py``).  Pass the ``n_steps`` the launches will have (per-call stepping:
        the default); with ``both_classes`` (default) the OTHER launch-length class (>= 4 env steps / shorter) is
        probed here too, so that ``step`` / ``rollout`` never stop to probe -- a probe synchronises the device.
        Every buffer a launch can change is saved and restored around the probe (also when a probe launch raises);
        the probe's actions come from a private generator (the caller's CUDA RNG stream is not advanced)."""
        best = self._probe_widths(n_steps, reps)
        if both_classes:
            other = not (n_steps >= 4)
            if other not in self._tuned:
                self._probe_widths(8 if other else 2, reps)
            self.sys.lanes_per_env = best
        return best

    def _probe_widths(self, n_steps: int, reps: int) -> int:
        saved = self.snapshot()
        width0, tuning0 = int(self.sys.lanes_per_env), self._tuning
        lo, hi = float(min(self.sys.act_lo[: self.sys.n_act])), float(max(self.sys.act_hi[: self.sys.n_act]))
        gen = torch.Generator(device=self.device).manual_seed(0x5EED)
        acts = torch.rand((n_steps, self.n, self.sys.n_act), device=self.device, generator=gen) * (hi - lo) + lo
        out = self.alloc_rollout(n_steps)
        best, best_ms = 0, float("inf")
        timings = {}
        self._tuning = True  # (the probe's own launches keep the width under test)
        try:
            if int(self.episode.max()) == 0:  # never reset: give the probe a valid state
                self.reset()
            for w in self.lane_widths():
                self.sys.lanes_per_env = w
                self.rollout(acts, out)  # warm-up (code object load)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    self.rollout(acts, out)
                e1.record()
                e1.synchronize()
                ms = e0.elapsed_time(e1) / reps
                timings[w] = ms
                if ms < best_ms:
                    best, best_ms = w, ms
        except BaseException:
            self.sys.lanes_per_env = width0  # (a failed probe changes nothing)
            raise
        else:
            self.sys.lanes_per_env = best
            self.autotune_ms = timings
            self._tuned[n_steps >= 4] = best  # per launch-length class (_shape_for)
        finally:
            self._tuning = tuning0
            self.restore(saved)
        return best

    def reset_indexed(self, idx, count):
        raise NotImplementedError("Brax families reset through a lane mask (reset(mask)) or in-kernel auto-reset")

    # ------------------------------------------------------------------ closed-loop rollout
    def _check_policy(self, policy, what: str) -> None:
        """the policy / model checks of the closed-loop launches (``rollout_policy``, ``evaluate_episodes``)"""
        from carl_amd.brax_policy import BraxMLPPolicy

        if not isinstance(policy, BraxMLPPolicy):
            raise TypeError(f"{type(self).__name__}.{what} takes a carl_amd.brax_policy.BraxMLPPolicy, not "
                            f"{type(policy).__name__}")
        if policy.obs_dim != self.D or policy.n_out != self.sys.n_act:
            raise ValueError(f"the policy was built for {policy.obs_dim} observations and {policy.n_out} actuators, this "
                             f"engine's model has {self.D} and {self.sys.n_act}")

    def _check_value_net(self, policy, value_net) -> None:
        """ValueError unless ``value_net`` is a critic the valued launch can run next to ``policy``: a one-output
        ``BraxMLPPolicy`` of this model with the actor's context rows, set layout and -- bit for bit -- transform"""
        from carl_amd.brax_policy import BraxMLPPolicy

        if (not isinstance(value_net, BraxMLPPolicy) or value_net.head != "value" or value_net.n_out != 1
                or value_net.obs_dim != self.D):
            raise ValueError(f"value_net must be a carl_amd.brax_policy.BraxMLPPolicy built with head='value' for this "
                             f"engine's model ({self.D} observations)")
        super()._check_value_net(policy, value_net)  # (the rules the two engines share)

    def rollout_policy(self, policy, n_steps: int, out: dict | None = None, mode: str = "transitions", *,
                       deterministic: bool = True, sample_seed: int = 0, log_prob: bool = False, value_net=None,
                       bootstrap_truncated: bool = True, gae: tuple | None = None) -> dict:
        """``n_steps`` steps in ONE launch, each env's action computed inside the rollout kernel by ``policy`` (a
        ``carl_amd.brax_policy.BraxMLPPolicy``) from the env's current context and observation (include/carl_amd.h:
        carl_brax_rollout_policy).  ``mode="transitions"``: ``rollout``'s dict (``alloc_rollout(T, action=True)`` layout)
        with ``"action"`` ``[T, N, n_act]`` float32, the actions each step took -- ``rollout`` of those actions from the
        same engine state gives the same bits.  ``mode="summary"``: no per-step output; ``{"episodes", "return_sum",
        "length_sum"}`` per lane, needs ``auto_reset``.  The launch starts from ``obs`` -- the observation ``reset`` and
        ``step`` leave there; after an open-loop ``rollout`` its last row is copied in first, read from that rollout's
        output as it is NOW (``rollout``'s docstring: a caller who changed it calls ``set_current_obs``) -- and leaves
        every env's last observation in ``obs``.  No host synchronisation.
        ``deterministic=False``: each action is sampled from a diagonal Gaussian around the head's outputs, of
        ``policy.log_std`` ``[n_sets, n_act]`` (include/carl_amd.h: carl_brax_rollout_policy_sampled), the draws keyed by
        ``sample_seed`` and by (env, episode, step in episode, actuator) -- the same in either mode, however the horizon is
        split into launches; ``"action"`` holds the raw samples, which the step clips as it clips any action, and
        ``rollout`` of them still gives the same bits.  ``log_prob=True`` (sampled, transitions mode) adds ``"log_prob"``
        ``[T, N]`` float32: the joint log-probability of each env-step's action (a buffer in ``out`` is checked like
        ``"action"``).
        ``value_net=critic`` (a ``BraxMLPPolicy`` with ``head="value"``; sampled, transitions mode): the critic runs inside
        the same launch on the inputs the actor sees (include/carl_amd.h: carl_brax_rollout_policy_valued) and the result
        gains ``"value"`` ``[T, N]`` (V of the input each action was chosen from), ``"last_value"`` ``[N]`` (V of each env's
        input after the last step: its current context and observation), ``"log_prob"`` (always) and, with
        ``bootstrap_truncated`` (needs ``auto_reset``), ``"boot_value"`` ``[T, N]``: V of the terminal observation under the
        context the episode ran in where a step ended an episode by truncation alone, +0 elsewhere (SB3's timeout
        bootstrap).  Right under every context selector.  Everything else the launch writes keeps its bits.  Buffers in
        ``out`` are checked like ``"log_prob"``.  ``gae=(gamma, lam)`` adds ``"advantage"`` and ``"return"`` ``[T, N]``
        from one ``gae`` launch of the launch's own columns on the same stream: a PPO collection step."""
        self._check_policy(policy, "rollout_policy")
        if value_net is not None and deterministic:
            raise ValueError("value_net: sampled launches only (deterministic=False); a deterministic valued launch "
                             "is not built for the Brax families")
        log_prob, gae = self._policy_keywords(policy, mode, deterministic, log_prob, value_net, bootstrap_truncated, gae)
        T = int(n_steps)
        if mode == "summary":
            res = self.alloc_policy_summary() if out is None else out
            for k, dt in self._SUMMARY_KEYS:  # (the exact dtypes, where the classic-control engine takes any 4-byte one)
                if not is_exact(res.get(k), self.device, dt, (self.n,)):
                    raise ValueError(f"rollout_policy summary '{k}' must be a contiguous {dt} [{self.n}] tensor on "
                                     f"{self.device}")
            io, summ = None, self._policy_summary(res)
        else:
            res = self.alloc_rollout(T, action=True) if out is None else out
            a = res.get("action")
            if not is_exact(a, self.device, torch.float32, (None, self.n, self.sys.n_act)) or a.shape[0] < T:
                raise ValueError(f"rollout_policy output needs a contiguous float32 'action' [>= {T}, {self.n}, "
                                 f"{self.sys.n_act}] buffer on {self.device}")
            if log_prob:
                self._policy_columns(res, ("log_prob",), T)
            if value_net is not None:
                self._policy_columns(res, ("value", "boot_value") if bootstrap_truncated else ("value",), T)
                self._policy_last_value(res)
            io, summ = C.byref(self._rollout_io(a, _lib.ACTION_F32, res, T)), None
        # (after ``autotune``: the width that was fastest for the OPEN-loop rollout of this length class.  The closed loop
        # has 164 more LDS rows per env and another instruction mix; whether its best width differs is not measured)
        self._shape_for(T)
        self._flush_obs()
        params = policy.device_params(self.device)
        pol = policy.struct(self.n, params.data_ptr())
        head = (C.byref(self.b), _ptr(self.sys_dev), C.byref(self.sys), _ptr(self.obs), C.byref(pol))
        if deterministic:
            fn = self.lib.carl_brax_rollout_policy
        else:  # the sampled twin, with its carl_policy_sampling_t behind the policy
            smp = _lib.PolicySampling(int(sample_seed) & (2**64 - 1), policy.device_log_std(self.device).data_ptr(),
                                      _ptr(res["log_prob"]) if log_prob else None)
            fn, head = self.lib.carl_brax_rollout_policy_sampled, (*head, C.byref(smp))
        tail = ()
        if value_net is not None:  # its valued twin: the critic behind the actor, the three columns behind the summary
            cparams = value_net.device_params(self.device)
            crit = value_net.struct(self.n, cparams.data_ptr())
            vout = _lib.PolicyValue(_ptr(res["value"]), _ptr(res["last_value"]),
                                    _ptr(res["boot_value"]) if bootstrap_truncated else None)
            fn, head, tail = self.lib.carl_brax_rollout_policy_valued, (*head[:5], C.byref(crit), head[5]), (C.byref(vout),)
        goal = self.sys.goal_mode and mode == "transitions"
        if goal:
            self.b.success = res["success"].data_ptr()  # [T][N] for the duration of this launch
        try:
            with torch.cuda.device(self.device):
                _lib.check(fn(*head, io, T, summ, *tail, self._stream()))
        finally:
            if goal:
                self.b.success = self.success.data_ptr()
        if gae is not None:
            self._policy_gae(res, T, gae, bootstrap_truncated)
        return res

    # ---- LaneEngine's PPO hooks (context_trace, ppo_workspace, ppo_grad): the Brax entry points, dense rows, an action
    # column [T, N, n_act], one log_std per actuator
    def _ppo_check_policy(self, policy) -> None:
        self._check_policy(policy, "ppo_grad")

    def _ppo_action_tail(self) -> tuple:
        return (int(self.sys.n_act),)

    def _ppo_log_std_floats(self) -> int:
        return int(self.sys.n_act)

    def _c_context_trace(self, ctx0, ep0, te, tr, T, pitch, out) -> int:
        if pitch != 0:
            raise ValueError(f"{type(self).__name__}.context_trace: dense rows only ({self.n} lanes per row)")
        return self.lib.carl_brax_policy_context_trace(self._b_ref, ctx0, ep0, te, tr, T, out, self._stream())

    def _c_ppo_workspace_floats(self, pol, crit, n_samples) -> int:
        return self.lib.carl_brax_ppo_workspace_floats(pol, crit, n_samples)

    def _c_ppo_grad(self, pb, pol, crit, log_std, po) -> int:
        return self.lib.carl_brax_ppo_grad(pb, self._sys_ref, pol, crit, log_std, po, self._stream())

    def _c_ppo_input_stats(self, pb, pol, st) -> int:
        return self.lib.carl_brax_ppo_input_stats(pb, pol, st, self._stream())

    def ppo_grad_sets(self, *args, **kwargs):
        raise NotImplementedError(f"{type(self).__name__}: ppo_grad_sets (a population of PPO learners, carl_ppo_grad_sets) "
                                  "covers the classic-control families only; the Brax actor kernel is a unit of its own")

    def ppo_sets_workspace(self, *args, **kwargs):
        raise NotImplementedError(f"{type(self).__name__}: ppo_sets_workspace (a population of PPO learners, "
                                  "carl_ppo_grad_sets) covers the classic-control families only")

    def evaluate_policy(self, *args, **kwargs):
        raise NotImplementedError(f"{type(self).__name__}: evaluate_policy (sampling, input statistics) covers the "
                                  "classic-control families only; the episodes mode of the Brax closed-loop rollout is "
                                  "evaluate_episodes")

    def evaluate_episodes(self, policy, n_episodes: int, max_steps: int, out: dict | None = None,
                          input_stats: bool = False) -> dict:
        """Run ``policy`` (a ``BraxMLPPolicy``, deterministic) on every env until the env has finished ``n_episodes``
        episodes or taken ``max_steps`` steps, in ONE launch, from the current engine state (include/carl_amd.h:
        carl_brax_evaluate_policy; a running episode is counted with its full length, ``CARLBraxEnv.evaluate_episodes``
        resets first).  Returns ``alloc_policy_episodes``' dict -- the keys, dtypes and shapes of
        ``VecEngine.evaluate_policy``'s result, so ``carl_amd.policy.episode_stats`` and ``carl_amd.es.set_fitness`` take
        it as it is: ``episodes`` / ``steps`` per env, and per env and episode k < ``episodes`` its fp32 ``return``,
        ``length``, the ``context_id`` it ran in and whether it ``terminated`` (NaN / 0 / -1 / 0 beyond).  An env stops at
        the step that ends its last episode, that step's auto-reset applied (its stored state is the start of the next
        episode), or at ``max_steps``, mid-episode; its records and its state are those of a transitions-mode
        ``rollout_policy`` of as many steps, bit for bit, and a wavefront stops stepping once none of its envs is live.
        The launch starts from ``obs`` and leaves every env's current observation there, as ``rollout_policy`` does.
        Needs ``auto_reset``.  No host synchronisation.  ``input_stats=True``: the launch also gathers, for every live
        env-step, the sums of ``d = x_raw - shift`` and ``d * d`` of every policy input (include/carl_amd.h:
        carl_brax_evaluate_policy_stats); the result gains ``"input_partial"``, the float64 ``[slabs, 2, 32]`` device tensor
        of per-wavefront sums (``carl_brax_policy_stats_slabs`` of them) that ``carl_amd.policy.InputStats.update`` merges,
        as ``VecEngine.evaluate_policy``'s does; with ``input_stats=False`` a reused ``out`` loses that key.  Records and
        engine state are the same bits either way."""
        self._check_policy(policy, "evaluate_episodes")
        K, T, res, eps = self._policy_episodes("evaluate_episodes", n_episodes, max_steps, out)
        self._shape_for(T)  # (as rollout_policy: the width autotune found for the open loop of this length class)
        self._flush_obs()
        params = policy.device_params(self.device)
        pol = policy.struct(self.n, params.data_ptr())
        head = (C.byref(self.b), _ptr(self.sys_dev), C.byref(self.sys), _ptr(self.obs), C.byref(pol), K, T, C.byref(eps))
        if input_stats:
            n_slabs = int(self.lib.carl_brax_policy_stats_slabs(C.byref(self.b), C.byref(self.sys), C.byref(pol), T))
            if n_slabs < 0:
                raise ValueError("evaluate_episodes: this batch and model have no closed-loop launch shape")
            st = self._policy_input_partial("evaluate_episodes", res, n_slabs)
            with torch.cuda.device(self.device):
                _lib.check(self.lib.carl_brax_evaluate_policy_stats(*head, C.byref(st), self._stream()))
            return res
        res.pop("input_partial", None)  # a reused dict must not carry an earlier launch's sums beside this launch's steps
        with torch.cuda.device(self.device):
            _lib.check(self.lib.carl_brax_evaluate_policy(*head, self._stream()))
        return res

    def reset_done(self):
        return self.reset((self.terminated | self.truncated))
