"""Device-resident batch of env lanes: buffers (PyTorch-ROCm tensors) + C-ABI calls.

``LaneEngine`` is what every lane engine does (buffers, contexts, the per-call step, the dense-row fused rollout);
``VecEngine`` is the classic-control engine on top of it, ``carl_amd.brax_engine.BraxVecEngine`` the Brax one.
``VecEngine`` is the object the CARL-shaped envs wrap -- the replacement for the
gymnasium env (+ TimeLimit) that ``CARLGymnasiumEnv`` builds with ``gymnasium.make``
(reference: carl/envs/gymnasium/carl_gymnasium_env.py:63-64) -- for N lanes at once.
PyTorch only provides device memory and streams here; all arithmetic runs in the HIP
library behind include/carl_amd.h.  No CPU fallback exists.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Sequence

import numpy as np
import torch

from carl_amd import _lib
from carl_amd._tensors import is_exact, is_rows, row_layout

_FAMILY_BY_NAME = {
    "cartpole": _lib.CARTPOLE, "pendulum": _lib.PENDULUM, "acrobot": _lib.ACROBOT,
    "mountaincar": _lib.MOUNTAINCAR, "mountaincar_cont": _lib.MOUNTAINCAR_CONT,
}


def _ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


# raw handles straight from torch's C binding (the public wrappers build Stream / device objects: ~1.5 us per call,
# a fifth of an eager step at 65 536 lanes)
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (
    lambda idx: torch.cuda.current_stream(idx).cuda_stream)
_current_device = getattr(torch._C, "_cuda_getDevice", None) or torch.cuda.current_device


class _PreparedRollout(NamedTuple):
    """A ``rollout`` up to its launch (``LaneEngine._prepare_rollout``): actions as converted, output buffers, the
    ``carl_step_io_t`` over both, and the step count."""
    a: torch.Tensor
    dt: int
    out: dict
    io: "_lib.StepIO"
    T: int


class CapturedStep:
    """``LaneEngine.capture_step``: a hipGraph of ``n_steps`` ``carl_step`` launches on a fixed action buffer."""

    def __init__(self, eng: "LaneEngine", action_buffer: torch.Tensor, n_steps: int = 1):
        a, dt = eng._action_tensor(action_buffer, ())
        if a.data_ptr() != action_buffer.data_ptr():
            raise ValueError("capture_step needs the action buffer in its final form (device, dtype, contiguous): "
                             "the graph reads this exact address on every replay")
        self.eng, self.action, self.n_steps = eng, action_buffer, int(n_steps)
        self.graph = None
        if self.n_steps == 1:
            # ONE step per replay: a graph launch costs ~11 us where the prepared eager call costs ~4 (measured, 65 536
            # CartPole lanes) -- the replayable object then IS the eager fast path on the fixed buffer (same results, same
            # interface), and a capture only happens where it pays (n_steps >= 2).
            return
        dev = eng.device
        # the first launch of a kernel loads its code object, which is not capturable: run one real step on
        # the capture stream first, on a snapshot that is put back afterwards
        snap = eng.snapshot()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            eng.step(action_buffer)
            eng.restore(snap)
            with torch.cuda.graph(self.graph, stream=side, capture_error_mode="thread_local"):
                for _ in range(self.n_steps):
                    eng.step(action_buffer)
        torch.cuda.current_stream(dev).wait_stream(side)

    def replay(self):
        if self.graph is None:
            return self.eng.step(self.action)
        self.graph.replay()
        e = self.eng
        e._obs_pending = None  # (BraxVecEngine: the replayed steps wrote every lane's observation)
        return e.obs, e.reward, e.terminated, e.truncated


class LaneEngine:
    """N lanes on one device: what the classic-control engine (``VecEngine``) and the Brax engine
    (``carl_amd.brax_engine.BraxVecEngine``) share.  A subclass computes its family info record (``info``: state / obs /
    action dimensions, feature count, default episode length) and its ``carl_batch_t.family`` value before it calls
    up, and supplies the library calls (``_c_reset``, ``_c_step``, ``_c_step_fast``, ``_c_rollout``), the row pitch of a
    fused rollout's arrays (``_row_pitch``, ``_out_pitch``) and, where it has any, its narrow action formats
    (``_narrow_action``); one whose rows can be longer than the lane count also ``_pad_action_rows``.  ``flags``: the
    subclass's ``CARL_FLAG_*`` bits; every other parameter is described at ``VecEngine``."""

    # every buffer a launch can change (snapshot / restore); a subclass appends its own, None = not built
    _obs_pending = None  # (BraxVecEngine: where the current observation is when ``obs`` does not hold it)
    _SNAPSHOT = ("state", "elapsed", "ctx_idx", "episode", "n_calls", "ep_return", "last_return", "last_length",
                 "episodes_done", "obs", "reward", "terminated", "truncated", "done", "final_obs", "ctx_obs", "fin_count")

    def __init__(self, info, family: int, ctx_table, n_lanes: int, device="cuda", *,
                 selector: int = _lib.SEL_ROUND_ROBIN, selector_stride: int = 1, auto_reset: bool = True,
                 max_episode_steps: int | None = None, seed: int = 0, lane_offset: int = 0,
                 ctx_obs_rows: Sequence[int] | None = None, ctx_idx0=None, fin_capacity: int = 0,
                 context_offset: int | None = None, flags: int = 0):
        self.lib = _lib.load()
        self.family, self.info = int(family), info
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.CarlHipError(
                f"{type(self).__name__} needs a ROCm device (got {self.device}); there is no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.n = int(n_lanes)
        S, D, F = self.info.state_dim, self.info.obs_dim, self.info.n_features
        self.S, self.D, self.F = S, D, F
        self._action_dim = int(self.info.action_dim)
        dev = self.device
        i32, f32 = torch.int32, torch.float32

        self.state = torch.zeros((S, self.n), dtype=f32, device=dev)
        self.elapsed = torch.zeros(self.n, dtype=i32, device=dev)
        self.episode = torch.zeros(self.n, dtype=i32, device=dev)  # uint32 bits
        self.n_calls = torch.zeros(self.n, dtype=i32, device=dev)
        self.ep_return = torch.zeros(self.n, dtype=f32, device=dev)
        self.last_return = torch.zeros(self.n, dtype=f32, device=dev)
        self.last_length = torch.zeros(self.n, dtype=i32, device=dev)
        self.episodes_done = torch.zeros(self.n, dtype=i32, device=dev)
        # step outputs (reused every call: returned tensors alias these buffers).  ONE allocation, the five outputs are
        # views of it: a scalar caller (num_envs = 1, the reference's return types) then reads a whole transition back with
        # one device-to-host copy instead of four (`read_transition`; per_call.dropin of the bench line: 84 -> ~40 us)
        def up(x):  # every view starts on a 256-byte boundary, like an allocation of its own
            return (x + 255) & ~255

        o_rew = up(4 * self.n * D)
        o_term = up(o_rew + 4 * self.n)
        o_trunc = up(o_term + self.n)
        o_done = up(o_trunc + self.n)
        self._out_offsets = (o_rew, o_term, o_trunc, o_done)
        self._out_slab = torch.zeros(up(o_done + self.n), dtype=torch.uint8, device=dev)
        self.obs = self._out_slab[: 4 * self.n * D].view(f32).view(self.n, D)
        self.reward = self._out_slab[o_rew: o_rew + 4 * self.n].view(f32)
        self.terminated = self._out_slab[o_term: o_term + self.n]
        self.truncated = self._out_slab[o_trunc: o_trunc + self.n]
        self.done = self._out_slab[o_done: o_done + self.n]  # terminated | truncated of the last step()
        self._out_host = None  # pinned mirror of the slab, made on first use (read_transition)
        self.final_obs = torch.zeros((self.n, D), dtype=f32, device=dev)
        # finished-episode log
        self.fin_capacity = int(fin_capacity)
        if self.fin_capacity > 0:
            self.fin_count = torch.zeros(1, dtype=i32, device=dev)
            self.fin_lane = torch.zeros(self.fin_capacity, dtype=torch.int64, device=dev)
            self.fin_return = torch.zeros(self.fin_capacity, dtype=f32, device=dev)
            self.fin_length = torch.zeros(self.fin_capacity, dtype=i32, device=dev)
        else:
            self.fin_count = self.fin_lane = self.fin_return = self.fin_length = None

        self.b = _lib.Batch()
        self.b.family = self.family
        self.b.n_lanes = self.n
        self.b.max_episode_steps = self.info.max_episode_steps if max_episode_steps is None else int(max_episode_steps)
        self.b.selector = int(selector)
        self.b.selector_stride = int(selector_stride)
        self.b.flags = (_lib.FLAG_AUTORESET if auto_reset else 0) | int(flags)
        self.b.lane_offset = int(lane_offset)
        self.b.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        # global id of context-table row 0 (see default_ctx_idx); None: decided per table
        self.context_offset = None if context_offset is None else int(context_offset)

        self.ctx_obs_rows = list(range(F)) if ctx_obs_rows is None else [int(r) for r in ctx_obs_rows]
        if len(self.ctx_obs_rows) > _lib.CARL_MAX_CTX_OBS:
            raise ValueError(f"at most {_lib.CARL_MAX_CTX_OBS} observed context features")
        self.ctx_obs = torch.zeros((len(self.ctx_obs_rows), self.n), dtype=f32, device=dev)
        self.ctx_table = None
        self.ctx_idx = None
        self._io = _lib.StepIO()
        self.set_contexts(ctx_table, ctx_idx0)  # (fills in every pointer: _sync_pointers)
        # per-call fast path (see step()): everything the ctypes call needs, prepared once
        self._dev_index = int(self.device.index)
        self._b_ref, self._io_ref = C.byref(self.b), C.byref(self._io)
        self._last_action = None
        self._last_action_meta = None
        self._a_host = None  # pinned staging buffer of stage_scalar_action, made on first use
        self._a_pending = False

    # ------------------------------------------------------------------ contexts
    def default_ctx_idx(self, n_contexts: int) -> torch.Tensor:
        """Context row each lane holds before its first reset: global lane g starts on global context
        ``g mod C_global`` (round robin: one stride earlier, so that the first reset lands there).  The LOCAL
        table may be a shard of the global one (multi-GPU: ``distributed.shard_context_rows``); row 0 of it has
        the global id ``context_offset``.  ``context_offset=None`` (default): a table with exactly one row per
        lane is this rank's own slice of a lane <-> context identity (row 0 = context ``lane_offset``), any
        other table is the whole, replicated context set (row 0 = context 0).  With the modulo taken on the
        global id instead -- as round 1 did -- an uneven split (10 lanes over 3 ranks: offset 4, count 3) read
        row (4 + i) mod 3 and handed lanes their neighbours' contexts."""
        from carl_amd.distributed import default_context_index

        idx = default_context_index(self.n, int(self.b.lane_offset), n_contexts,
                                    self.b.selector == _lib.SEL_ROUND_ROBIN, int(self.b.selector_stride),
                                    self.context_offset)
        return torch.as_tensor(idx).to(torch.int32)

    def set_contexts(self, ctx_table, ctx_idx0=None) -> None:
        """Upload a context set ([C, F], reference feature order) and (re)assign lanes.

        Batched counterpart of the ``contexts`` setter (carl_env.py:122-137) plus
        ``_update_context`` (carl_gymnasium_env.py:75-77)."""
        t = torch.as_tensor(np.asarray(ctx_table, dtype=np.float64) if not torch.is_tensor(ctx_table) else ctx_table)
        if t.ndim != 2 or t.shape[1] != self.F:
            raise ValueError(f"ctx_table must be [C, {self.F}], got {tuple(t.shape)}")
        # feature-major [F, C] fp32 on device
        self._adopt_contexts(t.to(torch.float32).t().contiguous().to(self.device), ctx_idx0, check_range=True)

    def set_contexts_device(self, table_fc, ctx_idx0=None) -> None:
        """Adopt a context table that already lives on this device as feature-major ``[F][C]``
        float32 (``carl_sample_contexts`` output, carl_amd/context/device_sampler.py): no copy."""
        t = table_fc
        if not torch.is_tensor(t) or t.ndim != 2 or t.shape[0] != self.F:
            raise ValueError(f"device context table must be a [{self.F}, C] tensor")
        if t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous():
            t = t.to(device=self.device, dtype=torch.float32).contiguous()
        self._adopt_contexts(t, ctx_idx0, check_range=False)  # (a range check would synchronise)

    def _adopt_contexts(self, table_fc: torch.Tensor, ctx_idx0, check_range: bool) -> None:
        """``table_fc`` (feature-major ``[F, C]`` float32 on this device) becomes the context table; lanes start on
        ``ctx_idx0`` (default: ``default_ctx_idx``)."""
        C_ = int(table_fc.shape[1])
        if C_ < 1:
            raise ValueError("empty context set")
        self.ctx_table = table_fc
        self.b.n_contexts = self.b.ctx_stride = C_
        if ctx_idx0 is None:
            idx = self.default_ctx_idx(C_)
        else:
            idx = torch.as_tensor(ctx_idx0).to(torch.int32).reshape(self.n)
            if check_range and idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= C_):
                raise ValueError("ctx_idx0 out of range")
        self.ctx_idx = idx.to(self.device).contiguous()
        self._sync_pointers()

    def set_ctx_idx(self, idx) -> None:
        """Host-driven context switch (``context_id`` setter, carl_env.py:139-157)."""
        idx = torch.as_tensor(idx).to(torch.int32).reshape(self.n)
        self.ctx_idx.copy_(idx.to(self.device))

    def refresh_ctx_obs(self) -> None:
        """ctx_obs[k, lane] = table[row_k, ctx_idx[lane]] for all lanes (the kernels only
        touch lanes they reset)."""
        if self.ctx_obs.shape[0]:
            rows = torch.as_tensor(self.ctx_obs_rows, device=self.device)
            self.ctx_obs.copy_(self.ctx_table[rows][:, self.ctx_idx.long()])

    # ------------------------------------------------------------------ library calls (the subclass's)
    def _c_reset(self, mask_ptr) -> int:
        raise NotImplementedError

    def _c_step(self, io) -> int:
        raise NotImplementedError

    def _c_step_fast(self, stream: int) -> int:  # self._io, prepared references
        raise NotImplementedError

    def _c_rollout(self, io, n_steps: int) -> int:
        raise NotImplementedError

    # ------------------------------------------------------------------ plumbing
    def _sync_pointers(self) -> None:
        b = self.b
        b.state, b.elapsed, b.ctx_idx = _ptr(self.state), _ptr(self.elapsed), _ptr(self.ctx_idx)
        b.episode, b.n_calls, b.ep_return = _ptr(self.episode), _ptr(self.n_calls), _ptr(self.ep_return)
        b.ctx_table = _ptr(self.ctx_table)
        b.n_ctx_obs = len(self.ctx_obs_rows)
        b.ctx_obs = _ptr(self.ctx_obs) if self.ctx_obs_rows else None
        for k, r in enumerate(self.ctx_obs_rows):
            b.ctx_obs_feat[k] = r
        b.last_return, b.last_length = _ptr(self.last_return), _ptr(self.last_length)
        b.episodes_done = _ptr(self.episodes_done)
        b.fin_capacity = self.fin_capacity
        b.fin_count, b.fin_lane = _ptr(self.fin_count), _ptr(self.fin_lane)
        b.fin_return, b.fin_length = _ptr(self.fin_return), _ptr(self.fin_length)
        io = self._io  # the per-call outputs never move: step() only fills in the action
        io.obs, io.reward = _ptr(self.obs), _ptr(self.reward)
        io.terminated, io.truncated = _ptr(self.terminated), _ptr(self.truncated)
        io.final_obs = _ptr(self.final_obs)
        io.done = _ptr(self.done)

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    @property
    def auto_reset(self) -> bool:
        return bool(self.b.flags & _lib.FLAG_AUTORESET)

    @auto_reset.setter
    def auto_reset(self, on: bool) -> None:
        self.b.flags = (self.b.flags | _lib.FLAG_AUTORESET) if on else (self.b.flags & ~_lib.FLAG_AUTORESET)

    @property
    def n_contexts(self) -> int:
        return int(self.b.n_contexts)

    def _narrow_action(self, a: torch.Tensor) -> tuple[torch.Tensor, int] | None:
        """``(a, CARL_ACTION_*)`` where ``a`` is in a narrow format that this engine's fused rollout reads as it is, else
        None.  Here: there is none -- every action is widened to int32 / int64 / float32 (a policy under autocast hands
        half-precision actions to an engine whose library calls read float32 only: ADVICE r04)."""
        return None

    def _action_tensor(self, action, lead: tuple[int, ...], allow_narrow: bool = False) -> tuple[torch.Tensor, int]:
        a = action if torch.is_tensor(action) else torch.as_tensor(np.asarray(action))
        narrow = self._narrow_action(a) if allow_narrow else None  # (a fused rollout's actions only)
        if narrow is not None:
            a, dt = narrow
        elif self.info.action_is_discrete:
            if a.dtype not in (torch.int32, torch.int64):
                a = a.to(torch.int64)
            dt = _lib.ACTION_I32 if a.dtype == torch.int32 else _lib.ACTION_I64
        else:
            if a.dtype != torch.float32:
                a = a.to(torch.float32)
            dt = _lib.ACTION_F32
        if a.device != self.device:
            a = a.to(self.device)
        n_expected = self.n * self._action_dim
        for d in lead:
            n_expected *= d
        if a.numel() != n_expected:
            raise ValueError(f"action has {a.numel()} elements, expected {n_expected} ({lead} x {self.n} lanes)")
        return a.contiguous(), dt

    # ------------------------------------------------------------------ API
    def seed(self, seed: int) -> None:
        """``reset(seed=s)`` semantics: new RNG key, per-lane episode counters back to 0."""
        self.b.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.episode.zero_()

    def reset(self, mask: torch.Tensor | None = None) -> torch.Tensor:
        """Reset all lanes (or those with ``mask != 0``); returns the obs buffer."""
        m = None
        if mask is not None:
            m = mask.to(device=self.device, dtype=torch.uint8).contiguous()
            if m.numel() != self.n:
                raise ValueError("mask must have one entry per lane")
        with torch.cuda.device(self.device):
            _lib.check(self._c_reset(_ptr(m)))
        return self.obs

    def step(self, action):
        """One step of every lane -> (obs[N,D], reward[N], terminated[N] u8, truncated[N] u8).

        This is the per-call path (one launch per env step) a policy-in-the-loop caller sits on, so the host
        side is pared down to what a launch needs: the output pointers of ``self._io`` are set once
        (``_sync_pointers``); an action tensor that is the SAME object at the same address as in the previous
        call (the usual case: the policy writes into one buffer) skips dtype / shape / device validation; the
        raw stream handle comes from torch's C binding; the ctypes function and its two by-reference arguments
        are prepared once; the device guard is only entered when another device is current."""
        io = self._io
        if (action is self._last_action and action.data_ptr() == io.action
                and (action.dtype, action.numel()) == self._last_action_meta):
            pass  # (dtype and element count are re-checked: resize_ / set_ / .data = keep the object and its address)
        else:
            a, dt = self._action_tensor(action, ())
            io.action, io.action_dtype = a.data_ptr(), dt
            # only a tensor used as-is can take the fast path next time (a converted copy is a temporary)
            self._last_action = action if a is action else None
            self._last_action_meta = (a.dtype, a.numel())
        if _current_device() == self._dev_index:
            code = self._c_step_fast(_raw_stream(self._dev_index))
        else:
            with torch.cuda.device(self.device):
                code = self._c_step(io)
        if code != 0:
            _lib.check(code)
        return self.obs, self.reward, self.terminated, self.truncated

    def stage_scalar_action(self, action):
        """A host scalar / small array as THE device action tensor of this engine (pinned staging buffer, asynchronous
        copy on the launch stream): what a scalar caller passes to ``step`` -- the same tensor object every call, so
        ``step`` takes its validated-once fast path, and no blocking host-to-device copy per call."""
        if self._a_host is None:
            dt = torch.int32 if self.info.action_is_discrete else torch.float32
            self._a_host = torch.empty(self.n * self._action_dim, dtype=dt).pin_memory()
            self._a_dev = torch.empty((self.n, self._action_dim) if self._action_dim > 1 or not self.info.action_is_discrete
                                      else (self.n,), dtype=dt, device=self.device)
            self._a_host_np = self._a_host.numpy()
        a = np.asarray(action).reshape(-1)
        if a.size != self._a_host_np.size:  # (NumPy would broadcast one value over every actuator silently)
            raise ValueError(f"action has {a.size} elements, this engine takes {self.n} x {self._action_dim}")
        if self._a_pending:
            # the previous asynchronous upload may still be reading the pinned buffer: wait for the stream before rewriting
            # it.  Never taken by the scalar step path -- ``read_transition`` synchronises the stream after every step and
            # clears the mark -- so the guard costs a flag test, not an event per call
            torch.cuda.current_stream(self.device).synchronize()
        self._a_host_np[:] = a
        self._a_dev.view(-1).copy_(self._a_host, non_blocking=True)
        self._a_pending = True
        return self._a_dev

    def read_transition(self):
        """The last step's outputs on the host with ONE device-to-host copy: (obs [N, D] float32, reward [N] float32,
        terminated [N] uint8, truncated [N] uint8) as NumPy views of a pinned buffer (valid until the next call).
        What a scalar caller of ``step`` needs (the reference's ``CARLEnv.step`` returns Python types,
        carl/envs/carl_env.py:321-342)."""
        if self._out_host is None:
            self._out_host = torch.empty(self._out_slab.shape, dtype=torch.uint8).pin_memory()
        self._out_host.copy_(self._out_slab, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        self._a_pending = False  # (everything on the stream is done: the staged action upload too)
        h = self._out_host.numpy()
        n, D = self.n, self.D
        o_rew, o_term, o_trunc, _ = self._out_offsets
        return (h[: 4 * n * D].view(np.float32).reshape(n, D), h[o_rew: o_rew + 4 * n].view(np.float32),
                h[o_term: o_term + n], h[o_trunc: o_trunc + n])

    # ------------------------------------------------------------------ replayable step (hipGraph)
    def snapshot(self) -> dict:
        """Copies of every buffer a launch can change (state, counters, bookkeeping, step outputs: ``_SNAPSHOT``), used
        by ``capture_step``'s warm-up and ``BraxVecEngine.autotune``'s probes."""
        return {k: getattr(self, k).clone() for k in self._SNAPSHOT if getattr(self, k) is not None}

    def restore(self, snap: dict) -> None:
        for k, v in snap.items():
            getattr(self, k).copy_(v)

    def capture_step(self, action_buffer: torch.Tensor, n_steps: int = 1) -> "CapturedStep":
        """Capture ``n_steps`` per-call step launches that read ``action_buffer`` (a device tensor whose
        ADDRESS stays fixed: the policy writes the next action into it) into a hipGraph.  ``replay()`` then
        costs ONE graph launch for ``n_steps`` env steps.  Measured (65 536 CartPole lanes): a graph launch costs
        ~11 us, so a ONE-step graph (10.9 us per env step) would be SLOWER than the eager ``step`` (4.3 us: prepared
        ctypes call, raw stream handle) -- ``n_steps=1`` therefore returns a replayable object that makes the eager call
        on the fixed buffer (round 5; no graph); the captured form pays off from ~4 steps per replay (``n_steps=100``:
        3.7 us per env step, the same as a ``torch.cuda.graph`` around 100 ``step`` calls) and is meant for a policy that
        is captured into the same graph region or for open-loop replays.  Engine state is untouched by the capture."""
        return CapturedStep(self, action_buffer, n_steps)

    def alloc_rollout(self, n_steps: int, final_obs: bool = False) -> dict:
        """Output buffers of a ``rollout`` of ``n_steps``: ``obs [T, N, D]``, ``reward`` / ``terminated`` / ``truncated``
        ``[T, N]``.  For a lane count that is not a multiple of 16 they are VIEWS ``[:, :N]`` of arrays whose rows are
        ``_row_pitch()`` lanes long (non-contiguous; ``.contiguous()`` copies) -- the padding columns receive the
        records of the padding lanes."""
        dev, n, D, P = self.device, self.n, self.D, self._row_pitch()

        def rows(tail, dtype, zero=False):
            full = (torch.zeros if zero else torch.empty)((n_steps, P) + tail, dtype=dtype, device=dev)
            return full if P == n else full[:, :n]

        out = {
            "obs": rows((D,), torch.float32),
            "reward": rows((), torch.float32),
            "terminated": rows((), torch.uint8),
            "truncated": rows((), torch.uint8),
        }
        if final_obs:
            out["final_obs"] = rows((D,), torch.float32, zero=True)
        return out

    def rollout(self, actions, out: dict | None = None) -> dict:
        """T steps in one launch; ``actions`` is [T, N] (or [T, N, 1]).  Every step's full
        transition is written to ``out`` (see ``alloc_rollout``).  Discrete families: int32 / int64, or ``torch.uint8`` --
        one byte per lane-step instead of four on the launch's only per-step read stream (CartPole x 65 536: +15 %
        env-steps/s); Box families: float32, or ``torch.float16`` / ``torch.bfloat16`` (widened exactly).  Same transitions
        bit for bit as the wide launch fed the same values."""
        return self._launch_rollout(self._prepare_rollout(actions, out))

    def _prepare_rollout(self, actions, out: dict | None) -> _PreparedRollout:
        """Everything ``rollout`` does before its launch, done once: the actions converted (narrow formats kept), the output
        buffers (``alloc_rollout``'s when none are given) and the ``carl_step_io_t`` over them."""
        T = int(actions.shape[0])
        a, dt = self._action_tensor(actions, (T,), allow_narrow=True)
        if out is None:
            out = self.alloc_rollout(T)
        return _PreparedRollout(a, dt, out, self._rollout_io(a, dt, out, T), T)

    def _launch_rollout(self, r: _PreparedRollout) -> dict:
        """The launch of a prepared ``rollout`` on the current stream -> its output dict."""
        with torch.cuda.device(self.device):
            _lib.check(self._c_rollout(r.io, r.T))
        return r.out

    def _rollout_io(self, a: torch.Tensor | None, dt: int | None, out: dict, T: int) -> "_lib.StepIO":
        """``carl_step_io_t`` of a fused launch of ``T`` steps into the caller's ``[T, ...]`` output buffers, rows of one
        common pitch (``_out_pitch``: ``alloc_rollout`` pads rows to a multiple of 16 lanes; dense caller-made buffers keep
        working; an engine without padded rows refuses any other pitch there).  Where the actions come from is the one
        difference: ``rollout`` passes its validated actions ``a`` of format ``dt``; for a padded layout they are copied once
        into rows of the same pitch, the padding columns repeating the last lane's action (the padding lanes run as clones
        of that lane: valid numbers).  ``rollout_policy`` passes ``a = None``: the launch writes each step's actions into
        ``out["action"]``, which must be ``[>= T, N]`` rows of the same pitch, of the family's int32 / float32 dtype, on
        this device."""
        n, policy = self.n, a is None
        keys = ("obs", "reward", "terminated", "truncated", "final_obs")
        if policy:
            if "action" not in out:
                raise ValueError("rollout_policy output needs an 'action' [T, N] buffer")
            adt = torch.int32 if self.info.action_is_discrete else torch.float32
            if out["action"].dtype != adt:
                raise ValueError(f"rollout_policy 'action' buffer must be {adt} for this family")
            a, dt = out["action"], _lib.ACTION_I32 if self.info.action_is_discrete else _lib.ACTION_F32
        elif out["reward"].shape[0] < T:
            raise ValueError("rollout output buffers are shorter than the action sequence")
        P = self._out_pitch(out)
        if policy:
            self._check_rows("rollout_policy", out, keys + ("action",), P, T, self.device)
        else:
            self._check_rows("rollout", out, keys, P)
            if P != n:
                a = self._pad_action_rows(a, T, P)
            self._rollout_actions = a  # (keeps a padded copy alive until the launch has been enqueued and beyond)
        io = _lib.StepIO()
        io.row_pitch = P if P != n else 0
        io.action, io.action_dtype = a.data_ptr(), dt
        io.obs, io.reward = _ptr(out["obs"]), _ptr(out["reward"])
        io.terminated, io.truncated = _ptr(out["terminated"]), _ptr(out["truncated"])
        io.final_obs = _ptr(out.get("final_obs"))
        io.branch_sig = _ptr(out.get("branch_sig"))
        return io

    def _check_rows(self, who: str, out: dict, keys, P: int, min_rows: int | None = None, device=None) -> None:
        """ValueError unless each of ``out[keys]`` that is present is ``[T, N]`` (``[T, N, D]``: obs, final_obs) rows of
        pitch ``P`` lanes -- with ``T >= min_rows`` and on ``device`` when those are given."""
        n, D = self.n, self.D
        for k in keys:
            t = out.get(k)
            if t is None:
                continue
            tail = (D,) if k in ("obs", "final_obs") else ()
            want = (P * D, D, 1) if tail else (P, 1)
            if t.dim() == 0 or t.shape[0] < (min_rows or 0) or tuple(t.shape[1:]) != (n,) + tail or (
                    device is not None and t.device != device) or any(
                    sz > 1 and st != w for sz, st, w in zip(t.shape, t.stride(), want)):
                rows = "T" if min_rows is None else f">= {min_rows}"
                raise ValueError(f"{who} output '{k}': shape {tuple(t.shape)} / strides {tuple(t.stride())} do not form "
                                 f"[{rows}, {n}{', ' + str(D) if tail else ''}] rows of one common pitch ({P} lanes)")

    def gae(self, reward, value, terminated, truncated, last_value, gamma: float, lam: float, boot_value=None,
            out: dict | None = None) -> dict:
        """Generalised advantage estimation in one launch (include/carl_amd.h: carl_gae) over ``[T, N]`` float32
        ``reward`` / ``value`` (/ ``boot_value``), uint8 or bool ``terminated`` / ``truncated`` and ``last_value`` ``[N]``:
        rows of one common pitch (``alloc_rollout``-style views or dense), on this engine's device.  Returns
        ``{"advantage", "return"}`` ``[T, N]`` float32 (``out``: buffers of the same layout to write into).  The rule is
        SB3's ``RolloutBuffer.compute_returns_and_advantage`` with ``boot_value`` as the timeout bootstrap; a finished
        step (either flag) cuts the recurrence.  No host synchronisation."""
        T, N, P = row_layout(reward)

        def rows(name, t, dtypes):
            if not is_rows(t, self.device, dtypes, T, N, P):
                raise ValueError(f"gae '{name}': needs {dtypes[0]} [{T}, {N}] rows of pitch {P} on {self.device}, got "
                                 f"{t.dtype} {tuple(t.shape)} strides {tuple(t.stride())}")
            return t

        if P < N:
            raise ValueError(f"gae 'reward': rows of pitch {P} < {N} lanes")
        f32, u8 = (torch.float32,), (torch.uint8, torch.bool)
        rows("reward", reward, f32), rows("value", value, f32), rows("terminated", terminated, u8)
        rows("truncated", truncated, u8)
        if boot_value is not None:
            rows("boot_value", boot_value, f32)
        if not is_exact(last_value, self.device, torch.float32, (N,)):
            raise ValueError(f"gae 'last_value': needs a contiguous float32 [{N}] tensor on {self.device}")
        res = {} if out is None else out
        for k in ("advantage", "return"):
            if k not in res:
                res[k] = torch.empty((T, P), dtype=torch.float32, device=self.device)[:, :N]
            rows(k, res[k], f32)
        g = _lib.Gae()
        g.n_lanes, g.n_steps, g.row_pitch, g.gamma, g.lam = N, T, (P if P != N else 0), float(gamma), float(lam)
        g.reward, g.value, g.boot_value, g.last_value = _ptr(reward), _ptr(value), _ptr(boot_value), _ptr(last_value)
        g.terminated, g.truncated = _ptr(terminated), _ptr(truncated)
        g.advantage, g.ret = _ptr(res["advantage"]), _ptr(res["return"])
        with torch.cuda.device(self.device):
            _lib.check(self.lib.carl_gae(C.byref(g), self._stream()))
        return res

    # ------------------------------------------------------------------ closed loop: the front end both engines share
    # What an engine brings to ``rollout_policy`` / ``evaluate_policy`` / ``evaluate_episodes``: its policy check, the rules
    # only it has, its checks of the summary's dtypes and of ``"action"``, and its C calls.
    # (key, dtype, per-episode rows) of an evaluate_policy / evaluate_episodes result
    _EPISODE_KEYS = (("episodes", torch.int32, False), ("steps", torch.int32, False), ("return", torch.float32, True),
                     ("length", torch.int32, True), ("context_id", torch.int32, True), ("terminated", torch.uint8, True))
    _SUMMARY_KEYS = (("episodes", torch.int32), ("return_sum", torch.float32), ("length_sum", torch.int32))

    def alloc_policy_summary(self) -> dict:
        """Per-lane totals of a summary-mode ``rollout_policy``: ``episodes`` / ``length_sum`` int32, ``return_sum``
        float32, ``[N]`` each."""
        return {k: torch.zeros(self.n, dtype=dt, device=self.device) for k, dt in self._SUMMARY_KEYS}

    def alloc_policy_episodes(self, n_episodes: int) -> dict:
        """Output buffers of ``evaluate_policy`` (a Brax engine: ``evaluate_episodes``): ``episodes`` / ``steps`` int32
        ``[N]``; ``return`` float32, ``length`` / ``context_id`` int32, ``terminated`` uint8, ``[n_episodes, N]`` each.
        The launch writes every element."""
        K = int(n_episodes)
        if K < 1:
            raise ValueError(f"n_episodes {K} < 1")
        return {k: torch.empty((K, self.n) if rows else (self.n,), dtype=dt, device=self.device)
                for k, dt, rows in self._EPISODE_KEYS}

    def _check_value_net(self, policy, value_net) -> None:
        """ValueError unless ``value_net`` is a critic the valued launch can run next to ``policy``: a value head, the same
        family, inputs and set layout, and a shift | scale | clip section equal to the actor's bit for bit (the critic
        reads the actor's transformed inputs; with equal sections the critic's packed block alone defines V)."""
        if getattr(value_net, "head", None) != "value":
            raise ValueError("value_net must be an MLPPolicy built with head='value'")
        if policy.head != "policy":
            raise ValueError("the acting policy must have head='policy'")
        if value_net.family != policy.family or value_net.obs_dim != policy.obs_dim:
            raise ValueError(f"value_net was built for family {value_net.family}, the policy for family {policy.family}")
        if list(value_net.ctx_rows) != list(policy.ctx_rows):
            raise ValueError(f"value_net reads context rows {value_net.ctx_rows}, the policy {policy.ctx_rows}: the critic "
                             "sees the actor's inputs")
        if value_net.n_sets != policy.n_sets or value_net.lanes_per_set != policy.lanes_per_set:
            raise ValueError(f"value_net has {value_net.n_sets} weight sets of {value_net.lanes_per_set} lanes, the policy "
                             f"{policy.n_sets} of {policy.lanes_per_set}: one set layout for both")
        a, c = policy.transform_section(), value_net.transform_section()
        if not np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(c).view(np.int32)):
            raise ValueError("value_net's input_shift / input_scale / input_clip must equal the policy's bit for bit: the "
                             "critic reads the actor's transformed inputs")

    def _policy_keywords(self, policy, mode: str, deterministic: bool, log_prob: bool, value_net, bootstrap_truncated: bool,
                         gae) -> tuple:
        """The keyword rules of ``rollout_policy``, either engine's -> (whether the launch stores log-probabilities,
        ``gae`` as floats)"""
        if mode not in ("transitions", "summary"):
            raise ValueError(f"mode {mode!r}: 'transitions' or 'summary'")
        if gae is not None and value_net is None:
            raise ValueError("gae=(gamma, lam) needs value_net: advantages are computed from the critic's values")
        if value_net is not None:
            if mode == "summary":
                raise ValueError("value_net: transitions mode only (mode='summary' stores nothing per step)")
            self._check_value_net(policy, value_net)
            if bootstrap_truncated and not self.auto_reset:
                raise ValueError("bootstrap_truncated=True needs auto_reset=True: without it no terminal observation is "
                                 "kept apart from the next one (pass bootstrap_truncated=False)")
            if gae is not None:
                gamma, lam = (float(v) for v in gae)
                gae = (gamma, lam)
            log_prob = log_prob or not deterministic  # (a sampled launch with a critic always stores the log-probabilities)
        if log_prob and deterministic:
            raise ValueError("log_prob=True: sampled launches only (deterministic=False)")
        if log_prob and mode == "summary":
            raise ValueError("log_prob=True: transitions mode only (a summary launch stores nothing per step)")
        if mode == "summary" and not self.auto_reset:
            raise ValueError("mode='summary' needs auto_reset=True: without it a finished lane reports done on every later "
                             "step, and the totals would count its episode on each of them")
        return log_prob, gae

    def _policy_summary(self, res: dict):
        """the ``carl_policy_summary_t`` over a checked summary dict, by reference"""
        return C.byref(_lib.PolicySummary(*(_ptr(res[k]) for k, _ in self._SUMMARY_KEYS)))

    def _policy_columns(self, out: dict, keys, T: int, dtype=torch.float32) -> None:
        """Each of ``out[keys]`` a ``[>= T, N]`` ``dtype`` column in rows of ``out``'s pitch (``_out_pitch``: a Brax
        engine's rows are dense) on this device: allocated where absent, ValueError otherwise (every dtype before any row
        layout; a buffer elsewhere is told where it must be, which ``_check_rows``' message does not say)."""
        P = self._out_pitch(out)
        for k in keys:
            if k not in out:
                out[k] = torch.empty((T, P), dtype=dtype, device=self.device)[:, : self.n]
            elif out[k].dtype != dtype:
                raise ValueError(f"rollout_policy '{k}' buffer must be {dtype}")
        for k in keys:
            if out[k].device != self.device:
                raise ValueError(f"rollout_policy '{k}' buffer must be on {self.device}")
        self._check_rows("rollout_policy", out, keys, P, T)

    def _policy_last_value(self, out: dict) -> torch.Tensor:
        """``out["last_value"]``, float32 ``[N]``: allocated where absent, checked otherwise"""
        if "last_value" not in out:
            out["last_value"] = torch.empty(self.n, dtype=torch.float32, device=self.device)
        if not is_exact(out["last_value"], self.device, torch.float32, (self.n,)):
            raise ValueError(f"rollout_policy 'last_value' must be a contiguous float32 [{self.n}] tensor on {self.device}")
        return out["last_value"]

    def _policy_gae(self, out: dict, T: int, gae: tuple, bootstrap_truncated: bool) -> None:
        """``out["advantage"]`` / ``out["return"]`` from one ``gae`` launch of a valued launch's own columns"""
        res = self.gae(out["reward"][:T], out["value"][:T], out["terminated"][:T], out["truncated"][:T], out["last_value"],
                       *gae, boot_value=out["boot_value"][:T] if bootstrap_truncated else None,
                       out={k: out[k] for k in ("advantage", "return") if k in out} or None)
        out["advantage"], out["return"] = res["advantage"], res["return"]

    def _policy_episodes(self, who: str, n_episodes: int, max_steps: int, out: dict | None) -> tuple:
        """The checks ``evaluate_policy`` and ``evaluate_episodes`` (``who``) share -> (K, T, the result dict, its
        ``carl_policy_episodes_t``)"""
        if not self.auto_reset:
            raise ValueError(f"{who} needs auto_reset=True: without it a finished lane reports done on every later step")
        K, T = int(n_episodes), int(max_steps)
        if K < 1:
            raise ValueError(f"n_episodes {K} < 1")
        if T < 0:
            raise ValueError(f"max_steps {T} < 0")
        if K * self.n >= 1 << 31:
            raise ValueError(f"{K} episodes x {self.n} lanes: more than 2^31 - 1 records")
        res = self.alloc_policy_episodes(K) if out is None else out
        for k, dt, rows in self._EPISODE_KEYS:
            shape = (K, self.n) if rows else (self.n,)
            if not is_exact(res.get(k), self.device, dt, shape):
                raise ValueError(f"{who} output '{k}' must be a contiguous {dt} {list(shape)} tensor on {self.device}")
        return K, T, res, _lib.PolicyEpisodes(*(_ptr(res[k]) for k, _, _ in self._EPISODE_KEYS))

    def _policy_input_partial(self, who: str, res: dict, n_slabs: int) -> "_lib.PolicyStats":
        """``res["input_partial"]``, float64 ``[n_slabs, 2, 32]``: allocated where absent, checked otherwise -> the
        ``carl_policy_stats_t`` over it"""
        shape = (n_slabs, 2, _lib.POLICY_MAX_IN)
        if res.get("input_partial") is None:
            res["input_partial"] = torch.empty(shape, dtype=torch.float64, device=self.device)
        if not is_exact(res["input_partial"], self.device, torch.float64, shape):
            raise ValueError(f"{who} output 'input_partial' must be a contiguous torch.float64 {list(shape)} tensor on "
                             f"{self.device}")
        return _lib.PolicyStats(_ptr(res["input_partial"]), n_slabs)

    # ------------------------------------------------------------------ the PPO update (carl_amd/ppo.py)
    # One set of argument checks for both engines.  What an engine brings: its C entry points (``_c_context_trace``,
    # ``_c_ppo_workspace_floats``, ``_c_ppo_grad``), its policy check (``_ppo_check_policy``), the trailing shape of its
    # action column (``_ppo_action_tail``: () -- one value per step -- or (n_act,)) and the length of ``log_std``
    # (``_ppo_log_std_floats``: 0 for a discrete family).
    def context_trace(self, ctx_idx0: torch.Tensor, episode0: torch.Tensor, terminated: torch.Tensor,
                      truncated: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """The context-table index each step of a launch ran in (include/carl_amd.h: carl_policy_context_trace):
        ``[T, N]`` int32 (the Brax families: carl_brax_policy_context_trace, dense rows), from clones of ``ctx_idx`` /
        ``episode`` taken BEFORE that launch and its ``terminated`` /
        ``truncated`` rows (``alloc_rollout``-style views or dense; uint8 or bool).  The selector's walk is replayed with
        this engine's selector, stride, seed, lane offset and auto-reset setting, so those must be what the launch ran
        under.  ``out``: an int32 buffer of the flags' row layout to write into.  One launch, no host synchronisation."""
        T, N, P = row_layout(terminated)
        if N != self.n or P < N:
            raise ValueError(f"context_trace: flag rows of {N} lanes (pitch {P}) for an engine of {self.n}")
        for name, t in (("terminated", terminated), ("truncated", truncated)):
            if not is_rows(t, self.device, (torch.uint8, torch.bool), T, N, P):
                raise ValueError(f"context_trace '{name}': needs uint8 [{T}, {N}] rows of pitch {P} on {self.device}")
        for name, t in (("ctx_idx0", ctx_idx0), ("episode0", episode0)):
            if not is_exact(t, self.device, torch.int32, (N,)):
                raise ValueError(f"context_trace '{name}': needs a contiguous int32 [{N}] tensor on {self.device}")
        if out is None:
            out = torch.empty((T, P), dtype=torch.int32, device=self.device)[:, :N]
        elif not is_rows(out, self.device, (torch.int32,), T, N, P):
            raise ValueError(f"context_trace 'out': needs int32 [{T}, {N}] rows of pitch {P} on {self.device}")
        with torch.cuda.device(self.device):
            _lib.check(self._c_context_trace(_ptr(ctx_idx0), _ptr(episode0), _ptr(terminated), _ptr(truncated), T,
                                             P if P != N else 0, _ptr(out)))
        return out

    def _ppo_buffer(self, who: str, buf: dict, obs0: torch.Tensor, context_id: torch.Tensor) -> tuple:
        """``ppo_grad``'s checks of a rollout buffer, ``obs0`` and ``context_id`` (messages begin with ``who``) -> (T, N, the
        rows' pitch)."""
        act = buf["action"]
        tail = self._ppo_action_tail()
        f32, i32 = torch.float32, torch.int32
        adt = i32 if self.info.action_is_discrete else f32
        if tail:  # [T, N, n_act]: dense rows
            if act.dim() != 3 or tuple(act.shape[2:]) != tail or not act.is_contiguous():
                raise ValueError(f"{who} 'action': needs a contiguous float32 [T, {self.n}, {tail[0]}] tensor on {self.device}")
            T, N = int(act.shape[0]), int(act.shape[1])
            P = N
        else:
            T, N, P = row_layout(act)
        if N != self.n:
            raise ValueError(f"{who}: a buffer of {N} lanes for an engine of {self.n}")
        cols = {"action": (act, adt), "log_prob": (buf["log_prob"], f32), "advantage": (buf["advantage"], f32),
                "return": (buf["return"], f32), "context_id": (context_id, i32)}
        if tail:  # (its shape is checked above)
            if act.dtype != adt or act.device != self.device:
                raise ValueError(f"{who} 'action': needs a contiguous float32 [T, {self.n}, {tail[0]}] tensor on {self.device}")
            del cols["action"]
        for k, (t, dt) in cols.items():
            if not is_rows(t, self.device, (dt,), T, N, P, at_least=True):
                raise ValueError(f"{who} '{k}': needs {dt} [{T}, {N}] rows of pitch {P} on {self.device}")
        self._ppo_observations(who, buf["obs"], obs0, T, N, P)
        return T, N, P

    def _ppo_observations(self, who: str, obs: torch.Tensor, obs0: torch.Tensor, T: int, N: int, P: int) -> None:
        """The checks of a buffer's ``obs`` (``[>= T, N, D]`` rows of pitch ``P``) and of ``obs0``"""
        if not is_rows(obs, self.device, (torch.float32,), T, N, P, (self.D,), at_least=True):
            raise ValueError(f"{who} 'obs': needs float32 [{T}, {N}, {self.D}] rows of pitch {P} on {self.device}")
        if not is_exact(obs0, self.device, torch.float32, (N, self.D)):
            raise ValueError(f"{who} 'obs0': needs a contiguous float32 [{N}, {self.D}] tensor on {self.device}")

    def _ppo_batch(self, T: int, N: int, P: int, buf: dict, obs0: torch.Tensor, context_id: torch.Tensor,
                   columns: bool = True) -> "_lib.PpoBatch":
        """The ``carl_ppo_batch_t`` of a buffer ``_ppo_buffer`` has checked, with everything but ``n_samples``, the
        coefficients, ``idx`` and ``adv_norm``.  ``columns=False`` (``ppo_input_stats``, which checks and reads the
        observations alone): the action's dtype and the four per-step columns stay zero / NULL."""
        pb = _lib.PpoBatch()
        pb.family, pb.n_lanes, pb.n_steps, pb.row_pitch, pb.obs_dim = self.family, N, T, (P if P != N else 0), self.D
        pb.n_contexts, pb.ctx_stride = int(self.b.n_contexts), int(self.b.ctx_stride)
        pb.obs0, pb.obs, pb.context_id, pb.ctx_table = _ptr(obs0), _ptr(buf["obs"]), _ptr(context_id), _ptr(self.ctx_table)
        if columns:
            pb.action_dtype = _lib.ACTION_I32 if self.info.action_is_discrete else _lib.ACTION_F32
            pb.action, pb.log_prob, pb.advantage, pb.ret = (_ptr(buf[k]) for k in ("action", "log_prob", "advantage", "return"))
        return pb

    def ppo_workspace(self, policy, value_net, n_samples: int) -> torch.Tensor:
        """A float32 workspace for ``ppo_grad`` of ``n_samples`` samples (carl_ppo_workspace_floats)."""
        need = int(self._c_ppo_workspace_floats(C.byref(policy.struct(self.n, 0x10)), C.byref(value_net.struct(self.n, 0x10)),
                                                int(n_samples)))
        if need < 0:
            raise ValueError(f"ppo_workspace: invalid shapes or n_samples {n_samples}")
        return torch.empty(need, dtype=torch.float32, device=self.device)

    def ppo_grad(self, policy, value_net, buf: dict, obs0: torch.Tensor, context_id: torch.Tensor, *, idx=None,
                 adv_norm=None, clip_range: float = 0.2, vf_coef: float = 0.5, ent_coef: float = 0.0,
                 forward: bool = False, out: dict | None = None, workspace: torch.Tensor | None = None) -> dict:
        """Loss and gradients of one PPO minibatch in three launches (include/carl_amd.h: carl_ppo_grad).  ``buf``: the dict
        of ``rollout_policy(..., deterministic=False, value_net=, gae=)`` (``obs``, ``action``, ``log_prob``, ``advantage``,
        ``return``: rows of one pitch); ``obs0`` ``[N, D]``: the observation its step 0 was chosen from; ``context_id``:
        ``context_trace``'s result for that launch (the same pitch).  ``idx``: int32 ``[M]`` flat sample indices
        ``t * pitch + lane`` (distinct, ``lane < N``; the pitch is ``buf["action"].stride(0)``), None: every sample.
        ``adv_norm``: a float32 ``[2]`` device tensor (mean, 1 / (std + eps)) or None.  Returns ``{"grad_actor"
        [set_floats], "grad_critic" [set_floats], "grad_log_std" [1] (Box families; ``[n_act]`` for a Brax model, whose ``action`` is ``[T, N, n_act]`` in dense rows:
        carl_brax_ppo_grad), "stats" [6]: policy loss, value
        loss, mean entropy, approx_kl, clip fraction, M}`` and, with ``forward=True``, ``"new_log_prob"`` / ``"new_value"``
        ``[M]`` -- float32 device tensors (``out``: such a dict to write into).  ``policy`` / ``value_net``: one-set policies
        (host-built or ``on_device``).  No host synchronisation."""
        self._ppo_check_policy(policy)
        T, N, P = self._ppo_buffer("ppo_grad", buf, obs0, context_id)
        f32 = torch.float32
        if idx is not None and not is_exact(idx, self.device, torch.int32, (None,)):
            raise ValueError(f"ppo_grad 'idx': needs a contiguous int32 [M] tensor on {self.device}")
        if adv_norm is not None and not is_exact(adv_norm, self.device, f32, 2):
            raise ValueError(f"ppo_grad 'adv_norm': needs a contiguous float32 [2] tensor on {self.device}")
        M = T * N if idx is None else int(idx.numel())
        res = {} if out is None else out
        n_ls = self._ppo_log_std_floats()
        box = n_ls > 0
        want = {"grad_actor": policy.set_floats, "grad_critic": value_net.set_floats, "stats": 6}
        if box:
            want["grad_log_std"] = n_ls
        if forward:
            want["new_log_prob"] = want["new_value"] = M
        for k, size in want.items():
            if k not in res:
                res[k] = torch.empty(size, dtype=f32, device=self.device)
            if not is_exact(res[k], self.device, f32, size):
                raise ValueError(f"ppo_grad output '{k}': needs a contiguous float32 [{size}] tensor on {self.device}")
        pol = policy.struct(self.n, policy.device_params(self.device).data_ptr())
        crit = value_net.struct(self.n, value_net.device_params(self.device).data_ptr())
        ws = self.ppo_workspace(policy, value_net, M) if workspace is None else workspace
        pb = self._ppo_batch(T, N, P, buf, obs0, context_id)
        pb.n_samples = M
        pb.clip_range, pb.vf_coef, pb.ent_coef = float(clip_range), float(vf_coef), float(ent_coef)
        pb.idx, pb.adv_norm = _ptr(idx), _ptr(adv_norm)
        po = _lib.PpoOut(_ptr(res["grad_actor"]), _ptr(res["grad_critic"]), _ptr(res.get("grad_log_std")), _ptr(res["stats"]),
                         _ptr(res.get("new_log_prob")) if forward else None, _ptr(res.get("new_value")) if forward else None,
                         _ptr(ws), int(ws.numel()))
        ls = policy.device_log_std(self.device).data_ptr() if box else None
        with torch.cuda.device(self.device):
            _lib.check(self._c_ppo_grad(C.byref(pb), C.byref(pol), C.byref(crit), ls, C.byref(po)))
        return res

    # ------------------------------------------------------------------ PPO's running normalisation (carl_amd/ppo.py)
    # What an engine brings: ``_c_ppo_input_stats`` (the return statistics serve both engines as they are).
    def ppo_input_stats(self, policy, buf: dict, obs0: torch.Tensor, context_id: torch.Tensor, out: dict | None = None) -> dict:
        """The shifted float64 sums of every policy input over a rollout buffer in one launch (include/carl_amd.h:
        carl_ppo_input_stats; a Brax model: carl_brax_ppo_input_stats).  ``buf["obs"]``, ``obs0`` and ``context_id`` as
        ``ppo_grad`` takes them; every sample ``(t, lane)`` counts, its input gathered as ``ppo_grad`` gathers it (row
        ``T - 1`` of ``obs`` is the next collection's ``obs0`` and is not counted).  Returns ``{"input_partial"
        [slabs, 2, 32] float64, "steps" [N] int32 filled with T}`` -- what ``InputStats.update(result, block,
        policy=policy)`` merges (``out``: such a dict to write into).  ``policy``: the one-set policy the collection ran
        (its shift centres the sums).  No host synchronisation."""
        self._ppo_check_policy(policy)
        i32 = torch.int32
        if context_id.dim() != 2:
            raise ValueError(f"ppo_input_stats 'context_id': needs int32 [T, {self.n}] rows on {self.device}")
        T, N, P = row_layout(context_id)
        if self._ppo_action_tail():
            P = N
        if N != self.n or T < 1:
            raise ValueError(f"ppo_input_stats: a buffer of {T} steps x {N} lanes for an engine of {self.n}")
        if not is_rows(context_id, self.device, (i32,), T, N, P) or P < N:
            raise ValueError(f"ppo_input_stats 'context_id': needs int32 [{T}, {N}] rows of pitch {P} on {self.device}")
        self._ppo_observations("ppo_input_stats", buf["obs"], obs0, T, N, P)
        slabs = int(self.lib.carl_ppo_input_stats_slabs(N, T))
        res = {} if out is None else out
        if "input_partial" not in res:
            res["input_partial"] = torch.empty((slabs, 2, _lib.POLICY_MAX_IN), dtype=torch.float64, device=self.device)
        if "steps" not in res:
            res["steps"] = torch.full((N,), T, dtype=i32, device=self.device)
        part = res["input_partial"]
        if not is_exact(part, self.device, torch.float64, (None, 2, _lib.POLICY_MAX_IN)) or part.shape[0] < slabs:
            raise ValueError(f"ppo_input_stats 'input_partial': needs a contiguous float64 [>= {slabs}, 2, "
                             f"{_lib.POLICY_MAX_IN}] tensor on {self.device}")
        if not is_exact(res["steps"], self.device, i32, (N,)):
            raise ValueError(f"ppo_input_stats 'steps': needs a contiguous int32 [{N}] tensor on {self.device} (filled with T)")
        if part.shape[0] != slabs:
            res["input_partial"] = part = part[:slabs]  # (the merge adds every slab of the tensor it is given)
        pol = policy.struct(self.n, policy.device_params(self.device).data_ptr())
        pb = self._ppo_batch(T, N, P, buf, obs0, context_id, columns=False)
        pb.n_samples = T * N
        st = _lib.PolicyStats(part.data_ptr(), slabs)
        with torch.cuda.device(self.device):
            _lib.check(self._c_ppo_input_stats(C.byref(pb), C.byref(pol), C.byref(st)))
        return res

    def ppo_return_stats(self, reward, terminated, truncated, ret, gamma: float, out: dict | None = None,
                         ret_rows: bool = False) -> dict:
        """One forward walk of the discounted return per lane (include/carl_amd.h: carl_ppo_return_stats): ``ret`` ``[N]``
        float32 is read, advanced by ``ret = gamma * ret + reward[t]`` over the ``[T, N]`` rows (float32, zeroed after a
        finished step: VecNormalize's order) and written back.  Returns ``{"return_partial" [slabs, 2] float64}`` -- each
        workgroup's sums of the returns and of their squares -- and, with ``ret_rows=True``, ``"ret_rows"`` ``[T, N]``:
        the return after each step's reward (rows of the reward's pitch).  No host synchronisation."""
        T, N, P = row_layout(reward)
        if N != self.n or P < N or T < 1:
            raise ValueError(f"ppo_return_stats: reward rows of {T} steps x {N} lanes (pitch {P}) for an engine of {self.n}")
        for name, t, dts in (("reward", reward, (torch.float32,)), ("terminated", terminated, (torch.uint8, torch.bool)),
                             ("truncated", truncated, (torch.uint8, torch.bool))):
            if not is_rows(t, self.device, dts, T, N, P):
                raise ValueError(f"ppo_return_stats '{name}': needs {dts[0]} [{T}, {N}] rows of pitch {P} on {self.device}")
        if not is_exact(ret, self.device, torch.float32, (N,)):
            raise ValueError(f"ppo_return_stats 'ret': needs a contiguous float32 [{N}] tensor on {self.device}")
        slabs = int(self.lib.carl_ppo_return_stats_slabs(N))
        res = {} if out is None else out
        if "return_partial" not in res:
            res["return_partial"] = torch.empty((slabs, 2), dtype=torch.float64, device=self.device)
        part = res["return_partial"]
        if not is_exact(part, self.device, torch.float64, (slabs, 2)):
            raise ValueError(f"ppo_return_stats 'return_partial': needs a contiguous float64 [{slabs}, 2] tensor on {self.device}")
        rows = None
        if ret_rows:
            if "ret_rows" not in res:
                res["ret_rows"] = torch.empty((T, P), dtype=torch.float32, device=self.device)[:, :N]
            rows = res["ret_rows"]
            if not is_rows(rows, self.device, (torch.float32,), T, N, P):
                raise ValueError(f"ppo_return_stats 'ret_rows': needs float32 [{T}, {N}] rows of pitch {P} on {self.device}")
        rs = _lib.PpoReturnStats()
        rs.n_lanes, rs.n_steps, rs.row_pitch, rs.gamma = N, T, (P if P != N else 0), float(gamma)
        rs.reward, rs.terminated, rs.truncated = _ptr(reward), _ptr(terminated), _ptr(truncated)
        rs.ret, rs.ret_rows, rs.partial, rs.partial_capacity = _ptr(ret), _ptr(rows), _ptr(part), slabs
        with torch.cuda.device(self.device):
            _lib.check(self.lib.carl_ppo_return_stats(C.byref(rs), self._stream()))
        return res

    def ppo_return_merge(self, partial: torch.Tensor, n_b: int, running: dict, eps: float = 1e-8,
                         scale: torch.Tensor | None = None) -> torch.Tensor:
        """Merge ``ppo_return_stats``'s slabs over ``n_b`` = T x N returns into ``running`` = ``{"count" int64 [1], "mean"
        float64 [1], "m2" float64 [1]}`` (device tensors, all zero before the first merge) by Chan's rule and write
        ``1 / sqrt(m2 / count + eps)`` to ``scale`` (a float32 ``[1]`` device tensor, allocated when None), which is
        returned (include/carl_amd.h: carl_ppo_return_merge).  No host synchronisation."""
        if not is_exact(partial, self.device, torch.float64, (None, 2)):
            raise ValueError(f"ppo_return_merge 'partial': needs a contiguous float64 [slabs, 2] tensor on {self.device}")
        for k, dt in (("count", torch.int64), ("mean", torch.float64), ("m2", torch.float64)):
            if not is_exact(running[k], self.device, dt, 1):
                raise ValueError(f"ppo_return_merge running['{k}']: needs a {dt} [1] tensor on {self.device}")
        if scale is None:
            scale = torch.empty(1, dtype=torch.float32, device=self.device)
        if not is_exact(scale, self.device, torch.float32, 1):
            raise ValueError(f"ppo_return_merge 'scale': needs a float32 [1] tensor on {self.device}")
        run = _lib.PolicyRunningStats(_ptr(running["count"]), _ptr(running["mean"]), _ptr(running["m2"]))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.carl_ppo_return_merge(_ptr(partial), int(partial.shape[0]), int(n_b), C.byref(run),
                                                      float(eps), _ptr(scale), self._stream()))
        return scale

    # ------------------------------------------------------------------ PPO's minibatch step (carl_amd/ppo.py: fused_step)
    def _advantage_storage(self, who: str, advantage: torch.Tensor) -> int:
        """The elements an ``advantage`` argument spans from its first: float32 ``[T, N]`` rows of any one pitch, or a
        contiguous 1-D storage (``ppo_adv_stats``, ``ppo_adv_stats_sets``: messages begin with ``who``)"""
        if (advantage.dtype != torch.float32 or advantage.device != self.device or advantage.dim() not in (1, 2)
                or advantage.numel() < 1 or (advantage.dim() == 1 and not advantage.is_contiguous())):
            raise ValueError(f"{who} 'advantage': needs float32 [T, N] rows or a contiguous float32 [n] tensor on {self.device}")
        if advantage.dim() == 1:
            return int(advantage.numel())
        T, N, P = row_layout(advantage)
        if (N > 1 and advantage.stride(1) != 1) or P < N:
            raise ValueError(f"{who} 'advantage': needs float32 [{T}, {N}] rows of one pitch on {self.device}")
        return (T - 1) * P + N

    def ppo_adv_stats(self, advantage: torch.Tensor, idx: torch.Tensor, batch_size: int, eps: float = 1e-8,
                      out: torch.Tensor | None = None) -> torch.Tensor:
        """The advantage mean and ``1 / (std + eps)`` of every minibatch of an epoch in one launch (include/carl_amd.h:
        carl_ppo_adv_stats).  ``advantage``: the float32 ``[T, N]`` rows ``ppo_grad`` reads (of any pitch), or a contiguous
        1-D float32 storage; ``idx``: int32 ``[n_total]`` flat indices into it, the epoch's minibatches of ``batch_size``
        samples in order (the last may be shorter).  Returns float32 ``[ceil(n_total / batch_size), 2]``: row ``k`` is
        ``ppo_grad``'s ``adv_norm`` for minibatch ``k`` (``out``: such a tensor to write into).  No host synchronisation."""
        f32 = torch.float32
        storage = self._advantage_storage("ppo_adv_stats", advantage)
        if not is_exact(idx, self.device, torch.int32, (None,)) or idx.numel() < 1:
            raise ValueError(f"ppo_adv_stats 'idx': needs a contiguous int32 [n_total >= 1] tensor on {self.device}")
        n_total, batch_size = int(idx.numel()), int(batch_size)
        rows = int(self.lib.carl_ppo_adv_stats_rows(n_total, batch_size))
        if rows < 1:
            raise ValueError(f"ppo_adv_stats: batch_size {batch_size} < 1")
        if out is None:
            out = torch.empty((rows, 2), dtype=f32, device=self.device)
        if not is_exact(out, self.device, f32, (rows, 2)):
            raise ValueError(f"ppo_adv_stats 'out': needs a contiguous float32 [{rows}, 2] tensor on {self.device}")
        a = _lib.PpoAdvStats(_ptr(advantage), _ptr(idx), _ptr(out), storage, n_total, batch_size, float(eps))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.carl_ppo_adv_stats(C.byref(a), self._stream()))
        return out

    def adam_state(self, params: Sequence[torch.Tensor], n_sets: int | None = None) -> dict:
        """Fresh state for ``adam_step`` over ``params``: ``{"m", "v"}`` zero tensors like each parameter, ``"step"`` int64
        ``[1]`` = 0, ``"beta_pow"`` float64 ``[2]`` = (1, 1), on the device.  ``n_sets``: the state of a population for
        ``adam_step_sets`` instead -- every parameter ``[n_sets, n_i]``, ``"step"`` ``[n_sets]``, ``"beta_pow"`` ``[n_sets, 2]``."""
        lead = ()
        if n_sets is not None:
            lead = (int(n_sets),)
            if lead[0] < 1 or any(p.dim() < 1 or p.shape[0] != lead[0] for p in params):
                raise ValueError(f"adam_state: n_sets {lead[0]} needs every parameter as [{lead[0]}, n] rows")
        return {"m": [torch.zeros_like(p) for p in params], "v": [torch.zeros_like(p) for p in params],
                "step": torch.zeros(lead or 1, dtype=torch.int64, device=self.device),
                "beta_pow": torch.ones(lead + (2,), dtype=torch.float64, device=self.device)}

    def _adam_args(self, who: str, params, grads, state: dict, norm_out, betas, eps: float, sets: bool) -> tuple:
        """``(carl_adam_t, n_sets)`` of ``adam_step`` (tensors of any shape, ``n`` elements each; ``n_sets`` None) or, with
        ``sets``, of ``adam_step_sets`` (``[n_sets, n]`` rows), the tensors checked; ``lr`` and ``max_grad_norm`` are
        the caller's."""
        f32, i64, f64, dev = torch.float32, torch.int64, torch.float64, self.device
        k = len(params)
        if not 1 <= k <= _lib.ADAM_MAX_TENSORS:
            raise ValueError(f"{who}: {k} tensors, the launch takes 1 to {_lib.ADAM_MAX_TENSORS}")
        if len(grads) != k or len(state["m"]) != k or len(state["v"]) != k:
            raise ValueError(f"{who}: {k} parameters need {k} gradients and {k} entries of state['m'] / state['v']")
        n_sets = None
        if sets:
            if params[0].dim() < 1 or params[0].shape[0] < 1:
                raise ValueError(f"{who} params[0]: needs [P, n] rows")
            n_sets = int(params[0].shape[0])
        a = _lib.Adam()
        a.n_tensors = k
        for i in range(k):
            if sets and (params[i].dim() < 1 or params[i].shape[0] != n_sets):
                raise ValueError(f"{who} params[{i}]: needs [{n_sets}, n] rows, one per member")
            n = int(params[i].numel()) // (n_sets or 1)
            for name, t in (("params", params[i]), ("grads", grads[i]), ("state['m']", state["m"][i]),
                            ("state['v']", state["v"][i])):
                if not is_exact(t, dev, f32, n * (n_sets or 1)) or (sets and (t.dim() < 1 or t.shape[0] != n_sets)):
                    raise ValueError(f"{who} {name}[{i}]: needs a contiguous float32 " + (
                        f"[{n_sets}, {n}] tensor" if sets else f"tensor of {n} elements") + f" on {dev}")
            a.n[i], a.param[i], a.grad[i] = n, _ptr(params[i]), _ptr(grads[i])
            a.m[i], a.v[i] = _ptr(state["m"][i]), _ptr(state["v"][i])
        step, bp = state["step"], state["beta_pow"]
        if sets:
            if not is_exact(step, dev, i64, (n_sets,)):
                raise ValueError(f"{who} state['step']: needs a contiguous int64 [{n_sets}] tensor on {dev}")
        elif not is_exact(step, dev, i64, 1):
            raise ValueError(f"{who} state['step']: needs an int64 [1] tensor on {dev}")
        pair, pair_text = ((n_sets, 2), f"[{n_sets}, 2]") if sets else (2, "[2]")
        if not is_exact(bp, dev, f64, pair):
            raise ValueError(f"{who} state['beta_pow']: needs a contiguous float64 {pair_text} tensor on {dev}")
        if norm_out is not None and not is_exact(norm_out, dev, f64, pair):
            raise ValueError(f"{who} 'norm_out': needs a contiguous float64 {pair_text} tensor on {dev}")
        a.beta1, a.beta2, a.eps = float(betas[0]), float(betas[1]), float(eps)
        a.step, a.beta_pow, a.norm_out = _ptr(step), _ptr(bp), _ptr(norm_out)
        return a, n_sets

    def adam_step(self, params: Sequence[torch.Tensor], grads: Sequence[torch.Tensor], state: dict, lr: float,
                  betas=(0.9, 0.999), eps: float = 1e-5, max_grad_norm: float | None = None,
                  norm_out: torch.Tensor | None = None) -> None:
        """The global-norm clip of ``grads`` and one Adam step on ``params`` in one launch (include/carl_amd.h:
        carl_adam_step): up to 4 contiguous float32 device tensors, ``grads[i]`` with as many elements as ``params[i]``.
        ``state``: ``adam_state(params)``'s dict, advanced in place.  ``max_grad_norm=None``: no clip.  ``norm_out``: a
        float64 ``[2]`` device tensor that receives the norm before the clip and the coefficient.  No host synchronisation."""
        a, _ = self._adam_args("adam_step", params, grads, state, norm_out, betas, eps, sets=False)
        a.lr, a.max_grad_norm = float(lr), float("inf") if max_grad_norm is None else float(max_grad_norm)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.carl_adam_step(C.byref(a), self._stream()))

    # ------------------------------------------------------------------ a population's minibatch step (carl_amd/population.py)
    def _check_hyper(self, who: str, hyper: torch.Tensor, n_sets: int) -> None:
        if not is_exact(hyper, self.device, torch.float64, (n_sets, _lib.PPO_HYPER)):
            raise ValueError(f"{who} 'hyper': needs a contiguous float64 [{n_sets}, {_lib.PPO_HYPER}] tensor on {self.device} "
                             f"(columns {', '.join(_lib.PPO_HYPER_NAMES)})")

    def ppo_adv_stats_sets(self, advantage: torch.Tensor, idx: torch.Tensor, batch_size: int, eps: float = 1e-8,
                           out: torch.Tensor | None = None) -> torch.Tensor:
        """``ppo_adv_stats`` for every member of a population in one launch (include/carl_amd.h:
        carl_ppo_adv_stats_sets).  ``advantage`` as ``ppo_adv_stats`` takes it; ``idx``: int32 ``[P, n_total]`` rows of
        unit stride (the row pitch may be larger), row ``s`` member ``s``'s epoch, its minibatches of ``batch_size`` in order
        (the last may be shorter).  Returns float32 ``[P, ceil(n_total / batch_size), 2]``: row ``(s, k)`` is bit-equal to
        ``ppo_adv_stats`` on row ``s`` (``out``: such a tensor to write into).  No host synchronisation."""
        f32, i32 = torch.float32, torch.int32
        storage = self._advantage_storage("ppo_adv_stats_sets", advantage)
        if (idx.dtype != i32 or idx.device != self.device or idx.dim() != 2 or idx.shape[0] < 1 or idx.shape[1] < 1
                or (idx.shape[1] > 1 and idx.stride(1) != 1) or (idx.shape[0] > 1 and idx.stride(0) < idx.shape[1])):
            raise ValueError(f"ppo_adv_stats_sets 'idx': needs int32 [P >= 1, n_total >= 1] rows of unit stride on {self.device}")
        n_sets, n_total, batch_size = int(idx.shape[0]), int(idx.shape[1]), int(batch_size)
        stride = int(idx.stride(0)) if n_sets > 1 else n_total
        rows = int(self.lib.carl_ppo_adv_stats_rows(n_total, batch_size))
        if rows < 1:
            raise ValueError(f"ppo_adv_stats_sets: batch_size {batch_size} < 1")
        if out is None:
            out = torch.empty((n_sets, rows, 2), dtype=f32, device=self.device)
        if not is_exact(out, self.device, f32, (n_sets, rows, 2)):
            raise ValueError(f"ppo_adv_stats_sets 'out': needs a contiguous float32 [{n_sets}, {rows}, 2] tensor on {self.device}")
        a = _lib.PpoAdvStats(_ptr(advantage), _ptr(idx), _ptr(out), storage, n_total, batch_size, float(eps))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.carl_ppo_adv_stats_sets(C.byref(a), n_sets, stride, self._stream()))
        return out

    def adam_step_sets(self, params: Sequence[torch.Tensor], grads: Sequence[torch.Tensor], state: dict, hyper: torch.Tensor,
                       betas=(0.9, 0.999), eps: float = 1e-5, norm_out: torch.Tensor | None = None) -> None:
        """``adam_step`` for every member of a population in one launch (include/carl_amd.h: carl_adam_step_sets): up to 4
        contiguous float32 device tensors ``[P, n_i]``, ``grads[i]`` of the same shape, row ``s`` member ``s``'s.  ``state``:
        ``adam_state(params, n_sets=P)``'s dict, advanced in place.  ``hyper``: the population's float64 ``[P, 5]`` device
        tensor; member ``s`` steps with its ``lr`` and clips by its ``max_grad_norm`` (``+inf``: no clip) -- values the host
        cannot see: finite and ``>= 0`` is the caller's to guarantee.  ``norm_out``: a float64 ``[P, 2]`` device tensor.
        Member ``s`` is bit-equal to ``adam_step`` on its rows.  No host synchronisation."""
        a, n_sets = self._adam_args("adam_step_sets", params, grads, state, norm_out, betas, eps, sets=True)
        self._check_hyper("adam_step_sets", hyper, n_sets)
        a.lr, a.max_grad_norm = 0.0, float("inf")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.carl_adam_step_sets(C.byref(a), n_sets, _ptr(hyper), self._stream()))

    def drain_finished(self):
        """Finished-episode log since the last drain -> (global lane ids, returns, lengths,
        n_dropped); resets the counter.  Synchronises."""
        if self.fin_count is None:
            raise RuntimeError("engine was built with fin_capacity=0")
        n = int(self.fin_count.item())
        k = min(n, self.fin_capacity)
        out = (self.fin_lane[:k].clone(), self.fin_return[:k].clone(), self.fin_length[:k].clone(), n - k)
        self.fin_count.zero_()
        return out


def _check_policy_family(eng, policy) -> None:
    """ValueError unless ``policy`` was built for the family and observation of ``eng`` (the closed-loop launches)."""
    if policy.family != eng.family or policy.obs_dim != eng.D:
        raise ValueError(f"the policy was built for family {policy.family}, this engine runs family {eng.family}")


class VecEngine(LaneEngine):
    """N lanes of one env family on one device.

    Parameters
    ----------
    family : int | str
        ``carl_family_t`` (or its lower-case name).
    ctx_table : array [C, F]
        Context set in the family's feature order (defaults already filled).
    n_lanes : int
    device : torch.device | str
    selector : int
        ``carl_selector_t`` rule applied on every lane reset.
    ctx_idx0 : array [n_lanes] | None
        Context id each lane holds BEFORE its first reset.  Default: round robin
        ``(g - stride) mod C`` (so the first reset lands on ``g mod C``; with one lane
        this is the reference's 0, 1, 2, ...), otherwise ``g mod C`` (g = global lane id).
    lane_offset : int
        Global id of lane 0: lanes sharded over GPUs keep their global ids, so RNG
        streams and initial context assignment do not depend on the GPU count.
    """

    def __init__(self, family, ctx_table, n_lanes: int, device="cuda", *, selector: int = _lib.SEL_ROUND_ROBIN,
                 selector_stride: int = 1, auto_reset: bool = True, max_episode_steps: int | None = None,
                 seed: int = 0, lane_offset: int = 0, cartpole_recompute: bool = False,
                 ctx_obs_rows: Sequence[int] | None = None, ctx_idx0=None, fin_capacity: int = 0,
                 acrobot_fp32: bool = False, context_offset: int | None = None):
        if isinstance(family, str):
            family = _FAMILY_BY_NAME[family]
        super().__init__(_lib.family_info(int(family)), family, ctx_table, n_lanes, device, selector=selector,
                         selector_stride=selector_stride, auto_reset=auto_reset, max_episode_steps=max_episode_steps,
                         seed=seed, lane_offset=lane_offset, ctx_obs_rows=ctx_obs_rows, ctx_idx0=ctx_idx0,
                         fin_capacity=fin_capacity, context_offset=context_offset,
                         flags=(_lib.FLAG_CARTPOLE_RECOMPUTE if cartpole_recompute else 0) | (
                             _lib.FLAG_ACROBOT_FP32 if acrobot_fp32 else 0))
        # done-mask compaction buffers
        self.done_idx = torch.zeros(max(self.n, 1), dtype=torch.int32, device=self.device)
        self.done_count = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._scratch = torch.zeros(int(self.lib.carl_done_compact_scratch_elems(self.n)), dtype=torch.int32,
                                    device=self.device)
        self._step_fn = self.lib.carl_step  # (_c_step_fast)
        self._warned_direct = False
        self._act_pad = None  # the one padded copy of a rollout's actions that is kept (_pad_action_rows)

    # ------------------------------------------------------------------ library calls
    def _c_reset(self, mask_ptr) -> int:
        return self.lib.carl_reset(C.byref(self.b), mask_ptr, _ptr(self.obs), self._stream())

    def _c_step(self, io) -> int:
        return self.lib.carl_step(C.byref(self.b), C.byref(io), self._stream())

    def _c_step_fast(self, stream: int) -> int:  # self._io, prepared references
        return self._step_fn(self._b_ref, self._io_ref, stream)

    def _c_rollout(self, io, n_steps: int) -> int:
        return self.lib.carl_rollout(C.byref(self.b), C.byref(io), n_steps, self._stream())

    def _narrow_action(self, a: torch.Tensor) -> tuple[torch.Tensor, int] | None:
        """The narrow rollout-only input formats (uint8 / float16 / bfloat16: include/carl_amd.h) that the classic-control
        kernels' loader wave reads."""
        if a.dtype == torch.uint8 and self.info.action_is_discrete:
            align, dt = 4, _lib.ACTION_U8
        elif a.dtype in (torch.float16, torch.bfloat16) and not self.info.action_is_discrete:
            align, dt = 8, _lib.ACTION_F16 if a.dtype == torch.float16 else _lib.ACTION_BF16
        else:
            return None
        # (a view into a larger buffer: the kernel reads dwords / 8-byte pieces)
        return (a.clone() if a.is_contiguous() and a.data_ptr() % align else a), dt

    def done_compact(self) -> tuple[torch.Tensor, torch.Tensor]:
        """Ascending ids of lanes whose last step ended their episode -> (idx[n], count[1])."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.carl_done_compact(
                _ptr(self.terminated), _ptr(self.truncated), self.n, _ptr(self.done_idx),
                _ptr(self.done_count), _ptr(self._scratch), self._stream()))
        return self.done_idx, self.done_count

    def reset_indexed(self, idx: torch.Tensor, count: torch.Tensor) -> torch.Tensor:
        with torch.cuda.device(self.device):
            _lib.check(self.lib.carl_reset_indexed(C.byref(self.b), _ptr(idx), _ptr(count), _ptr(self.obs),
                                                   self._stream()))
        return self.obs

    def reset_done(self) -> torch.Tensor:
        """Explicit-reset path: compact the done mask, reset exactly those lanes."""
        idx, count = self.done_compact()
        return self.reset_indexed(idx, count)

    def _row_pitch(self) -> int:
        """Lanes per ROW of a rollout's action / output arrays (``carl_step_io_t.row_pitch``): the lane count rounded up
        to a multiple of 16, so that every row's 16-byte pieces stay aligned and ANY lane count -- 10, 65 537, the uneven
        shards of ``distributed.lane_shard`` -- takes the staged kernel (round 6; such batches used to fall back to the
        ~50 % slower direct-store kernel).  Dense rows under ``FLAG_ROLLOUT_DIRECT`` (the A/B switch)."""
        if self.b.flags & _lib.FLAG_ROLLOUT_DIRECT:
            return self.n
        return int(self.lib.carl_rollout_pitch(self.n))

    def _launch_rollout(self, r: _PreparedRollout) -> dict:
        """``LaneEngine._launch_rollout`` with what the staged / direct-store pair of kernels adds: one warning when a
        launch takes the direct-store kernel, and narrow actions widened once where only wide ones are read."""
        if not self._warned_direct and \
                self.lib.carl_rollout_variant_io(self._b_ref, C.byref(r.io)) == _lib.ROLLOUT_DIRECT_SHAPE:
            import warnings

            self._warned_direct = True
            warnings.warn(f"carl_rollout: {self.n} lanes in rows {r.io.row_pitch or self.n} lanes long (not a multiple of 16, "
                          "or a view into a wider array, or an array that does not start on a 16-byte boundary) -- this launch "
                          "takes the direct-store kernel (~50 % slower than the staged one; same results).  Use "
                          "alloc_rollout()'s buffers (rows padded to a multiple of 16) for the fast path.",
                          RuntimeWarning, stacklevel=3)
        with torch.cuda.device(self.device):
            code = self._c_rollout(r.io, r.T)
            if code == _lib.ERR_UNSUPPORTED and r.dt in (_lib.ACTION_U8, _lib.ACTION_F16, _lib.ACTION_BF16):
                # the narrow formats are read by the lean staged rollout only (moving selectors, the finished-episode
                # log, terminal observations and dense rows of an odd lane count take kernels that read int32 /
                # float32): widen once, same results
                a, dt = self._action_tensor(r.a.to(torch.int32 if r.dt == _lib.ACTION_U8 else torch.float32), (r.T,))
                code = self._c_rollout(self._rollout_io(a, dt, r.out, r.T), r.T)
            _lib.check(code)
        return r.out

    def _out_pitch(self, out: dict) -> int:
        """Lanes per row of a ``[T, N, ...]`` output dict, read off its ``reward`` array (a one-row buffer may carry any
        stride)."""
        r = out["reward"]
        return max(self.n, int(r.stride(0))) if r.dim() == 2 else self.n

    def _pad_action_rows(self, a: torch.Tensor, T: int, P: int) -> torch.Tensor:
        key = (T, P, a.dtype)
        buf = self._act_pad.get(key) if self._act_pad else None
        if buf is None:
            self._act_pad = {key: torch.empty((T, P), dtype=a.dtype, device=self.device)}  # (one size kept)
            buf = self._act_pad[key]
        rows = a.view(T, self.n)
        buf[:, : self.n] = rows
        buf[:, self.n:] = rows[:, self.n - 1:]
        return buf

    # ------------------------------------------------------------------ closed loop (carl_amd/policy.py)
    def _sampling(self, policy, deterministic: bool, sample_seed: int, log_prob: torch.Tensor | None = None):
        """the ``carl_policy_sampling_t`` of a sampled launch (include/carl_amd.h), None for a deterministic one"""
        if deterministic:
            if log_prob is not None:
                raise ValueError("log_prob: sampled launches only (deterministic=False)")
            return None
        s = _lib.PolicySampling()
        s.seed = int(sample_seed) & (2**64 - 1)
        s.log_std = None if policy.discrete else policy.device_log_std(self.device).data_ptr()
        s.log_prob = _ptr(log_prob)
        return s

    # ---- LaneEngine's PPO hooks: the classic-control entry points
    def _ppo_check_policy(self, policy) -> None:
        _check_policy_family(self, policy)

    def _ppo_action_tail(self) -> tuple:
        return ()

    def _ppo_log_std_floats(self) -> int:
        return 0 if self.info.action_is_discrete else 1

    def _c_context_trace(self, ctx0, ep0, te, tr, T, pitch, out) -> int:
        return self.lib.carl_policy_context_trace(self._b_ref, ctx0, ep0, te, tr, T, pitch, out, self._stream())

    def _c_ppo_workspace_floats(self, pol, crit, n_samples) -> int:
        return self.lib.carl_ppo_workspace_floats(pol, crit, n_samples)

    def _c_ppo_grad(self, pb, pol, crit, log_std, po) -> int:
        return self.lib.carl_ppo_grad(pb, pol, crit, log_std, po, self._stream())

    def _c_ppo_input_stats(self, pb, pol, st) -> int:
        return self.lib.carl_ppo_input_stats(pb, pol, st, self._stream())

    # ---- a population of PPO learners (carl_amd/population.py): the classic-control families only
    def _check_population(self, who: str, policy, value_net) -> tuple[int, int]:
        """(P, L) of a stacked actor and critic whose sets tile this engine's lanes"""
        _check_policy_family(self, policy)
        _check_policy_family(self, value_net)
        P, L = policy.n_sets, policy.lanes_per_set
        if L is None or value_net.lanes_per_set != L or value_net.n_sets != P:
            raise ValueError(f"{who}: the actor and the critic need the same weight sets and lanes_per_set (MLPPolicy.stack / "
                             f"on_device), got {P} x {L} and {value_net.n_sets} x {value_net.lanes_per_set}")
        if P * L != self.n:
            raise ValueError(f"{who}: {P} sets x {L} lanes are not this engine's {self.n} lanes (member s owns lanes "
                             "[s * lanes_per_set, (s + 1) * lanes_per_set))")
        return P, L

    def ppo_sets_workspace(self, policy, value_net, n_samples: int) -> torch.Tensor:
        """A float32 workspace for ``ppo_grad_sets`` with ``n_samples`` samples per member
        (carl_ppo_sets_workspace_floats): as many one-set workspaces as the policy has sets -- up to about 13 MB per member
        at 256 workgroups of 64-wide networks."""
        need = int(self.lib.carl_ppo_sets_workspace_floats(C.byref(policy.struct(self.n, 0x10)),
                                                           C.byref(value_net.struct(self.n, 0x10)), int(n_samples)))
        if need < 0:
            raise ValueError(f"ppo_sets_workspace: invalid shapes or n_samples {n_samples}")
        return torch.empty(need, dtype=torch.float32, device=self.device)

    def ppo_grad_sets(self, policy, value_net, buf: dict, obs0: torch.Tensor, context_id: torch.Tensor, *, idx: torch.Tensor,
                      hyper: torch.Tensor, adv_norm: torch.Tensor | None = None, out: dict | None = None,
                      workspace: torch.Tensor | None = None) -> dict:
        """``ppo_grad`` for ``P`` independent learners in its three launches (include/carl_amd.h: carl_ppo_grad_sets).
        ``policy`` / ``value_net``: ``P`` weight sets of ``L`` lanes each (``MLPPolicy.stack`` / ``on_device``) with ``P * L``
        this engine's lanes; member ``s`` owns lanes ``[s * L, (s + 1) * L)`` of ``buf`` (``buf``, ``obs0``, ``context_id`` as
        ``ppo_grad`` takes them).  ``idx``: int32 ``[P, M]`` rows of unit stride, row ``s`` the flat indices ``t * pitch +
        lane`` of member ``s``'s minibatch (a lane outside the member's contributes zero).  ``hyper``: float64 ``[P, 5]`` on
        the device (lr, clip_range, vf_coef, ent_coef, max_grad_norm; finite and ``>= 0``, which the host cannot check there).
        ``adv_norm``: float32 ``[P, 2]`` rows of unit stride or None.  Returns ``{"grad_actor" [P, set_floats], "grad_critic"
        [P, set_floats], "grad_log_std" [P] (Box families), "stats" [P, 6]}``, row ``s`` bit-equal to ``ppo_grad`` with
        member ``s``'s one-set networks, index row, ``adv_norm`` row and float32 coefficients (``out``: such a dict to write
        into).  No host synchronisation."""
        P, L = self._check_population("ppo_grad_sets", policy, value_net)
        T, N, pitch = self._ppo_buffer("ppo_grad_sets", buf, obs0, context_id)
        f32, i32 = torch.float32, torch.int32
        if (not isinstance(idx, torch.Tensor) or idx.dtype != i32 or idx.device != self.device or idx.dim() != 2
                or idx.shape[0] != P or idx.shape[1] < 1 or (idx.shape[1] > 1 and idx.stride(1) != 1)
                or (P > 1 and idx.stride(0) < idx.shape[1])):
            raise ValueError(f"ppo_grad_sets 'idx': needs int32 [{P}, M >= 1] rows of unit stride on {self.device}")
        M = int(idx.shape[1])
        if M > T * L:
            raise ValueError(f"ppo_grad_sets 'idx': {M} samples per member, a member has {T} steps x {L} lanes")
        if adv_norm is not None and (adv_norm.dtype != f32 or adv_norm.device != self.device or tuple(adv_norm.shape) != (P, 2)
                                     or adv_norm.stride(1) != 1 or (P > 1 and adv_norm.stride(0) < 2)):
            raise ValueError(f"ppo_grad_sets 'adv_norm': needs float32 [{P}, 2] rows of unit stride on {self.device}")
        self._check_hyper("ppo_grad_sets", hyper, P)
        res = {} if out is None else out
        box = not self.info.action_is_discrete
        want = {"grad_actor": (P, policy.set_floats), "grad_critic": (P, value_net.set_floats), "stats": (P, 6)}
        if box:
            want["grad_log_std"] = (P,)
        for k, shape in want.items():
            if k not in res:
                res[k] = torch.empty(shape, dtype=f32, device=self.device)
            if not is_exact(res[k], self.device, f32, shape):
                raise ValueError(f"ppo_grad_sets output '{k}': needs a contiguous float32 {list(shape)} tensor on {self.device}")
        pol = policy.struct(self.n, policy.device_params(self.device).data_ptr())
        crit = value_net.struct(self.n, value_net.device_params(self.device).data_ptr())
        ws = self.ppo_sets_workspace(policy, value_net, M) if workspace is None else workspace
        pb = self._ppo_batch(T, N, pitch, buf, obs0, context_id)
        pb.n_samples = M
        st = _lib.PpoSets(_ptr(hyper), _ptr(idx), _ptr(adv_norm), int(idx.stride(0)) if P > 1 else M,
                          0 if adv_norm is None else (int(adv_norm.stride(0)) if P > 1 else 2))
        po = _lib.PpoOut(_ptr(res["grad_actor"]), _ptr(res["grad_critic"]), _ptr(res.get("grad_log_std")), _ptr(res["stats"]),
                         None, None, _ptr(ws), int(ws.numel()))
        ls = policy.device_log_std(self.device).data_ptr() if box else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.carl_ppo_grad_sets(C.byref(pb), C.byref(pol), C.byref(crit), ls, C.byref(st), C.byref(po),
                                                   self._stream()))
        return res

    def _policy_call(self, fn, *args) -> None:
        """One closed-loop C call ``fn(batch, *args, stream)`` on the current stream, its error code raised."""
        with torch.cuda.device(self.device):
            _lib.check(fn(self._b_ref, *args, self._stream()))

    def rollout_policy(self, policy, n_steps: int, out: dict | None = None, mode: str = "transitions",
                       final_obs: bool = False, deterministic: bool = True, sample_seed: int = 0,
                       log_prob: bool = False, *, value_net=None, bootstrap_truncated: bool = True,
                       gae: tuple | None = None) -> dict:
        """``n_steps`` steps in ONE launch, each lane's action chosen on the device by ``policy`` (``carl_amd.policy.
        MLPPolicy``) from the lane's current context and observation -- closed loop, where ``rollout`` replays actions
        written beforehand.
        ``mode="transitions"``: ``rollout``'s dict (``alloc_rollout`` layout; ``final_obs=True`` adds the terminal
        observations) plus ``"action"`` ``[T, N]`` (int32 / float32): the action each step took -- ``rollout`` of those
        actions from the same engine state gives the same bits.  ``mode="summary"``: no per-step output at all; returns
        ``{"episodes", "return_sum", "length_sum"}`` per lane (episodes finished in the launch, the float32 sum of their
        returns in step order, the sum of their lengths).  Either way the engine state advances exactly as in
        ``rollout``; a summary needs ``auto_reset`` (ValueError otherwise).  No host synchronisation (the policy's parameters
        are uploaded on its first use on a device).
        ``deterministic=False``: each action is sampled from the policy's distribution (a categorical over the logits /
        a Gaussian of ``policy.log_std``; include/carl_amd.h: carl_rollout_policy_sampled), the draws keyed by
        ``sample_seed`` and by (lane, episode, step in episode).  ``log_prob=True`` (transitions mode) adds
        ``"log_prob"`` ``[T, N]`` float32: each action's log-probability under the policy.
        ``value_net=critic`` (an ``MLPPolicy`` with ``head="value"``; transitions mode): the critic runs inside the same
        launch on the inputs the actor sees (include/carl_amd.h: carl_rollout_policy_valued) and ``out`` gains ``"value"``
        ``[T, N]`` (V of the input each action was chosen from), ``"last_value"`` ``[N]`` (V of each lane's input after the
        last step) and, with ``bootstrap_truncated`` (needs ``auto_reset``), ``"boot_value"`` ``[T, N]``: V of the
        terminal observation where a step ended an episode by truncation alone, +0 elsewhere (SB3's timeout bootstrap).
        A sampled launch with a critic always returns ``"log_prob"``.  Everything else the launch writes keeps its bits.
        ``gae=(gamma, lam)`` adds ``"advantage"`` and ``"return"`` ``[T, N]`` from one ``carl_gae`` launch on the same
        stream (``VecEngine.gae`` of the launch's own columns)."""
        _check_policy_family(self, policy)
        if final_obs and mode == "summary":
            raise ValueError("final_obs: transitions mode only (a summary launch stores nothing per step)")
        # (named by its class: test_policy_sampling.py drives this method on a stand-in ``self`` without the helpers)
        log_prob, gae = LaneEngine._policy_keywords(self, policy, mode, deterministic, log_prob, value_net,
                                                    bootstrap_truncated, gae)
        T = int(n_steps)
        params = policy.device_params(self.device)
        pol = policy.struct(self.n, params.data_ptr())

        def launch(smp, io, summ):  # the deterministic entry point or its sampled twin
            if smp is None:
                self._policy_call(self.lib.carl_rollout_policy, C.byref(pol), io, T, summ)
            else:
                self._policy_call(self.lib.carl_rollout_policy_sampled, C.byref(pol), C.byref(smp), io, T, summ)

        if mode == "summary":
            res = self.alloc_policy_summary() if out is None else out
            for k, _ in self._SUMMARY_KEYS:  # (any 4-byte element type is taken here; the Brax engine wants the exact ones)
                t = res[k]
                if t.device != self.device or not t.is_contiguous() or t.numel() != self.n or t.element_size() != 4:
                    raise ValueError(f"summary output '{k}' must be a contiguous 4-byte [{self.n}] tensor on {self.device}")
            launch(self._sampling(policy, deterministic, sample_seed), None, self._policy_summary(res))
            return res
        if out is None:
            out = self.alloc_rollout(T, final_obs=final_obs)
            self._policy_columns(out, ("action",), T, torch.int32 if self.info.action_is_discrete else torch.float32)
        io = self._rollout_io(None, None, out, T)
        if log_prob:
            self._policy_columns(out, ("log_prob",), T)
        smp = self._sampling(policy, deterministic, sample_seed, out["log_prob"] if log_prob else None)
        if value_net is None:
            launch(smp, C.byref(io), None)
            return out
        self._policy_columns(out, ("value", "boot_value") if bootstrap_truncated else ("value",), T)
        lv = self._policy_last_value(out)
        cparams = value_net.device_params(self.device)
        crit = value_net.struct(self.n, cparams.data_ptr())
        vout = _lib.PolicyValue(_ptr(out["value"]), _ptr(lv), _ptr(out["boot_value"]) if bootstrap_truncated else None)
        self._policy_call(self.lib.carl_rollout_policy_valued, C.byref(pol), C.byref(crit),
                          None if smp is None else C.byref(smp), C.byref(io), T, None, C.byref(vout))
        if gae is not None:
            self._policy_gae(out, T, gae, bootstrap_truncated)
        return out

    def evaluate_policy(self, policy, n_episodes: int, max_steps: int, out: dict | None = None,
                        deterministic: bool = True, sample_seed: int = 0, input_stats: bool = False) -> dict:
        """Run ``policy`` (``carl_amd.policy.MLPPolicy``) on every lane until the lane has finished ``n_episodes``
        episodes or taken ``max_steps`` steps, in ONE launch, from the current engine state (a running episode is counted
        with its full length; ``CARLEnv.evaluate_policy`` resets first).  Returns ``alloc_policy_episodes``' dict:
        ``episodes`` / ``steps`` per lane, and per lane and episode k < ``episodes`` its fp32 ``return``, ``length``, the
        ``context_id`` it ran in and whether it ``terminated`` (NaN / 0 / -1 / 0 beyond).  A lane's records are those of
        its first episodes in a transitions-mode ``rollout_policy``, bit for bit, and the engine state advances exactly as
        for the steps each lane took.  Needs ``auto_reset``.  ``carl_amd.policy.episode_stats`` reduces the result per
        context.  No host synchronisation.  ``deterministic=False``: sampled actions, as ``rollout_policy``'s (SB3's
        ``evaluate_policy(..., deterministic=False)``); the records are then those of a sampled transitions launch with
        the same ``sample_seed``.  ``input_stats=True``: the launch also gathers, for every live lane-step, the sums of
        ``d = x_raw - shift`` and ``d * d`` of every policy input (include/carl_amd.h: carl_evaluate_policy_stats); the
        result gains ``"input_partial"``, the float64 ``[workgroups, 2, 32]`` device tensor of per-workgroup sums that
        ``carl_amd.policy.InputStats.update`` merges (with ``input_stats=False`` a reused ``out`` loses that key, so the
        sums of an earlier launch are never merged beside this launch's ``steps``).  Records and engine state are the
        same bits either way."""
        _check_policy_family(self, policy)
        K, T, res, eps = self._policy_episodes("evaluate_policy", n_episodes, max_steps, out)
        params = policy.device_params(self.device)
        pol = policy.struct(self.n, params.data_ptr())
        smp = self._sampling(policy, deterministic, sample_seed)
        tail = (K, T, C.byref(eps))
        if input_stats:
            st = self._policy_input_partial("evaluate_policy", res, int(self.lib.carl_policy_stats_workgroups(self.n)))
            self._policy_call(self.lib.carl_evaluate_policy_stats, C.byref(pol), None if smp is None else C.byref(smp),
                              *tail, C.byref(st))
            return res
        res.pop("input_partial", None)  # a reused dict must not carry an earlier launch's sums beside this launch's steps
        if smp is None:
            self._policy_call(self.lib.carl_evaluate_policy, C.byref(pol), *tail)
        else:
            self._policy_call(self.lib.carl_evaluate_policy_sampled, C.byref(pol), C.byref(smp), *tail)
        return res

    def rollout_variant(self) -> int:
        """Which kernel ``rollout`` launches for this batch into ``alloc_rollout``'s buffers: ``_lib.ROLLOUT_STAGED``
        (fast path: rows of a pitch that is a multiple of 16 -- any lane count since round 6), ``ROLLOUT_DIRECT_FLAG``
        (the A/B switch); ``ROLLOUT_DIRECT_SHAPE`` only for caller-made dense buffers of an odd lane count
        (carl_rollout_variant_io)."""
        io = _lib.StepIO()
        io.row_pitch = self._row_pitch()
        return int(self.lib.carl_rollout_variant_io(C.byref(self.b), C.byref(io)))
