"""Closed-loop rollout throughput: CartPole x 65 536 lanes x 1 000 steps per launch, env-steps/s of

  policy_rollout   VecEngine.rollout_policy (transitions / summary) with a linear policy, a 2x32 and a 2x64 tanh MLP
                   (each seeing the eight context features and the observation);
  open_loop        VecEngine.rollout of pre-written int32 actions (the staged kernel), same T;
  graph_step_mlp   what a caller has without the feature: a captured hipGraph of `step` + a torch forward of the same
                   MLP + argmax per env step (100 steps per graph, replayed to 1 000).
  evaluate         VecEngine.evaluate_policy (episodes mode), linear and 2x64 tanh: K = 10 episodes per lane, at most
                   5 000 steps, every launch from the same snapshot.  Reports the launch time, the lane-steps taken
                   (sum of `steps`), lane-steps/s, the same policy's summary-mode env-steps/s, the early-exit
                   overhead (sum over wavefronts of 64 x that wave's largest `steps`, over the sum of `steps`), and
                   the launch time per step of its longest lane against summary mode's time per step.

  --sampled        also the sampled launches (rollout_policy(..., deterministic=False)) of the same policies:
                   transitions with and without log_prob, and summary.

  --legs value     the critic inside the launch and GAE on the device, T = 256 and --steps, linear / 2x32 / 2x64 tanh for
                   both networks, each against the way to the same arrays without them:
                   (a) rollout_policy(..., value_net=) against the sampled + log_prob launch followed by the torch critic
                       on the inputs rebuilt from its `obs` rows (static selector: the context part is constant);
                   (b) VecEngine.gae against the torch reverse loop over the same columns.
                   Written to key "value" of --out.

  --legs es        one ES generation, CartPole x --lanes, --lanes / 256 weight sets of 256 lanes, linear and 2x64 tanh,
                   n_episodes = 1, max_steps = 500: (a) EvolutionStrategy.step against (b) the way to the same centre
                   update without it -- NumPy noise, one MLPPolicy per member, stack, upload, evaluate_policy, read-back,
                   NumPy ranks and sum -- both as a host clock around a generation that ends in a device synchronise;
                   and the two new launches on their own (device events around 50 back-to-back launches).
                   Written to key "es" of --out.

  --legs stats     evaluate_policy(..., input_stats=True) against the same launch without statistics (the kernel of the
                   parent commit: profiles/policy_stats_isa_identity.txt), CartPole x --lanes, K = 1, max_steps = 500, linear
                   and 2x64 tanh, every launch from the same snapshot; and the merge launch (InputStats.update writing one
                   block) on its own, device events around 50 back-to-back launches.  Written to key "stats" of --out.

  --legs brax_es   the episodes mode of the Brax closed loop and ES on it (runs on its own engines; --lanes is not used):
                   (a) BraxVecEngine.evaluate_episodes, K = 1, against summary-mode rollout_policy of S and of 1 000 steps,
                       Ant x 32 768 and Hopper x 32 768, 2x64 tanh, static selector, for TimeLimit = max_steps = 1 000
                       (S = 1 000) and TimeLimit 100 with max_steps = 1 000 (S = 100): every env stops by step S.  State
                       restored before each launch; device events; the median of --reps after a warm-up.
                   (b) one EvolutionStrategy generation, Ant x 32 768 in sets of 256 (P = 128), TimeLimit 100, max_steps
                       1 000: a host clock around step() that ends in a device synchronise, beside the evaluate_episodes
                       launch alone.  Written to key "brax_es" of --out.

  --legs brax_stats  input statistics inside the Brax episodes launch (runs on its own engine; --lanes is not used), brax_es's
                   set-up: Ant x 32 768, 2x64 tanh, K = 1, TimeLimit 100, max_steps 1 000.  evaluate_episodes(...,
                   input_stats=True) against evaluate_episodes without it (the kernel of the parent commit:
                   profiles/brax_stats_isa_identity.txt) in the same process, state restored before each launch, device
                   events, the two sides interleaved; and one normalised EvolutionStrategy generation (merge included)
                   against one unnormalised, a host clock around step() that ends in a device synchronise.  The median of
                   --reps after a warm-up (the launches: of two interleaved runs of --reps per side).  Written to key
                   "brax_stats" of --out.

  --legs brax_sample  sampled actions and log-probabilities inside the Brax closed-loop launch (runs on its own engines;
                   --lanes is not used): Ant x 32 768 and Halfcheetah x 32 768, 100-step transitions launches, 2x64 tanh,
                   TimeLimit 1 000, log_std 0.  rollout_policy(deterministic=False) with and without log_prob against the
                   deterministic launch (the kernel of the parent commit: profiles/brax_policy_sample_isa_identity.txt) in
                   the same process, state restored before each launch, device events, the three sides interleaved over
                   two rounds; a warm-up, then the median of --reps per round (reported: of both rounds together, and the
                   spread of the deterministic side's repetitions, which a difference has to exceed to count).  Written
                   to key "brax_sample" of --out.

  --legs brax_value  a critic inside the sampled Brax launch (runs on its own engines; --lanes is not used): Ant x 32 768 and
                   Halfcheetah x 32 768, 100-step transitions launches, 2x64 tanh actor and critic, static selector,
                   TimeLimit 1 000.  Sides: (a) the sampled launch with log_prob (the kernel of the parent commit:
                   profiles/brax_policy_value_isa_identity.txt); (b) rollout_policy(value_net=); (c) the route to the same
                   arrays without it: (a) with final_obs, then a torch critic of the same shape on the observation rows
                   and the terminal rows (right only because the selector is static: no context inputs); (d) (b) and (c)
                   each followed by gae.  State restored before each launch, device events, the sides interleaved over
                   two rounds, a warm-up per side and round, the median and range of the 2 x --reps repetitions.
                   Written to key "brax_value" of --out.

Host timing with torch.cuda events around `--reps` launches after one warm-up launch; the median per launch is
reported.  Kernel times belong to a separate `rocprofv3 --kernel-trace --stats` run of this script.

  python tools/policy_rollout_bench.py [--lanes 65536] [--steps 1000] [--reps 5] [--legs rollout,evaluate,value,es,stats,brax_es,brax_stats,brax_sample,brax_value] [--out FILE]

--out FILE: a JSON file whose keys of the legs run ("results": rollout, "evaluate") are replaced, others kept.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from carl_amd import _lib  # noqa: E402
from carl_amd.engine import VecEngine  # noqa: E402
from carl_amd.envs import CARLCartPole  # noqa: E402
from carl_amd.policy import MLPPolicy  # noqa: E402


def make_engine(n, seed=0):
    rng = np.random.default_rng(seed)
    names = list(CARLCartPole.get_context_features())
    t = np.tile([float(f.default_value) for f in CARLCartPole.get_context_features().values()], (n, 1))
    t[:, names.index("gravity")] = rng.uniform(5, 15, n)
    t[:, names.index("length")] = rng.uniform(0.3, 1.0, n)
    eng = VecEngine(_lib.CARTPOLE, t, n, "cuda", selector=_lib.SEL_STATIC, auto_reset=True, seed=seed)
    eng.reset()
    return eng


def make_mlp(widths, n_in, seed=0):
    torch.manual_seed(seed)
    mods, prev = [], n_in
    for w in widths:
        mods += [torch.nn.Linear(prev, w), torch.nn.Tanh()]
        prev = w
    mods.append(torch.nn.Linear(prev, 2))
    return torch.nn.Sequential(*mods)


def time_launches(fn, reps):
    fn()  # warm-up (code object load, first-touch of the buffers)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts)), ts


def graph_step_mlp(eng, mlp, T, per_graph=100):
    """a hipGraph of `per_graph` x (torch forward of mlp on [ctx_obs, obs] -> argmax -> step)"""
    dev = eng.device
    act = torch.zeros(eng.n, dtype=torch.int32, device=dev)

    def one():
        x = torch.cat([eng.ctx_obs.t(), eng.obs], dim=1)
        act.copy_(mlp(x).argmax(dim=1).to(torch.int32))
        eng.step(act)

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(3):
            one()
        with torch.cuda.graph(g, stream=side):
            for _ in range(per_graph):
                one()
    torch.cuda.current_stream(dev).wait_stream(side)

    def run():
        for _ in range(T // per_graph):
            g.replay()

    return run


def evaluate_leg(eng, n_in, T_summary, reps, K=10, max_steps=5000):
    """the episodes mode against the same policy's summary mode (module docstring)"""
    rows = []
    snap = eng.snapshot()
    for name, widths in {"linear": [], "mlp_2x64_tanh": [64, 64]}.items():
        pol = MLPPolicy.from_sequential(eng, make_mlp(widths, n_in))
        res = eng.alloc_policy_episodes(K)
        ts = []
        for _ in range(reps + 1):  # (the first: warm-up)
            eng.restore(snap)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.evaluate_policy(pol, K, max_steps, out=res)
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e-3)
        sec = float(np.median(ts[1:]))
        steps = res["steps"].to(torch.int64)
        lane_steps = int(steps.sum())
        wave_max = steps[: eng.n // 64 * 64].view(-1, 64).max(dim=1).values
        eng.restore(snap)
        s = eng.alloc_policy_summary()
        ssec, sts = time_launches(lambda: eng.rollout_policy(pol, T_summary, out=s, mode="summary"), reps)
        r = {"config": f"evaluate_{name}", "lanes": eng.n, "n_episodes": K, "max_steps": max_steps,
             "sec_per_launch": sec, "lane_steps": lane_steps, "lane_steps_per_s": lane_steps / sec,
             "episodes_finished": int(res["episodes"].sum()), "max_lane_steps": int(steps.max()),
             "early_exit_overhead": float(64 * wave_max.sum()) / max(lane_steps, 1),
             "summary_steps": T_summary, "summary_env_steps_per_s": eng.n * T_summary / ssec,
             "lane_steps_per_s_over_summary": (lane_steps / sec) / (eng.n * T_summary / ssec),
             # the launch lasts as long as its longest lane: time per step of that lane against summary mode's per step
             "ns_per_step_longest_lane": sec / max(int(steps.max()), 1) * 1e9, "summary_ns_per_step": ssec / T_summary * 1e9,
             "reps_sec": ts[1:]}
        rows.append(r)
        print(json.dumps(r), flush=True)
    eng.restore(snap)
    return rows


def torch_gae(reward, value, te, tr, last_value, boot, gamma, lam):
    """the reverse loop a caller writes without carl_gae (SB3's rule, timeout bootstrap folded into the reward)"""
    T = reward.shape[0]
    adv = torch.empty_like(reward)
    a = torch.zeros_like(last_value)
    nxt = last_value
    for t in range(T - 1, -1, -1):
        live = 1.0 - (te[t] | tr[t]).float()
        rew = reward[t] + gamma * boot[t]
        delta = rew + gamma * nxt * live - value[t]
        a = delta + gamma * lam * live * a
        adv[t] = a
        nxt = value[t]
    return adv, adv + value


def value_leg(eng, n_in, steps, reps, block=64):
    rows = []
    ctx = eng.ctx_obs.t().contiguous()
    for T in sorted({256, steps}):
        for name, widths in {"linear": [], "mlp_2x32_tanh": [32, 32], "mlp_2x64_tanh": [64, 64]}.items():
            actor = make_mlp(widths, n_in)
            critic = make_mlp(widths, n_in, seed=1)
            critic[-1] = torch.nn.Linear(critic[-1].in_features, 1)
            pol = MLPPolicy.from_sequential(eng, actor)
            vf = MLPPolicy.from_sequential(eng, critic, head="value")
            critic = critic.to(eng.device)
            kw = dict(deterministic=False, sample_seed=1)
            vout = eng.rollout_policy(pol, T, value_net=vf, **kw)
            sout = eng.rollout_policy(pol, T, log_prob=True, **kw)
            val = torch.empty((T, eng.n), device=eng.device)

            def parent_way():
                obs0 = eng.obs.clone()
                eng.rollout_policy(pol, T, out=sout, log_prob=True, **kw)
                with torch.no_grad():
                    for t0 in range(0, T, block):
                        t1 = min(T, t0 + block)
                        o = torch.cat([obs0[None] if t0 == 0 else sout["obs"][t0 - 1: t0], sout["obs"][t0: t1 - 1]])
                        x = torch.cat([ctx[None].expand(t1 - t0, -1, -1), o], dim=2)
                        val[t0:t1] = critic(x)[..., 0]
                    critic(torch.cat([ctx, sout["obs"][T - 1]], dim=1))  # last_value

            sec_v, ts_v = time_launches(lambda: eng.rollout_policy(pol, T, out=vout, value_net=vf, **kw), reps)
            sec_s, _ = time_launches(lambda: eng.rollout_policy(pol, T, out=sout, log_prob=True, **kw), reps)
            sec_p, ts_p = time_launches(parent_way, reps)
            g = {k: vout[k] for k in ("advantage", "return")} if "advantage" in vout else None
            args = (vout["reward"], vout["value"], vout["terminated"], vout["truncated"], vout["last_value"])
            res = eng.gae(*args, 0.99, 0.95, boot_value=vout["boot_value"], out=g)
            sec_g, ts_g = time_launches(lambda: eng.gae(*args, 0.99, 0.95, boot_value=vout["boot_value"], out=res), reps)
            sec_t, ts_t = time_launches(lambda: torch_gae(*args, vout["boot_value"], 0.99, 0.95), max(1, reps // 2))
            r = {"config": f"value_{name}", "lanes": eng.n, "steps": T, "valued_launch_sec": sec_v,
                 "sampled_log_prob_launch_sec": sec_s, "valued_over_sampled": sec_v / sec_s,
                 "sampled_launch_plus_torch_critic_sec": sec_p, "valued_speedup_over_parent_way": sec_p / sec_v,
                 "gae_sec": sec_g, "gae_bytes_per_s": 26.0 * eng.n * T / sec_g, "torch_reverse_loop_sec": sec_t,
                 "gae_speedup_over_torch_loop": sec_t / sec_g, "reps_sec": {"valued": ts_v, "parent": ts_p, "gae": ts_g,
                                                                             "torch_gae": ts_t}}
            rows.append(r)
            print(json.dumps(r), flush=True)
    return rows


def host_generation(eng, tmpl, center, P, L, sigma, lr, rng, K, max_steps):
    """one ES generation the way a caller writes it without carl_amd.es: everything around the launch on the host"""
    N, n = tmpl.weight_floats, tmpl.n_in
    z = rng.standard_normal((P // 2, N)).astype(np.float32)
    sets = []
    for i in range(P // 2):
        for sign in (1.0, -1.0):
            flat = center.copy()
            flat[:N] += np.float32(sign * sigma) * z[i]
            layers, off = [], 0
            for W, b in tmpl.layers:
                layers.append((flat[off: off + W.size].reshape(W.shape), flat[off + W.size: off + W.size + b.size]))
                off += W.size + b.size
            sets.append(MLPPolicy.for_env(eng, layers, tmpl.activation, flat[off: off + n], flat[off + n: off + 2 * n],
                                          float(flat[off + 2 * n])))
    pop = MLPPolicy.stack(sets, L)
    eng.reset()
    res = eng.evaluate_policy(pop, K, max_steps)
    ret, ep = res["return"].cpu().numpy(), res["episodes"].cpu().numpy()
    valid = np.arange(K)[:, None] < ep[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        lane = np.where(valid, ret, 0).sum(0) / ep
        has = (ep > 0).reshape(P, L)
        fit = np.where(has, lane.reshape(P, L), 0).sum(1) / has.sum(1)
    fit = np.where(has.any(1), fit, -np.inf).astype(np.float32)
    rank = np.empty(P, np.int64)
    rank[np.argsort(fit, kind="stable")] = np.arange(P)
    u = rank.astype(np.float32) / np.float32(P - 1) - np.float32(0.5)
    grad = (u[0::2] - u[1::2]) @ z
    center[:N] += np.float32(lr / (P * sigma)) * grad
    return center


def es_leg(eng, n_in, reps, L=256, K=1, max_steps=500, sigma=0.1, lr=0.05):
    import ctypes as C
    import time

    from carl_amd.es import EvolutionStrategy

    def clock(fn):
        fn()  # warm-up
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), ts

    rows, P = [], eng.n // L
    for name, widths in {"linear": [], "mlp_2x64_tanh": [64, 64]}.items():
        tmpl = MLPPolicy.from_sequential(eng, make_mlp(widths, n_in))
        es = EvolutionStrategy(eng, tmpl, lanes_per_set=L, sigma=sigma, lr=lr, seed=0)
        sec_a, ts_a = clock(lambda: es.step(n_episodes=K, max_steps=max_steps))
        res = eng.alloc_policy_episodes(K)
        eng.reset()
        sec_e, _ = time_launches(lambda: eng.evaluate_policy(es.population, K, max_steps, out=res), reps)
        state = {"center": tmpl.params[0].copy(), "rng": np.random.default_rng(0)}

        def host_way():
            state["center"] = host_generation(eng, tmpl, state["center"], P, L, sigma, lr, state["rng"], K, max_steps)

        sec_b, ts_b = clock(host_way)
        st = es.struct()
        stream = torch.cuda.current_stream(eng.device).cuda_stream
        weight = torch.randn(P // 2, device=eng.device)
        grad = torch.empty(es.n_noisy, device=eng.device)
        many = 50
        sec_p, _ = time_launches(lambda: [_lib.check(eng.lib.carl_es_perturb(C.byref(st), es.center.data_ptr(),
                                                                             es.population.params.data_ptr(), None, stream))
                                          for _ in range(many)], reps)
        sec_g, _ = time_launches(lambda: [_lib.check(eng.lib.carl_es_gradient(C.byref(st), weight.data_ptr(),
                                                                              grad.data_ptr(), stream))
                                          for _ in range(many)], reps)
        r = {"config": f"es_{name}", "lanes": eng.n, "sets": P, "lanes_per_set": L, "n_episodes": K, "max_steps": max_steps,
             "set_floats": es.set_floats, "n_noisy": es.n_noisy, "es_step_sec": sec_a, "host_generation_sec": sec_b,
             "host_over_es_step": sec_b / sec_a, "evaluate_policy_launch_sec": sec_e,
             "perturb_sec_per_launch_back_to_back": sec_p / many, "gradient_sec_per_launch_back_to_back": sec_g / many,
             "perturb_bytes": 4 * es.set_floats * (P + 1), "reps_sec": {"es_step": ts_a, "host_generation": ts_b}}
        rows.append(r)
        print(json.dumps(r), flush=True)
    return rows


def stats_leg(eng, n_in, reps, K=1, max_steps=500):
    from carl_amd.policy import InputStats

    rows = []
    snap = eng.snapshot()
    for name, widths in {"linear": [], "mlp_2x64_tanh": [64, 64]}.items():
        tmpl = MLPPolicy.from_sequential(eng, make_mlp(widths, n_in))
        block = torch.as_tensor(tmpl.params).to(eng.device).contiguous().clone()
        pol = MLPPolicy.on_device(tmpl, block, (eng.n + 255) // 256 * 256)
        res = eng.alloc_policy_episodes(K)
        sec = {}
        for key, kw in (("plain", {}), ("stats", {"input_stats": True})):
            ts = []
            for _ in range(reps + 1):  # (the first: warm-up)
                eng.restore(snap)
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                eng.evaluate_policy(pol, K, max_steps, out=res, **kw)
                b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b) * 1e-3)
            sec[key] = (float(np.median(ts[1:])), ts[1:])
        lane_steps = int(res["steps"].to(torch.int64).sum())
        stats = InputStats(tmpl, eng.device)
        many = 50
        sec_m, _ = time_launches(lambda: [stats.update(res, pol, n_write=1) for _ in range(many)], reps)
        r = {"config": f"stats_{name}", "lanes": eng.n, "n_episodes": K, "max_steps": max_steps, "lane_steps": lane_steps,
             "evaluate_policy_sec": sec["plain"][0], "evaluate_policy_stats_sec": sec["stats"][0],
             "stats_over_plain": sec["stats"][0] / sec["plain"][0], "merge_sec_per_launch_back_to_back": sec_m / many,
             "workgroups": int(res["input_partial"].shape[0]),
             "reps_sec": {"plain": sec["plain"][1], "stats": sec["stats"][1]}}
        rows.append(r)
        print(json.dumps(r), flush=True)
    eng.restore(snap)
    return rows


def brax_bench_engine(cls, n, time_limit):
    """the Brax legs' engine: the model's default context, static selector, no context inputs"""
    from carl_amd.brax_engine import BraxVecEngine
    from carl_amd.envs.brax.models import SYSTEMS

    feats = cls.get_context_features()
    names = list(feats)
    row = np.array([[float(f.default_value) for f in feats.values()]])
    eng = BraxVecEngine(SYSTEMS[cls.env_name](names), len(names), row, n, "cuda", selector=_lib.SEL_STATIC, seed=0,
                        ctx_obs_rows=[], max_episode_steps=time_limit)
    eng.reset()
    return eng


def brax_bench_policy(eng, seed=0):
    """the Brax legs' policy: 2 x 64 tanh"""
    from carl_amd.brax_policy import BraxMLPPolicy

    rng = np.random.default_rng(seed)
    dims = [eng.D, 64, 64, eng.sys.n_act]
    layers = [((rng.normal(size=(o, i)) / np.sqrt(i)).astype(np.float32), np.zeros(o, np.float32))
              for i, o in zip(dims[:-1], dims[1:])]
    return BraxMLPPolicy.for_env(eng, layers, "tanh")


def timed_from_snapshot(eng, snap, fn, reps):
    """device events around fn(), the state restored before each launch: (median of `reps` after a warm-up, the reps)"""
    ts = []
    for _ in range(reps + 1):  # (the first: warm-up)
        eng.restore(snap)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts[1:])), ts[1:]


def brax_es_leg(reps, n=32768, L=256, long_steps=1000):
    import time

    from carl_amd import envs as E
    from carl_amd.es import EvolutionStrategy

    def engine(cls, time_limit):
        return brax_bench_engine(cls, n, time_limit)

    policy = brax_bench_policy

    def launched_width(eng, pol):
        """lanes per env of the launch (carl_brax_policy_launch_shape answers for both closed-loop entry points)"""
        import ctypes as C

        shape = _lib.BraxLaunchShape()
        st = pol.struct(eng.n, pol.device_params(eng.device).data_ptr())
        _lib.check(eng.lib.carl_brax_policy_launch_shape(C.byref(eng.b), C.byref(eng.sys), C.byref(st), long_steps,
                                                         C.byref(shape)))
        return int(shape.lanes_per_env)

    def timed(eng, snap, fn):
        return timed_from_snapshot(eng, snap, fn, reps)

    rows = []
    for model, cls in (("ant", E.CARLBraxAnt), ("hopper", E.CARLBraxHopper)):
        for S in (long_steps, 100):
            eng = engine(cls, S)
            pol = policy(eng)
            snap = eng.snapshot()
            res, summ = eng.alloc_policy_episodes(1), eng.alloc_policy_summary()
            sec_e, ts_e = timed(eng, snap, lambda: eng.evaluate_episodes(pol, 1, long_steps, out=res))
            steps = res["steps"].to(torch.int64)
            assert int(steps.max()) <= S and int(res["episodes"].min()) == 1
            sec_s, ts_s = timed(eng, snap, lambda: eng.rollout_policy(pol, S, out=summ, mode="summary"))
            sec_l, ts_l = (sec_s, ts_s) if S == long_steps else timed(
                eng, snap, lambda: eng.rollout_policy(pol, long_steps, out=summ, mode="summary"))
            r = {"config": f"brax_episodes_{model}_timelimit_{S}", "envs": n, "n_episodes": 1, "max_steps": long_steps,
                 "time_limit": S, "lanes_per_env": launched_width(eng, pol), "env_steps_taken": int(steps.sum()),
                 "longest_env_steps": int(steps.max()), "mean_env_steps": float(steps.double().mean()),
                 "evaluate_episodes_sec": sec_e, f"summary_{S}_steps_sec": sec_s, f"summary_{long_steps}_steps_sec": sec_l,
                 "episodes_over_summary_S_steps": sec_e / sec_s, "episodes_over_summary_1000_steps": sec_e / sec_l,
                 "reps_sec": {"evaluate_episodes": ts_e, "summary_S": ts_s, "summary_long": ts_l}}
            rows.append(r)
            print(json.dumps(r), flush=True)
    eng = engine(E.CARLBraxAnt, 100)
    es = EvolutionStrategy(eng, policy(eng), lanes_per_set=L, sigma=0.1, lr=0.05, seed=0)
    ts = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        es.step(n_episodes=1, max_steps=long_steps)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    eng.reset()
    snap = eng.snapshot()
    res = eng.alloc_policy_episodes(1)
    sec_e, ts_e = timed(eng, snap, lambda: eng.evaluate_episodes(es.population, 1, long_steps, out=res))
    r = {"config": "brax_es_ant_2x64_tanh", "envs": n, "sets": es.n_sets, "lanes_per_set": L, "n_episodes": 1,
         "max_steps": long_steps, "time_limit": 100, "set_floats": es.set_floats, "n_noisy": es.n_noisy,
         "es_step_sec": float(np.median(ts[1:])), "evaluate_episodes_launch_sec": sec_e,
         "reps_sec": {"es_step": ts[1:], "evaluate_episodes": ts_e}}
    rows.append(r)
    print(json.dumps(r), flush=True)
    return rows


def brax_stats_leg(reps, n=32768, L=256, max_steps=1000, time_limit=100):
    """the statistics launch against the episodes launch, and a normalised ES generation (merge included) against an
    unnormalised one: brax_es_leg's set-up (Ant, 2 x 64 tanh, K = 1), every launch from the same state"""
    import time

    from carl_amd import envs as E
    from carl_amd.es import EvolutionStrategy
    from carl_amd.policy import InputStats

    eng = brax_bench_engine(E.CARLBraxAnt, n, time_limit)
    pol = brax_bench_policy(eng)
    snap = eng.snapshot()
    plain, with_stats = eng.alloc_policy_episodes(1), eng.alloc_policy_episodes(1)
    eng.evaluate_episodes(pol, 1, max_steps, out=with_stats, input_stats=True)  # (allocates the slabs once)
    # interleaved A, B, A, B: a drift of the clock over the run lands on both sides
    ts_p, ts_s = [], []
    for _ in range(2):
        ts_p += timed_from_snapshot(eng, snap, lambda: eng.evaluate_episodes(pol, 1, max_steps, out=plain), reps)[1]
        ts_s += timed_from_snapshot(
            eng, snap, lambda: eng.evaluate_episodes(pol, 1, max_steps, out=with_stats, input_stats=True), reps)[1]
    sec_p, sec_s = float(np.median(ts_p)), float(np.median(ts_s))
    assert torch.equal(plain["steps"], with_stats["steps"])

    def generation(es):
        ts = []
        for _ in range(reps + 1):  # (the first: warm-up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            es.step(n_episodes=1, max_steps=max_steps)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts[1:])), ts[1:]

    tmpl = brax_bench_policy(eng)
    gen_p, tg_p = generation(EvolutionStrategy(eng, tmpl, lanes_per_set=L, sigma=0.1, lr=0.05, seed=0))
    gen_s, tg_s = generation(EvolutionStrategy(eng, tmpl, lanes_per_set=L, sigma=0.1, lr=0.05, seed=0,
                                               input_stats=InputStats(tmpl, eng.device)))
    r = {"config": "brax_stats_ant_2x64_tanh", "envs": n, "lanes_per_set": L, "n_episodes": 1, "max_steps": max_steps,
         "time_limit": time_limit, "slabs": int(with_stats["input_partial"].shape[0]),
         "env_steps_taken": int(plain["steps"].to(torch.int64).sum()),
         "evaluate_episodes_sec": sec_p, "evaluate_episodes_input_stats_sec": sec_s, "input_stats_over_plain": sec_s / sec_p,
         "es_step_sec": gen_p, "es_step_normalised_sec": gen_s, "normalised_over_plain": gen_s / gen_p,
         "reps_sec": {"evaluate_episodes": ts_p, "evaluate_episodes_input_stats": ts_s, "es_step": tg_p,
                      "es_step_normalised": tg_s}}
    print(json.dumps(r), flush=True)
    return [r]


def brax_sample_leg(reps, n=32768, steps=100, time_limit=1000):
    """the sampled transitions launch, with and without log_prob, against the deterministic one: Ant and Halfcheetah"""
    from carl_amd import envs as E

    rows = []
    for model, cls in (("ant", E.CARLBraxAnt), ("halfcheetah", E.CARLBraxHalfcheetah)):
        eng = brax_bench_engine(cls, n, time_limit)
        pol = brax_bench_policy(eng)
        snap = eng.snapshot()
        out = eng.alloc_rollout(steps, action=True)
        out_lp = dict(out, log_prob=torch.empty((steps, n), dtype=torch.float32, device=eng.device))
        kw = dict(deterministic=False, sample_seed=1)
        sides = {"deterministic": lambda: eng.rollout_policy(pol, steps, out=out),
                 "sampled": lambda: eng.rollout_policy(pol, steps, out=out, **kw),
                 "sampled_log_prob": lambda: eng.rollout_policy(pol, steps, out=out_lp, log_prob=True, **kw)}
        ts = {k: [] for k in sides}
        for _ in range(2):  # interleaved A, B, C, A, B, C: a drift of the clock over the run lands on every side
            for k, fn in sides.items():
                ts[k] += timed_from_snapshot(eng, snap, fn, reps)[1]
        sec = {k: float(np.median(v)) for k, v in ts.items()}
        det = ts["deterministic"]
        r = {"config": f"brax_sample_{model}_2x64_tanh", "envs": n, "steps": steps, "time_limit": time_limit,
             "deterministic_sec": sec["deterministic"], "sampled_sec": sec["sampled"],
             "sampled_log_prob_sec": sec["sampled_log_prob"],
             "sampled_over_deterministic": sec["sampled"] / sec["deterministic"],
             "sampled_log_prob_over_deterministic": sec["sampled_log_prob"] / sec["deterministic"],
             "deterministic_spread": (max(det) - min(det)) / sec["deterministic"],
             "env_steps_per_s": {k: n * steps / v for k, v in sec.items()}, "reps_sec": ts}
        rows.append(r)
        print(json.dumps(r), flush=True)
    return rows


def brax_value_leg(reps, n=32768, steps=100, time_limit=1000):
    """the valued launch against the sampled one, and against the sampled one followed by a torch critic: Ant and
    Halfcheetah"""
    from carl_amd import envs as E
    from carl_amd.brax_policy import BraxMLPPolicy

    rows = []
    for model, cls in (("ant", E.CARLBraxAnt), ("halfcheetah", E.CARLBraxHalfcheetah)):
        eng = brax_bench_engine(cls, n, time_limit)
        pol = brax_bench_policy(eng)
        rng = np.random.default_rng(1)
        dims = [eng.D, 64, 64, 1]
        layers = [((rng.normal(size=(o, i)) / np.sqrt(i)).astype(np.float32), np.zeros(o, np.float32))
                  for i, o in zip(dims[:-1], dims[1:])]
        crit = BraxMLPPolicy.for_env(eng, layers, "tanh", head="value")
        net = torch.nn.Sequential(torch.nn.Linear(eng.D, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(),
                                  torch.nn.Linear(64, 1)).to(eng.device)
        with torch.no_grad():
            for lin, (W, b) in zip([m for m in net if isinstance(m, torch.nn.Linear)], layers):
                lin.weight.copy_(torch.as_tensor(W))
                lin.bias.copy_(torch.as_tensor(b))
        snap = eng.snapshot()
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=eng.device)  # noqa: E731
        out_a = dict(eng.alloc_rollout(steps, action=True), log_prob=f32(steps, n))
        out_b = dict(eng.alloc_rollout(steps, action=True), log_prob=f32(steps, n), value=f32(steps, n),
                     boot_value=f32(steps, n), last_value=f32(n), advantage=f32(steps, n))
        out_b["return"] = f32(steps, n)
        out_c = dict(eng.alloc_rollout(steps, final_obs=True, action=True), log_prob=f32(steps, n))
        gae_c = {"advantage": f32(steps, n), "return": f32(steps, n)}
        kw = dict(deterministic=False, sample_seed=1)

        def torch_route(gae):
            obs0 = eng.obs.clone()
            o = eng.rollout_policy(pol, steps, out=out_c, log_prob=True, **kw)
            with torch.no_grad():
                before = torch.cat([obs0[None], o["obs"][:-1]])
                value = net(before.reshape(steps * n, -1)).reshape(steps, n)
                last = net(o["obs"][-1]).reshape(n)
                cut = o["truncated"].bool() & ~o["terminated"].bool()
                boot = torch.where(cut, net(torch.nan_to_num(o["final_obs"]).reshape(steps * n, -1)).reshape(steps, n),
                                   torch.zeros((), device=eng.device))
            if gae:
                eng.gae(o["reward"], value, o["terminated"], o["truncated"], last, 0.99, 0.95, boot_value=boot, out=gae_c)

        sides = {"sampled_log_prob": lambda: eng.rollout_policy(pol, steps, out=out_a, log_prob=True, **kw),
                 "valued": lambda: eng.rollout_policy(pol, steps, out=out_b, value_net=crit, **kw),
                 "sampled_then_torch_critic": lambda: torch_route(False),
                 "valued_gae": lambda: eng.rollout_policy(pol, steps, out=out_b, value_net=crit, gae=(0.99, 0.95), **kw),
                 "sampled_then_torch_critic_gae": lambda: torch_route(True)}
        ts = {k: [] for k in sides}
        for _ in range(2):  # interleaved: a drift of the clock over the run lands on every side
            for k, fn in sides.items():
                ts[k] += timed_from_snapshot(eng, snap, fn, reps)[1]
        sec = {k: float(np.median(v)) for k, v in ts.items()}
        r = {"config": f"brax_value_{model}_2x64_tanh", "envs": n, "steps": steps, "time_limit": time_limit,
             "median_sec": sec, "range_sec": {k: [min(v), max(v)] for k, v in ts.items()},
             "valued_over_sampled": sec["valued"] / sec["sampled_log_prob"],
             "valued_over_torch_route": sec["valued"] / sec["sampled_then_torch_critic"],
             "valued_gae_over_torch_route_gae": sec["valued_gae"] / sec["sampled_then_torch_critic_gae"],
             "env_steps_per_s": {k: n * steps / v for k, v in sec.items()}, "reps_sec": ts}
        rows.append(r)
        print(json.dumps(r), flush=True)
    return rows


BRAX_LEGS = (("brax_es", brax_es_leg), ("brax_stats", brax_stats_leg), ("brax_sample", brax_sample_leg),
             ("brax_value", brax_value_leg))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--legs", default="rollout,evaluate")
    ap.add_argument("--out", default=None)
    ap.add_argument("--sampled", action="store_true")
    args = ap.parse_args()
    legs = set(args.legs.split(","))
    if legs <= {k for k, _ in BRAX_LEGS}:  # (their own engines: the CartPole engine below is not built)
        return write(args.out, {k: leg(args.reps) for k, leg in BRAX_LEGS if k in legs})
    n, T = args.lanes, args.steps
    eng = make_engine(n)
    n_in = len(eng.ctx_obs_rows) + eng.D
    rows = []
    doc = {}
    if "evaluate" in legs:
        doc["evaluate"] = evaluate_leg(eng, n_in, T, args.reps)
    if "value" in legs:
        doc["value"] = value_leg(eng, n_in, T, args.reps)
    if "es" in legs:
        doc["es"] = es_leg(eng, n_in, args.reps)
    if "stats" in legs:
        doc["stats"] = stats_leg(eng, n_in, args.reps)
    if "brax_es" in legs:
        doc["brax_es"] = brax_es_leg(args.reps)
    if "brax_stats" in legs:
        doc["brax_stats"] = brax_stats_leg(args.reps)
    if "brax_sample" in legs:
        doc["brax_sample"] = brax_sample_leg(args.reps)
    if "brax_value" in legs:
        doc["brax_value"] = brax_value_leg(args.reps)
    if "rollout" not in legs:
        return write(args.out, doc)

    def record(name, sec, ts):
        r = {"config": name, "lanes": n, "steps": T, "sec_per_launch": sec, "env_steps_per_s": n * T / sec,
             "ns_per_step": sec / T * 1e9, "reps_sec": ts}
        rows.append(r)
        print(json.dumps(r), flush=True)

    acts = torch.randint(0, 2, (T, n), dtype=torch.int32, device=eng.device)
    out = eng.alloc_rollout(T)
    record("open_loop_rollout_int32", *time_launches(lambda: eng.rollout(acts, out=out), args.reps))

    policies = {"linear": [], "mlp_2x32_tanh": [32, 32], "mlp_2x64_tanh": [64, 64]}
    for name, widths in policies.items():
        mlp = make_mlp(widths, n_in)
        pol = MLPPolicy.from_sequential(eng, mlp)
        pout = eng.rollout_policy(pol, T)  # buffers reused by every timed launch
        record(f"policy_transitions_{name}", *time_launches(lambda: eng.rollout_policy(pol, T, out=pout), args.reps))
        s = eng.alloc_policy_summary()
        record(f"policy_summary_{name}", *time_launches(lambda: eng.rollout_policy(pol, T, out=s, mode="summary"),
                                                       args.reps))
        if args.sampled:
            kw = dict(deterministic=False, sample_seed=1)
            sout = eng.rollout_policy(pol, T, log_prob=True, **kw)
            record(f"sampled_transitions_{name}", *time_launches(lambda: eng.rollout_policy(
                pol, T, out={k: v for k, v in sout.items() if k != "log_prob"}, **kw), args.reps))
            record(f"sampled_transitions_log_prob_{name}", *time_launches(lambda: eng.rollout_policy(
                pol, T, out=sout, log_prob=True, **kw), args.reps))
            record(f"sampled_summary_{name}", *time_launches(lambda: eng.rollout_policy(pol, T, out=s, mode="summary",
                                                                                        **kw), args.reps))
        with torch.no_grad():
            run = graph_step_mlp(eng, mlp.to(eng.device), T)
            record(f"graph_step_torch_{name}", *time_launches(run, max(1, args.reps // 2)))
    doc["results"] = rows
    write(args.out, doc)


def write(path, doc):
    if not path:
        return
    old = {}
    if os.path.exists(path):
        with open(path) as f:
            old = json.load(f)
    old.update(device=torch.cuda.get_device_name(0), **doc)
    with open(path, "w") as f:
        json.dump(old, f, indent=1)


if __name__ == "__main__":
    main()
