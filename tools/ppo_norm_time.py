"""Measurements of PPO's running normalisation on the device.

    python tools/ppo_norm_time.py [--out profiles/ppo_norm_time.json] [--steps NAME,NAME,...] [--parent-tree DIR]

runs its steps, each in a child process of its own under its own time limit, and stops at the first one that fails:

  launch_cartpole    65 536 lanes x 128 steps of CartPole (every context input): the input-sums launch, and the return walk
                     plus its merge, against the same quantities by torch ops on the same buffers in the same process (the
                     gather of the inputs, then mean / var; the T-step return recurrence, then mean / var).  Device events,
                     the paths alternating; medians and ranges.  The input sums also as bytes read over time.
  launch_ant         the same for Brax Ant, 32 768 envs x 8 steps, two context inputs
  iteration_cartpole PPO.learn iterations with the flags off, on, off, on, ... in one process (tools/ppo_update_time.py's
                     shape): the off path's rounds give its own round-to-round range
  iteration_ant      the same at tools/brax_ppo_update_time.py's shape
  beside_cartpole    with --parent-tree DIR (a built checkout of the parent commit): PPO.learn iterations with the flags off
  beside_ant         in child processes that import carl_amd from DIR and from this tree in turn, three processes each,
                     at the two shapes above: the parent's round-to-round range beside the off path's
  learn_pendulum     tools/ppo_update_time.py's Pendulum run, without and with normalisation
  learn_halfcheetah  tools/brax_ppo_update_time.py's Halfcheetah run, without and with normalisation

`--step NAME` runs one step in this process and prints its JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("CARL_PPO_NORM_TREE") or HERE  # the tree carl_amd, tests/ and tools/ are imported from (the off-path steps)
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

LIMITS = {"launch_cartpole": 300, "launch_ant": 300, "iteration_cartpole": 420, "iteration_ant": 300,
          "beside_cartpole": 600, "beside_ant": 300, "offpath_cartpole": 120, "offpath_ant": 120,
          "learn_pendulum": 420, "learn_halfcheetah": 420}  # seconds per step
ORDER = ["launch_cartpole", "launch_ant", "iteration_cartpole", "iteration_ant", "learn_pendulum", "learn_halfcheetah"]
NORM = dict(normalize_inputs=True, normalize_reward=True)


def _stat(v):
    return {"median_ms": statistics.median(v), "min_max_ms": [min(v), max(v)]}


def _launch(eng, actor, critic, T, label):
    import torch

    import ppo_update_time as PU
    from carl_amd import PPO

    N = eng.n
    ppo = PPO(eng, actor, critic, n_steps=T, n_epochs=1, batch_size=N * T)
    buf = ppo.collect()
    cid, obs0, obs = buf["context_id"], buf["obs0"], buf["obs"]
    dense = T == 1 or int(cid.stride(0)) == N
    assert dense, "the timing run uses dense rows"
    pol = ppo._actor
    out = {}
    rows = torch.as_tensor(actor.ctx_rows, device=eng.device, dtype=torch.long)
    shift = torch.as_tensor(actor.shift, device=eng.device)

    def kernel_inputs():
        eng.ppo_input_stats(pol, buf, obs0, cid, out=out)

    def torch_inputs():
        o = torch.cat([obs0[None], obs[: T - 1]], dim=0).reshape(T * N, -1)
        x = torch.cat([eng.ctx_table[rows][:, cid.reshape(-1).long()].t(), o], dim=1) if len(actor.ctx_rows) else o
        d = (x - shift).double()
        return d.mean(dim=0), d.var(dim=0, unbiased=False)

    rew, te, tr = buf["reward"][:T], buf["terminated"][:T], buf["truncated"][:T]
    ret = torch.zeros(N, device=eng.device)
    run = {"count": torch.zeros(1, dtype=torch.int64, device=eng.device),
           "mean": torch.zeros(1, dtype=torch.float64, device=eng.device),
           "m2": torch.zeros(1, dtype=torch.float64, device=eng.device)}
    scale = torch.ones(1, device=eng.device)
    rout = {}

    def kernel_returns():
        eng.ppo_return_stats(rew, te, tr, ret, 0.99, out=rout)
        eng.ppo_return_merge(rout["return_partial"], T * N, run, 1e-8, scale)

    tret = torch.zeros(N, device=eng.device)
    done = (te | tr).bool()

    def torch_returns():
        nonlocal tret
        rows_ = []
        r = tret
        for t in range(T):
            r = r * 0.99 + rew[t]
            rows_.append(r)
            r = torch.where(done[t], torch.zeros_like(r), r)
        tret = r
        a = torch.stack(rows_).double()
        return a.mean(), a.var(unbiased=False)

    # the two input paths agree (the device's sums against torch's float64 mean of the same d)
    kernel_inputs()
    m, _ = torch_inputs()
    S1 = out["input_partial"][:, 0, : actor.n_in].sum(dim=0) / (T * N)
    agree = float((S1 - m).abs().max() / (m.abs().max() + 1e-30))
    for _ in range(3):
        kernel_inputs(), torch_inputs(), kernel_returns(), torch_returns()
    ki, ti, kr, trn = [], [], [], []
    for _ in range(15):  # alternating
        ki.append(PU._timed(kernel_inputs, 10))
        ti.append(PU._timed(torch_inputs, 10))
        kr.append(PU._timed(kernel_returns, 10))
        trn.append(PU._timed(torch_returns, 10))
    read = 4 * N * eng.D * T + 4 * N * T * (1 if actor.ctx_rows else 0)  # observation rows (obs0 + T - 1 rows) and id rows
    med = statistics.median(ki)
    return {"step": label, "lanes": N, "steps": T, "n_in": actor.n_in, "n_ctx": len(actor.ctx_rows),
            "slabs": int(out["input_partial"].shape[0]), "mean_d_max_relative_difference_to_torch": agree,
            "input_sums": _stat(ki), "input_sums_torch_gather_mean_var": _stat(ti),
            "input_sums_bytes_read": read, "input_sums_GB_per_s": read / med / 1e6,
            "return_walk_and_merge": _stat(kr), "return_walk_torch_recurrence_mean_var": _stat(trn)}


def step_launch_cartpole():
    import ppo_update_time as PU
    from carl_amd import _lib

    return _launch(*PU._setup(_lib.CARTPOLE, 65536), 128, "launch_cartpole")


def step_launch_ant():
    import brax_ppo_update_time as BU

    return _launch(*BU._setup("ant", 32768), 8, "launch_ant")


def _iteration(make, T, label, **kw):
    import torch

    import ppo_update_time as PU
    from carl_amd import PPO

    runs = {}
    for name, flags in (("off", {}), ("on", NORM)):
        eng, actor, critic = make()
        runs[name] = PPO(eng, actor, critic, n_steps=T, **kw, **flags)
        runs[name].learn(2)  # warm-up: uploads, code objects, Adam's state
    torch.cuda.synchronize()
    ms = {"off": [], "on": []}
    for _ in range(6):  # alternating rounds
        for name in ("off", "on"):
            ms[name].append(PU._timed(lambda: runs[name].learn(1), 2))
    return {"step": label, "lanes": runs["off"].engine.n, "steps": T, "settings": kw, "iteration_flags_off": _stat(ms["off"]),
            "iteration_flags_off_rounds_ms": ms["off"], "iteration_flags_on": _stat(ms["on"]), "iteration_flags_on_rounds_ms": ms["on"]}


def step_iteration_cartpole():
    import ppo_update_time as PU
    from carl_amd import _lib

    return _iteration(lambda: PU._setup(_lib.CARTPOLE, 65536), 128, "iteration_cartpole", n_epochs=1, batch_size=65536,
                      ent_coef=0.01)


def step_iteration_ant():
    import brax_ppo_update_time as BU

    return _iteration(lambda: BU._setup("ant", 32768), 8, "iteration_ant", n_epochs=1, batch_size=65536, ent_coef=0.01)


def _offpath(make, T, label, **kw):
    """flags off, through the arguments the parent commit's PPO has: runs in either tree"""
    import torch

    import ppo_update_time as PU
    from carl_amd import PPO

    ppo = PPO(*make(), n_steps=T, **kw)
    ppo.learn(2)
    torch.cuda.synchronize()
    ms = [PU._timed(lambda: ppo.learn(1), 2) for _ in range(6)]
    return {"step": label, "tree": ROOT, "rounds_ms": ms}


def step_offpath_cartpole():
    import ppo_update_time as PU
    from carl_amd import _lib

    return _offpath(lambda: PU._setup(_lib.CARTPOLE, 65536), 128, "offpath_cartpole", n_epochs=1, batch_size=65536, ent_coef=0.01)


def step_offpath_ant():
    import brax_ppo_update_time as BU

    return _offpath(lambda: BU._setup("ant", 32768), 8, "offpath_ant", n_epochs=1, batch_size=65536, ent_coef=0.01)


def _beside(which, parent_tree):
    """three processes per tree, alternating: the parent's, this tree's with the flags off"""
    rounds = {"parent": [], "this": []}
    for _ in range(3):
        for name, tree in (("parent", parent_tree), ("this", HERE)):
            env = dict(os.environ, CARL_PPO_NORM_TREE=os.path.abspath(tree), CARL_AMD_NO_BUILD="1")
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "offpath_" + which], capture_output=True,
                               text=True, timeout=LIMITS["offpath_" + which], env=env, check=True)
            rounds[name].append(json.loads(p.stdout.strip().splitlines()[-1])["rounds_ms"])
    flat = {k: [x for r in v for x in r] for k, v in rounds.items()}
    return {"step": "beside_" + which, "processes_per_tree": 3, "rounds_per_process": 6,
            "parent_commit_iteration": _stat(flat["parent"]), "parent_commit_process_medians_ms": [statistics.median(r) for r in rounds["parent"]],
            "flags_off_iteration": _stat(flat["this"]), "flags_off_process_medians_ms": [statistics.median(r) for r in rounds["this"]]}


def step_beside_cartpole():
    return _beside("cartpole", os.environ["CARL_PPO_NORM_PARENT"])


def step_beside_ant():
    return _beside("ant", os.environ["CARL_PPO_NORM_PARENT"])


def step_learn_pendulum():
    import ppo_update_time as PU
    from carl_amd import _lib

    kw = dict(n_epochs=6, batch_size=32768, lr=1e-3, gamma=0.9, ent_coef=0.0)  # (tools/ppo_update_time.py: learn_pendulum)
    off = PU._learn(_lib.PENDULUM, "learn_pendulum", 4096, 200, 30, **kw)
    on = PU._learn(_lib.PENDULUM, "learn_pendulum", 4096, 200, 30, **kw, **NORM)
    return {**off, "mean_last_episode_return_normalized": on["mean_last_episode_return"]}


def step_learn_halfcheetah():
    import brax_ppo_update_time as BU

    kw = dict(n_epochs=4, batch_size=16384, lr=3e-4, ent_coef=0.0)  # (tools/brax_ppo_update_time.py: learn_halfcheetah)
    off = BU._learn("halfcheetah", "learn_halfcheetah", 2048, 32, 20, max_episode_steps=100, **kw)
    on = BU._learn("halfcheetah", "learn_halfcheetah", 2048, 32, 20, max_episode_steps=100, **kw, **NORM)
    return {**off, "mean_last_episode_return_normalized": on["mean_last_episode_return"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(LIMITS))
    ap.add_argument("--steps", help="comma-separated subset, in the given order (default: all)")
    ap.add_argument("--out")
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit, for the beside_* steps")
    args = ap.parse_args()
    if args.parent_tree:
        os.environ["CARL_PPO_NORM_PARENT"] = os.path.abspath(args.parent_tree)
    if args.step:
        print(json.dumps(globals()["step_" + args.step]()), flush=True)
        return 0
    results = []
    if args.out and os.path.exists(args.out):  # a run of some steps keeps the other steps' earlier results
        with open(args.out) as f:
            results = json.load(f)
    for name in (args.steps.split(",") if args.steps else ORDER):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True,
                               timeout=LIMITS[name])
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {LIMITS[name]} s -- stopping", flush=True)
            return 1
        if p.returncode != 0:
            print(f"{name}: exit status {p.returncode} -- stopping\n{p.stderr[-2000:]}", flush=True)
            return 1
        res = json.loads(p.stdout.strip().splitlines()[-1])
        results = [r for r in results if r["step"] != name] + [res]
        print(json.dumps(res), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(results, f, indent=1)
                f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
