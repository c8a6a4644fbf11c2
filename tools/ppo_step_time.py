"""Measurements of PPO's fused minibatch step on the device.

    python tools/ppo_step_time.py [--out profiles/ppo_step_time.json] [--steps NAME,NAME,...] [--parent-tree DIR]

runs its steps, each in a child process of its own under its own time limit, and stops at the first one that fails:

  epoch_cartpole        one epoch of PPO.update() on CartPole, 65 536 lanes x 128 steps, minibatches of 65 536 (128 of
                        them), with fused_step off and on: two PPO objects on engines of their own alternate in one
                        process, device events after warm-up, medians with min-max over 15 repetitions.  At this shape
                        also each launch alone: the epoch's advantage statistics against the torch gather / mean / std of
                        its 128 minibatches, the clip + Adam launch against the torch clip and torch.optim.Adam, and
                        ppo_grad's three launches.
  epoch_cartpole_small  the same epoch at 4 096 lanes x 64 steps, minibatches of 16 384 (16 of them)
  epoch_ant             the same epoch for Brax Ant, 32 768 envs x 8 steps, minibatches of 65 536 (4 of them)
  beside_cartpole       with --parent-tree DIR (a built checkout of the parent commit): the epoch with fused_step off in
  beside_cartpole_small child processes that import carl_amd from DIR and from this tree in turn, three processes each:
  beside_ant            the parent's round-to-round range beside the off path's

`--step NAME` runs one step in this process and prints its JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("CARL_PPO_STEP_TREE") or HERE  # the tree carl_amd, tests/ and tools/ are imported from (the off-path steps)
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

SHAPES = {"cartpole": (65536, 128, 65536), "cartpole_small": (4096, 64, 16384), "ant": (32768, 8, 65536)}  # lanes, steps, minibatch
LIMITS = {"epoch_cartpole": 420, "epoch_cartpole_small": 240, "epoch_ant": 300, "beside_cartpole": 900,
          "beside_cartpole_small": 600, "beside_ant": 600, "offpath_cartpole": 240, "offpath_cartpole_small": 180,
          "offpath_ant": 180}  # seconds per step
ORDER = ["epoch_cartpole", "epoch_cartpole_small", "epoch_ant"]
REPS = 15


def _stat(v):
    return {"median_ms": statistics.median(v), "min_max_ms": [min(v), max(v)]}


def _make(which):
    if which == "ant":
        import brax_ppo_update_time as BU

        return BU._setup("ant", SHAPES[which][0])
    import ppo_update_time as PU
    from carl_amd import _lib

    return PU._setup(_lib.CARTPOLE, SHAPES[which][0])


def _ppo(which, **kw):
    from carl_amd import PPO

    _, T, M = SHAPES[which]
    ppo = PPO(*_make(which), n_steps=T, n_epochs=1, batch_size=M, ent_coef=0.01, **kw)
    ppo.collect()
    for _ in range(2):  # warm-up: uploads, code objects, the optimiser's state
        ppo.update()
    return ppo


def _launches(ppo_on):
    """each launch of the fused step alone, and the torch operations it replaces, on the fused object's buffer"""
    import torch

    import ppo_update_time as PU

    eng, buf, T = ppo_on.engine, ppo_on._buf, ppo_on.n_steps
    mbs = ppo_on.minibatches()
    epoch, B = ppo_on._epoch_idx, ppo_on.batch_size
    adv = buf["advantage"][:T]
    P = int(adv.stride(0))
    storage = torch.as_strided(adv, (T * P,), (1,)) if P != eng.n else adv.reshape(-1)
    rows = torch.empty((len(mbs), 2), dtype=torch.float32, device=eng.device)

    def kernel_stats():
        eng.ppo_adv_stats(adv, epoch, B, 1e-8, out=rows)

    def torch_stats():
        out = []
        for idx in mbs:
            a = storage[idx.long()]
            out.append(torch.stack([a.mean(), 1.0 / (a.std() + 1e-8)]).contiguous())
        return out

    out = {}

    def grad():
        return eng.ppo_grad(ppo_on._actor, ppo_on._critic, buf, buf["obs0"], buf["context_id"], idx=mbs[0], adv_norm=rows[0],
                            clip_range=0.2, vf_coef=0.5, ent_coef=0.01, out=out, workspace=ppo_on._ws)

    kernel_stats()
    g = grad()
    params = [p.clone() for p in ppo_on._opt_params]
    grads = [g["grad_actor"].view_as(params[0]), g["grad_critic"].view_as(params[1])] + (
        [g["grad_log_std"].view_as(params[2])] if ppo_on.box else [])
    state = eng.adam_state(params)
    norm_out = torch.empty(2, dtype=torch.float64, device=eng.device)

    def kernel_adam():
        eng.adam_step(params, grads, state, 3e-4, eps=1e-5, max_grad_norm=0.5, norm_out=norm_out)

    tparams = [p.clone() for p in ppo_on._opt_params]
    opt = torch.optim.Adam(tparams, lr=3e-4, eps=1e-5)

    def torch_adam():
        total = torch.sqrt(sum((x.double() ** 2).sum() for x in grads)).float()
        coef = torch.clamp(0.5 / (total + 1e-6), max=1.0)
        for p, x in zip(tparams, grads):
            p.grad = x * coef
        opt.step()

    fns = {"adv_stats_of_the_epoch": kernel_stats, "adv_stats_torch_gather_mean_std_per_minibatch": torch_stats,
           "ppo_grad_three_launches": grad, "clip_and_adam": kernel_adam, "clip_and_adam_torch": torch_adam}
    for fn in fns.values():
        for _ in range(3):
            fn()
    ms = {k: [] for k in fns}
    for _ in range(REPS):  # alternating
        for k, fn in fns.items():
            ms[k].append(PU._timed(fn, 10))
    return {"minibatches": len(mbs), "parameters": sum(p.numel() for p in params), **{k: _stat(v) for k, v in ms.items()}}


def _epoch(which):
    import torch

    import ppo_update_time as PU

    runs = {"off": _ppo(which), "on": _ppo(which, fused_step=True)}
    torch.cuda.synchronize()
    ms = {"off": [], "on": []}
    for _ in range(REPS):  # alternating rounds
        for name in ("off", "on"):
            ms[name].append(PU._timed(runs[name].update, 1))
    N, T, M = SHAPES[which]
    res = {"step": "epoch_" + which, "lanes": N, "steps": T, "batch_size": M, "minibatches": -(-N * T // M),
           "repetitions": REPS, "epoch_fused_step_off": _stat(ms["off"]), "epoch_fused_step_on": _stat(ms["on"]),
           "fused_below_unfused": statistics.median(ms["on"]) < statistics.median(ms["off"])}
    if which == "cartpole":
        res["launches"] = _launches(runs["on"])
    return res


def step_epoch_cartpole():
    return _epoch("cartpole")


def step_epoch_cartpole_small():
    return _epoch("cartpole_small")


def step_epoch_ant():
    return _epoch("ant")


def _offpath(which):
    """fused_step off, through the arguments the parent commit's PPO has: runs in either tree"""
    import torch

    import ppo_update_time as PU

    ppo = _ppo(which)
    torch.cuda.synchronize()
    return {"step": "offpath_" + which, "tree": ROOT, "rounds_ms": [PU._timed(ppo.update, 1) for _ in range(REPS)]}


def step_offpath_cartpole():
    return _offpath("cartpole")


def step_offpath_cartpole_small():
    return _offpath("cartpole_small")


def step_offpath_ant():
    return _offpath("ant")


def _beside(which, parent_tree):
    """three processes per tree, alternating: the parent's, this tree's with fused_step off"""
    rounds = {"parent": [], "this": []}
    for _ in range(3):
        for name, tree in (("parent", parent_tree), ("this", HERE)):
            env = dict(os.environ, CARL_PPO_STEP_TREE=os.path.abspath(tree), CARL_AMD_NO_BUILD="1")
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "offpath_" + which], capture_output=True,
                               text=True, timeout=LIMITS["offpath_" + which], env=env, check=True)
            rounds[name].append(json.loads(p.stdout.strip().splitlines()[-1])["rounds_ms"])
    flat = {k: [x for r in v for x in r] for k, v in rounds.items()}
    lo, hi = min(flat["parent"]), max(flat["parent"])
    return {"step": "beside_" + which, "processes_per_tree": 3, "rounds_per_process": REPS,
            "parent_commit_epoch": _stat(flat["parent"]), "parent_commit_process_medians_ms": [statistics.median(r) for r in rounds["parent"]],
            "fused_step_off_epoch": _stat(flat["this"]), "fused_step_off_process_medians_ms": [statistics.median(r) for r in rounds["this"]],
            "off_path_median_inside_parent_range": lo <= statistics.median(flat["this"]) <= hi}


def step_beside_cartpole():
    return _beside("cartpole", os.environ["CARL_PPO_STEP_PARENT"])


def step_beside_cartpole_small():
    return _beside("cartpole_small", os.environ["CARL_PPO_STEP_PARENT"])


def step_beside_ant():
    return _beside("ant", os.environ["CARL_PPO_STEP_PARENT"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(LIMITS))
    ap.add_argument("--steps", help="comma-separated subset, in the given order (default: the epoch_* steps)")
    ap.add_argument("--out")
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit, for the beside_* steps")
    args = ap.parse_args()
    if args.parent_tree:
        os.environ["CARL_PPO_STEP_PARENT"] = os.path.abspath(args.parent_tree)
    if args.step:
        print(json.dumps(globals()["step_" + args.step]()), flush=True)
        return 0
    results = []
    if args.out and os.path.exists(args.out):  # a run of some steps keeps the other steps' earlier results
        with open(args.out) as f:
            results = json.load(f)
    names = args.steps.split(",") if args.steps else ORDER + (["beside_" + w for w in SHAPES] if args.parent_tree else [])
    for name in names:
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
