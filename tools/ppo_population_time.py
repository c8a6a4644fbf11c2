"""Measurements of a population of PPO learners on the device.

    python tools/ppo_population_time.py [--out profiles/ppo_population_time.json] [--steps NAME,NAME,...] [--parent-tree DIR]

runs its steps, each in a child process of its own under its own time limit, and stops at the first one that fails:

  epoch_cartpole_16x256   one epoch of PopulationPPO.update() with P members against P one-member PPO(fused_step=True)
  epoch_cartpole_4x4096   updates of the same per-member shape run back to back, in one process: the population on one
  epoch_pendulum_16x256   engine of P x L lanes, the P learners on engines of L lanes of their own; alternating rounds,
                          device events after warm-up, medians with min-max over 15 repetitions.  The sequential side is
                          code the population does not touch: the parent commit's path.
  beside_<shape>          with --parent-tree DIR (a built checkout of the parent commit): ONE member's
                          PPO(fused_step=True) epoch in child processes that import carl_amd from DIR and from this tree
                          in turn, three processes each: the parent's round-to-round range beside this tree's
  learn_cartpole          a short learning run, as evidence: CartPole, 8 members -- four learning rates x two seeds -- of
                          256 lanes x 64 steps, 40 iterations; each member's mean episode length per iteration

`--step NAME` runs one step in this process and prints its JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("CARL_PPO_POPULATION_TREE") or HERE  # the tree carl_amd, tests/ and tools/ are imported from (onemember_*)
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

SHAPES = {"cartpole_16x256": ("cartpole", 16, 256, 64, 4096), "cartpole_4x4096": ("cartpole", 4, 4096, 64, 16384),
          "pendulum_16x256": ("pendulum", 16, 256, 64, 4096)}  # family, members, lanes per member, steps, minibatch
LIMITS = {**{"epoch_" + k: 300 for k in SHAPES}, **{"beside_" + k: 600 for k in SHAPES},
          **{"onemember_" + k: 180 for k in SHAPES}, "learn_cartpole": 300}  # seconds per step
ORDER = ["epoch_" + k for k in SHAPES]
REPS = 15
HYPER = dict(lr=3e-4, clip_range=0.2, vf_coef=0.5, ent_coef=0.01, max_grad_norm=0.5)


def _stat(v):
    return {"median_ms": statistics.median(v), "min_max_ms": [min(v), max(v)]}


def _family(name):
    from carl_amd import _lib

    return {"cartpole": _lib.CARTPOLE, "pendulum": _lib.PENDULUM}[name]


def _engine(family, n, seed=0):
    import policy_cases as PC

    return PC.make_engine(_family(family), n, n_contexts=64, seed=seed)


def _networks(eng, seed):
    """ppo_update_time._setup's 2 x 64 tanh actor and critic for `eng`, from `seed`"""
    import numpy as np

    import policy_cases as PC
    import value_cases as VC

    rng = np.random.default_rng(seed)
    box = not eng.info.action_is_discrete
    actor = PC.make_policy(eng, (64, 64), "tanh", rng, ctx="all", clip=10.0, log_std=0.0 if box else None)
    W, b = actor.layers[-1]  # a small head: a near-uniform starting policy, as SB3 initialises one
    W *= 0.01
    b *= 0.0
    actor = type(actor).unpack(actor, actor._pack(), 0.0 if box else None)
    return actor, VC.make_critic(eng, actor, (64, 64), "tanh", rng)


def _one_member(shape, seed=0):
    """a warmed one-member PPO(fused_step=True) of the shape's per-member size, on an engine of its own"""
    from carl_amd import PPO

    family, _, L, T, M = SHAPES[shape]
    eng = _engine(family, L, seed)
    ppo = PPO(eng, *_networks(eng, seed), n_steps=T, n_epochs=1, batch_size=M, fused_step=True, **HYPER)
    ppo.collect()
    for _ in range(2):  # warm-up: uploads, code objects, the persistent gradient tensors
        ppo.update()
    return ppo


def _epoch(shape):
    import torch

    import ppo_update_time as PU
    from carl_amd import PopulationPPO

    family, P, L, T, M = SHAPES[shape]
    eng = _engine(family, P * L)
    nets = [_networks(eng, s) for s in range(P)]
    pop = PopulationPPO(eng, [a for a, _ in nets], [c for _, c in nets], lanes_per_set=L, n_steps=T, n_epochs=1, batch_size=M,
                        **HYPER)
    pop.collect()
    for _ in range(2):
        pop.update()
    learners = [_one_member(shape, s) for s in range(P)]

    def sequential():
        for ppo in learners:
            ppo.update()

    torch.cuda.synchronize()
    ms = {"population": [], "sequential": []}
    for _ in range(REPS):  # alternating rounds
        ms["sequential"].append(PU._timed(sequential, 1))
        ms["population"].append(PU._timed(pop.update, 1))
    per_epoch = -(-L * T // M)
    return {"step": "epoch_" + shape, "family": family, "members": P, "lanes_per_member": L, "steps": T, "batch_size": M,
            "minibatches_per_member": per_epoch, "launches_population": 4 * per_epoch + 1,
            "launches_sequential": P * (4 * per_epoch + 1), "repetitions": REPS,
            "epoch_population": _stat(ms["population"]), "epoch_sequential_fused_ppo": _stat(ms["sequential"]),
            "population_median_below_sequential_min": statistics.median(ms["population"]) < min(ms["sequential"])}


def _onemember(shape):
    """one member's PPO(fused_step=True) epoch: runs in either tree"""
    import torch

    import ppo_update_time as PU

    ppo = _one_member(shape)
    torch.cuda.synchronize()
    return {"step": "onemember_" + shape, "tree": ROOT, "rounds_ms": [PU._timed(ppo.update, 1) for _ in range(REPS)]}


def _beside(shape, parent_tree):
    """three processes per tree, alternating: the parent's, this tree's"""
    rounds = {"parent": [], "this": []}
    for _ in range(3):
        for name, tree in (("parent", parent_tree), ("this", HERE)):
            env = dict(os.environ, CARL_PPO_POPULATION_TREE=os.path.abspath(tree), CARL_AMD_NO_BUILD="1")
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "onemember_" + shape], capture_output=True,
                               text=True, timeout=LIMITS["onemember_" + shape], env=env, check=True)
            rounds[name].append(json.loads(p.stdout.strip().splitlines()[-1])["rounds_ms"])
    flat = {k: [x for r in v for x in r] for k, v in rounds.items()}
    lo, hi = min(flat["parent"]), max(flat["parent"])
    return {"step": "beside_" + shape, "processes_per_tree": 3, "rounds_per_process": REPS,
            "parent_commit_epoch": _stat(flat["parent"]), "parent_commit_process_medians_ms": [statistics.median(r) for r in rounds["parent"]],
            "this_tree_epoch": _stat(flat["this"]), "this_tree_process_medians_ms": [statistics.median(r) for r in rounds["this"]],
            "this_tree_median_inside_parent_range": lo <= statistics.median(flat["this"]) <= hi}


def step_learn_cartpole():
    import torch

    from carl_amd import PopulationPPO

    lrs, seeds, L, T, iterations = [1e-4, 3e-4, 1e-3, 3e-3], [0, 1], 256, 64, 40
    members = [(lr, seed) for lr in lrs for seed in seeds]
    eng = _engine("cartpole", len(members) * L)
    nets = [_networks(eng, seed) for _, seed in members]
    pop = PopulationPPO(eng, [a for a, _ in nets], [c for _, c in nets], lanes_per_set=L, n_steps=T, n_epochs=4, batch_size=4096,
                        **{**HYPER, "lr": [lr for lr, _ in members]})
    ends = []
    for _ in range(iterations):
        buf = pop.collect()
        pop.update()
        done = (buf["terminated"][:T] != 0) | (buf["truncated"][:T] != 0)
        ends.append(done.float().unflatten(1, (len(members), L)).mean(dim=(0, 2)))
    curves = torch.stack(ends).cpu().numpy()  # [iterations, P]
    return {"step": "learn_cartpole", "lanes_per_member": L, "steps": T, "iterations": iterations, "n_epochs": 4,
            "batch_size": 4096, "what": "each member's mean episode length over every collection: steps per episode end "
            "(terminated or truncated) among its 256 x 64 steps",
            "members": [{"lr": lr, "seed": seed, "mean_episode_length": [round(1.0 / max(float(v), 1e-9), 2) for v in curves[:, i]]}
                        for i, (lr, seed) in enumerate(members)]}


def _steps():
    fns = {"learn_cartpole": step_learn_cartpole}
    for shape in SHAPES:
        fns["epoch_" + shape] = lambda shape=shape: _epoch(shape)
        fns["onemember_" + shape] = lambda shape=shape: _onemember(shape)
        fns["beside_" + shape] = lambda shape=shape: _beside(shape, os.environ["CARL_PPO_POPULATION_PARENT"])
    return fns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(LIMITS))
    ap.add_argument("--steps", help="comma-separated subset, in the given order (default: the epoch_* steps)")
    ap.add_argument("--out")
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit, for the beside_* steps")
    args = ap.parse_args()
    if args.parent_tree:
        os.environ["CARL_PPO_POPULATION_PARENT"] = os.path.abspath(args.parent_tree)
    if args.step:
        print(json.dumps(_steps()[args.step]()), flush=True)
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
