"""Measurements of the PPO update on the device for the Brax families; tools/ppo_update_time.py's
sibling.

    python tools/brax_ppo_update_time.py [--out profiles/brax_ppo_update_time.json]

runs three steps, each in a child process of its own under its own time limit, and stops at the first one that fails:

  time               32 768 envs x 8 steps of Ant, 2 x 64 tanh actor and critic, two context inputs: one carl_brax_ppo_grad
                     minibatch of 65 536 samples, torch-ROCm autograd of the same loss on the same gathered minibatch, and
                     one full epoch of PPO.update.  Device events around repeated calls, the two minibatch paths
                     alternating in one process; medians and ranges.  The two paths' gradients are compared first.
  learn_pendulum     a learning run on the inverted pendulum: mean return of the envs' last finished episodes per iteration
  learn_halfcheetah  the same for Halfcheetah

`--step NAME` runs one step in this process and prints its JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

LIMITS = {"time": 300, "learn_pendulum": 240, "learn_halfcheetah": 300}  # seconds per step


def _setup(model, n, seed=0, max_episode_steps=None):
    import numpy as np

    import brax_policy_cases as BP
    from carl_amd import _lib
    from carl_amd.brax_engine import BraxVecEngine
    from carl_amd.brax_policy import BraxMLPPolicy

    s, names, default = BP.build_model(model)
    rng = np.random.default_rng(seed)
    rows = BP.context_rows(rng, 16, default, names)
    feats = [names.index("gravity"), names.index("friction")]
    kw = {} if max_episode_steps is None else {"max_episode_steps": max_episode_steps}
    eng = BraxVecEngine(s, len(names), rows, n, "cuda", selector=_lib.SEL_ROUND_ROBIN, seed=seed, ctx_obs_rows=feats, **kw)
    n_in = 2 + eng.D
    shift = np.zeros(n_in, np.float32)
    shift[:2] = default[feats]
    scale = np.ones(n_in, np.float32)
    scale[:2] = 1.0 / np.maximum(np.abs(default[feats]), 1e-3)
    actor_layers = BP.make_layers(rng, n_in, (64, 64), s.n_act, gain=0.01)  # a near-zero head, as SB3 initialises one
    actor = BraxMLPPolicy.for_env(eng, actor_layers, "tanh", shift, scale, 10.0, log_std=np.zeros(s.n_act, np.float32))
    critic = BraxMLPPolicy.for_env(eng, BP.make_layers(rng, n_in, (64, 64), 1, gain=0.1), "tanh", shift, scale, 10.0,
                                   head="value")
    return eng, actor, critic


def _timed(fn, inner):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner  # ms per call


def step_time():
    import math

    import torch

    from carl_amd import PPO, _lib

    N, T, M = 32768, 8, 65536
    eng, actor, critic = _setup("ant", N)
    ppo = PPO(eng, actor, critic, n_steps=T, n_epochs=1, batch_size=M, ent_coef=0.01)
    buf = ppo.collect()
    idx = ppo.minibatches()[0]
    a = buf["advantage"][:T].reshape(-1)[idx.long()]
    norm = torch.stack([a.mean(), 1.0 / (a.std() + 1e-8)]).contiguous()
    out = {}

    def kernel_mb():
        eng.ppo_grad(ppo._actor, ppo._critic, buf, buf["obs0"], buf["context_id"], idx=idx, adv_norm=norm, clip_range=0.2,
                     vf_coef=0.5, ent_coef=0.01, out=out, workspace=ppo._ws)

    pa = ppo.actor_params[0].clone().requires_grad_()
    pc = ppo.critic_params[0].clone().requires_grad_()
    ls = ppo.log_std[0].clone().requires_grad_()
    rows = torch.as_tensor(actor.ctx_rows, device=eng.device)
    n_act = eng.sys.n_act
    obs_prev = torch.cat([buf["obs0"][None], buf["obs"][: T - 1]], dim=0).reshape(T * N, -1)
    flat = lambda k: buf[k][:T].reshape(-1)  # noqa: E731
    actions = buf["action"][:T].reshape(T * N, n_act)

    def net(p, pol, x):
        off, h = 0, x
        for k, (W, b) in enumerate(pol.layers):
            o, i = W.shape
            h = torch.addmm(p[off + o * i: off + o * i + o], h, p[off: off + o * i].view(o, i).t())
            off += o * i + o
            if k < len(pol.layers) - 1:
                h = torch.tanh(h)
        return h

    def torch_mb():
        pa.grad = pc.grad = ls.grad = None
        j = idx.long()
        x = torch.cat([eng.ctx_table[rows][:, buf["context_id"].reshape(-1)[j].long()].t(), obs_prev[j]], dim=1)
        off, n_in = actor.weight_floats, actor.n_in
        x = torch.clamp((x - pa[off: off + n_in].detach()) * pa[off + n_in: off + 2 * n_in].detach(), -10.0, 10.0)
        mu = net(pa, actor, x)
        V = net(pc, critic, x)[:, 0]
        z = (actions[j] - mu) * torch.exp(-ls)
        lp = (-0.5 * z * z - ls - 0.5 * math.log(2 * math.pi)).sum(dim=1)
        H = (0.5 + 0.5 * math.log(2 * math.pi) + ls).sum()
        A = (flat("advantage")[j] - norm[0]) * norm[1]
        r = torch.exp(lp - flat("log_prob")[j])
        pl = -torch.min(r * A, torch.clamp(r, 0.8, 1.2) * A).mean()
        loss = pl - 0.01 * H + 0.5 * ((flat("return")[j] - V) ** 2).mean()
        loss.backward()

    kernel_mb()
    torch_mb()
    torch.cuda.synchronize()
    pairs = ((out["grad_actor"], pa.grad), (out["grad_critic"], pc.grad), (out["grad_log_std"], ls.grad))
    agree = max(float((g - t).abs().max() / t.abs().max()) for g, t in pairs)
    for _ in range(3):  # warm-up of both paths
        kernel_mb()
        torch_mb()
    k_ms, t_ms = [], []
    for _ in range(15):  # alternating
        k_ms.append(_timed(kernel_mb, 10))
        t_ms.append(_timed(torch_mb, 10))
    ppo.update()  # warm-up of the epoch's torch ops
    e_ms = [_timed(ppo.update, 1) for _ in range(5)]
    med = statistics.median
    return {"step": "time", "model": "ant", "envs": N, "steps": T, "minibatch": M,
            "networks": "2 x 64 tanh, actor and critic, two context inputs",
            "gradients_max_difference_over_max_gradient": agree,
            "carl_brax_ppo_grad_ms": med(k_ms), "carl_brax_ppo_grad_ms_min_max": [min(k_ms), max(k_ms)],
            "torch_autograd_ms": med(t_ms), "torch_autograd_ms_min_max": [min(t_ms), max(t_ms)],
            "epoch_ms": med(e_ms), "epoch_minibatches": T * N // M, "epoch_ms_min_max": [min(e_ms), max(e_ms)],
            "workgroups": int(_lib.load().carl_brax_ppo_grad_workgroups(M))}


def _learn(model, name, n, T, iterations, max_episode_steps=None, **kw):
    from carl_amd import PPO

    eng, actor, critic = _setup(model, n, seed=1, max_episode_steps=max_episode_steps)
    ppo = PPO(eng, actor, critic, n_steps=T, **kw)
    curve = []
    for _ in range(iterations):
        ppo.collect()
        ppo.update()
        done = eng.episodes_done > 0
        curve.append(round(float(eng.last_return[done].mean()), 2))  # (a tool: one read-back per iteration)
    return {"step": name, "model": model, "envs": n, "steps": T, "iterations": iterations,
            "max_episode_steps": max_episode_steps, "settings": kw, "mean_last_episode_return": curve}


def step_learn_pendulum():
    return _learn("inverted_pendulum", "learn_pendulum", 4096, 64, 20, max_episode_steps=200, n_epochs=4, batch_size=16384,
                  lr=1e-3, ent_coef=0.0)


def step_learn_halfcheetah():
    return _learn("halfcheetah", "learn_halfcheetah", 2048, 32, 20, max_episode_steps=100, n_epochs=4, batch_size=16384,
                  lr=3e-4, ent_coef=0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(LIMITS))
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.step:
        print(json.dumps(globals()["step_" + args.step]()), flush=True)
        return 0
    results = []
    for name in ("time", "learn_pendulum", "learn_halfcheetah"):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True,
                               timeout=LIMITS[name])
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {LIMITS[name]} s -- stopping", flush=True)
            return 1
        if p.returncode != 0:
            print(f"{name}: exit status {p.returncode} -- stopping\n{p.stderr[-2000:]}", flush=True)
            return 1
        results.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(results, f, indent=1)
                f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
