"""Measurements of the PPO update on the device.

    python tools/ppo_update_time.py [--out profiles/ppo_update_time.json]

runs three steps, each in a child process of its own under its own time limit, and stops at the first one that fails:

  time            65 536 lanes x 128 steps of CartPole, 2 x 64 tanh networks: one carl_ppo_grad minibatch of 65 536 samples,
                  torch-ROCm autograd of the same loss on the same gathered minibatch (what a user would otherwise write),
                  and one full epoch of PPO.update (128 minibatches: permutation, advantage statistics, gradients, clip,
                  Adam).  Device events around repeated calls, the two minibatch paths alternating in one process; medians.
                  The two paths' gradients are compared first.
  learn_cartpole  a learning run: mean return of the lanes' last finished episodes after every iteration
  learn_pendulum  the same for Pendulum

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

LIMITS = {"time": 420, "learn_cartpole": 240, "learn_pendulum": 240}  # seconds per step


def _setup(family, n, seed=0):
    import numpy as np

    import policy_cases as PC
    import value_cases as VC

    eng = PC.make_engine(family, n, n_contexts=64, seed=seed)
    rng = np.random.default_rng(seed)
    box = not eng.info.action_is_discrete
    actor = PC.make_policy(eng, (64, 64), "tanh", rng, ctx="all", clip=10.0, log_std=0.0 if box else None)
    # a small head: a near-uniform starting policy, as SB3 initialises one
    W, b = actor.layers[-1]
    W *= 0.01
    b *= 0.0
    actor = type(actor).unpack(actor, actor._pack(), 0.0 if box else None)
    critic = VC.make_critic(eng, actor, (64, 64), "tanh", rng)
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
    import torch

    from carl_amd import PPO, _lib

    N, T, M = 65536, 128, 65536
    eng, actor, critic = _setup(_lib.CARTPOLE, N)
    ppo = PPO(eng, actor, critic, n_steps=T, n_epochs=1, batch_size=M, ent_coef=0.01)
    buf = ppo.collect()
    idx = ppo.minibatches()[0]
    P = int(buf["action"].stride(0))
    adv_all = buf["advantage"].reshape(-1) if P == N else torch.as_strided(buf["advantage"], (T * P,), (1,))
    a = adv_all[idx.long()]
    norm = torch.stack([a.mean(), 1.0 / (a.std() + 1e-8)]).contiguous()
    out = {}

    def kernel_mb():
        eng.ppo_grad(ppo._actor, ppo._critic, buf, buf["obs0"], buf["context_id"], idx=idx, adv_norm=norm, clip_range=0.2,
                     vf_coef=0.5, ent_coef=0.01, out=out, workspace=ppo._ws)

    # the same loss in torch: leaves are the packed tensors, the layers views of them
    pa = ppo.actor_params[0].clone().requires_grad_()
    pc = ppo.critic_params[0].clone().requires_grad_()
    rows = torch.as_tensor(actor.ctx_rows, device=eng.device)
    obs_prev = torch.cat([buf["obs0"][None], buf["obs"][: T - 1]], dim=0).reshape(T * P, -1) if P == N else None
    assert obs_prev is not None, "the timing run uses dense rows"
    flat = lambda k: buf[k].reshape(-1)  # noqa: E731

    def net(p, pol, x):
        off, h = 0, x
        for k, (W, b) in enumerate(pol.layers):
            o, i = W.shape
            h = torch.addmm(p[off + o * i: off + o * i + o], h, p[off: off + o * i].view(o, i).t())
            off += o * i + o
            if k < len(pol.layers) - 1:
                h = torch.tanh(h)
        return h, off

    def torch_mb():
        pa.grad = pc.grad = None
        j = idx.long()
        x = torch.cat([eng.ctx_table[rows][:, flat("context_id")[j].long()].t(), obs_prev[j]], dim=1)
        off, n_in = actor.weight_floats, actor.n_in
        x = torch.clamp((x - pa[off: off + n_in].detach()) * pa[off + n_in: off + 2 * n_in].detach(), -10.0, 10.0)
        y, _ = net(pa, actor, x)
        V = net(pc, critic, x)[0][:, 0]
        logp = torch.log_softmax(y, dim=1)
        lp = logp.gather(1, flat("action")[j].long()[:, None])[:, 0]
        H = -(logp.exp() * logp).sum(dim=1)
        A = (flat("advantage")[j] - norm[0]) * norm[1]
        r = torch.exp(lp - flat("log_prob")[j])
        pl = -torch.min(r * A, torch.clamp(r, 0.8, 1.2) * A).mean()
        loss = pl - 0.01 * H.mean() + 0.5 * ((flat("return")[j] - V) ** 2).mean()
        loss.backward()

    kernel_mb()
    torch_mb()
    torch.cuda.synchronize()
    ga, gc = out["grad_actor"], out["grad_critic"]
    agree = max(float((ga - pa.grad).abs().max() / pa.grad.abs().max()), float((gc - pc.grad).abs().max() / pc.grad.abs().max()))
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
    return {"step": "time", "lanes": N, "steps": T, "minibatch": M, "networks": "2 x 64 tanh, actor and critic",
            "gradients_max_difference_over_max_gradient": agree,
            "carl_ppo_grad_ms": med(k_ms), "carl_ppo_grad_ms_min_max": [min(k_ms), max(k_ms)],
            "torch_autograd_ms": med(t_ms), "torch_autograd_ms_min_max": [min(t_ms), max(t_ms)],
            "epoch_ms": med(e_ms), "epoch_minibatches": T * N // M, "epoch_ms_min_max": [min(e_ms), max(e_ms)],
            "workgroups": int(_lib.load().carl_ppo_grad_workgroups(M))}


def _learn(family, name, n, T, iterations, **kw):
    from carl_amd import PPO

    eng, actor, critic = _setup(family, n, seed=1)
    ppo = PPO(eng, actor, critic, n_steps=T, **kw)
    curve = []
    for _ in range(iterations):
        ppo.collect()
        ppo.update()
        done = eng.episodes_done > 0
        curve.append(round(float(eng.last_return[done].mean()), 2))  # (a tool: one read-back per iteration)
    return {"step": name, "lanes": n, "steps": T, "iterations": iterations, "settings": kw,
            "mean_last_episode_return": curve}


def step_learn_cartpole():
    from carl_amd import _lib

    return _learn(_lib.CARTPOLE, "learn_cartpole", 4096, 64, 30, n_epochs=4, batch_size=16384, lr=1e-3, ent_coef=0.0)


def step_learn_pendulum():
    from carl_amd import _lib

    return _learn(_lib.PENDULUM, "learn_pendulum", 4096, 200, 30, n_epochs=6, batch_size=32768, lr=1e-3, gamma=0.9,
                  ent_coef=0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(LIMITS))
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.step:
        print(json.dumps(globals()["step_" + args.step]()), flush=True)
        return 0
    results = []
    for name in ("time", "learn_cartpole", "learn_pendulum"):
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
