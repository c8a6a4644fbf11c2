"""The Brax closed-loop rollout with a critic (include/carl_amd.h: carl_brax_rollout_policy_valued;
BraxVecEngine.rollout_policy(deterministic=False, value_net=critic)) on the GPU.  Every column is held to the exact host
reference of the critic's packed block (value_cases.check_values: identity / relu bit for bit, tanh within the
reference's own bound) on inputs that do not come from the launch's bookkeeping:

  * value       on the teacher-forced inputs of a per-call replay of the recorded actions (policy_checks.teacher), which
                reads each env's context and observation from the engine before every step -- no env-step is exempted;
  * last_value  on inputs rebuilt from the engine's ctx_table, ctx_idx and obs after the launch;
  * boot_value  where a step truncated an episode without terminating it, on [the context values the step ran under, the
                terminal observation of a sampled launch with final_obs from the same snapshot]; the bits of +0.0f
                everywhere else.

Everything else the launch writes is pinned bit for bit to the sampled launch from the same snapshot.

Shapes: 300 envs in two weight sets of 256 with different actors and critics (one wavefront holds envs of both sets at
every width), 8 steps under a TimeLimit of 3, a round-robin selector over 5 contexts: every env crosses auto-resets
inside the launch and changes its context there."""
import numpy as np
import pytest
import torch

import brax_policy_cases as BP
import brax_sampling_cases as BS
import policy_checks as PC
import value_cases as VC
from carl_amd import _lib
from carl_amd.brax_policy import BraxMLPPolicy

pytestmark = pytest.mark.gpu

N, T = 300, 8
RECORDS = ("obs", "reward", "terminated", "truncated")
COLUMNS = ("value", "boot_value")
ZERO_BITS = 0  # +0.0f


def _first_of_each_class():
    """one (model, width) per kernel class: lean, multi-hinge, general, planar"""
    seen = {}
    for m, w in BP.instance_cases():
        seen.setdefault(BP.MODELS[m], (m, w))
    assert len(seen) == 4
    return set(seen.values())


ALL_NETWORKS = _first_of_each_class()


def make_critic(eng, actor, widths, act, seed):
    """a random value network over the actor's inputs, one weight set per actor set, each with that set's shift | scale |
    clip (the critic reads the actor's transformed inputs)"""
    rng = np.random.default_rng(seed)
    n = actor.n_in
    crits = []
    for sec in actor.transform_section():
        dims = [n, *widths, 1]
        layers = [(rng.normal(0, 1.5 / np.sqrt(i), (o, i)), rng.normal(0, 0.3, o)) for i, o in zip(dims[:-1], dims[1:])]
        crits.append(BraxMLPPolicy.for_env(eng, layers, act, sec[:n], sec[n: 2 * n], float(sec[2 * n]),
                                           context_features=actor.ctx_rows, head="value"))
    return crits[0] if actor.lanes_per_set is None else BraxMLPPolicy.stack(crits, actor.lanes_per_set, head="value")


def launch(eng, pol, steps, crit=None, **kw):
    if crit is not None:
        kw["value_net"] = crit
    return eng.rollout_policy(pol, steps, deterministic=False, sample_seed=BS.SEED, **kw)


def sets_of(eng, pol):
    return (np.arange(eng.n) // (pol.lanes_per_set or (1 << 30))).astype(np.int32)


def same_bits(a, b, what):
    if a.is_floating_point():
        a, b = a.view(torch.int32), b.view(torch.int32)
    assert torch.equal(a, b), what


def current_inputs(eng, pol):
    """[n, n_in] from the engine as it stands: the context values of each env's context, then its observation"""
    tab = eng.ctx_table.cpu().numpy()
    cidx = eng.ctx_idx.cpu().numpy().astype(np.int64)
    return np.concatenate([tab[pol.ctx_rows][:, cidx].T, eng.obs.cpu().numpy()], axis=1).astype(np.float32)


def check_columns(eng, pol, crit, snap, out, steps, boot=True):
    """value, last_value and boot_value of the valued launch `out` from `snap` against the host reference; the engine is
    left in the launch's end state.  -> (the boot mask [steps, n], the sampled launch with final_obs)"""
    n, M = eng.n, steps * eng.n
    sets = sets_of(eng, pol)
    n_ctx = len(pol.ctx_rows)
    last_x = current_inputs(eng, pol)  # (the engine is in the launch's end state here)
    VC.check_values(crit, last_x, out["last_value"].cpu().numpy(), sets)
    # the sampled launch with terminal observations from the same snapshot: every other output's bits, and final_obs
    eng.restore(snap)
    ref = launch(eng, pol, steps, log_prob=True, out=eng.alloc_rollout(steps, final_obs=True, action=True))
    for k in RECORDS + ("action", "log_prob"):
        same_bits(out[k][:steps], ref[k][:steps], k)
    x = PC.teacher(eng, pol, snap, out["action"][:steps])[0]
    VC.check_values(crit, x.reshape(M, -1), out["value"][:steps].cpu().numpy(), np.tile(sets, steps))
    te, tr = (out[k][:steps].cpu().numpy().astype(bool) for k in ("terminated", "truncated"))
    mask = tr & ~te
    if boot:
        bv = out["boot_value"][:steps].cpu().numpy()
        xb = np.concatenate([x[:, :, :n_ctx], ref["final_obs"][:steps].cpu().numpy()], axis=2)
        assert np.isfinite(xb[mask]).all()
        VC.check_values(crit, xb.reshape(M, -1), bv, np.tile(sets, steps), where=mask)
        assert (bv.view(np.int32)[~mask] == ZERO_BITS).all(), "boot_value is not +0.0f off the truncated-only steps"
    else:
        assert "boot_value" not in out
    return mask, ref


def check_pinned(eng, pol, crit, snap, out, steps, after, split=3):
    """the valued launch `out` from `snap`, against the other launches from the same snapshot"""
    eng.restore(snap)
    plain = launch(eng, pol, steps, log_prob=True)                     # the sampled launch: everything it writes
    for k in RECORDS + ("action", "log_prob"):
        same_bits(plain[k], out[k][:steps], k)
    same_bits(eng.obs, out["obs"][steps - 1], "obs")
    PC.assert_same_state(after, PC.engine_state(eng))
    eng.restore(snap)
    a, b = launch(eng, pol, split, crit), launch(eng, pol, steps - split, crit)  # the horizon in two launches
    for k in RECORDS + ("action", "log_prob") + COLUMNS:
        same_bits(torch.cat([a[k], b[k]]), out[k][:steps], k)
    same_bits(b["last_value"], out["last_value"], "last_value")
    PC.assert_same_state(after, PC.engine_state(eng))
    eng.restore(snap)
    nb = launch(eng, pol, steps, crit, bootstrap_truncated=False)       # the launch with boot_value absent
    assert "boot_value" not in nb
    for k in RECORDS + ("action", "log_prob", "value", "last_value"):
        same_bits(nb[k], out[k][:steps] if k != "last_value" else out[k], k)
    PC.assert_same_state(after, PC.engine_state(eng))


@pytest.mark.parametrize("model,width", BP.instance_cases(), ids=str)
def test_every_kernel_instance_against_the_reference_and_pinned(device, model, width):
    """case 1: every instantiated (class, width) with 2 x 64 tanh networks, one instance per class with the 1 x 32 relu
    and the linear critic as well (bit for bit); the tanh launch is then pinned to the sampled launch, the 3 + 5 split and
    the launch without boot_value"""
    seed = 9500 + 100 * list(BP.MODELS).index(model) + width
    eng = BS.make_engine(model, width, N, device, seed)
    assert BP.launch_shape(eng.b, eng.sys, BS.make_policy(eng, (), "identity", 0).struct(N, 0x10), T)[1].lanes_per_env == width
    pol = BS.two_set_policy(eng, (64, 64), "tanh", seed)
    nets = BP.NETWORKS if (model, width) in ALL_NETWORKS else BP.NETWORKS[:1]
    for k, (widths, act) in enumerate(nets):
        crit = make_critic(eng, pol, widths, act, seed + 10 * k + 5)
        assert crit.n_sets == 2 and (crit.params[0] != crit.params[1]).any()
        snap = eng.snapshot()
        out = launch(eng, pol, T, crit)
        after = PC.engine_state(eng)
        assert tuple(out["value"].shape) == tuple(out["boot_value"].shape) == tuple(out["log_prob"].shape) == (T, N)
        assert tuple(out["last_value"].shape) == (N,) and out["value"].dtype == torch.float32
        mask, _ = check_columns(eng, pol, crit, snap, out, T)
        PC.assert_same_state(after, PC.engine_state(eng))  # (the per-call replay ends in the launch's state)
        done = (out["terminated"] | out["truncated"]).bool()
        assert int(done.sum(0).min()) >= 2 and mask.sum() >= N  # TimeLimit 3 inside 8 steps: auto-resets in every env
        print(f"{model}/{width} critic {act}{list(widths)}: {int(mask.sum())} bootstrap values")
        if k == 0:
            check_pinned(eng, pol, crit, snap, out, T, after)
    assert len(torch.unique(eng.ctx_idx)) >= 3


HOPPER_GAIN, HOPPER_LOG_STD = 5.0, 1.0


def test_terminations_and_truncations_together(device):
    """case 2: Hopper under a TimeLimit of 24 for 48 steps with a policy loud enough to make it fall: episodes end both
    ways inside one launch.  boot_value is the bits of +0.0f on every terminated step (a step both terminated and
    truncated included) and the critic's value of the terminal observation on the truncated-only ones.  The TimeLimit,
    the head's gain and the log_std were chosen with the float64 oracle (oracle/brax.py: Engine) stepping this policy's
    sampled actions from the same seeds: there 81 env-steps terminate and 519 are truncated alone (at a TimeLimit of 12
    with gain 1.5, log_std 0, none terminates: Hopper needs longer to fall); both counts are asserted here."""
    steps = 48
    eng = BS.make_engine("hopper", 4, 300, device, 21, max_episode_steps=24)
    rng = np.random.default_rng(22)
    n_in = 2 + eng.D
    shift, scale, clip = BP.transform(rng, n_in)
    pol = BraxMLPPolicy.for_env(eng, BP.make_layers(rng, n_in, (64, 64), eng.sys.n_act, gain=HOPPER_GAIN), "tanh", shift,
                                scale, clip, log_std=HOPPER_LOG_STD)
    crit = make_critic(eng, pol, (64, 64), "tanh", 23)
    snap = eng.snapshot()
    out = launch(eng, pol, steps, crit)
    after = PC.engine_state(eng)
    mask, _ = check_columns(eng, pol, crit, snap, out, steps)
    PC.assert_same_state(after, PC.engine_state(eng))
    te = out["terminated"].cpu().numpy().astype(bool)
    print(f"hopper: {int(te.sum())} terminated env-steps, {int(mask.sum())} truncated alone")
    assert te.sum() >= 32 and mask.sum() >= 32
    assert (out["boot_value"].cpu().numpy().view(np.int32)[te] == ZERO_BITS).all()


def test_fragment_hand_over(device):
    """case 3: Ant pinned to 16 lanes per env, 6 steps, the smallest env count whose launch cuts a group between two
    wavefronts: all three columns equal, bit for bit, the launch at 9 lanes per env, which does not cut this batch --
    last_value is written by the fragment that runs the last step, value and boot_value by whoever runs theirs"""
    steps = 6
    s = BP.build_model("ant")[0]

    def plan(n, width):
        s.lanes_per_env = width
        b = _lib.Batch()
        b.n_lanes, b.flags = n, _lib.FLAG_AUTORESET
        code, sh = BP.launch_shape(b, s, _lib.Policy(), steps)
        assert code == 0 and sh.lanes_per_env == width
        return sh

    def waits(n, width):
        sh = plan(n, width)
        return sh, [f for f in BP.fragments(sh, n, steps) if f[5]]

    lo = 1  # the smallest group count (4 envs per group at 16 lanes) with fewer wavefronts than groups
    while lo < 1 << 13:
        sh = plan(4 * (lo - 1) + 1, 16)
        if sh.grid * sh.waves_per_workgroup < lo:
            break
        lo += 1
    n = 4 * (lo - 1) + 1
    shape, wait = waits(n, 16)
    assert wait, "no wait_head fragment"
    assert not waits(n, 9)[1], "9 lanes per env cuts this batch too"
    eng = BS.make_engine("ant", 16, n, device, 13, max_episode_steps=4)
    pol = BS.make_policy(eng, (64, 64), "tanh", 14, log_std=np.linspace(-1.0, 0.2, 8))
    crit = make_critic(eng, pol, (64, 64), "tanh", 15)
    snap = eng.snapshot()
    out = launch(eng, pol, steps, crit)
    after = PC.engine_state(eng)
    eng.restore(snap)
    eng.sys.lanes_per_env = 9
    whole = launch(eng, pol, steps, crit)
    for k in RECORDS + ("action", "log_prob", "last_value") + COLUMNS:
        same_bits(whole[k], out[k], k)
    PC.assert_same_state(after, PC.engine_state(eng))
    mask, _ = check_columns(eng, pol, crit, snap, whole, steps)
    assert mask.any()


def test_canaries(device):
    """rows beyond T in caller buffers and the floats before lane 0 and beyond lane N - 1 keep their canaries; a wrong
    buffer is refused like log_prob"""
    n, extra, pad = 70, 3, 32
    eng = BS.make_engine("hopper", 4, n, device, 61)
    pol = BS.make_policy(eng, (32,), "relu", 62, log_std=-0.5)
    crit = make_critic(eng, pol, (32,), "relu", 63)
    full = eng.alloc_rollout(T + extra, action=True)
    flat = {k: torch.full((2 * pad + (T + extra) * n,), PC.LOG_PROB_FILL, dtype=torch.int32, device=device).view(torch.float32)
            for k in ("log_prob",) + COLUMNS}
    flat["last_value"] = torch.full((2 * pad + n,), PC.LOG_PROB_FILL, dtype=torch.int32, device=device).view(torch.float32)
    for k, f in flat.items():
        full[k] = f[pad: f.numel() - pad].view((T + extra, n) if k != "last_value" else (n,))
    snap = eng.snapshot()
    out = launch(eng, pol, T, crit, out=full)
    assert out is full
    torch.cuda.synchronize()
    for k, f in flat.items():
        assert bool(PC.is_canary(f[:pad], PC.LOG_PROB_FILL).all()) and bool(PC.is_canary(f[-pad:], PC.LOG_PROB_FILL).all()), k
        if k != "last_value":
            assert bool(PC.is_canary(full[k][T:], PC.LOG_PROB_FILL).all()), f"{k}: a row >= T was written"
            assert not bool(PC.is_canary(full[k][:T], PC.LOG_PROB_FILL).any()), f"{k}: a slot of rows [0, T) is missing"
    assert not bool(PC.is_canary(full["last_value"], PC.LOG_PROB_FILL).any())
    check_columns(eng, pol, crit, snap, out, T)
    for k in COLUMNS + ("last_value",):
        with pytest.raises(ValueError, match=k):
            launch(eng, pol, T, crit, out={**full, k: full[k].double()})
    with pytest.raises(ValueError, match="value"):
        launch(eng, pol, T, crit, out={**full, "value": full["value"][:, :69]})


@pytest.mark.parametrize("mode", ["redraw", "first_state"])
def test_auto_reset_modes(device, mode):
    """case 4: both auto-reset modes give the same rule; bootstrap_truncated=False returns no boot_value and the other
    columns' bits (check_pinned)"""
    eng = BS.make_engine("halfcheetah", 7, 70, device, 71, autoreset_mode=mode)
    if mode == "first_state":
        eng.reset()  # (the first_state copy is taken by an explicit reset)
    pol = BS.make_policy(eng, (32,), "relu", 72, log_std=-0.3)
    crit = make_critic(eng, pol, (32,), "relu", 73)
    snap = eng.snapshot()
    out = launch(eng, pol, T, crit)
    after = PC.engine_state(eng)
    mask, _ = check_columns(eng, pol, crit, snap, out, T)
    assert mask.any()
    check_pinned(eng, pol, crit, snap, out, T, after)


def test_without_auto_reset(device):
    eng = BS.make_engine("halfcheetah", 7, 70, device, 75, auto_reset=False)
    pol = BS.make_policy(eng, (32,), "relu", 76, log_std=-0.3)
    crit = make_critic(eng, pol, (32,), "relu", 77)
    with pytest.raises(ValueError, match="bootstrap_truncated=False"):
        launch(eng, pol, T, crit)
    snap = eng.snapshot()
    out = launch(eng, pol, T, crit, bootstrap_truncated=False)
    check_columns(eng, pol, crit, snap, out, T, boot=False)


def test_goal_wrapper_env_front_end_and_on_device_critic(device):
    """case 4: the goal wrapper once (its terminations are the wrapper's), CARLBraxEnv.rollout_policy with the critic
    keywords, a critic from a Sequential, and an on_device critic"""
    from carl_amd.envs import CARLBraxAnt

    contexts = {k: {"target_distance": d, "target_direction": c, "target_radius": 0.3}
                for k, (d, c) in enumerate([(0.05, 112), (0.4, 334), (1.0, 1), (2.0, 32)])}
    env = CARLBraxAnt(batch_size=64, contexts=contexts, obs_context_features=["target_distance", "target_direction"],
                      device=device)
    env.reset(seed=3)
    eng = env.env
    assert eng.sys.goal_mode == 1
    rng = np.random.default_rng(3)
    pol = BraxMLPPolicy.for_env(env, BP.make_layers(rng, 2 + eng.D, (16,), eng.sys.n_act), "relu", log_std=-1.0)
    crit = BraxMLPPolicy.for_env(env, BP.make_layers(rng, 2 + eng.D, (16,), 1), "relu", head="value")
    snap = eng.snapshot()
    out = env.rollout_policy(pol, 5, deterministic=False, sample_seed=BS.SEED, value_net=crit)
    ref_success = out["success"].clone()
    _, ref = check_columns(eng, pol, crit, snap, out, 5)
    same_bits(ref_success, ref["success"], "success")

    env = CARLBraxAnt(batch_size=64, obs_context_features=["gravity", "friction"], device=device)
    env.reset(seed=4)
    pol = BraxMLPPolicy.from_sequential(env, torch.nn.Sequential(torch.nn.Linear(29, 16), torch.nn.Tanh(),
                                                                 torch.nn.Linear(16, 8)), log_std=np.full(8, -0.7))
    crit = BraxMLPPolicy.from_sequential(env, torch.nn.Sequential(torch.nn.Linear(29, 16), torch.nn.ReLU(),
                                                                  torch.nn.Linear(16, 1)), head="value")
    assert crit.head == "value" and crit.n_out == 1
    eng = env.env
    snap = eng.snapshot()
    out = env.rollout_policy(pol, 4, deterministic=False, sample_seed=BS.SEED, value_net=crit)
    assert "log_prob" in out and tuple(out["value"].shape) == (4, 64) and tuple(out["last_value"].shape) == (64,)
    check_columns(eng, pol, crit, snap, out, 4)
    eng.restore(snap)
    nb = env.rollout_policy(pol, 4, deterministic=False, sample_seed=BS.SEED, value_net=crit, bootstrap_truncated=False)
    assert "boot_value" not in nb
    same_bits(nb["value"], out["value"], "value")
    same_bits(nb["last_value"], out["last_value"], "last_value")
    # an on_device critic: the caller's block, never copied
    dev = BraxMLPPolicy.on_device(crit, crit.device_params(device).clone(), 256)
    assert dev.log_std.shape == (1, 0)
    with pytest.raises(ValueError, match="one set layout for both"):  # (the actor's one set covers every lane)
        env.rollout_policy(pol, 4, deterministic=False, sample_seed=BS.SEED, value_net=dev)
    actor = BraxMLPPolicy.on_device(pol, pol.device_params(device).clone(), 256, log_std=torch.full((1, 8), -0.7, device=device))
    eng.restore(snap)
    twin = env.rollout_policy(actor, 4, deterministic=False, sample_seed=BS.SEED, value_net=dev)
    for k in COLUMNS + ("last_value",):
        same_bits(twin[k], out[k], k)


@pytest.mark.parametrize("boot", [True, False])
def test_gae_from_the_launch(device, boot):
    """case 5: gae=(0.99, 0.95): advantage and return equal value_cases.gae_ref of the launch's own columns exactly"""
    steps, n = 8, 70
    eng = BS.make_engine("hopper", 4, n, device, 81, max_episode_steps=3)
    pol = BS.make_policy(eng, (32,), "relu", 82, log_std=-0.5)
    crit = make_critic(eng, pol, (32,), "tanh", 83)
    out = launch(eng, pol, steps, crit, gae=(0.99, 0.95), bootstrap_truncated=boot)
    assert ("boot_value" in out) == boot
    h = {k: v.cpu().numpy() for k, v in out.items()}
    assert h["truncated"].any() and not h["truncated"].all()
    a, r = VC.gae_ref(h["reward"], h["value"], h["terminated"], h["truncated"], h["last_value"], 0.99, 0.95,
                      boot_value=h["boot_value"] if boot else None)
    np.testing.assert_array_equal(h["advantage"].view(np.int32), a.view(np.int32))
    np.testing.assert_array_equal(h["return"].view(np.int32), r.view(np.int32))
    with pytest.raises(ValueError, match="needs value_net"):
        launch(eng, pol, steps, gae=(0.99, 0.95))
