"""Compile the HIP engine for gfx950 with hipcc (in-tree, no JIT cache).

``python -m carl_amd.build`` -> carl_amd/lib/libcarl_amd.so.  hipcc cross-compiles
without a GPU, so this also runs in the build container.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_DIR = os.path.join(_HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libcarl_amd.so")
ARCH = "gfx950"

# translation unit -> extra compile flags.  No SLP vectorizer in either unit: carl_brax.hip -- see its header comment;
# carl_amd.hip (r04, tools/ab_probe.sh, interleaved builds on one box): with it the Acrobot + MountainCar pair launch
# is 3.5 % slower at 65 536 lanes per family and 2.5 % at 8 192, CartPole at 8 192 lanes 2 % slower, and the one
# packing that paid (Pendulum's sine / cosine polynomials) is written out by hand in fast_math.hip.h: sincos_fast_pk.
# carl_policy.hip (the closed-loop rollout) and carl_policy_sample.hip (its sampled twins) instantiate the same device
# templates as carl_amd.hip, and so does carl_policy_value.hip (the rollout with a critic, and GAE): same flags.
# carl_es.hip (evolution strategies: perturb / gradient) shares Philox with them and takes the same flags.
# carl_policy_stats.hip (the episodes launch gathering input statistics, and their merge) instantiates the episodes body
# once more: same flags.
# carl_brax_policy.hip (the Brax closed-loop rollout) instantiates carl_brax.hip's device templates in another mode: its flags.
# carl_brax_episodes.hip (the episodes mode of that rollout) instantiates the same mode's episodes variant: the same flags.
# carl_brax_policy_stats.hip (that mode gathering input statistics) instantiates the episodes variant once more: its flags.
# carl_brax_policy_sample.hip (the sampled twin of carl_brax_policy.hip's rollout) instantiates that mode's sampled variant: its flags.
# carl_brax_policy_value.hip (the sampled rollout with a critic) instantiates the sampled variant's valued variant: its flags.
# (The five closed-loop units expand one list of instances and share one host launch path: csrc/brax_policy_host.hpp.)
# carl_ppo.hip (the PPO update: context trace, minibatch gradients) calls the closed-loop rollout's device functions: same flags.
# It holds the library's one trace walk and classic reduction, and the function that launches the trace.
# carl_brax_ppo.hip (that update for the Brax families) calls the same device helpers (csrc/ppo_device.hip.h) in its actor
# kernel and its reduction, instantiates the network kernel (csrc/ppo_net_kernel.hip.h) for its critic and runs the trace
# through carl_ppo.hip's launch function: same flags.  (The two PPO units share one host path: csrc/ppo_host.hpp.)
# carl_ppo_norm.hip (PPO's running normalisation: input sums over a rollout buffer, return statistics) has kernels of its
# own (csrc/ppo_norm_kernels.hip.h) and instantiates none of another unit's: same flags.
# carl_ppo_step.hip (PPO's minibatch step: advantage statistics, global-norm clip and Adam) likewise has kernels of its own
# (csrc/ppo_step_kernels.hip.h): same flags.
# carl_ppo_sets.hip (a population of PPO learners: gradients, advantage statistics and Adam for several weight sets in one
# launch sequence) includes the bodies of the two PPO units' kernels textually (csrc/ppo_sets_kernels.hip.h) and
# instantiates none of their kernels: same flags.
SOURCES = {"carl_amd.hip": ["-fno-slp-vectorize"], "carl_brax.hip": ["-fno-slp-vectorize"],
           "carl_policy.hip": ["-fno-slp-vectorize"], "carl_policy_sample.hip": ["-fno-slp-vectorize"],
           "carl_policy_value.hip": ["-fno-slp-vectorize"], "carl_es.hip": ["-fno-slp-vectorize"],
           "carl_policy_stats.hip": ["-fno-slp-vectorize"], "carl_brax_policy.hip": ["-fno-slp-vectorize"],
           "carl_brax_episodes.hip": ["-fno-slp-vectorize"], "carl_brax_policy_stats.hip": ["-fno-slp-vectorize"],
           "carl_brax_policy_sample.hip": ["-fno-slp-vectorize"], "carl_brax_policy_value.hip": ["-fno-slp-vectorize"],
           "carl_ppo.hip": ["-fno-slp-vectorize"], "carl_brax_ppo.hip": ["-fno-slp-vectorize"],
           "carl_ppo_norm.hip": ["-fno-slp-vectorize"], "carl_ppo_step.hip": ["-fno-slp-vectorize"],
           "carl_ppo_sets.hip": ["-fno-slp-vectorize"]}


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC or install ROCm under /opt/rocm)")


def _deps() -> list[str]:
    out = []
    for root in (CSRC, os.path.join(os.path.dirname(_HERE), "include")):
        for f in sorted(os.listdir(root)):
            if f.endswith((".hip", ".h", ".hpp", ".inc")):
                out.append(os.path.join(root, f))
    return out


HASH_PATH = os.path.join(LIB_DIR, "build.sha256")


def _source_hash(extra_flags: list[str] | None = None) -> str:
    """Content hash of every source / header and of the flags.  File times do not survive a copy
    of the tree (the GPU boxes receive a snapshot), so staleness is decided on content."""
    import hashlib

    h = hashlib.sha256()
    root = os.path.dirname(_HERE)
    for d in _deps():
        h.update(os.path.relpath(d, root).encode())
        with open(d, "rb") as f:
            h.update(f.read())
    h.update(repr(sorted(SOURCES.items())).encode())
    h.update(repr(extra_flags or []).encode())
    return h.hexdigest()


def needs_build(extra_flags: list[str] | None = None) -> bool:
    if not os.path.exists(LIB_PATH) or not os.path.exists(HASH_PATH):
        return True
    with open(HASH_PATH) as f:
        return f.read().strip() != _source_hash(extra_flags)


def _refuse_ablation(extra_flags: list[str] | None) -> None:
    """The profiling-only switches of rounds 1-3 (CARL_EXP_*: kernels that skip stores / the done path) no longer
    exist in the sources (removed in round 4; commit 3a3c7b2 still builds them): a flag that names one is a mistake."""
    bad = [f for f in (extra_flags or []) if "CARL_EXP_" in f or "CARL_ABLATION" in f or "CARL_STORERS" in f]
    if bad:
        raise ValueError(f"{bad}: the CARL_EXP_* / CARL_STORERS ablation switches were removed from the sources in round 4")


def build(force: bool = False, verbose: bool = False, extra_flags: list[str] | None = None) -> str:
    _refuse_ablation(extra_flags)
    path = _build_product(force, verbose, extra_flags)
    if not extra_flags:  # (an experiment's flags are the product's alone)
        # the test library follows the headers and its own source: rebuilt by content hash whether or not the product was
        build_probe(force=force, verbose=verbose)
    return path


def _build_product(force: bool, verbose: bool, extra_flags: list[str] | None) -> str:
    if not force and not needs_build(extra_flags):
        return LIB_PATH
    import fcntl

    os.makedirs(LIB_DIR, exist_ok=True)
    # one builder at a time: the ranks of a multi-GPU launch import the package simultaneously
    with open(os.path.join(LIB_DIR, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and not needs_build(extra_flags):  # another process built it while we waited
            return LIB_PATH
        return _build_locked(verbose, extra_flags)


def _build_locked(verbose: bool, extra_flags: list[str] | None) -> str:
    obj_dir = os.path.join(LIB_DIR, "obj")
    os.makedirs(obj_dir, exist_ok=True)
    common = [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function",
              *(extra_flags or [])]
    procs, objs = [], []
    for src, flags in SOURCES.items():  # the translation units compile side by side
        obj = os.path.join(obj_dir, src.replace(".hip", ".o"))
        cmd = [_hipcc(), *common, *flags, "-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((cmd, subprocess.Popen(cmd)))
        objs.append(obj)
    for cmd, p in procs:
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, cmd)
    tmp = LIB_PATH + f".tmp{os.getpid()}"
    link = [_hipcc(), f"--offload-arch={ARCH}", "-shared", "-fPIC", "-fno-gpu-rdc", *objs, "-o", tmp]
    if verbose:
        print(" ".join(link), flush=True)
    subprocess.run(link, check=True)
    os.replace(tmp, LIB_PATH)  # atomic: a concurrent loader never maps a half-written file
    with open(HASH_PATH, "w") as f:
        f.write(_source_hash(extra_flags) + "\n")
    return LIB_PATH


# ---- the math probe: a TEST library (tests/probe/math_probe.hip: one trivial kernel per device math primitive of
# fast_math.hip.h / classic_control.hip.h / brax_kernels.hip.h, for tests/test_gpu_math_primitives.py).  A shared object
# of its own beside the product's, same common flags, same content-hash staleness rule; NOT in SOURCES, never linked
# into libcarl_amd.so.  One translation unit, compiled and linked in one hipcc call (no object file is kept).
PROBE_SRC = os.path.join(os.path.dirname(_HERE), "tests", "probe", "math_probe.hip")
PROBE_LIB_PATH = os.path.join(LIB_DIR, "libcarl_math_probe.so")
PROBE_HASH_PATH = os.path.join(LIB_DIR, "math_probe.sha256")
PROBE_FLAGS = ["-fno-slp-vectorize"]


def _probe_hash() -> str:
    import hashlib

    h = hashlib.sha256(_source_hash().encode())
    with open(PROBE_SRC, "rb") as f:
        h.update(f.read())
    h.update(repr(PROBE_FLAGS).encode())
    return h.hexdigest()


def probe_needs_build() -> bool:
    if not os.path.exists(PROBE_LIB_PATH) or not os.path.exists(PROBE_HASH_PATH):
        return True
    with open(PROBE_HASH_PATH) as f:
        return f.read().strip() != _probe_hash()


def build_probe(force: bool = False, verbose: bool = False) -> str | None:
    """libcarl_math_probe.so; None where the tree has no tests/ (an installed package)."""
    if not os.path.exists(PROBE_SRC):
        return None
    if not force and not probe_needs_build():
        return PROBE_LIB_PATH
    import fcntl

    os.makedirs(LIB_DIR, exist_ok=True)
    with open(os.path.join(LIB_DIR, ".probe.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and not probe_needs_build():
            return PROBE_LIB_PATH
        tmp = PROBE_LIB_PATH + f".tmp{os.getpid()}"
        cmd = [_hipcc(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wall",
               "-Wno-unused-function", *PROBE_FLAGS, "-shared", f"-I{CSRC}", PROBE_SRC, "-o", tmp]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
        os.replace(tmp, PROBE_LIB_PATH)
        with open(PROBE_HASH_PATH, "w") as f:
            f.write(_probe_hash() + "\n")
    return PROBE_LIB_PATH


if __name__ == "__main__":
    flags = [a for a in sys.argv[1:] if a.startswith("-") and a not in ("--force",)]
    print(build(force=True, verbose=True, extra_flags=flags))
