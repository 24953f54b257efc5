"""SN_OPT_PLAY_GROUP: on the decode-ahead path one k_play launch plays all
the consecutive 10-step chunks of a call that lie in one twist group, moving
from episode record to episode record at every deal.  It changes how many
launches play a rollout, never what they play: actions, rewards, done flags,
observations, scores, results and every exported numpy MT19937 state equal
the one-launch-per-chunk form's and the CPU oracle's, bit for bit.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

SEED = 23
# 200 games of 4 players: three full waves and one of 8 live lanes
SHAPES = {"n4": (200, 4), "n2": (130, 2), "n3": (130, 3)}
# fused launches that start mid-group (after the 25, the 7, the 3, ...) and mid-episode (all
# but the first), that hold one to four deals (K = 4: steps 129 .. 169 hold four), and one
# that ends exactly on a deal (the first 40)
PLAN = (40, 25, 7, 3, 30, 10, 1, 13, 40, 20)


def _sample(B):
    return sorted(set(range(0, B, 17)) | {63, 64, B - 1})


def _np_form(key, pos):
    """(key, pos) with a pending twist applied, so equal streams compare equal."""
    key = np.array(key, dtype=np.uint32)
    if pos < 624:
        return np.append(key, np.uint32(pos))
    rs = np.random.RandomState()
    rs.set_state(("MT19937", key, 624, 0, 0.0))
    rs.randint(0, 2**32, size=1, dtype=np.uint64)  # forces the twist, consumes word 0
    k2, p2 = rs.get_state()[1:3]
    return np.append(np.array(k2, dtype=np.uint32), np.uint32(p2 - 1))


@functools.lru_cache(maxsize=None)
def _oracle(shape, plan=PLAN, summ=True):
    """outputs of the whole plan, and the sampled games' numpy states after every call"""
    B, N = SHAPES[shape]
    ref = O.VecOracle(B, N, rng_mode=O.RNG_NUMPY_MT, seed=SEED)
    ref.reset()
    parts, out = [], {}
    for i, T in enumerate(plan):
        parts.append(ref.rollout(T, include_summaries=summ, want_obs=True))
        rngs = ref.v.contents.rngs
        for g in _sample(B):
            out[f"mt{i}_{g}"] = _np_form(np.frombuffer(bytes(rngs[g].mt), dtype=np.uint32), rngs[g].pos)
    for j, k in enumerate(("rewards", "done", "actions", "obs")):
        out[k] = np.concatenate([p[j] for p in parts])
    out.update(scores=ref.scores(), sums=ref.sum_results(), eps=ref.episodes())
    return out


@functools.lru_cache(maxsize=None)
def _device(shape, group, K, export_each=False, plan=PLAN, want_obs=True, summ=True):
    """the plan on the device; numpy states of the sampled games after every call
    (export_each: each export syncs and restarts the pipeline) or after the last"""
    from rl_6_nimmt.vec_env import VecSechsNimmtEnv

    B, N = SHAPES[shape]
    env = VecSechsNimmtEnv(B, N, seed=SEED, rng="numpy", include_summaries=summ)
    env.set_option(play_group=group, twist_every=K)
    env.reset()
    env.time_kernels(64)
    parts, out = [], {}
    for i, T in enumerate(plan):
        o = env.rollout(T, want_actions=True, want_obs=want_obs)
        parts.append({k: v.cpu().numpy() for k, v in o.items()})
        if export_each or i == len(plan) - 1:
            if i == len(plan) - 1:
                out["launches"] = env.kernel_times()[2]
            for g in _sample(B):
                out[f"mt{i}_{g}"] = _np_form(*env.get_mt_state(g))
    for k in parts[0]:
        out[k] = np.concatenate([p[k] for p in parts])
    if want_obs:
        out["obs"] = out["obs"][..., : O.obs_len(summ)]
    s, e = env.results()
    out.update(scores=env.scores().cpu().numpy(), sums=s.cpu().numpy(), eps=e.cpu().numpy())
    out["pipe_errors"] = env.pipe_errors()
    env.close()
    return out


def _launches(plan, K, group, chunk=10):
    """play launches of the plan from a fresh pipeline: a fused launch covers the call's
    chunks up to the end of the call or of the twist group of K chunks"""
    n = p = 0
    for T in plan:
        c = -(-T // chunk)
        while c:
            m = min(c, K - p % K) if group else 1
            n, p, c = n + 1, p + m, c - m
    return n


def _same(got, want, tag):
    assert got["pipe_errors"] == 0
    keys = [k for k in got if k not in ("pipe_errors", "launches")]
    assert {"rewards", "done", "actions", "scores", "sums", "eps"} <= set(keys)
    assert any(k.startswith("mt") for k in keys)
    for k in keys:
        assert k in want, (tag, k)
        assert got[k].shape == np.shape(want[k]) and np.array_equal(got[k], want[k]), (tag, k)


@pytest.mark.parametrize("shape,K", [("n4", 4), ("n4", 1), ("n4", 5), ("n2", 4), ("n3", 4)])
def test_one_launch_per_group_plays_the_same_games(shape, K):
    """189 steps in calls of 40 / 25 / 7 / 3 / 30 / 10 / 1 / 13 / 40 / 20, groups of
    K = 4, 1, 5 chunks: the fused form, the one-launch-per-chunk form and the oracle
    give the same actions, rewards, done flags, int8 observations of every step, the
    same scores, results and final numpy states, and no draw overran.  The fused form
    issues the launches the chunk arithmetic says (K = 1: as many as unfused)."""
    fused, chunks, ref = _device(shape, 1, K), _device(shape, 0, K), _oracle(shape)
    _same(fused, chunks, "chunks")
    _same(chunks, ref, "oracle")
    _same(fused, ref, "oracle")
    assert chunks["launches"] == _launches(PLAN, K, 0) == 22  # the plan's 10-step chunks
    assert fused["launches"] == _launches(PLAN, K, 1)
    assert _launches(PLAN, 1, 1) == 22 and _launches(PLAN, 4, 1) == 10 and _launches(PLAN, 5, 1) == 13


@pytest.mark.parametrize("shape", ["n4", "n3"])
def test_states_exported_after_every_call(shape):
    """the same plan with the sampled games' numpy states exported after every call:
    each export syncs the pipeline, which restarts at the games' step within their
    episode (phi0 > 0), so every fused launch starts a group mid-episode"""
    fused, chunks, ref = _device(shape, 1, 4, True), _device(shape, 0, 4, True), _oracle(shape)
    assert sum(k.startswith("mt") for k in fused) == len(PLAN) * len(_sample(SHAPES[shape][0]))
    _same(fused, chunks, "chunks")
    _same(fused, ref, "oracle")


def test_export_between_two_whole_group_calls():
    """40 steps, an export (pipeline sync and restart), 40 steps: two launches of four deals"""
    plan = (40, 40)
    fused, chunks, ref = _device("n4", 1, 4, True, plan), _device("n4", 0, 4, True, plan), _oracle("n4", plan)
    _same(fused, chunks, "chunks")
    _same(fused, ref, "oracle")
    assert fused["launches"] == 2 and chunks["launches"] == 8


def test_without_observations_and_without_summaries():
    """obs = NULL (no staging area in LDS), and 35-byte rows (SN_NO_SUMMARIES)"""
    ref = _oracle("n4")
    fused, chunks = _device("n4", 1, 4, want_obs=False), _device("n4", 0, 4, want_obs=False)
    assert "obs" not in fused
    _same(fused, chunks, "chunks")
    _same(fused, ref, "oracle")
    ref = _oracle("n4", summ=False)
    fused, chunks = _device("n4", 1, 4, summ=False), _device("n4", 0, 4, summ=False)
    assert fused["obs"].shape[-1] == 35
    _same(fused, chunks, "chunks")
    _same(fused, ref, "oracle")


_DEBUG_WORKLOAD = r"""
import ctypes, sys, torch
sys.path.insert(0, sys.argv[1])
from rl_6_nimmt import _native as nat
from rl_6_nimmt.vec_env import VecSechsNimmtEnv
L = nat.lib()
cnt, line = ctypes.c_uint32(), ctypes.c_uint32()
nat.check(L.sn_debug_failures(ctypes.byref(cnt), ctypes.byref(line), 1), "selftest")
assert cnt.value == 1, cnt.value  # the deliberately failing check was counted
plan = [int(t) for t in sys.argv[2].split(",")]
for K in (4, 5):
    env = VecSechsNimmtEnv(200, 4, seed=23, rng="numpy")
    env.set_option(play_group=1, twist_every=K)
    env.reset()
    for T in plan:
        env.rollout(T, want_actions=True, want_obs=True)
    for g in (0, 63, 64, 199):
        env.get_mt_state(g)
    assert env.pipe_errors() == 0
    env.close()
torch.cuda.synchronize()
nat.check(L.sn_debug_failures(ctypes.byref(cnt), ctypes.byref(line), 0), "failures")
print("debug failures", cnt.value, "first line", line.value)
assert cnt.value == 0, (cnt.value, line.value)
"""


def test_debug_library_assertions_hold_on_multi_episode_launches():
    """libsechs_debug.so (SN_DASSERT live: the self-test's deliberate failure is
    counted) plays the plan with fused launches, K = 4 and 5: the step loop's checks
    (every drawn index within the hand, the step within the record's episode) count
    no failure on launches of up to five deals"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "rl-6-nimmt_amd", "libsechs_debug.so")
    assert os.path.exists(lib), "make -C rl-6-nimmt_amd libsechs_debug.so"
    envv = dict(os.environ, SECHS_LIB=lib)
    plan = ",".join(str(t) for t in PLAN + (50, 50))
    r = subprocess.run([sys.executable, "-c", _DEBUG_WORKLOAD, os.path.join(root, "rl-6-nimmt_amd"), plan], env=envv,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "debug failures 0" in r.stdout
