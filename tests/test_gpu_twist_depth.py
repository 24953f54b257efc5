"""SN_OPT_TWIST_DEPTH: the twist-ahead's refill hysteresis (a refilling game
twists depth extra MT19937 rounds, chained in LDS; the start-up twist
staggers the games) changes when words are twisted, never which: every
depth gives the games, outputs and exported numpy states of depth 0 and of
the CPU oracle, bit for bit.
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

B = 67  # a partial twist block (4 games per block) and a partial decode wave
SEED = 11
SHAPES = {"n4": (4, 104, 400), "n3c40": (3, 40, 800), "n10": (10, 104, 200)}


def _plan(steps):
    """25 / 1 / 7 / 3 / 30 (launches that start mid-episode and cross deals), then tens"""
    plan = [25, 1, 7, 3, 30]
    left = steps - sum(plan)
    return plan + [10] * (left // 10) + ([left % 10] if left % 10 else [])


def _np_form(key, pos):
    """(key, pos) with a pending twist applied, so equal streams compare equal."""
    key = np.array(key, dtype=np.uint32)
    if pos < 624:
        return key, pos
    rs = np.random.RandomState()
    rs.set_state(("MT19937", key, 624, 0, 0.0))
    rs.randint(0, 2**32, size=1, dtype=np.uint64)  # forces the twist, consumes word 0
    k2, p2 = rs.get_state()[1:3]
    return np.array(k2, dtype=np.uint32), p2 - 1


def _ref_states(ref, n):
    rngs = ref.v.contents.rngs
    return [_np_form(np.frombuffer(bytes(rngs[g].mt), dtype=np.uint32), rngs[g].pos) for g in range(n)]


def _pad_hands(hands, N):
    out = np.full((len(hands), N, 10), -1, dtype=np.int8)
    for g, hs in enumerate(hands):
        for p, h in enumerate(hs):
            out[g, p, : len(h)] = h
    return out


# Per-step observations of a 10-player handle do not fit the pipelined
# k_play's LDS (the rollout would leave the ring path this test is about), so
# that shape compares the observation after the last step instead.
def _step_obs(N):
    return N <= 4


@functools.lru_cache(maxsize=None)
def _oracle(shape):
    N, C, steps = SHAPES[shape]
    ref = O.VecOracle(B, N, C, rng_mode=O.RNG_NUMPY_MT, seed=SEED)
    ref.reset()
    rr, rd, ra, ro = ref.rollout(steps, want_obs=_step_obs(N))
    out = {"rewards": rr, "done": rd, "actions": ra, "obs": ro if _step_obs(N) else ref.obs(),
           "sums": ref.sum_results(), "eps": ref.episodes(), "hands": _pad_hands(ref.hands(), N)}
    for g, (k, p) in enumerate(_ref_states(ref, B)):
        out[f"mt{g}"] = np.append(k, np.uint32(p))
    return out


@functools.lru_cache(maxsize=None)
def _device(shape, depth, dec):
    from rl_6_nimmt.vec_env import VecSechsNimmtEnv

    N, C, steps = SHAPES[shape]
    env = VecSechsNimmtEnv(B, N, C, seed=SEED, rng="numpy")
    env.set_option(twist_depth=depth, pipe_dec=dec)
    env.reset()
    parts = []
    for T in _plan(steps):
        o = env.rollout(T, want_actions=True, want_obs=_step_obs(N))
        parts.append({k: v.cpu().numpy() for k, v in o.items()})
    out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    if _step_obs(N):
        out["obs"] = out["obs"][..., :47]
    else:
        out["obs"] = env.obs().cpu().numpy()
    s, e = env.results()
    out.update(sums=s.cpu().numpy(), eps=e.cpu().numpy(), hands=env.hands().cpu().numpy())
    for g in range(B):
        k, p = _np_form(*env.get_mt_state(g))
        out[f"mt{g}"] = np.append(k, np.uint32(p))
    out["pipe_errors"] = env.pipe_errors()
    env.close()
    return out


@pytest.mark.parametrize("dec", [1, 0])
@pytest.mark.parametrize("depth", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_depth_plays_the_same_games(shape, depth, dec):
    """67 games, launch plan 25 / 1 / 7 / 3 / 30 then tens, with decode-ahead
    and with k_play drawing from the ring itself: 400 steps of 4 players (at
    depth 3 a game refills about every 13 episodes: three refills or more),
    800 steps of 3 players with 40 cards, 200 steps of 10 players (the ring
    path at 5-step launches).  Actions, rewards, done flags, observations,
    results(), hands() and every game's exported numpy MT19937 state equal
    depth 0's and the oracle's; no draw ran past the twisted words."""
    got, base, ref = _device(shape, depth, dec), _device(shape, 0, dec), _oracle(shape)
    assert got["pipe_errors"] == 0
    assert set(got) == set(ref) | {"pipe_errors"}
    for k in ref:
        assert np.array_equal(got[k], base[k]), (k, "depth 0")
        assert np.array_equal(got[k], ref[k]), (k, "oracle")


@pytest.mark.parametrize("K,dec", [(4, 1), (5, 1), (5, 0)])
def test_export_at_the_deepest_run_ahead(K, dec):
    """Depth 3 with K = 4 and K = 5 (the largest lead: the start-up twist runs
    up to 600 (K + 1) + 3 x 624 + 623 words ahead), 60 launches alternating 1
    and 10 steps, every game's numpy state exported after every launch:
    k_pipe_code untwists the most rounds the mt0 bound allows, and the
    pipeline restarts -- staggered start-up twist, first decode -- after each
    export.  Every state, action and reward equals the oracle's."""
    from rl_6_nimmt.vec_env import VecSechsNimmtEnv

    n, N = 16, 4
    env = VecSechsNimmtEnv(n, N, seed=SEED, rng="numpy")
    env.set_option(twist_depth=3, twist_every=K, pipe_dec=dec)
    env.reset()
    ref = O.VecOracle(n, N, rng_mode=O.RNG_NUMPY_MT, seed=SEED)
    ref.reset()
    for i in range(60):
        T = 1 if i % 2 == 0 else 10
        out = env.rollout(T, want_actions=True)
        rr, rd, ra, _ = ref.rollout(T)
        assert np.array_equal(out["actions"].cpu().numpy(), ra), i
        assert np.array_equal(out["rewards"].cpu().numpy(), rr), i
        for g, (rk, rp) in enumerate(_ref_states(ref, n)):
            k, p = _np_form(*env.get_mt_state(g))
            assert p == rp and np.array_equal(k, rk), (i, g)
    assert env.pipe_errors() == 0
    env.close()


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
for dec in (1, 0):
    env = VecSechsNimmtEnv(67, 4, seed=11, rng="numpy")
    env.set_option(twist_depth=3, pipe_dec=dec)
    env.reset()
    for T in plan:
        env.rollout(T, want_actions=True, want_obs=True)
    for g in (0, 1, 2, 3, 66):
        env.get_mt_state(g)
    assert env.pipe_errors() == 0
    env.close()
torch.cuda.synchronize()
nat.check(L.sn_debug_failures(ctypes.byref(cnt), ctypes.byref(line), 0), "failures")
print("debug failures", cnt.value, "first line", line.value)
assert cnt.value == 0, (cnt.value, line.value)
"""


def test_debug_library_span_assertions_hold_at_depth_3():
    """libsechs_debug.so (SN_DASSERT live: the self-test's deliberate failure
    is counted) plays the 4-player plan above at depth 3, with and without
    decode-ahead, and exports states: k_mt_ahead's span assertions (the
    twisted end within kPipeSpanMax of its consumer, a refill reaching its
    high threshold on a round boundary, the crossings within mt0) and
    k_pipe_code's (every round undone) count no failure."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "rl-6-nimmt_amd", "libsechs_debug.so")
    assert os.path.exists(lib), "make -C rl-6-nimmt_amd libsechs_debug.so"
    envv = dict(os.environ, SECHS_LIB=lib)
    plan = ",".join(str(t) for t in _plan(SHAPES["n4"][2]))
    r = subprocess.run([sys.executable, "-c", _DEBUG_WORKLOAD, os.path.join(root, "rl-6-nimmt_amd"), plan], env=envv,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "debug failures 0" in r.stdout
