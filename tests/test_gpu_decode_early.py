"""SN_OPT_DEC_EARLY: k_decode touches the next episode's ring window (one dword of each ring
chunk it spans) as soon as the window's position is known, so that the window's own loads hit
L2.  It changes when lines travel, never what is decoded: the episode records and the
decoder's position slots are the same word for word with and without the touches, overruns
are counted alike, and the outputs and every exported numpy MT19937 state equal the CPU
oracle's.  (The issue priorities and the loads-before-stores form measured beside it were not
kept, DESIGN.md section 4, so there is nothing of them to test.)
"""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

B = 67  # one full decoder wave and one of three live lanes
SEED = 5
# starts mid-episode (all but the first call) and crosses deals; the export after the third
# call syncs the pipeline, which restarts at step 3 of an episode (phi0 = 3)
PLAN = (25, 1, 7, 3, 30, 10, 40)
EXPORT_AFTER = 2
# (players, cards): 104 cards and the smallest deck, 10 N + 4
SHAPES = [(4, 104), (4, 44), (2, 104), (2, 24)]
SAMPLE = (0, 17, 63, 64, B - 1)
REC_SLOTS, REC_QUADS, DEC_SLOTS = 16, 6, (8, 9)  # kDecRecords, kDecQuads, kDecSlot + (0, 1)
FORMS = (1,)  # dec_early under test; 0 is the decoder without touches
EARLY = FORMS[-1]


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


def _pipe_words(env):
    """all 16 record slots and the decoder's two position slots, as the device holds them now"""
    from rl_6_nimmt import _native as nat

    n = env.num_games
    rec = np.zeros((REC_SLOTS, REC_QUADS, n, 4), dtype=np.uint32)
    for s in range(REC_SLOTS):
        nat.check(nat.lib().sn_debug_pipe_words(env._h, 2, s, rec[s].ctypes.data_as(ctypes.c_void_p)), "records")
    pos = np.zeros((len(DEC_SLOTS), n), dtype=np.uint32)
    for i, s in enumerate(DEC_SLOTS):
        nat.check(nat.lib().sn_debug_pipe_words(env._h, 0, s, pos[i].ctypes.data_as(ctypes.c_void_p)), "pabsc")
    return rec, pos


@functools.lru_cache(maxsize=None)
def _oracle(N, C, plan=PLAN, export_after=EXPORT_AFTER):
    ref = O.VecOracle(B, N, C, rng_mode=O.RNG_NUMPY_MT, seed=SEED)
    ref.reset()
    parts, out = [], {}
    for i, T in enumerate(plan):
        parts.append(ref.rollout(T, want_obs=True))
        if i == export_after or i == len(plan) - 1:
            rngs = ref.v.contents.rngs
            for g in SAMPLE:
                out[f"mt{i}_{g}"] = _np_form(np.frombuffer(bytes(rngs[g].mt), dtype=np.uint32), rngs[g].pos)
    for j, k in enumerate(("rewards", "done", "actions", "obs")):
        out[k] = np.concatenate([p[j] for p in parts])
    out["scores"] = ref.scores()
    return out


@functools.lru_cache(maxsize=None)
def _device(N, C, K, early, plan=PLAN, export_after=EXPORT_AFTER):
    """the plan on the device: outputs, exported states, and the pipeline words after every call"""
    from rl_6_nimmt.vec_env import VecSechsNimmtEnv

    env = VecSechsNimmtEnv(B, N, C, seed=SEED, rng="numpy")
    env.set_option(dec_early=early, twist_every=K)
    env.reset()
    parts, out, words = [], {}, []
    for i, T in enumerate(plan):
        o = env.rollout(T, want_actions=True, want_obs=True)
        parts.append({k: v.cpu().numpy() for k, v in o.items()})
        words.append(_pipe_words(env))
        if i == export_after or i == len(plan) - 1:
            for g in SAMPLE:
                out[f"mt{i}_{g}"] = _np_form(*env.get_mt_state(g))
    for k in parts[0]:
        out[k] = np.concatenate([p[k] for p in parts])
    out["obs"] = out["obs"][..., : O.obs_len(True)]
    out["scores"] = env.scores().cpu().numpy()
    errors = env.pipe_errors()
    env.close()
    return out, words, errors


def _same_words(a, b):
    assert len(a) == len(b)
    written = 0
    for call, ((ra, pa), (rb, pb)) in enumerate(zip(a, b)):
        assert np.array_equal(ra, rb), ("records", call, np.argwhere(ra != rb)[:4].tolist())
        assert np.array_equal(pa, pb), ("decoder position", call)
        written += int(ra.any())
    assert written == len(a)  # the records were there to compare (decode-ahead ran)


def _same_outputs(got, want):
    assert set(got) == set(want) and any(k.startswith("mt") for k in got)
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


# ---- 1. records word for word ------------------------------------------------------------
@pytest.mark.parametrize("early", FORMS)
@pytest.mark.parametrize("K", [4, 1, 5])
@pytest.mark.parametrize("N,C", SHAPES)
def test_records_equal_the_late_form_and_outputs_the_oracle(N, C, K, early):
    """67 games, calls of 25 / 1 / 7 / 3 / 30 / 10 / 40 steps with an MT export after the
    third (the pipeline restarts mid-episode), twist groups of K = 4, 1, 5, N = 4 and 2 with
    104 cards and the smallest deck: after every call all 16 episode records and both decoder
    position slots of the touching form equal the other form's word for word, neither counted
    an overrun, and the touching form's actions, rewards, done flags, observations, scores and the
    numpy states of five games exported mid-rollout and at the end equal the oracle's."""
    (got, w1, e1), (_, w0, e0) = _device(N, C, K, early), _device(N, C, K, 0)
    assert e1 == 0 and e0 == 0
    _same_words(w1, w0)
    _same_outputs(got, _oracle(N, C))


# ---- 2. windows cut by the twisted end -----------------------------------------------------
# test knobs, as the overrun tests of tests/test_gpu_env.py set them: exact-lead twists beside
# every launch with a lead below two episodes' words, and the default schedule whose steady
# twists twist nothing (the start-up lead runs dry after about twelve episodes)
SHORT = {"lead96": dict(pipe_lead=96, twist_round=0, twist_every=1),
         "lead288": dict(pipe_lead=288, twist_round=0, twist_every=1),
         "twist_skip": dict(twist_skip=1)}


@functools.lru_cache(maxsize=None)
def _short_window(early, knobs, calls=30, steps=10):
    """(index of the call that raised, outputs of the calls before it, the pipeline words after
    every call up to and including it, the overrun count)"""
    from rl_6_nimmt._native import PipeOverrunError
    from rl_6_nimmt.vec_env import VecSechsNimmtEnv

    env = VecSechsNimmtEnv(B, 4, seed=SEED, rng="numpy")
    env.set_option(dec_early=early, **SHORT[knobs])
    env.reset()
    parts, words, raised = [], [], None
    for i in range(calls):
        try:
            o = env.rollout(steps, want_actions=True, want_obs=True, check=True)
        except PipeOverrunError:
            raised = i
            words.append(_pipe_words(env))
            break
        parts.append({k: v.cpu().numpy() for k, v in o.items()})
        words.append(_pipe_words(env))
    errors = env.pipe_errors()
    env.close()
    return raised, parts, words, errors


@pytest.mark.parametrize("early", FORMS)
@pytest.mark.parametrize("knobs", list(SHORT))
def test_window_cut_by_the_twisted_end(knobs, early):
    """The window is cut by the twisted end, so the touches reach ring chunks past it (and,
    once the decoder has overrun, chunks the twist never filled), and a draw then needs a word
    past the end.  Both forms raise
    PipeOverrunError on the same 10-step call, count the same number of overruns, their outputs
    until that call equal the oracle's, and their records and decoder positions are equal after
    every call, the raising one included: the touched bytes feed nothing and count nothing."""
    r1, p1, w1, e1 = _short_window(early, knobs)
    r0, p0, w0, e0 = _short_window(0, knobs)
    assert r1 is not None and r1 == r0
    assert (r1 > 0) == (knobs == "twist_skip")
    assert e1 > 0 and e1 == e0
    ref = O.VecOracle(B, 4, rng_mode=O.RNG_NUMPY_MT, seed=SEED)
    ref.reset()
    assert len(p1) == len(p0) == r1
    for a, b in zip(p1, p0):
        rr, rd, ra, ro = ref.rollout(10, want_obs=True)
        for got in (a, b):
            assert np.array_equal(got["rewards"], rr) and np.array_equal(got["done"], rd)
            assert np.array_equal(got["actions"], ra) and np.array_equal(got["obs"][..., : O.obs_len(True)], ro)
    assert len(w1) == len(w0) == r1 + 1
    for call, ((ra_, pa), (rb_, pb)) in enumerate(zip(w1, w0)):
        assert np.array_equal(ra_, rb_), ("records", call)
        assert np.array_equal(pa, pb), ("decoder position", call)


# ---- 3. dispatches of one episode, of K + 1 episodes and of none ---------------------------
# K = 1 with 10-step calls: the start-up decodes K + 1 = 2 episodes, every later dispatch one.
# K = 4 with 1-step calls: the start-up decodes 5 episodes and the first group's decode 4 more;
# the decode beside the fifth call finds them all decoded (ne == 0) and only moves the position
# to its slot.
ONE_EPISODE = dict(K=1, plan=(10,) * 6, export_after=3)
NO_EPISODE = dict(K=4, plan=(1,) * 13 + (10, 10), export_after=8)


@pytest.mark.parametrize("early", FORMS)
@pytest.mark.parametrize("case", ["one_episode", "no_episode"])
def test_dispatches_of_one_episode_and_of_none(case, early):
    """Records, positions, outputs and exported states as in the first test on plans whose
    decodes hold one episode (the last of its dispatch: nothing is touched) or none (the
    decoder loads nothing at all); after the empty dispatch both position slots hold the same
    position: it moved although nothing was decoded."""
    a = dict(ONE_EPISODE if case == "one_episode" else NO_EPISODE)
    K = a.pop("K")
    (got, w1, e1), (_, w0, e0) = _device(4, 104, K, early, **a), _device(4, 104, K, 0, **a)
    assert e1 == 0 and e0 == 0
    _same_words(w1, w0)
    _same_outputs(got, _oracle(4, 104, **a))
    if case == "no_episode":
        for words in (w1, w0):
            _, pos = words[4]  # the fifth call starts group 1: its decode has nothing left to decode
            assert pos.any() and np.array_equal(pos[0], pos[1])


def test_bad_option_values_are_refused():
    from rl_6_nimmt.vec_env import VecSechsNimmtEnv

    env = VecSechsNimmtEnv(B, 4, seed=SEED, rng="numpy")
    for bad in (-1, 2):
        with pytest.raises(ValueError):
            env.set_option(dec_early=bad)
    env.close()


# ---- 4. the debug library ------------------------------------------------------------------
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
for early in (int(sys.argv[3]), 0):
    for K in (4, 1, 5):
        env = VecSechsNimmtEnv(67, 4, seed=5, rng="numpy")
        env.set_option(dec_early=early, twist_every=K)
        env.reset()
        for i, T in enumerate(plan):
            env.rollout(T, want_actions=True, want_obs=True)
            if i == 2:
                env.get_mt_state(17)
        for g in (0, 63, 64, 66):
            env.get_mt_state(g)
        assert env.pipe_errors() == 0
        env.close()
torch.cuda.synchronize()
nat.check(L.sn_debug_failures(ctypes.byref(cnt), ctypes.byref(line), 0), "failures")
print("debug failures", cnt.value, "first line", line.value)
assert cnt.value == 0, (cnt.value, line.value)
"""


def test_debug_library_assertions_hold():
    """libsechs_debug.so (SN_DASSERT live: the self-test's deliberate failure is counted) plays
    the first test's N = 4 plan in both forms, K = 4, 1, 5, with the export mid-rollout: no
    invariant check of the decoder, the play loop or the twist counts a failure."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "rl-6-nimmt_amd", "libsechs_debug.so")
    assert os.path.exists(lib), "make -C rl-6-nimmt_amd libsechs_debug.so"
    envv = dict(os.environ, SECHS_LIB=lib)
    plan = ",".join(str(t) for t in PLAN)
    r = subprocess.run([sys.executable, "-c", _DEBUG_WORKLOAD, os.path.join(root, "rl-6-nimmt_amd"), plan, str(EARLY)],
                       env=envv, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "debug failures 0" in r.stdout
