"""SN_OPT_DEC_WALK: k_decode reads the DrunkHamster draws of a step from its LDS
window by stream position (walk_draws=1, the default) instead of through the
byte buffer (walk_draws=0).  It changes how the decoder finds the words, never
which: the episode records (start, the ten u16 offsets, the nibble draws, rows
and hands) and the decoder's position slots are the same word for word, so the
outputs and every exported numpy MT19937 state equal the CPU oracle's.
"""
import ctypes
import functools

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
# (players, cards): a deck holds at least 10 N + 4 cards, so at N = 4 the small deck is 44
SHAPES = [(4, 104), (4, 44), (3, 104), (3, 40), (2, 104), (2, 40), (1, 104), (1, 40)]
SAMPLE = (0, 17, 63, 64, B - 1)
REC_SLOTS, REC_QUADS, DEC_SLOTS = 16, 6, (8, 9)  # kDecRecords, kDecQuads, kDecSlot + (0, 1)


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
def _oracle(N, C, plan=PLAN, seed=SEED, offset=0, export_after=EXPORT_AFTER):
    ref = O.VecOracle(B, N, C, rng_mode=O.RNG_NUMPY_MT, seed=seed, game_offset=offset)
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
def _device(N, C, K, walk, plan=PLAN, seed=SEED, offset=0, export_after=EXPORT_AFTER):
    """the plan on the device: outputs, exported states, and the pipeline words after every call"""
    from rl_6_nimmt.vec_env import VecSechsNimmtEnv

    env = VecSechsNimmtEnv(B, N, C, seed=seed, game_offset=offset, rng="numpy")
    env.set_option(walk_draws=walk, twist_every=K)
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


@pytest.mark.parametrize("K", [4, 1, 5])
@pytest.mark.parametrize("N,C", SHAPES)
def test_records_equal_the_byte_buffer_form(N, C, K):
    """67 games, calls of 25 / 1 / 7 / 3 / 30 / 10 / 40 steps with an MT export after the
    third, twist groups of K = 4, 1, 5: after every call all 16 episode records and both
    decoder position slots of the walking form equal the byte-buffer form's word for word,
    and neither form counted an overrun."""
    (_, w1, e1), (_, w0, e0) = _device(N, C, K, 1), _device(N, C, K, 0)
    assert e1 == 0 and e0 == 0
    _same_words(w1, w0)


@pytest.mark.parametrize("K", [4, 1, 5])
@pytest.mark.parametrize("N,C", SHAPES)
def test_walking_form_equals_the_oracle(N, C, K):
    """the same runs of the walking form against oracle.VecOracle: actions, rewards, done
    flags, int8 observations of all 116 steps, the scores, and the numpy states of five
    games exported mid-rollout and at the end -- exact, no tolerance"""
    got, _, errors = _device(N, C, K, 1)
    assert errors == 0
    _same_outputs(got, _oracle(N, C))


# ---- the 16-word refill: a step whose look holds fewer than N accepted words -----------
REFILL_SEED, REFILL_OFFSET, REFILL_PLAN = 41, 603, (40,) * 9


def _refill_episodes(seed, episodes, N=4, C=104):
    """per episode of np.random.seed(seed)'s game: does a step's first 16-word look (from the
    stream position the step starts at, masked as random_interval(9 - t) masks) hold fewer
    than N accepted words?  The stream: the deal's C - 1 shuffle targets, then N draws per
    step t = 0 .. 8, per episode (env.py:99-112, agents/random.py:9)."""
    w = np.random.RandomState(seed).randint(0, 2**32, size=400 * (episodes + 1), dtype=np.uint32).astype(np.int64) & 0xFF
    i, hits = 0, []

    def interval(mx):
        nonlocal i
        m = (1 << mx.bit_length()) - 1
        while True:
            v = w[i] & m
            i += 1
            if v <= mx:
                return v

    for _ in range(episodes):
        for k in range(C - 1, 0, -1):
            interval(k)
        hit = False
        for t in range(9):
            mx = 9 - t
            hit = hit or np.count_nonzero((w[i:i + 16] & ((1 << mx.bit_length()) - 1)) <= mx) < N
            for _p in range(N):
                interval(mx)
        hits.append(hit)
    return hits


def test_refill_when_sixteen_words_hold_fewer_than_n_draws():
    """np.random.seed(41 + 603 + g), g = 0 .. 66, 360 steps = 36 episodes a game: in 11 of the
    67 x 36 game-episodes some step's 16-word look holds fewer than four accepted words
    (counted here on the CPU from numpy's own MT19937 words, which the oracle's stream is
    checked against first; the test needs at least 8), so the walking form takes its second
    look there.  Its records equal the byte-buffer form's word for word and its outputs the
    oracle's."""
    r = O.Rng(O.RNG_NUMPY_MT, REFILL_SEED + REFILL_OFFSET)
    first = np.random.RandomState(REFILL_SEED + REFILL_OFFSET).randint(0, 2**32, size=700, dtype=np.uint32)
    assert [r.next() for _ in range(700)] == first.tolist()
    episodes = sum(REFILL_PLAN) // 10
    hits = sum(sum(_refill_episodes(REFILL_SEED + REFILL_OFFSET + g, episodes)) for g in range(B))
    assert hits == 11 and hits >= 8
    args = dict(plan=REFILL_PLAN, seed=REFILL_SEED, offset=REFILL_OFFSET, export_after=4)
    (got, w1, e1), (_, w0, e0) = _device(4, 104, 4, 1, **args), _device(4, 104, 4, 0, **args)
    assert e1 == 0 and e0 == 0
    _same_words(w1, w0)
    _same_outputs(got, _oracle(4, 104, **args))




# ---- a window cut short by the twisted end ----------------------------------------------
# test knobs, as the overrun tests of tests/test_gpu_env.py set them: exact-lead twists beside
# every launch with a lead below two episodes' words (the start-up lead is already too short),
# and the default schedule whose steady twists twist nothing (the start-up lead runs dry after
# about twelve episodes; until then the games are exact)
SHORT = {"lead96": dict(pipe_lead=96, twist_round=0, twist_every=1),
         "lead288": dict(pipe_lead=288, twist_round=0, twist_every=1),
         "twist_skip": dict(twist_skip=1)}


def _short_window(walk, knobs, calls=30, steps=10):
    """(index of the call that raised, outputs of the calls before it, the pipeline words after
    every call up to and including it, the overrun count)"""
    from rl_6_nimmt._native import PipeOverrunError
    from rl_6_nimmt.vec_env import VecSechsNimmtEnv

    env = VecSechsNimmtEnv(B, 4, seed=SEED, rng="numpy")
    env.set_option(walk_draws=walk, **SHORT[knobs])
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


@pytest.mark.parametrize("knobs", list(SHORT))
def test_short_window_hands_over_to_the_byte_buffer(knobs):
    """The decoder's window is cut by the twisted end, so steps find fewer than 16 live bytes
    and go through the byte buffer, and a draw then needs a word past the end.  Both forms
    raise PipeOverrunError on the same 10-step call (the first with a short lead, a later one
    with twist_skip, where the calls before it are compared), neither hangs, their outputs
    until that call equal the oracle's, and their records and decoder positions are equal
    after every call, the raising one included."""
    r1, p1, w1, e1 = _short_window(1, knobs)
    r0, p0, w0, e0 = _short_window(0, knobs)
    assert r1 is not None and r1 == r0
    assert (r1 > 0) == (knobs == "twist_skip")
    assert e1 > 0 and e0 > 0
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
