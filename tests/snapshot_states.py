"""The inputs of the snapshot sweep (tests/test_gpu_snapshot_states.py) and their oracle side, shared with the CPU
test that keeps the inputs as wide as they are (tests/test_snapshot_cpu.py).  No GPU here.

640 numpy-MT games; game g starts from np.random.RandomState(1000 + g) advanced to pos = g % 625, so the start
states stand at every stream position 0 .. 624 (0: set by hand, numpy never shows it).  The oracle's rngs[g].mt /
.pos are numpy's own (key, pos): what a snapshot record must hold."""
import ctypes
import functools

import numpy as np

from oracle import oracle as O

B = 640
SEED = 5  # the handles' (the MT streams are placed by hand; the header carries it)
SHAPES = [(4, 104), (2, 24), (10, 104)]
CHUNKS = (1, 2, 7, 13, 17)
MT_N = 624


@functools.lru_cache(maxsize=None)
def start_states():
    """(key uint32 [B, 624], pos int [B]), read-only"""
    key, pos = np.zeros((B, MT_N), dtype=np.uint32), np.zeros(B, dtype=np.int64)
    for g in range(B):
        p = g % 625
        rs = np.random.RandomState(1000 + g)
        rs.bytes(4 * (MT_N + p) if p else 4 * MT_N)
        _, k, q = rs.get_state()[:3]
        assert q == (p if p else MT_N)
        key[g], pos[g] = k, p
    key.setflags(write=False), pos.setflags(write=False)
    return key, pos


def place(ref, key, pos):
    """the states into the oracle's generators, as RandomState.set_state would"""
    rngs = ref.v.contents.rngs
    for g in range(ref.B):
        k = np.ascontiguousarray(key[g], dtype=np.uint32)
        ctypes.memmove(rngs[g].mt, k.ctypes.data, 4 * MT_N)
        rngs[g].pos = int(pos[g])


def mt_states(ref):
    """numpy's (key [B, 624], pos [B]) of every game, as the oracle holds them: nothing normalised"""
    rngs = ref.v.contents.rngs
    key = np.stack([np.frombuffer(rngs[g].mt, dtype=np.uint32).copy() for g in range(ref.B)])
    pos = np.array([rngs[g].pos for g in range(ref.B)], dtype=np.int64)
    return key, pos


def _heads(c):
    c1 = c + 1
    return 7 if c1 == 55 else 5 if c1 % 11 == 0 else 3 if c1 % 10 == 0 else 2 if c1 % 10 == 5 else 1


def game_fields(ref):
    """the oracle's games in the record's words (csrc/sechs_state.h): hand [B, N, 3] = the sorted hand bytes, 0xFF
    past the hand; row_lo [B, 4] = cards 0..3, row_hi [B, 4] = card4 | len << 8 | heads << 16 | end << 24 (zero
    bytes past len); score, sum_res [B, N] int32; episodes [B] int32"""
    n = ref.N
    hand = np.full((ref.B, n, 12), 0xFF, dtype=np.uint8)
    lo, hi = np.zeros((ref.B, 4, 4), dtype=np.uint8), np.zeros((ref.B, 4), dtype=np.uint32)
    score = np.zeros((ref.B, n), dtype=np.int32)
    for g in range(ref.B):
        G = ref.v.contents.games[g]
        for p in range(n):
            k = G.hand_len[p]
            hand[g, p, :k] = G.hands[p][:k]
            score[g, p] = G.scores[p]
        for r in range(4):
            k = G.row_len[r]
            cards = G.rows[r][:k]
            lo[g, r, : min(k, 4)] = cards[:4]
            hi[g, r] = (cards[4] if k > 4 else 0) | k << 8 | sum(_heads(c) for c in cards) << 16 | cards[k - 1] << 24
    return {"hand": hand.view("<u4").reshape(ref.B, n, 3), "row_lo": lo.view("<u4").reshape(ref.B, 4), "row_hi": hi,
            "score": score, "sum_res": ref.sum_results().astype(np.int32), "episodes": ref.episodes().astype(np.int32)}


def _oracle(n, c):
    return O.VecOracle(B, n, num_cards=c, rng_mode=O.RNG_NUMPY_MT, seed=SEED)


def _play(ref, after=None):
    """the chunks of the schedule; after(ref) is called behind each.  -> [rewards / done / actions / obs per chunk]"""
    outs = []
    for steps in CHUNKS:
        rew, done, act, obs = ref.rollout(steps, want_obs=True)
        outs.append({"rewards": rew, "done": done, "actions": act, "obs": obs})
        if after:
            after(ref)
    return outs


@functools.lru_cache(maxsize=None)
def sweep(n, c):
    """the save sweep's oracle side: the start states placed, reset, the chunks played.  -> (saves, outs): saves[0]
    = {key, pos} as placed (nothing drawn; no game dealt yet), saves[1 + i] = {key, pos, and game_fields} after chunk
    i; outs[i] = chunk i's rewards / done / actions / obs"""
    key, pos = start_states()
    ref = _oracle(n, c)
    place(ref, key, pos)
    k0, p0 = mt_states(ref)
    saves = [{"key": k0, "pos": p0}]
    ref.reset()

    def save(ref):
        k, p = mt_states(ref)
        saves.append(dict(game_fields(ref), key=k, pos=p))

    return saves, _play(ref, save)


@functools.lru_cache(maxsize=None)
def dealt(n, c):
    """the load sweep's oracle side: games freshly dealt (from the oracle's seeded streams), THEN the start states
    placed, so the record of game g is (a fresh deal, start state g) at every pos 0 .. 624.  -> (fields incl. key /
    pos, outs of the chunks played from there)"""
    key, pos = start_states()
    ref = _oracle(n, c)
    ref.reset()
    place(ref, key, pos)
    fields = dict(game_fields(ref), key=np.array(key), pos=np.array(pos, dtype=np.int32))
    return fields, _play(ref)
