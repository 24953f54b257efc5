"""The snapshot format on the host (no GPU): rl_6_nimmt/snapshot.py, the model of csrc/sechs_snapshot.h.

mt_canonical_host is the conversion k_snapshot_save performs on the device.  The lazy states it is given here are
built from numpy's own rounds -- K[r] = the key after r twists of np.random.RandomState(seed) -- so the expected
answer of every branch is RandomState.get_state() itself, and a RandomState set to the converted state must go on
drawing what the original draws.  The layout is held against sn_state_bytes of the built library."""
import ctypes

import numpy as np
import pytest

from rl_6_nimmt import snapshot as S

MT_N = 624


def rounds(seed, n):
    """K[0] = the seeded key (pos 624), K[r] = the key after r twists"""
    rs = np.random.RandomState(seed)
    keys = [rs.get_state()[1].copy()]
    for _ in range(n):
        rs.bytes(4 * MT_N)  # one 32-bit word per 4 bytes: a whole round
        keys.append(rs.get_state()[1].copy())
    return keys


def at(seed, words):
    """a RandomState that has drawn `words` 32-bit words since np.random.seed(seed)"""
    rs = np.random.RandomState(seed)
    if words:
        rs.bytes(4 * words)
    return rs


def check_continues(key, pos, ref):
    """(key, pos) is ref's state, and a RandomState set to it draws ref's next 1 000 words and a shuffle
    (numpy's masked-rejection random_interval) after them"""
    _, rkey, rpos = ref.get_state()[:3]
    assert pos == rpos
    assert np.array_equal(key, rkey)
    rs = np.random.RandomState(0)
    rs.set_state(("MT19937", key, pos))
    assert rs.bytes(4000) == ref.bytes(4000)
    a, b = np.arange(104), np.arange(104)
    rs.shuffle(a)
    ref.shuffle(b)
    assert np.array_equal(a, b)
    assert [rs.randint(0, m + 1) for m in (9, 103, 5)] == [ref.randint(0, m + 1) for m in (9, 103, 5)]


def test_words_per_draw():
    """the construction's premise: bytes(4 k) advances the legacy stream by k words"""
    rs = at(5, 0)
    assert rs.get_state()[2] == MT_N
    rs.bytes(4 * 13)
    assert rs.get_state()[2] == 13
    rs.bytes(4 * MT_N)
    assert rs.get_state()[2] == 13


@pytest.mark.parametrize("seed", [0, 7, 123456789])
def test_complete_round_seed_state(seed):
    """code 0 (csrc/sechs_device.h: np.random.seed(s) == init_genrand(s) with code 0): pos 624, the key as it is"""
    K = rounds(seed, 0)
    key, pos = S.mt_canonical_host(K[0], 0)
    check_continues(key, pos, at(seed, 0))


@pytest.mark.parametrize("drawn", [0, 1, 13, 623, 624])
def test_complete_round_imported(drawn):
    """an imported numpy state (key, p) is code 624 | (624 - p) << 16: a complete round with 624 - p words left"""
    seed = 11
    ref = at(seed, MT_N + drawn) if drawn else at(seed, MT_N)
    _, rkey, rpos = ref.get_state()[:3]
    code = MT_N | ((MT_N - rpos) << 16)
    key, pos = S.mt_canonical_host(rkey, code)
    check_continues(key, pos, ref)


@pytest.mark.parametrize("k", [1, 3, 13, 227, 229, 397, 401, 619, 623])
def test_mid_round(k):
    """k draws into round 2 with k % 8 != 0: the lazy twist stands at p = the next multiple of 8, words [p, 624)
    are still round 1's, p - k twisted words are unconsumed"""
    assert k % 8
    seed = 3
    K = rounds(seed, 2)
    p = (k + 7) // 8 * 8
    raw = np.concatenate((K[2][:p], K[1][p:]))
    key, pos = S.mt_canonical_host(raw, p | ((p - k) << 16))
    assert pos == k
    check_continues(key, pos, at(seed, MT_N + k))


@pytest.mark.parametrize("p,q", [(8, 620), (8, 1), (232, 300), (400, 100), (616, 300), (616, 623)])
def test_straddled(p, q):
    """the consumer stands at word q of round 1 while the twist has run p words into round 2 (cnt = p + 624 - q
    > p): round 1's head [0, p) comes back from round 2's words and the old mt[0]"""
    seed = 9
    K = rounds(seed, 2)
    cnt = p + MT_N - q
    assert p < cnt <= 0x3FF
    raw = np.concatenate((K[2][:p], K[1][p:]))
    key, pos = S.mt_canonical_host(raw, p | (cnt << 16), old0=K[1][0])
    assert pos == q
    check_continues(key, pos, at(seed, q))


@pytest.mark.parametrize("p", [8, 64, 224, 232, 400, 616])
def test_last_word_of_a_round_drawn(p):
    """cnt == p < 624: the consumer has drawn word 623 of round 1 and the twist has run p words into round 2.
    numpy twists at the next draw, so get_state() is still round 1's key at pos 624 -- not round 2's at pos 0"""
    seed = 9
    K = rounds(seed, 2)
    raw = np.concatenate((K[2][:p], K[1][p:]))
    key, pos = S.mt_canonical_host(raw, p | (p << 16), old0=K[1][0])
    assert pos == MT_N
    check_continues(key, pos, at(seed, MT_N))


def test_imported_pos_zero_stays_zero():
    """code 624 | 624 << 16 is mt_code_from_numpy(0): a state set at pos 0 (numpy never shows it by itself) is a
    complete round with nothing drawn; it is saved as it was set, and continues with the round's word 0"""
    K = rounds(4, 1)
    key, pos = S.mt_canonical_host(K[1], MT_N | (MT_N << 16))
    assert pos == 0 and np.array_equal(key, K[1])
    rs = np.random.RandomState(0)
    rs.set_state(("MT19937", key, pos))
    assert rs.bytes(4000) == at(4, 0).bytes(4000)  # round 1 from its word 0: what the seeded state draws first


@pytest.mark.parametrize("n,c", [(4, 104), (2, 24), (10, 104)])
def test_sweep_inputs_stay_wide(n, c):
    """The inputs of tests/test_gpu_snapshot_states.py, with the oracle alone: at each of the five save points of
    the schedule at least 100 of the 640 games stand in each of the pos bands 1-227, 228-397 and 398-623, and the
    positions reached over the five points cover at least 600 of the 624 values 1 .. 624 (measured: the smallest
    band count is 165, a single point already has about 400 distinct positions).  An edit of the inputs that
    narrows the sweep fails here."""
    import snapshot_states as X

    assert (n, c) in X.SHAPES and X.B == 640 and X.CHUNKS == (1, 2, 7, 13, 17)
    key0, pos0 = X.start_states()
    assert sorted(set(pos0.tolist())) == list(range(625))  # the start states: every position, 0 and 624 included
    saves, _ = X.sweep(n, c)
    assert len(saves) == 6
    seen, least = set(), X.B
    for s in saves[1:]:
        pos = s["pos"]
        assert pos.min() >= 1 and pos.max() <= MT_N  # numpy's own range
        for lo, hi in ((1, 227), (228, 397), (398, 623)):
            k = int(((pos >= lo) & (pos <= hi)).sum())
            least = min(least, k)
            assert k >= 100, (lo, hi, k)
        seen |= set(pos.tolist())
    print(f"{n} players, {c} cards: smallest band count {least}, {len(seen)} distinct positions")
    assert len(seen) >= 600


def test_pack_unpack_round_trip():
    rng = np.random.RandomState(1)
    for mode, league in ((S.RNG_NUMPY_MT, False), (S.RNG_NUMPY_MT, True), (S.RNG_PHILOX, False), (S.RNG_PHILOX, True)):
        B, N = 5, 3
        hdr = {"B": B, "N": N, "C": 104, "rng_mode": mode, "league": int(league), "seed": 2**63 + 5, "game_offset": 1000,
               "lg_K": 4 if league else 0, "lg_lo": 2 if league else 0, "lg_hi": 3 if league else 0, "phase": 7,
               "lg_phase": -1}
        f = {"hand": rng.randint(0, 2**32, (B, N, 3), dtype=np.uint32), "row_lo": rng.randint(0, 2**32, (B, 4), dtype=np.uint32),
             "row_hi": rng.randint(0, 2**32, (B, 4), dtype=np.uint32), "score": rng.randint(0, 60, (B, N)).astype(np.int32),
             "sum_res": -rng.randint(0, 600, (B, N)).astype(np.int32), "episodes": rng.randint(0, 9, (B,)).astype(np.int32)}
        if league:
            f["lgs"] = rng.randint(0, 2**32, (B,), dtype=np.uint32)
            f["lmem"] = rng.randint(0, 2**32, (B, N, 4), dtype=np.uint32)
        if mode == S.RNG_NUMPY_MT:
            f["pos"] = rng.randint(0, 625, (B,)).astype(np.int32)
            f["key"] = rng.randint(0, 2**32, (B, MT_N), dtype=np.uint32)
        else:
            f["ctr"] = rng.randint(0, 2**62, (B,)).astype(np.uint64)
        blob = S.pack_host(hdr, f)
        assert blob.dtype == np.uint8 and blob.size == S.state_bytes(B, N, mode, league)
        h2, f2 = S.unpack_host(blob)
        for k, v in hdr.items():
            assert h2[k] == v, k
        assert h2["magic"] == S.MAGIC and h2["version"] == S.VERSION
        assert sorted(f2) == sorted(f)
        for k in f:
            assert np.array_equal(f2[k], f[k]), k
        assert np.array_equal(S.pack_host(h2, f2), blob)


def test_layout_properties():
    assert S.HEADER_BYTES % 64 == 0
    for N in range(1, 11):
        for mode in (S.RNG_PHILOX, S.RNG_NUMPY_MT):
            for league in (False, True):
                L = S.layout(N, mode, league)
                assert L["record_bytes"] % 16 == 0
                if mode == S.RNG_NUMPY_MT:
                    assert L["key"] % 4 == 0 and L["pos"] == L["key"] - 1 >= L["small"]  # 16-byte aligned key
                    assert L["dwords"] >= L["key"] + MT_N
                else:
                    assert L["ctr"] % 2 == 0 and L["ctr"] >= L["small"]
                assert (L["lgs"] >= 0) == league


@pytest.mark.parametrize("N", [2, 4, 10])
@pytest.mark.parametrize("mode", [S.RNG_PHILOX, S.RNG_NUMPY_MT])
@pytest.mark.parametrize("league", [0, 1])
def test_sn_state_bytes_is_the_layout(N, mode, league):
    from rl_6_nimmt import _native

    lib = _native.lib()
    hb, rb = ctypes.c_int64(), ctypes.c_int64()
    for B in (0, 1, 130, 65536):
        total = lib.sn_state_bytes(B, N, mode, league, ctypes.byref(hb), ctypes.byref(rb))
        L = S.layout(N, mode, bool(league))
        assert (hb.value, rb.value) == (S.HEADER_BYTES, L["record_bytes"])
        assert total == S.state_bytes(B, N, mode, bool(league)) == hb.value + B * rb.value
    assert lib.sn_state_bytes(1, 11, mode, league, None, None) == -1
    assert lib.sn_state_bytes(1, N, 7, league, None, None) == -1


def test_new_symbols_are_exported_and_bound():
    from rl_6_nimmt import _native

    lib = _native.lib()
    for s in ("sn_state_bytes", "sn_state_size", "sn_state_save", "sn_state_load"):
        assert hasattr(lib, s) and s in _native.SIGNATURES
    assert lib.sn_state_bytes.restype is ctypes.c_int64
    # refusals that need no GPU: NULL handle / blob
    assert lib.sn_state_save(None, None, 0, None) == _native.SN_EINVAL
    assert lib.sn_state_load(None, None, 0, 0, None) == _native.SN_EINVAL
    assert lib.sn_state_size(None) == -1
