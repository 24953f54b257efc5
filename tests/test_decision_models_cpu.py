"""CPU checks of the decision streams' host side: the tag table of csrc/sechs_decide.h against its Python copy,
the stream word's fields, the models of tests/decision_models.py on hand-worked examples, and the share of
ambiguous sampling decisions in every input set tests/test_gpu_decision_streams.py uploads."""
import os
import re

import numpy as np

import decision_models as M
from conftest import PKG_ROOT


def _header_constants():
    """the `constexpr uint32_t kName = value;` lines of sechs_decide.h, a value being a literal or an earlier name"""
    text = open(os.path.join(PKG_ROOT, "csrc", "sechs_decide.h")).read()
    out = {}
    for name, value in re.findall(r"^constexpr uint32_t (k\w+) = (\w+);", text, flags=re.M):
        out[name] = out[value] if value in out else int(value.rstrip("uU"), 0)
    return out


def test_tags_are_the_device_headers():
    from rl_6_nimmt import dqn, engine

    k = _header_constants()
    assert k["kSelectTag"] == engine.SELECT_TAG == 0xFFFFE and k["kSampleTag"] == engine.SAMPLE_TAG == 0xFFFFF
    assert k["kRolloutTagEnd"] == engine.ROLLOUT_TAG_END == 0xFFF00
    assert k["kNoisyTag0"] == dqn.NOISY_TAG0 and k["kNoisyLayers"] == dqn.NOISY_MAX_LAYERS
    # the header's order: rollouts, then the noise tags, the select tag, the sample tag, all inside 20 bits
    assert engine.ROLLOUT_TAG_END <= dqn.NOISY_TAG0 and dqn.noisy_tag(dqn.NOISY_MAX_LAYERS - 1, 1) < engine.SELECT_TAG \
        < engine.SAMPLE_TAG < 1 << 20
    assert dqn.philox4x32_10_host is engine.philox4x32_10_host


def test_stream_word_fields_do_not_overlap():
    from rl_6_nimmt.engine import ROLLOUT_TAG_END, SAMPLE_TAG, SELECT_TAG, dec_stream_host

    tags = np.array(sorted({0, 1, 2, 5, 255, 256, 0xFFFF, 0x10000, ROLLOUT_TAG_END - 1, ROLLOUT_TAG_END,
                            ROLLOUT_TAG_END + 127, SELECT_TAG, SAMPLE_TAG} | {1 << b for b in range(20)}),
                    dtype=np.uint64)
    assert int(tags.max()) == (1 << 20) - 1
    gids = np.array([0, 1, 129, 2**31, 2**32 - 1], dtype=np.uint64)
    gid, seat, tag, low = np.meshgrid(gids, np.arange(10, dtype=np.uint64), tags, np.arange(11, dtype=np.uint64),
                                      indexing="ij")
    s = dec_stream_host(gid, seat, tag, low)
    assert s.dtype == np.uint64
    parts = (gid << np.uint64(32), seat << np.uint64(28), tag << np.uint64(8), low)
    assert np.array_equal(s, sum(parts[1:], parts[0]))  # OR == sum: no two fields share a bit
    assert np.array_equal(s >> np.uint64(32), gid) and np.array_equal((s >> np.uint64(28)) & np.uint64(15), seat)
    assert np.array_equal((s >> np.uint64(8)) & np.uint64(0xFFFFF), tag) and np.array_equal(s & np.uint64(255), low)
    assert np.unique(s).size == s.size
    # the game id is the low 32 bits of game_offset + g, and the low byte defaults to 0
    assert int(dec_stream_host(2**32 + 5, 9, SAMPLE_TAG)) == (5 << 32) | (9 << 28) | (SAMPLE_TAG << 8)
    assert int(dec_stream_host(2**32 - 3 + 4, 0, 0, 3)) == (1 << 32) | 3


def test_decision_words_are_philox_at_the_documented_counter():
    """decision_words_host against the oracle's Philox block function, word for word: key (seed lo ^ step, seed
    hi), counter (c, 0, stream lo, stream hi)"""
    from oracle import oracle as O
    from rl_6_nimmt.engine import decision_words_host, dec_stream_host

    seed, step = 0x1234567890ABCDEF, 0x80000001
    gid, seat = np.array([0, 7, 2**32 - 1], dtype=np.uint64)[:, None], np.array([0, 9], dtype=np.uint64)[None, :]
    counters = np.array([0, 1, 9, 2**32 - 1], dtype=np.uint64)
    got = decision_words_host(seed, step, gid[..., None], seat[..., None], 0xABCDE, 7, counters[None, None, :])
    assert got.shape == (3, 2, 4, 4) and got.dtype == np.uint32
    key = [(seed & 0xFFFFFFFF) ^ step, seed >> 32]
    for i, g in enumerate(gid[:, 0]):
        for j, p in enumerate(seat[0]):
            stream = int(dec_stream_host(g, p, 0xABCDE, 7))
            for k, c in enumerate(counters):
                want = O.philox([int(c), 0, stream & 0xFFFFFFFF, stream >> 32], key)
                assert np.array_equal(got[i, j, k], want), (i, j, k)


def test_select_model_on_worked_words():
    words = np.array([[0x80000000, 0xC0000000, 0, 0],     # u1 = 0.5, u2 = 0.75
                      [0x4CCCCD00, 0x00000000, 0, 0],     # u1 = 0.3000000119 > 0.3 in float64: greedy
                      [0x4CCCCC00, 0x19999A00, 0, 0],     # u1 = 0.2999999523: explores; u2 = 0.1000000238
                      [0x000000FF, 0xFFFFFFFF, 0, 0]],    # the low byte is dropped: u1 = 0; u2 = 1 - 2^-24
                     dtype=np.uint32)
    assert M.uniform24(words[:, 0]).tolist() == [0.5, float(np.float32(5033165 * 2.0 ** -24)),
                                                 float(np.float32(5033164 * 2.0 ** -24)), 0.0]
    explore, idx = M.select_model(words, 0.3, 10)
    assert explore.tolist() == [False, False, True, True] and idx.tolist() == [7, 0, 1, 9]
    explore, idx = M.select_model(words, 0.6, 7)
    assert explore.tolist() == [True, True, True, True] and idx.tolist() == [5, 0, 0, 6]
    for eps, want in ((0.0, False), (-1.0, False), (1.0, True), (2.0, True)):  # the ends never / always explore
        assert M.select_model(words, eps, 10)[0].tolist() == [want] * 4
    assert M.select_model(words, 1.0, 1)[1].tolist() == [0, 0, 0, 0]
    # f32(u2) * f32(n) is rounded to float32 before the cast: the largest u2, 1 - 2^-24, times n rounds to a
    # float32 below n at every hand size, so the index stays inside the hand (the clamp is a second guard)
    assert [int(M.select_model(words[3:], 1.0, n)[1][0]) for n in range(1, 11)] == list(range(10))


def test_sample_model_on_a_worked_row():
    x = np.log(np.array([1.0, 2.0, 1.0, 4.0]))  # e / max = 1/4, 1/2, 1/4, 1: cumsum 0.25 0.75 1 2 of a sum 2
    for u, want in ((0.0, 0), (0.1249, 0), (0.1251, 1), (0.3749, 1), (0.3751, 2), (0.4999, 2), (0.5001, 3), (0.999, 3)):
        idx, dist, near = M.sample_model(x, np.float64(u))
        assert int(idx) == want, u
    idx, dist, near = M.sample_model(x, np.float64(0.3749))
    assert int(idx) == 1 and int(near) == 1 and abs(float(dist) - 1e-4) < 1e-12
    index, amb, lo, hi = M.sample_allowed(x, np.float64(0.3749))
    assert not bool(amb) and int(lo) == int(hi) == 1  # 1e-4 > 2^-14: exact
    index, amb, lo, hi = M.sample_allowed(x, np.float64(0.37499))
    assert bool(amb) and (int(lo), int(hi)) == (1, 2)  # 1e-5 from the boundary between 1 and 2
    index, amb, lo, hi = M.sample_allowed(x, np.float64(0.99999))
    assert bool(amb) and (int(lo), int(hi)) == (3, 3)  # past the last boundary there is only n - 1
    assert int(M.sample_model(np.zeros(1), np.float64(0.7))[0]) == 0


def test_deal_model_on_a_worked_example():
    asked, script = [], iter([2, 4, 0, 1])

    def draw(m):
        asked.append(m)
        return next(script)

    # memory 3 7 20 41 50 90, two cards each for seats 1 and 2: the 2nd-smallest (20), then the 4th of what is
    # left (90); then the 0th (3) and the 1st of 7 41 50 (41)
    assert M.deal_from_draws(draw, [50, 3, 90, 7, 41, 20], 2, 3) == [[20, 90], [3, 41]]
    assert asked == [5, 4, 3, 2]
    # a short memory runs dry mid-seat; seats past `players` stay empty and draw nothing
    asked.clear()
    script = iter([1, 0, 0])
    assert M.deal_from_draws(draw, [9, 8, 7], 2, 3, seats=5) == [[7, 8], [9], [], []]
    assert asked == [2, 1, 0]


def test_deal_model_draws_the_streams_low_bytes():
    """deal_model (the oracle's generator on dec_stream_host's word) against the draws restated from
    decision_words_host: numpy's legacy masked rejection over the words of blocks 0, 1, 2, ... in order"""
    from rl_6_nimmt.engine import decision_words_host

    seed, step, gid, seat, rollout = 2**64 - 1, 2**31, 2**32 - 3, 9, 5
    words = iter(decision_words_host(seed, step, gid, seat, rollout, 0, np.arange(64)).reshape(-1).tolist())

    def draw(m):
        if m == 0:
            return 0
        mask = (1 << int(m).bit_length()) - 1
        while True:
            v = next(words) & mask
            if v <= m:
                return v

    avail = [c for c in range(104) if c % 7 != 3]
    want = M.deal_from_draws(draw, avail, 10, 10)
    assert M.deal_model(seed, step, gid, seat, rollout, avail, 10, 10) == want
    assert [len(h) for h in want] == [10] * 8 + [9]  # 89 cards for 9 x 10: the memory runs dry at the last seat
    other = M.deal_model(seed, step, gid, seat, rollout + 1, avail, 10, 10)
    assert other != want  # another rollout, another stream


def test_ambiguous_share_of_every_gpu_input_set():
    names = []
    for name, logits, u in M.sampling_inputs():
        assert logits.dtype == np.float32 and u.dtype == np.float32 and logits.shape[:-1] == u.shape, name
        assert float(np.abs(logits).max()) <= M.LOGIT_MAX and 0.0 <= float(u.min()) and float(u.max()) < 1.0, name
        index, amb, lo, hi = M.sample_allowed(logits, u)
        share = float(amb.mean())
        print(f"{name}: {amb.size} decisions, {int(amb.sum())} in the band ({100 * share:.3f} %)")
        assert share <= M.MAX_AMBIGUOUS, (name, share)
        assert bool(((lo == index) | (hi == index)).all()), name  # the model's own index is always allowed
        names.append(name)
    assert len(names) == 8 + len(M.KEY_CASES) + 3 + 2 * len(M.STEP_SHAPES)
