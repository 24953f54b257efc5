"""CPU checks of the Philox league: the test hook is declared, and the host
model of the stream law (tests/league_philox_model.py) keeps the law's own
promises -- no two playouts share a (key, stream), none meets a slot's main
stream, and a search of one playout returns that playout's move under Q6."""
import os
import re

import numpy as np

import league_philox_model as M
from conftest import PKG_ROOT, ROOT
from oracle import oracle as O

# roster (b): a league's player count is at most its agent count (tournament.py:170), so players 2..6 seat six agents
ROSTER_B = dict(kinds="RRRMMR", mc_per_card=[10, 10, 10, 2, 1, 10], mc_max=[100, 100, 100, 12, 70, 100])


def test_hook_is_declared_in_the_header_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sechs.h")).read(), flags=re.S)
    m = re.search(r"sn_status\s+sn_mcs_decide_philox\s*\(([^)]*)\)", text)
    assert m, "include/sechs.h declares sn_mcs_decide_philox"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 14
    assert params[8].startswith("const uint32_t*") and params[9].startswith("const uint64_t*")  # keys, streams
    src = open(os.path.join(PKG_ROOT, "rl_6_nimmt", "_native.py")).read()
    assert '"sn_mcs_decide_philox"' in src
    from rl_6_nimmt import _native

    args, res = _native.SIGNATURES["sn_mcs_decide_philox"]
    assert len(args) == 14 and res is _native._I


def test_model_streams_are_pairwise_distinct():
    out = M.league(min_players=2, max_players=6, seed=0x1234_5678_9ABC_DEF0, game_offset=5, slots=6, games=2, **ROSTER_B)
    streams = out["streams"]
    assert len(streams) > 1000  # both MCS agents were seated and searched
    assert len(set(streams)) == len(streams)
    assert not set(streams) & set(out["main"])
    # the layout: the slot's id in the high word, then seat, playout number and hand size
    gids = {s >> 32 for _, s in streams}
    assert gids <= set(range(5, 11)) and len(gids) > 1
    assert {s & 0xFF for _, s in streams} <= set(range(2, 11))
    assert max((s >> 8) & 0xFFFFF for _, s in streams) == 69  # MCSAgent(1, 70) at n >= 5
    # records are well formed: k seats, results <= 0, nothing past k
    rec = out["records"]
    k = rec[..., 0] & 15
    assert k.min() >= 2 and k.max() <= 6 and rec[..., 1:].max() <= 0
    assert out["rewards"].sum(axis=0).reshape(6, 6).tolist() == rec[..., 1:].sum(axis=0).tolist()
    assert (out["ctr"] > 0).all()


def test_model_search_of_one_playout_returns_its_move_with_q6():
    board, hand, avail = O.mcs_position(4, 5, 77)
    key, stream0 = M.mcs_key(0xABCDEF, 321), M.mcs_stream(9, 2, 5)
    card, q6, sums, counts = M.search(board, hand, avail, 4, 1, 1, key, stream0)
    assert q6 and counts.sum() == 1
    i = int(np.argmax(counts))
    assert card == sorted(hand)[i] and sums[i] <= 0 and not np.delete(sums, i).any()
    # the playout is a pure function of (key, stream): the same call again, and as playout 0 of a larger search
    again = M.search(board, hand, avail, 4, 1, 1, key, stream0)
    assert again[0] == card and np.array_equal(again[2], sums)
    seen = []
    M.search(board, hand, avail, 4, 1, 3, key, stream0, seen)
    assert seen == [(key, stream0), (key, stream0 | 1 << 8), (key, stream0 | 2 << 8)]
    # a memory one card short of (k - 1) n deals nobody
    short = M.search(board, hand, sorted(avail)[:14], 4, 10, 100, key, stream0)
    assert short[0] == -1 and not short[2].any() and not short[3].any()
