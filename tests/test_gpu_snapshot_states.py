"""The checkpoint's numpy-MT form on the device, at every stream position and under every pipeline setting.

k_snapshot_save (csrc/sechs_snapshot.hip) brings each game's lazy MT19937 state (mt, mt_pos, mt0) to
np.random.get_state() form along three different paths -- complete round (copied), mid-round (finished in place in
224-word chunks), straddled (the head untwisted with mt0, its two loops changing shape at tp <= 227, <= 397 and
above) -- and k_snapshot_load puts a record back.  Here the reference is numpy itself: the CPU oracle's rngs[g].mt /
.pos are RandomState's own (key, pos), placed in the handle with set_mt_state, and a record must equal them with
nothing normalised: a game that has drawn a round's last word shows that round at pos 624, as numpy does.

The inputs (tests/snapshot_states.py; tests/test_snapshot_cpu.py keeps them wide): 640 games starting at every
pos 0 .. 624, three shapes, saves after set_mt_state alone and after rollouts of 1, 2, 7, 13 and 17 steps, under
the issue's eight settings of the SN_OPT_* knobs and a ninth (i, below); sn_set_option refuses none, none is
dropped.  Every comparison is exact.

What the sweep found (kept as the cases of test_save_is_numpys_state): every setting wrote a game standing
exactly on a round boundary as the NEXT round's key at pos 0 where numpy shows the finished round at pos 624
(codes cnt == pos: the mid-round path finished a round the consumer had not entered; and cnt == pos == 624 behind
k_pipe_code, read as an imported pos 0).  mt_code_straddles (csrc/sechs_device.h) now sends cnt == pos < 624 down
the straddled path, k_pipe_code undoes a round at rem == 624 too (unless the game has drawn nothing since a pos 0
was imported: test_pos_zero_survives_a_pipeline_that_draws_nothing), and MtGenT::save drops a held-back chunk
none of whose words was drawn."""
import collections
import ctypes
import functools

import numpy as np
import pytest
import torch

import snapshot_states as X
from rl_6_nimmt import snapshot as S

pytestmark = pytest.mark.gpu

B, SHAPES, CHUNKS = X.B, X.SHAPES, X.CHUNKS
SETTINGS = {
    "a": {},
    "b": {"pipe_dec": 0},
    "c": {"pipeline": 0, "ring_words": 0},
    "d": {"pipeline": 0, "ring_words": 64},
    "e": {"pipeline": 0, "ring_words": 512},
    "f": {"twist_round": 0},
    "g": {"twist_depth": 3},
    "h": {"twist_every": 3},
    # past the issue's eight: a pipelined handle whose lead (600 words) stays below a round, twisted word by word,
    # so that k_pipe_code undoes nothing and leaves straddled and mid-round codes against any twist pointer
    "i": {"pipe_dec": 0, "twist_round": 0, "twist_every": 1},
}
CLASSES = ("complete", "mid-round", "straddled tp<=227", "straddled 227<tp<=397", "straddled tp>397")
FIELDS = ("hand", "row_lo", "row_hi", "score", "sum_res", "episodes")


def _env(n, c, setting):
    from rl_6_nimmt.vec_env import VecSechsNimmtEnv

    env = VecSechsNimmtEnv(B, n, num_cards=c, seed=X.SEED, rng="numpy")
    env.set_option(**SETTINGS[setting])
    return env


def _place(env):
    key, pos = X.start_states()
    for g in range(B):
        env.set_mt_state(key[g], int(pos[g]), game=g)


def _codes(env):
    """mt_pos[g] as it stands (sn_debug_pipe_words, what = 3): behind a save, the codes k_snapshot_save read"""
    from rl_6_nimmt import _native as nat

    out = np.zeros(B, dtype=np.uint32)
    nat.check(nat.lib().sn_debug_pipe_words(env._h, 3, 0, out.ctypes.data_as(ctypes.c_void_p)), "sn_debug_pipe_words")
    return out


def _classify(code):
    """the path k_snapshot_save takes for a state code (mt_code_straddles, then its mid-round test)"""
    p, cnt = int(code) & 0x7FF, (int(code) >> 16) & 0x3FF
    if p > 0 and (cnt > p or (cnt == p and p < 624)):
        tp = min(p, 624)
        return CLASSES[2] if tp <= 227 else CLASSES[3] if tp <= 397 else CLASSES[4]
    return CLASSES[1] if 0 < p < 624 else CLASSES[0]


def _play(env, steps):
    out = env.rollout(steps, want_actions=True, want_obs=True)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _out_problems(got, want, what):
    bad = []
    for k in ("actions", "rewards", "done"):
        if not np.array_equal(got[k], want[k]):
            bad.append(f"{what}: {k} differ from the oracle's")
    if not np.array_equal(got["obs"][..., : want["obs"].shape[-1]], want["obs"]):
        bad.append(f"{what}: obs differ from the oracle's")
    return bad


def _save_problems(blob, codes, want, i, n, c):
    """a saved blob against numpy's states (and, once dealt, the oracle's games): [] or what differs, by class"""
    h, f = S.unpack_host(blob)
    bad = []
    if blob.size != S.state_bytes(B, n, S.RNG_NUMPY_MT, False) or (h["B"], h["N"], h["C"], h["seed"]) != (B, n, c, X.SEED):
        bad.append(f"save {i}: header {h}")
    wrong = np.flatnonzero((f["pos"] != want["pos"]) | (f["key"] != want["key"]).any(axis=1))
    for g in wrong[:4]:
        nk = int((f["key"][g] != want["key"][g]).sum())
        bad.append(f"save {i}: game {g}, class {_classify(codes[g])} (code {int(codes[g]):#x}): pos {int(f['pos'][g])}, "
                   f"numpy's {int(want['pos'][g])}; {nk} key words differ")
    if len(wrong) > 4:
        bad.append(f"save {i}: {len(wrong)} games differ in all")
    for k in FIELDS if i else ():
        if not np.array_equal(f[k], want[k]):
            bad.append(f"save {i}: {k} differ from the oracle's")
    return bad


@functools.lru_cache(maxsize=None)
def _run(n, c, setting):
    """one handle through the schedule: a save after set_mt_state alone and after every chunk.  Keeps setting a's
    blobs (the others are compared with them here), what differed from numpy / the oracle, and the census"""
    saves, outs = X.sweep(n, c)
    base = _run(n, c, "a") if setting != "a" else None
    env = _env(n, c, setting)
    _place(env)
    blobs, problems, same, census = [], [], [], collections.Counter()
    for i in range(len(CHUNKS) + 1):
        if i == 1:
            env.reset()
        if i:
            problems += _out_problems(_play(env, CHUNKS[i - 1]), outs[i - 1], f"chunk {i - 1}")
        blob = env.snapshot().cpu().numpy()
        codes = _codes(env)
        census.update(_classify(x) for x in codes)
        problems += _save_problems(blob, codes, saves[i], i, n, c)
        same.append(base is None or np.array_equal(blob, base["blobs"][i]))
        blobs.append(blob if base is None else None)
    errors = env.pipe_errors()
    env.close()
    return {"blobs": blobs, "problems": problems, "same": same, "census": census, "pipe_errors": errors}


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("n,c", SHAPES)
def test_save_is_numpys_state(n, c, setting):
    """Section 1: at all six save points every record's (key, pos) is numpy's own state of that game -- rngs[g].mt
    and .pos of the oracle, pos 624 where a round's last word was just drawn, pos 0 only where it was set -- the
    game fields (from the first deal on) are the oracle's word for word, every chunk's actions, rewards, done and
    observations are the oracle's, and no draw overran."""
    r = _run(n, c, setting)
    assert not r["problems"], "\n".join(r["problems"])
    assert r["pipe_errors"] == 0


@pytest.mark.parametrize("n,c", SHAPES)
def test_blobs_do_not_depend_on_the_settings(n, c):
    """include/sechs.h: "records do not depend on the SN_OPT_* settings or on where the pipelines stand" -- at
    every save point the whole blob of every setting is byte-equal to the default's"""
    for setting in SETTINGS:
        assert all(_run(n, c, setting)["same"]), (setting, _run(n, c, setting)["same"])


def test_every_path_of_the_save_kernel_ran():
    """Section 2, the census: the state codes as they stood behind each save of the sweep (3 shapes x 8 settings x
    6 saves x 640 games), by the path k_snapshot_save takes for them.  Every class must have occurred, and all are
    reachable, so none is asserted empty -- but not from everywhere, which the printed rows show: a pipelined
    handle (N <= 6) under settings a, b, f, g, h leads its consumer by more than a round in this schedule, so
    k_pipe_code undoes at least one and leaves a complete round (twist pointer 624); under setting i its lead of
    600 words is below a round, k_pipe_code undoes nothing and every straddled shape must have come from the
    pipelined shapes alone (asserted); the lazy per-lane path (c) never twists across a boundary and leaves
    complete and mid-round codes only; k_mt_prep's ring (d: up to 64 words across a boundary, e and every
    setting's 10-player handles: up to 512) leaves all of them.  Printed; DESIGN.md 4d records the counts."""
    total = collections.Counter()
    for setting in SETTINGS:
        for n, c in SHAPES:
            census = _run(n, c, setting)["census"]
            total += census
            print(f"setting {setting}, {n} players: " + ", ".join(f"{k} {census[k]}" for k in CLASSES))
            if setting == "i" and n <= 6:  # k_pipe_code's exits with rem < 624 against a twist pointer below 624
                for k in CLASSES[2:]:
                    assert census[k] > 0, (n, k)
    print("whole sweep: " + ", ".join(f"{k} {total[k]}" for k in CLASSES))
    assert sum(total.values()) == len(SHAPES) * len(SETTINGS) * (len(CHUNKS) + 1) * B
    for k in CLASSES:
        assert total[k] > 0, k


def _header(n, c):
    return {"B": B, "N": n, "C": c, "rng_mode": S.RNG_NUMPY_MT, "league": 0, "seed": X.SEED, "game_offset": 0,
            "lg_K": 0, "lg_lo": 0, "lg_hi": 0, "phase": 0, "lg_phase": 0}


@pytest.mark.parametrize("setting", ["a", "c"])
@pytest.mark.parametrize("n,c", SHAPES)
def test_load_at_every_position(n, c, setting):
    """Section 3: a blob packed on the host -- freshly dealt games of the oracle, the start states at every pos 0 ..
    624 -- loaded into a fresh handle: get_mt_state and a second snapshot return exactly what was loaded (pos 0
    and 624 included), and the 40 steps played from there are the oracle's from the same states."""
    fields, outs = X.dealt(n, c)
    blob = S.pack_host(_header(n, c), fields)
    env = _env(n, c, setting)
    env.load_snapshot(torch.from_numpy(blob))
    for g in range(B):
        key, pos = env.get_mt_state(g)
        assert pos == fields["pos"][g] == g % 625, g
        assert np.array_equal(key, fields["key"][g]), g
    again = env.snapshot().cpu().numpy()
    assert np.array_equal(again, blob)
    for i, steps in enumerate(CHUNKS):
        bad = _out_problems(_play(env, steps), outs[i], f"chunk {i}")
        assert not bad, bad
    assert env.pipe_errors() == 0
    env.close()


def test_load_reads_a_pos_past_624_as_624():
    """k_snapshot_load clamps the record's pos (an unsigned word) to 624 before it builds the state code: 625,
    2^31 and 2^32 - 1 all load as the complete round they name, key unchanged (include/sechs.h, sn_state_load)"""
    n, c = 4, 104
    fields, _ = X.dealt(n, c)
    fields = dict(fields, pos=np.array(fields["pos"]))
    odd = {3: 625, 300: 2**31, 639: 2**32 - 1}
    for g, p in odd.items():
        fields["pos"][g] = np.array(p, dtype=np.uint32).view(np.int32)
    env = _env(n, c, "a")
    env.load_snapshot(torch.from_numpy(S.pack_host(_header(n, c), fields)))
    for g in list(odd) + [2, 4, 624]:
        key, pos = env.get_mt_state(g)
        assert pos == (624 if g in odd else g % 625), g
        assert np.array_equal(key, fields["key"][g]), g
    env.close()


def test_pos_zero_survives_a_pipeline_that_draws_nothing():
    """624 | 624 << 16 is both the import of pos 0 and, behind k_pipe_code, a consumer one whole array behind the
    twist.  k_pipe_code tells them apart by the words drawn since the pipeline started: finished games stepped
    without auto-reset draw nothing, yet the step starts the pipeline, which twists rounds ahead and is then
    synchronised.  States set at pos 0, 1 .. 127 and 624 must come back exactly (set, then get, is the identity),
    in get_mt_state and in the record, and the blob must be the one a handle without the pipeline saves."""
    n, c = 4, 104
    key, pos = X.start_states()
    picks = list(range(128)) + [625, 624]  # pos 0 .. 127, 0 again, 624
    blobs = {}
    for setting in ("a", "c"):
        env = _env(n, c, setting)
        env.reset()
        for _ in range(10):
            _, done, _ = env.step(None)
        assert bool(done.all())
        for g in range(B):
            s = picks[g % len(picks)]
            env.set_mt_state(key[s], int(pos[s]), game=g)
        for _ in range(2):
            env.step(None)  # no card left to play: nothing is drawn
        for g in range(0, B, 5):
            s = picks[g % len(picks)]
            k, p = env.get_mt_state(g)
            assert p == pos[s], (setting, g)
            assert np.array_equal(k, key[s]), (setting, g)
        blobs[setting] = env.snapshot().cpu().numpy()
        _, f = S.unpack_host(blobs[setting])
        want = [picks[g % len(picks)] for g in range(B)]
        assert np.array_equal(f["pos"], pos[want]) and np.array_equal(f["key"], key[want]), setting
        assert env.pipe_errors() == 0
        env.close()
    assert np.array_equal(blobs["a"], blobs["c"])


def test_resume_across_settings():
    """Section 4: saved after 10 steps under ring_words = 512 without the pipeline and loaded into a fresh default
    handle, and the other way round: savers and loaders all play the remaining 30 steps as the oracle does and
    end in byte-equal blobs (the default run's of the sweep)."""
    n, c = 4, 104
    _, outs = X.sweep(n, c)
    savers = {s: _env(n, c, s) for s in ("e", "a")}
    blobs = {}
    for s, env in savers.items():
        _place(env)
        env.reset()
        for i in range(3):  # 1 + 2 + 7 steps
            assert not _out_problems(_play(env, CHUNKS[i]), outs[i], f"{s}: chunk {i}")
        blobs[s] = env.snapshot()
    assert torch.equal(blobs["e"].cpu(), blobs["a"].cpu())
    loaders = {"e->a": _env(n, c, "a"), "a->e": _env(n, c, "e")}
    loaders["e->a"].load_snapshot(blobs["e"])
    loaders["a->e"].load_snapshot(blobs["a"])
    final = _run(n, c, "a")["blobs"][-1]
    for name, env in list(loaders.items()) + list(savers.items()):
        for i in (3, 4):
            bad = _out_problems(_play(env, CHUNKS[i]), outs[i], f"{name}: chunk {i}")
            assert not bad, bad
        assert np.array_equal(env.snapshot().cpu().numpy(), final), name
        assert env.pipe_errors() == 0
        env.close()


@pytest.mark.parametrize("at", [1, 4, 9])
def test_tournament_handle_states(at):
    """Section 5: the mid-round tournament handle of test_gpu_snapshot.test_tournament_handle_resumes_mid_round (two
    MCS seats: the wave search leaves its own lazy states, wmt_store).  Every record's (key, pos) equals
    get_mt_state(g), and a RandomState set to it continues as the matching game of a twin that was never saved
    (test_snapshot_cpu.check_continues: the same state, the next 1 000 words, a shuffle, three randints)."""
    from rl_6_nimmt import agents as A
    from rl_6_nimmt.league import BatchedTournament
    from test_gpu_snapshot import _league_steps
    from test_snapshot_cpu import check_continues

    def make():
        t = BatchedTournament(130, 2, 4, seed=6, game_offset=20, fused=False)
        t.add_player("m0", A.MCSAgent(mc_max=20))
        t.add_player("h0")
        t.add_player("m1", A.MCSAgent(mc_max=20, mc_per_card=2))
        t.add_player("h1")
        t._start()
        return t

    a, twin = make(), make()
    _league_steps(a, at, reset=True), _league_steps(twin, at, reset=True)
    h, f = S.unpack_host(a.env.snapshot().cpu().numpy())
    assert h["league"] == 1 and h["lg_phase"] == at
    for g in range(130):
        key, pos = a.env.get_mt_state(g)
        assert pos == f["pos"][g] and 1 <= pos <= 624, g
        assert np.array_equal(key, f["key"][g]), g
        ref = np.random.RandomState(0)
        tk, tp = twin.env.get_mt_state(g)
        ref.set_state(("MT19937", tk, tp))
        check_continues(f["key"][g], int(f["pos"][g]), ref)
    assert a.env.pipe_errors() == 0
    a.close(), twin.close()
