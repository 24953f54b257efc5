"""GPU checks of checkpoint and resume: k_snapshot_save / k_snapshot_load behind sn_state_save / sn_state_load
(csrc/sechs_snapshot.hip), VecSechsNimmtEnv.state_dict / load_state_dict, the engines' state_dict and
BatchedTournament.save / load.

The references are the project's own pinned paths: the canonical RNG form is held to get_mt_state (sn_mt_get's
host conversion) and philox_counter over every game, the game fields to the accessors, and a resumed handle or
league to an uninterrupted twin -- equality is exact throughout.  B = 130 is the smallest batch with a partial
block (4 games a block) and a partial wave of the one-lane-per-game kernels."""
import numpy as np
import pytest
import torch

from rl_6_nimmt import snapshot as S

pytestmark = pytest.mark.gpu

B = 130
SHAPES = [(2, 24), (4, 104), (10, 104)]


def _env(n, c, rng, seed=5, games=B, offset=0, pipeline=None):
    from rl_6_nimmt.vec_env import VecSechsNimmtEnv

    env = VecSechsNimmtEnv(games, n, num_cards=c, seed=seed, game_offset=offset, rng=rng)
    if pipeline is not None:
        env.set_option(pipeline=pipeline)
    return env


def _play(env, steps):
    out = env.rollout(steps, want_actions=True, want_obs=True)
    return {k: v.cpu() for k, v in out.items()}


def _same_out(a, b, sl=slice(None)):
    for k in ("rewards", "done", "actions", "obs"):
        assert torch.equal(a[k][:, sl], b[k]), k


def _check_canonical(env):
    """the blob against the handle's own accessors, over all games"""
    n, games = env.num_players, env.num_games
    blob = env.snapshot().cpu().numpy()
    h, f = S.unpack_host(blob)
    assert blob.size == S.state_bytes(games, n, h["rng_mode"], False)
    assert (h["B"], h["N"], h["C"], h["seed"], h["game_offset"]) == (games, n, env.num_cards, env.seed, env.game_offset)
    if env.rng == "numpy":
        for g in range(games):
            key, pos = env.get_mt_state(g)
            assert pos == f["pos"][g], g
            assert np.array_equal(key, f["key"][g]), g
    else:
        for g in range(games):
            assert env.philox_counter(g) == int(f["ctr"][g]), g
    hb = f["hand"].reshape(games, n, 3).copy()
    hb[..., 2] &= 0xFFFF
    hands = np.ascontiguousarray(hb).view(np.int8).reshape(games, n, 12)[..., :10]
    assert np.array_equal(hands, env.hands().cpu().numpy())
    lo = np.ascontiguousarray(f["row_lo"]).view(np.uint8).reshape(games, 4, 4).astype(np.int64)
    card4, length = (f["row_hi"] & 0xFF).astype(np.int64), ((f["row_hi"] >> 8) & 0xFF).astype(np.int64)
    board = np.full((games, 4, 6), -1, dtype=np.int64)
    board[..., :4], board[..., 4] = lo, card4
    board = np.where(np.arange(6)[None, None, :] < np.minimum(length, 5)[..., None], board, -1)
    assert np.array_equal(board, env.board().cpu().numpy().astype(np.int64))
    assert np.array_equal(f["score"], env.scores().cpu().numpy())
    res, epi = env.results()
    assert np.array_equal(f["sum_res"], res.cpu().numpy()) and np.array_equal(f["episodes"], epi.cpu().numpy())
    return blob


@pytest.mark.parametrize("rng,pipeline", [("numpy", 1), ("numpy", 0), ("philox", None)])
@pytest.mark.parametrize("n,c", SHAPES)
def test_canonical_form(n, c, rng, pipeline):
    """after reset alone and after rollouts of 1, 7, 10 and 23 steps (pipeline on and off: the option is
    numpy-MT's): every game's (key, pos) / counter and its game fields in the blob equal the accessors'; a twin
    that is never saved plays the same"""
    env, twin = _env(n, c, rng, pipeline=pipeline), _env(n, c, rng, pipeline=pipeline)
    env.reset(), twin.reset()
    blob0 = _check_canonical(env)
    assert np.array_equal(blob0, env.snapshot().cpu().numpy())  # a save changes nothing a save reads
    for steps in (1, 7, 10, 23):
        a, b = _play(env, steps), _play(twin, steps)
        _same_out(a, b)
        _check_canonical(env)
    assert env.pipe_errors() == 0
    assert np.array_equal(env.snapshot().cpu().numpy(), twin.snapshot().cpu().numpy())
    env.close(), twin.close()


@pytest.mark.parametrize("rng", ["numpy", "philox"])
@pytest.mark.parametrize("n,c", SHAPES)
def test_resume_is_exact_mid_episode(n, c, rng):
    """A plays 7, saves, plays 13; B (fresh) loads and plays 13; C plays 20 uninterrupted"""
    ea, eb, ec = _env(n, c, rng), _env(n, c, rng), _env(n, c, rng)
    ea.reset(), ec.reset()
    _play(ea, 7)
    sd = ea.state_dict()
    assert sd["blob"].device.type == "cpu" and sd["blob"].dtype == torch.uint8
    a = _play(ea, 13)
    eb.load_state_dict(sd)
    b = _play(eb, 13)
    full = _play(ec, 20)
    last = {k: v[7:] for k, v in full.items()}
    _same_out(a, last), _same_out(b, last)
    fa, fb, fc = (e.state_dict()["blob"] for e in (ea, eb, ec))
    assert torch.equal(fa, fc) and torch.equal(fb, fc)
    for e in (ea, eb, ec):
        assert e.pipe_errors() == 0
        e.close()


@pytest.mark.parametrize("rng", ["numpy", "philox"])
def test_reshard(rng):
    """records 64..191 of a 192-game handle at offset 1000 are the state of a 128-game handle at offset 1064"""
    big, part = _env(4, 104, rng, games=192, offset=1000), _env(4, 104, rng, games=128, offset=1064)
    big.reset()
    _play(big, 7)
    sd = big.state_dict()
    part.load_state_dict(sd, first=64)
    a, b = _play(big, 13), _play(part, 13)
    _same_out(a, b, slice(64, 192))
    hb, fb = S.unpack_host(big.snapshot().cpu().numpy())
    hp, fp = S.unpack_host(part.snapshot().cpu().numpy())
    assert hp["game_offset"] == 1064 and hp["B"] == 128
    for k in fb:
        assert np.array_equal(fb[k][64:], fp[k]), k
    assert big.pipe_errors() == 0 and part.pipe_errors() == 0
    big.close(), part.close()


def test_refusals_leave_the_handle_untouched():
    """wrong N, rng_mode, seed, offset, a short blob, a wrong magic: each raises, and the handle then plays exactly
    what an untouched twin plays"""
    src = _env(4, 104, "numpy")
    src.reset()
    _play(src, 7)
    sd = src.state_dict()
    blob = sd["blob"]
    bad_magic = blob.clone()
    bad_magic[0] ^= 0xFF
    victims = {
        "wrong N": (lambda: _env(2, 104, "numpy"), blob, 0),
        "wrong rng_mode": (lambda: _env(4, 104, "philox"), blob, 0),
        "wrong seed": (lambda: _env(4, 104, "numpy", seed=6), blob, 0),
        "wrong offset": (lambda: _env(4, 104, "numpy", offset=1), blob, 0),
        "wrong first": (lambda: _env(4, 104, "numpy"), blob, 1),
        "short blob": (lambda: _env(4, 104, "numpy"), blob[: blob.numel() - 16], 0),
        "header only": (lambda: _env(4, 104, "numpy"), blob[:100], 0),
        "wrong magic": (lambda: _env(4, 104, "numpy"), bad_magic, 0),
    }
    for what, (make, b, first) in victims.items():
        env, twin = make(), make()
        env.reset(), twin.reset()
        _play(env, 3), _play(twin, 3)
        with pytest.raises(ValueError):
            env.load_state_dict(dict(sd, blob=b), first=first)
        _same_out(_play(env, 13), _play(twin, 13))
        assert np.array_equal(env.snapshot().cpu().numpy(), twin.snapshot().cpu().numpy()), what
        assert env.pipe_errors() == 0
        env.close(), twin.close()
    src.close()


def test_a_handle_that_overran_is_not_resumed():
    """the twist_skip test knob runs the ring dry (tests/test_gpu_env.py): such a handle's streams are lost.  Its
    save is refused outright once the host mirror shows the count; a save enqueued before that carries the
    count in its header, and the load refuses it, leaving the handle as it was"""
    from rl_6_nimmt._native import PipeOverrunError

    env = _env(4, 104, "numpy")
    env.set_option(twist_skip=1)
    env.reset()
    env.rollout(240, want_rewards=False, want_done=False)  # the start-up lead lasts about twelve episodes
    try:
        blob = env.snapshot()
    except PipeOverrunError:
        blob = None
    assert env.pipe_errors() > 0
    if blob is not None:
        assert S.read_header(blob.cpu().numpy())["overruns"] > 0
        fresh, twin = _env(4, 104, "numpy"), _env(4, 104, "numpy")
        fresh.reset(), twin.reset()
        with pytest.raises(ValueError, match="overruns"):
            fresh.load_snapshot(blob)
        _same_out(_play(fresh, 13), _play(twin, 13))
        fresh.close(), twin.close()
    with pytest.raises(PipeOverrunError):  # the mirror is set now (pipe_errors): refused before anything is launched
        env.snapshot()
    env.close()


# ---------------------------------------------------------------- leagues
def _league_steps(t, n, reset):
    """n sn_league_step calls of a league without net agents (after sn_reset: seat draw + deal, if `reset`):
    (rewards [n, B, N], cards played [n, B, N], records [B, 1 + N] of the games that ended) on the host"""
    from rl_6_nimmt import _native as nat

    env, L = t.env, nat.lib()
    slots, N, dev = t.num_slots, t.max_players, env.device
    if reset:
        nat.check(L.sn_reset(env._h, None, env._stream()), "sn_reset")
    acts = torch.zeros((slots, N), dtype=torch.int32, device=dev)
    rew = torch.zeros((n, slots, N), dtype=torch.int32, device=dev)
    played = torch.zeros((n, slots, N), dtype=torch.int32, device=dev)
    rec = torch.zeros((slots, 1 + N), dtype=torch.int32, device=dev)
    invalid = torch.zeros((slots,), dtype=torch.int32, device=dev)
    status = torch.zeros((slots,), dtype=torch.int32, device=dev)
    for i in range(n):
        nat.check(L.sn_league_step(env._h, nat.ptr(acts), nat.ptr(rew[i]), nat.ptr(played[i]), nat.ptr(rec),
                                   nat.ptr(invalid), nat.ptr(status), env._stream()), "sn_league_step")
    return rew.cpu(), played.cpu(), rec.cpu()


@pytest.mark.parametrize("at", [1, 4, 9])
def test_tournament_handle_resumes_mid_round(at):
    """A league checkpoint lies between rounds, where the next sn_reset redraws the seats, re-deals and restarts
    the MCS card memory; the seat words, the card memory and the games of a tournament handle are live state
    only inside a round.  So: a handle with two MCS seats is saved after `at` steps of a round and loaded into
    a freshly configured twin, which must finish the round as the saved handle does -- the MCS searches deal
    their opponents from the card memory, the step resolves the seats by the seat word."""
    from rl_6_nimmt import agents as A
    from rl_6_nimmt.league import BatchedTournament

    def make():
        t = BatchedTournament(B, 2, 4, seed=6, game_offset=20, fused=False)
        t.add_player("m0", A.MCSAgent(mc_max=20))
        t.add_player("h0")
        t.add_player("m1", A.MCSAgent(mc_max=20, mc_per_card=2))
        t.add_player("h1")
        t._start()
        return t

    a, b = make(), make()
    _league_steps(a, at, reset=True)
    sd = a.env.state_dict()
    h, f = S.unpack_host(sd["blob"].numpy())
    assert h["league"] == 1 and h["lg_phase"] == at and h["lg_K"] == 4
    assert list(h["lg_kind"][:4]) == [1, 0, 1, 0] and list(h["lg_mpc"][:4]) == [10, 10, 2, 10]
    k, ids = a.seats()
    k, ids = k.cpu().numpy(), ids.cpu().numpy()
    assert np.array_equal(f["lgs"] & 15, k)
    for p in range(4):
        seat = (f["lgs"] >> (4 + 4 * p)) & 15
        assert np.array_equal(seat[k > p], ids[:, p][k > p])
        mcs = (k > p) & ((ids[:, p] == 0) | (ids[:, p] == 2))  # a seated MCS agent remembers cards; nobody else does
        assert bool((f["lmem"][mcs, p] != 0).any(axis=1).all()) and not f["lmem"][~mcs, p].any()
    b.env.load_state_dict(sd)
    ra, rb = _league_steps(a, 10 - at, reset=False), _league_steps(b, 10 - at, reset=False)
    for x, y in zip(ra, rb):
        assert torch.equal(x, y)
    assert bool((ra[2][:, 0] != 0).all())  # every slot's game ended and left its record
    assert torch.equal(a.env.state_dict()["blob"], b.env.state_dict()["blob"])
    ra, rb = _league_steps(a, 10, reset=True), _league_steps(b, 10, reset=True)  # and the next round
    for x, y in zip(ra, rb):
        assert torch.equal(x, y)
    assert a.env.pipe_errors() == 0 and b.env.pipe_errors() == 0
    a.close(), b.close()


def _roundtrip(t, tmp_path):
    from rl_6_nimmt.league import BatchedTournament

    path = str(tmp_path / "league.pt")
    t.save(path)
    return BatchedTournament.load(path)


def _same_league(a, b, same_calls=True):
    """same_calls: both leagues played the same play_games calls, so their tallies were folded from the same
    record blocks and every figure is bit-equal.  Else (one played 3 games in one call, the other 1 + 2) the
    integer tallies, the Elo (a sequential replay) and the winner are still equal, but the relative-position
    column is a float64 sum of the same fractions folded block by block (league._fold: one GEMM per block), in
    another order: each sum of n terms x_i >= 0 is within (n - 1) 2^-53 sum(x) of the exact one to first order
    (the bound of floating-point summation in any order), so the two lie within n 2^-52 sum(x) of each other,
    which is what is asked of that column."""
    ra, rb = torch.cat([r for r, _ in a.records]).cpu(), torch.cat([r for r, _ in b.records]).cpu()
    assert torch.equal(ra, rb)
    sa, sb = a.agent_stats(), b.agent_stats()
    if same_calls:
        assert torch.equal(sa, sb)
    else:
        for col in (0, 1, 3):  # games, score, wins: sums of integers, exact in any order
            assert torch.equal(sa[:, col], sb[:, col]), col
        n, tot = sa[:, 0], torch.maximum(sa[:, 2], sb[:, 2])
        assert bool(((sa[:, 2] - sb[:, 2]).abs() <= n * 2.0 ** -52 * tot).all())
    assert np.array_equal(a.replay_elo(), b.replay_elo())
    assert a.total_games == b.total_games and a.q6_slot_rounds == b.q6_slot_rounds
    assert a.winner().__name__ == b.winner().__name__


def test_fused_league(tmp_path):
    """130 slots, four DrunkHamsters: 1 game, save / load, 2 games.  Against 3 games in one call (records, the
    integer tallies, Elo and winner equal; the position sums to their rounding, see _same_league) and, bit for
    bit in everything, against an uninterrupted league that makes the same two calls."""
    from rl_6_nimmt.league import BatchedTournament

    def make():
        t = BatchedTournament(B, 2, 4, seed=2, game_offset=7)
        for i in range(4):
            t.add_player(f"h{i}")
        return t

    ref, ctl, t = make(), make(), make()
    ref.play_games(3)
    ctl.play_games(1), ctl.play_games(2)
    t.play_games(1)
    u = _roundtrip(t, tmp_path)
    assert u.mode == "fused" and u.names == t.names
    u.play_games(2)
    _same_league(ctl, u)
    _same_league(ref, u, same_calls=False)
    _same_league(ref, ctl, same_calls=False)  # the uninterrupted league stands to `ref` as the resumed one does
    assert u.env.pipe_errors() == 0
    for x in (ref, ctl, t, u):
        x.close()


def _mixed(train, acer=False, slots=96):
    from rl_6_nimmt import agents as A
    from rl_6_nimmt.league import BatchedTournament

    torch.manual_seed(11)
    t = BatchedTournament(slots, 2, 4, seed=3, game_offset=40, fused=False, train=train)
    t.add_player("h")
    t.add_player("m", A.MCSAgent(mc_max=20))
    t.add_player("p", A.PUCTAgent(mc_max=20))
    q = A.DDQN_PRBAgent(history_length=64, minibatch=16)
    q.eps = 0.3
    t.add_player("q", q)
    if acer:
        t.add_player("a", A.BatchedACERAgent(minibatch=2))
    return t


def test_mixed_league_exact(tmp_path):
    """DrunkHamster, MCS, PUCT and an epsilon-greedy DDQN_PRB seat, no training: 4 rounds = 2 rounds, save / load
    into a new object, 2 rounds -- bit for bit (the step counters, seat words, card memory and streams all count)"""
    ref, t = _mixed(False), _mixed(False)
    ref.play_games(2), ref.play_games(2)
    t.play_games(2)
    u = _roundtrip(t, tmp_path)
    assert u is not t and u.env is not t.env
    assert {n: e.step_id for n, e in u.engines.items()} == {n: e.step_id for n, e in t.engines.items()}
    assert u.engines["p"].step_id == 20
    u.play_games(2)
    _same_league(ref, u)
    assert u.env.pipe_errors() == 0
    for x in (ref, t, u):
        x.close()


def _tensors(obj, prefix=""):
    """every tensor under a nest of dicts / lists / tuples, by path"""
    out = {}
    if torch.is_tensor(obj):
        out[prefix] = obj.detach().cpu()
    elif isinstance(obj, dict):
        for k, v in obj.items():
            out.update(_tensors(v, f"{prefix}/{k}"))
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            out.update(_tensors(v, f"{prefix}/{i}"))
    return out


def _training_state(t):
    """everything the round trip must keep, as {path: CPU tensor or plain value}"""
    st = {}
    for n in t.names:
        a = t.agents[n]
        st.update(_tensors(a.state_dict(), f"{n}/param"))
        if getattr(a, "optimizer", None) is not None:
            st.update(_tensors(a.optimizer.state_dict()["state"], f"{n}/optim"))
    for n, e in t.engines.items():
        st[f"{n}/step_id"], st[f"{n}/rows_evaluated"] = e.step_id, e.rows_evaluated
    q = t.engines["q"]
    st["q/tree"], st["q/pointer"], st["q/len"], st["q/beta"] = q.replay.tree().cpu(), q.replay.pointer, len(q.replay), q.replay.beta
    st["q/rows"] = q.replay.gather(torch.arange(q.replay.capacity, dtype=torch.int32, device=t.env.device)).cpu()
    st["q/episode"], st["q/update_count"], st["q/eps_history"] = q.episode, q.update_count, list(q.eps_history)
    a = t.engines["a"]
    for k in ("rep_rows", "rep_act", "rep_logp", "rep_rew"):
        st[f"a/{k}"] = getattr(a, k).cpu()
    st["a/episodes"], st["a/rep_nd"], st["a/gen"] = a.episodes, list(a.rep_nd), a._gen.get_state().cpu()
    st["torch_rng"], st["device_rng"] = torch.get_rng_state(), torch.cuda.get_rng_state(t.env.device)
    st["optimizer_steps"] = dict(t.optimizer_steps)
    return st


def _weights(t):
    return {k: v for k, v in _training_state(t).items() if "/param" in k}


def test_training_state_round_trip(tmp_path):
    """the mixed roster plus ACER, training: after 2 rounds, save / load restores every parameter, optimiser
    tensor, replay, counter and generator state bit for bit; 2 more rounds stay within the spread of two
    uninterrupted controls: bit-equal to them when they are bit-equal, else within 4x their largest absolute
    weight difference (one pair underestimates the spread).  Prints which case held (on the MI355X: the
    controls were bit-equal)."""
    def run(rounds):
        t = _mixed(True, acer=True)
        for _ in range(rounds):
            t.play_games(1)
        return t

    t = run(2)
    saved = _training_state(t)
    assert any("/optim" in k for k in saved) and saved["q/len"] > 0 and saved["a/episodes"] == 2
    u = _roundtrip(t, tmp_path)
    loaded = _training_state(u)
    assert saved.keys() == loaded.keys()
    for k, v in saved.items():
        w = loaded[k]
        assert torch.equal(v, w) if torch.is_tensor(v) else v == w, k
    u.play_games(1), u.play_games(1)
    wu = _weights(u)
    t.close()
    c1 = run(4)
    w1 = _weights(c1)
    c1.close()
    c2 = run(4)
    w2 = _weights(c2)
    c2.close()
    spread = max(float((w1[k].double() - w2[k].double()).abs().max()) for k in w1)
    diff = max(float((w1[k].double() - wu[k].double()).abs().max()) for k in w1)
    if spread == 0.0:
        print("controls bit-equal: the loaded league must equal them")
        for k in w1:
            assert torch.equal(w1[k], wu[k]), k
    else:
        print(f"controls differ by {spread:.3e}; the loaded league differs from control 1 by {diff:.3e}")
        assert diff <= 4.0 * spread
    u.close()
