"""The PUCT rollout kernels (sechs_puct.hip) pinned word for word at every
player count and group size.

A crafted actor makes the policy deterministic: every candidate's logit is
+-S * nrm(card) and nothing else, so softmax puts all of its float32 mass on
a seat's highest (or lowest) card and Categorical.sample returns it for
every uniform (tests/test_puct_cpu.py proves the logit gap on the CPU).  A
search is then a pure function of the dealt rollout states, and a plain
Python model -- the oracle's Game for the rules, a numpy float64 restatement
of PUCTAgent._compute_pucts (mcts.py:282-315) for the root choice, the
backup of mcts.py:100 -- predicts every word of `stats` and `hist` and the
move played.  The three step forms (sn_puct_rollouts, k_puct_step_seats,
k_puct_step) are each compared with that model, not merely with each other.

Instantiations held to the model (N, lanes L, form, decisions per group):
  test_search_equals_oracle_model[N-n-polarity]
      k_puct_rollouts<N,L>, (3,4) (4,4) (5,8) (6,8) (7,8) (8,8), one decision per group;
      k_puct_step_seats<N,L>, (2,2) (3,4) (4,4) (5,8) (6,8) (7,8) (8,8);
      k_puct_step<N>, N = 2..10;  k_puct_deal<N> and k_puct_deal_batch<N>, N = 2..10
  test_rollout_groups_equal_oracle_model[N]
      k_puct_rollouts<N,L>, N = 3, 4, 5, 7, 8 at 1, 2, 3 and 8 (L = 4) or 4 (L = 8) decisions per group
  test_tournament_search_equals_oracle_model[polarity]
      the three N = 6, L = 8 forms on games of 2..6 players (absent-seat lanes), the fused one at 4 per group
The crafted policy prefers the same hand index at every seat, so which seat's
logits a lane reads is pinned separately: by the model again, with logits
written by the test that prefer another index at every seat and step, and by
bit equality of the forms under a stochastic policy:
  test_step_kernels_read_each_seats_own_logits[N]      k_puct_step_seats / k_puct_step, N = 2, 3, 5, 8, 9, 10
  test_step_forms_agree_under_a_stochastic_policy[N]   N = 2..8, the fused form at 1 and the most per group
  test_host_sized_groups_equal_step_launches[N]        the library's own group sizing at its maximum (L = 4, 8)
"""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

S_LOGIT = 2.0 ** 14  # logit scale: adjacent cards end up >= 150 apart (test_puct_cpu.py)
MC_MAX, MC_PER_CARD = 12, 3
# the root policy is one-hot here, and at the reference's c_puct = 2 the exploration term of its one move
# outweighs every other move's q in [0, 1] for all 12 rollouts: every backup would land in the same words.
# At 0.25 the unvisited moves' q = 0.5 (later the normalised median) wins whenever the preferred card did
# badly, and a search backs up into several moves
C_PUCT = 0.25


# ---------------------------------------------------------------- the crafted actor
def crafted_weights(polarity, scale=S_LOGIT):
    """state dict of make_actor() whose logit is polarity * scale * row[0] (the normalised card): hidden units
    0 / 1 of layer 1 read +- column 0, layer 2 passes them through, the head weighs them +- scale; every other
    weight and every bias is 0, so nothing is added in front of a ReLU and nothing but nrm(card) is rounded"""
    from rl_6_nimmt.puct import make_actor

    w = {k: torch.zeros_like(v) for k, v in make_actor().state_dict().items()}
    w["latent_net.0.weight"][0, 0], w["latent_net.0.weight"][1, 0] = 1.0, -1.0
    w["latent_net.2.weight"][0, 0], w["latent_net.2.weight"][1, 1] = 1.0, 1.0
    w["head_nets.0.0.weight"][0, 0], w["head_nets.0.0.weight"][0, 1] = polarity * scale, -polarity * scale
    return w


# ---------------------------------------------------------------- the host model
def puct_choose_ref(st, hist, probs, n, c_puct):
    """PUCTAgent._compute_pucts + the argmax loop (mcts.py:282-315) on the kernels' statistics words (sums[10]
    counts[10] total min max, outcome histogram -171..0), in numpy with the reference's types: c_puct * probs
    float32, everything else float64; the median of all outcomes fills unvisited moves once 10 are in; strict
    '>' from -inf, so the first index wins ties and NaN never wins.  Returns (choice, pucts)."""
    st = np.asarray(st)
    cnt = st[10:10 + n].astype(np.int64)
    total, n_total = int(st[20]), int(cnt.sum())
    if total < 10:
        mx, mn, med = 0.0, -10.0, -5.0
    else:
        mx, mn = float(st[22]), float(st[21])
        med = float(np.median(np.repeat(np.arange(-171, 1), np.asarray(hist))))
    with np.errstate(all="ignore"):
        q = np.where(cnt > 0, st[:n].astype(np.float64) / np.maximum(cnt, 1), med)
        q = np.clip((q - mn) / np.float64(mx - mn), 0.0, 1.0)
        t = (np.float32(c_puct) * np.asarray(probs[:n], dtype=np.float32)).astype(np.float64)
        pucts = q + t * np.sqrt(np.float64(n_total) + 1e-9) / (1.0 + cnt)
    best, choice = -math.inf, 0
    for k in range(n):
        if pucts[k] > best:
            best, choice = pucts[k], k
    return choice, pucts


def model_search(n, deals, probs, pick, c_puct):
    """one decision's search: deals = [(board rows, hands of the game's seats)] per rollout, seat 0 the decider.
    At step t of rollout r seat q plays pick(r, t, q, its sorted hand), except seat 0 at the first step, which
    plays the root choice; the outcome is the sum of seat 0's rewards (minus its penalties).  Returns (stats
    [24], hist [172], index of the best-mean move)."""
    from oracle import oracle as O

    st = np.zeros(24, dtype=np.int32)
    st[21], st[22] = 1, -1000  # k_puct_init's min / max before the first backup
    hist = np.zeros(172, dtype=np.int32)
    for r, (board, hands) in enumerate(deals):
        first, _ = puct_choose_ref(st, hist, probs, n, c_puct)
        game = O.Game(len(hands))
        game.set_position(board, hands)
        hs = [list(h) for h in hands]
        outcome = 0
        for t in range(n):
            acts = [pick(r, t, q, h) for q, h in enumerate(hs)]
            if t == 0:
                acts[0] = hs[0][first]
            for h, a in zip(hs, acts):
                h.remove(a)
            bad, rew = game.step(acts)
            assert bad == -1
            outcome += int(rew[0])
        st[first] += outcome
        st[10 + first] += 1
        st[20] += 1
        st[21] = outcome if st[20] == 1 else min(st[21], outcome)
        st[22] = outcome if st[20] == 1 else max(st[22], outcome)
        hist[outcome + 171] += 1
    best, bm = 0, -math.inf
    for k in range(n):  # _choose_action_from_outcomes (mcts.py:156-165): strict '>'
        if st[10 + k] and st[k] / st[10 + k] > bm:
            best, bm = k, st[k] / st[10 + k]
    return st, hist, best


# ---------------------------------------------------------------- the dealt states
_CARD_LUT = (np.float32(-1.0) + (np.float32(2.0) * np.arange(-1, 104).astype(np.float32)) / np.float32(103.0))


def _cards_of(x):
    """invert nrm(card, 0, 103) in f32 by table (card -1 = an empty slot)"""
    c = np.rint((x.astype(np.float64) + 1.0) * 103.0 / 2.0).astype(np.int64)
    assert c.min() >= -1 and c.max() <= 103 and np.array_equal(_CARD_LUT[c + 1], x)
    return c


def dealt_states(env, eng, n, players):
    """the initial rollout states of the search eng.decide(n) is about to run (call right before it): every
    rollout dealt by sn_puct_deal_batch -- and by one sn_puct_deal each, which must agree -- decoded to
    (board rows, hands) lists [nr][D], with the deal's invariants asserted on every one.  Hands come from the
    packed words (byte k of a seat's three words = its k-th card, 0xFF empty), the board from sn_puct_rows in
    f32.  players [D]: the seats of each decision's game."""
    from rl_6_nimmt import _native as nat

    L, h, st = nat.lib(), env._h, env._stream()
    N, D, nr = env.num_players, eng.D, eng.n_mc(n)
    eng.memorize()
    q = eng._params(n)
    buf = torch.zeros((nr, D, 48), dtype=torch.int32, device=env.device)
    nat.check(L.sn_puct_deal_batch(h, ctypes.byref(q), 0, nr, buf.data_ptr(), st), "sn_puct_deal_batch")
    rows = torch.empty((nr, D * N * n, 48), dtype=torch.float32, device=env.device)
    for r in range(nr):
        q.rollout = r
        nat.check(L.sn_puct_deal(h, ctypes.byref(q), st), "sn_puct_deal")
        torch.cuda.synchronize()
        assert torch.equal(eng.ro[:D], buf[r]), r
        q.rollouts = buf[r].data_ptr()
        nat.check(L.sn_puct_rows(h, ctypes.byref(q), n, nat.ptr(rows[r]), 0, st), "sn_puct_rows")
        q.rollouts = eng.ro.data_ptr()
    torch.cuda.synchronize()
    ro = buf.cpu().numpy()
    assert (ro[:, :, 40] == 0).all() and (ro[:, :, 41] == -1).all()
    hb = np.ascontiguousarray(ro[:, :, 8:8 + 3 * N]).view(np.uint8).reshape(nr, D, N, 12).astype(np.int64)
    assert (hb[..., 10:] == 0xFF).all()
    hands = np.where(hb[..., :10] == 0xFF, -1, hb[..., :10])  # [nr, D, N, 10]
    board = _cards_of(rows.view(nr, D, N, n, 48)[:, :, 0, 0, 24:].cpu().numpy()).reshape(nr, D, 4, 6)
    # seat 0's row also carries its hand: the same cards as the packed words
    assert np.array_equal(_cards_of(rows.view(nr, D, N, n, 48)[:, :, 0, 0, 1:11].cpu().numpy()), hands[:, :, 0])
    flat = eng.decider_index().cpu().numpy()
    real = env.hands().cpu().numpy().astype(np.int64).reshape(-1, 10)[flat]          # [D, 10]
    real_board = env.board().cpu().numpy().astype(np.int64)[flat // N]               # [D, 4, 6]
    av = eng.avail.cpu().numpy().view(np.uint32)[:, flat]                              # [4, D]
    in_avail = ((av[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1).transpose(1, 0, 2).reshape(D, 128)
    out = []
    for r in range(nr):
        per_d = []
        for d in range(D):
            kp = int(players[d])
            assert np.array_equal(hands[r, d, 0], real[d]) and (real[d, :n] >= 0).all() and (real[d, n:] < 0).all()
            assert np.array_equal(board[r, d], real_board[d])
            hs = [[int(c) for c in hands[r, d, p] if c >= 0] for p in range(N)]
            assert all(len(hs[p]) == n and hs[p] == sorted(hs[p]) for p in range(kp)), (r, d, hs)
            assert all(not hs[p] for p in range(kp, N)), (r, d, hs)
            rows_ = [[int(c) for c in row if c >= 0] for row in board[r, d]]
            assert all(1 <= len(row) <= 5 for row in rows_)
            cards = [c for x in hs + rows_ for c in x]
            assert len(set(cards)) == len(cards), (r, d)  # hands pairwise disjoint, and disjoint from the board
            assert all(in_avail[d, c] for p in range(1, kp) for c in hs[p]), (r, d)
            per_d.append((rows_, hs[:kp]))
        out.append(per_d)
    return out


# ---------------------------------------------------------------- a search against the model
FORMS = {"fused": ("1", "1"), "seats": ("0", "1"), "lane": ("0", "0")}  # SECHS_PUCT_ROLLOUTS, SECHS_PUCT_STEP_SEATS


def forms_of(N):
    """the step forms sn_puct_* has for N players: whole rollouts in one kernel for 3..8, a lane per seat up to
    8 (sn_puct_step takes the one-lane kernel above that whatever the knob says), a lane per decision always"""
    return [f for f in FORMS if (f != "fused" or 3 <= N <= 8) and (f != "seats" or N <= 8)]


def set_form(monkeypatch, form, group=None):
    ro, lanes = FORMS[form]
    monkeypatch.setenv("SECHS_PUCT_ROLLOUTS", ro)
    monkeypatch.setenv("SECHS_PUCT_STEP_SEATS", lanes)
    if group is None:
        monkeypatch.delenv("SECHS_PUCT_GROUP", raising=False)
    else:
        monkeypatch.setenv("SECHS_PUCT_GROUP", str(group))


def position_of(env, eng):
    return env.board().cpu(), env.hands().cpu(), eng.avail.cpu().clone(), eng.step_id


def search_and_compare(env, eng, n, polarity, players, model, tag):
    """run eng.decide(n) and hold stats, hist, the best index and the cards played to the model's; `model`: a
    dict filled by the first form that gets here (the deal does not depend on the step form) and reused"""
    D = eng.D
    eng.memorize()
    if "want" not in model:
        deals = dealt_states(env, eng, n, players)
        model["position"] = position_of(env, eng)
    else:  # the same position as the modelled one, reached through this form's own searches
        for a, b in zip(position_of(env, eng), model["position"]):
            assert (a == b) if isinstance(a, int) else torch.equal(a, b), tag
    acts = eng.decide(n).clone()
    torch.cuda.synchronize()
    probs = eng.root_probs[:D].cpu().numpy()
    hot = np.zeros((D, 10), dtype=np.float32)
    hot[:, n - 1 if polarity > 0 else 0] = 1.0
    assert np.array_equal(probs, hot), tag  # all of the root policy's mass on the preferred card
    if "want" not in model:
        pick = (lambda r, t, q, h: h[-1]) if polarity > 0 else (lambda r, t, q, h: h[0])  # highest / lowest card
        res = [model_search(n, [deals[r][d] for r in range(len(deals))], probs[d], pick, eng.c_puct)
               for d in range(D)]
        model["want"] = (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.array([r[2] for r in res]))
        assert int(model["want"][0][:, 20].min()) >= 10  # the median fill was reached
        assert int((model["want"][0][:, 10:20] > 0).sum()) > D  # the backups spread over several root moves
    st, hist, best = model["want"]
    got_st, got_hist = eng.stats[:D].cpu().numpy(), eng.hist[:D].cpu().numpy()
    bad = np.nonzero((got_st != st).any(axis=1) | (got_hist != hist).any(axis=1))[0]
    assert bad.size == 0, (tag, "decisions", bad[:8], got_st[bad[:1]], st[bad[:1]])
    assert np.array_equal(eng.best_index[:D].cpu().numpy(), best), tag
    flat = eng.decider_index().cpu().numpy()
    real = env.hands().cpu().numpy().reshape(-1, 10)[flat]
    assert np.array_equal(acts.cpu().numpy().reshape(-1)[flat], real[np.arange(D), best]), tag
    return acts


def plain_engine(N, B, mask, polarity, seed=5):
    from rl_6_nimmt.puct import BatchedPUCT, make_actor
    from rl_6_nimmt.vec_env import VecSechsNimmtEnv

    env = VecSechsNimmtEnv(B, N, seed=seed, rng="philox")
    env.reset()
    actor = make_actor()
    actor.load_state_dict(crafted_weights(polarity))
    eng = BatchedPUCT(env, actor, mc_per_card=MC_PER_CARD, mc_max=MC_MAX, c_puct=C_PUCT, seed=seed, seats_mask=mask,
                      net_dtype=torch.bfloat16)
    assert eng.sync_net().fused() is not None  # the MFMA rollout-logit kernels, not the generic path
    return env, eng


def play_to(env, eng, n, mask):
    """step the env to hand size n with the engine's own moves (the other seats play their lowest card)"""
    N = env.num_players
    keep = torch.tensor([(mask >> p) & 1 for p in range(N)], device=env.device, dtype=torch.bool)
    for t in range(10 - n):
        acts = torch.where(keep[None, :], eng.decide(10 - t), env.hands()[:, :, 0].to(torch.int32))
        _, _, inv = env.step(acts)
        assert bool((inv == -1).all())


def shape_of(N):
    """(B, seats_mask): an odd decision count that is no multiple of any group size -- every seat of 37 games
    for N <= 4 (D = 37 N), one middle seat of 41 games above"""
    return (37, (1 << N) - 1) if N <= 4 else (41, 1 << (N // 2))


@pytest.mark.parametrize("polarity", [1, -1], ids=["highest", "lowest"])
@pytest.mark.parametrize("n", [10, 4])
@pytest.mark.parametrize("N", [2, 3, 4, 5, 6, 7, 8, 9, 10])
def test_search_equals_oracle_model(monkeypatch, N, n, polarity):
    """every step form N players have, on a fresh deal (n = 10) and mid-game (n = 4, reached with the engine's
    own moves): stats, hist, best index and the cards played equal the oracle-backed model word for word"""
    B, mask = shape_of(N)
    model = {}
    for form in forms_of(N):
        set_form(monkeypatch, form)
        env, eng = plain_engine(N, B, mask, polarity)
        assert eng.fused_rollouts == (form == "fused") and eng.D == B * bin(mask).count("1")
        play_to(env, eng, n, mask)
        search_and_compare(env, eng, n, polarity, [N] * eng.D, model, (N, n, polarity, form))


@pytest.mark.parametrize("N", [3, 4, 5, 7, 8])
def test_rollout_groups_equal_oracle_model(monkeypatch, N):
    """sn_puct_rollouts with SECHS_PUCT_GROUP decisions per wave's group -- 1, 2, 3 and the most a group holds
    (8 at L = 4, 4 at L = 8) -- on D = 37 decisions, which leaves a ragged last group at each (37 = 4 x 8 + 5 =
    9 x 4 + 1 = 12 x 3 + 1 = 18 x 2 + 1): the decision-of-seat mapping, the cached game / seat words and the
    repeated rows past the last seat all give the model's words"""
    B, mask, n = 37, 1 << (N // 2), 10
    polarity = 1 if N % 2 else -1
    model = {}
    for group in (1, 2, 3, 32 // (4 if N <= 4 else 8)):
        set_form(monkeypatch, "fused", group)
        env, eng = plain_engine(N, B, mask, polarity, seed=11)
        assert eng.fused_rollouts and eng.D == 37
        search_and_compare(env, eng, n, polarity, [N] * eng.D, model, (N, "group", group))


@pytest.mark.parametrize("N", [2, 3, 5, 8, 9, 10])
def test_step_kernels_read_each_seats_own_logits(monkeypatch, N):
    """sn_puct_step driven with logits written here instead of the net's: 200 at index (d + 3 q + t + r) mod
    n_cur of seat q of decision d at step t of rollout r, 0 elsewhere (a gap above 104: the other candidates'
    exp is exactly 0), and a root policy one-hot at d mod n.  Every seat now prefers another hand index at
    every step, so a lane that read a neighbour's logits, or its own at the wrong step width, would play
    another card than the model: the seat-lane kernel and the one-lane kernel (the only form at N = 9, 10)
    against the oracle-backed model, word for word"""
    from rl_6_nimmt import _native as nat

    (B, mask), n = shape_of(N), 10
    for form in [f for f in forms_of(N) if f != "fused"]:
        set_form(monkeypatch, form)
        env, eng = plain_engine(N, B, mask, 1)
        D, nr, dev = eng.D, eng.n_mc(n), env.device
        deals = dealt_states(env, eng, n, [N] * D)
        L, h, st = nat.lib(), env._h, env._stream()
        q = eng._params(n)
        dd, qq = torch.meshgrid(torch.arange(D, device=dev), torch.arange(N, device=dev), indexing="ij")
        root = torch.zeros((D, n), device=dev)
        root[dd[:, 0], dd[:, 0] % n] = 200.0
        nat.check(L.sn_puct_init(h, ctypes.byref(q), nat.ptr(root), st), "sn_puct_init")
        for r in range(nr):
            q.rollout = r
            nat.check(L.sn_puct_deal(h, ctypes.byref(q), st), "sn_puct_deal")
            for t in range(n):
                m = n - t
                lg = torch.zeros((D, N, m), device=dev).scatter_(2, ((dd + 3 * qq + t + r) % m)[..., None], 200.0)
                nat.check(L.sn_puct_step(h, ctypes.byref(q), nat.ptr(lg), t, m, st), "sn_puct_step")
        torch.cuda.synchronize()
        probs = eng.root_probs[:D].cpu().numpy()
        assert np.array_equal(probs.argmax(axis=1), np.arange(D) % n) and (probs.max(axis=1) == 1.0).all()
        got_st, got_hist = eng.stats[:D].cpu().numpy(), eng.hist[:D].cpu().numpy()
        for d in range(D):
            st_, hist_, _ = model_search(n, [deals[r][d] for r in range(nr)], probs[d],
                                         lambda r, t, q, hand, d=d: hand[(d + 3 * q + t + r) % len(hand)], eng.c_puct)
            assert np.array_equal(got_st[d], st_) and np.array_equal(got_hist[d], hist_), (N, form, d, got_st[d], st_)


@pytest.mark.parametrize("N", [2, 3, 4, 5, 6, 7, 8])
def test_step_forms_agree_under_a_stochastic_policy(monkeypatch, N):
    """what the crafted policy cannot see: it prefers the same hand index at every seat, so a seat reading
    another seat's logits would still play the model's card.  With the default actor (a stochastic policy: the
    sampled index depends on the seat's own logits and uniform) the forms N players have -- the fused kernel at
    one decision per group and at the largest group -- must give bit-equal statistics, histograms and moves at
    n = 10 and then n = 9; the logits themselves are held to the f64 net per player count in
    test_gpu_puct.py::test_mlp_seats_kernel_matches_fp32_reference_net_at_other_player_counts"""
    from rl_6_nimmt.puct import BatchedPUCT, make_actor
    from rl_6_nimmt.vec_env import VecSechsNimmtEnv

    B, mask = shape_of(N)
    keep = torch.tensor([(mask >> p) & 1 for p in range(N)], device="cuda", dtype=torch.bool)
    res = {}
    for form, group in [(f, g) for f in forms_of(N) for g in ((1, 32 // (4 if N <= 4 else 8)) if f == "fused" else (None,))]:
        set_form(monkeypatch, form, group)
        env = VecSechsNimmtEnv(B, N, seed=19, rng="philox")
        env.reset()
        torch.manual_seed(0)
        eng = BatchedPUCT(env, make_actor(), mc_per_card=MC_PER_CARD, mc_max=MC_MAX, seed=19, seats_mask=mask,
                          net_dtype=torch.bfloat16)
        assert eng.fused_rollouts == (form == "fused")
        acts = [eng.decide(10).clone()]
        env.step(torch.where(keep[None, :], acts[0], env.hands()[:, :, 0].to(torch.int32)))
        acts.append(eng.decide(9).clone())
        torch.cuda.synchronize()
        res[form, group] = (acts, eng.stats.clone(), eng.hist.clone())
    assert len(res) >= 2
    first = next(iter(res.values()))
    assert len(torch.unique(first[1][:, 10:20].argmax(dim=1))) > 2  # the searches differ from each other
    for key, got in res.items():
        assert all(torch.equal(a, b) for a, b in zip(got[0], first[0])), key
        assert torch.equal(got[1], first[1]) and torch.equal(got[2], first[2]), key


@pytest.mark.parametrize("N", [4, 7])
def test_host_sized_groups_equal_step_launches(monkeypatch, N):
    """the library's own group sizing above one decision per group, no knob: D = 8 cus (max - 1) + 37 decisions
    make sn_puct_rollouts' formula pick the largest group (restated here from the device's CU count) with a
    ragged last one.  The model would be too slow there: statistics, histograms and moves must be bit-equal to
    the launch-per-step loop's, over a stochastic policy (the default actor), n = 10 then 9."""
    from rl_6_nimmt.puct import BatchedPUCT, make_actor
    from rl_6_nimmt.vec_env import VecSechsNimmtEnv

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    dg_max = 32 // (4 if N <= 4 else 8)
    D = 8 * cus * (dg_max - 1) + 37
    slots = 8 * cus
    rounds = max(1, -(-D // (dg_max * slots)))
    assert min(dg_max, max(1, -(-D // (rounds * slots)))) == dg_max and D % dg_max  # sn_puct_rollouts' sizing
    res = {}
    for form in ("fused", "seats"):
        set_form(monkeypatch, form)
        env = VecSechsNimmtEnv(D, N, seed=23, rng="philox")
        env.reset()
        torch.manual_seed(0)
        eng = BatchedPUCT(env, make_actor(), mc_per_card=2, mc_max=4, seed=23, seats_mask=0b10,
                          net_dtype=torch.bfloat16)
        assert eng.D == D and eng.fused_rollouts == (form == "fused")
        acts = [eng.decide(10).clone()]
        env.step(torch.where(torch.arange(N, device=env.device)[None, :] == 1, acts[0],
                             env.hands()[:, :, 0].to(torch.int32)))
        acts.append(eng.decide(9).clone())
        torch.cuda.synchronize()
        res[form] = (acts, eng.stats.clone(), eng.hist.clone())
    assert all(torch.equal(a, b) for a, b in zip(res["fused"][0], res["seats"][0]))
    assert torch.equal(res["fused"][1], res["seats"][1]) and torch.equal(res["fused"][2], res["seats"][2])
    assert int(res["fused"][1][:, 20].min()) == 4  # every decision backed up its four rollouts


@pytest.mark.parametrize("polarity", [1, -1], ids=["highest", "lowest"])
def test_tournament_search_equals_oracle_model(monkeypatch, polarity):
    """a 2..6-player tournament's decision list (an N = 6 handle, L = 8 lanes per decision, games of fewer
    players leaving absent-seat lanes): the PUCT agent's seats searched by each of the three forms, the fused
    one at the largest group, against the model with each game's players taken from the seats words"""
    from rl_6_nimmt import _native as nat
    from rl_6_nimmt.agents import DrunkHamster, PUCTAgent
    from rl_6_nimmt.league import BatchedTournament

    model = {}
    for form in forms_of(6):
        set_form(monkeypatch, form, 4 if form == "fused" else None)
        t = BatchedTournament(53, 2, 6, seed=13)
        agent = PUCTAgent(c_puct=C_PUCT, mc_max=MC_MAX, mc_per_card=MC_PER_CARD)
        agent.actor.load_state_dict(crafted_weights(polarity))
        t.add_player("P", agent)
        for i in range(5):
            t.add_player(f"R{i}", DrunkHamster())
        t._start()
        assert t.mode == "step"
        env = t.env
        nat.check(nat.lib().sn_reset(env._h, None, env._stream()), "sn_reset")  # a seat draw + deal
        t._use_decisions()
        eng = t.engines["P"]
        if eng.D % 4 == 0:  # keep the last group of four ragged
            eng.use_decisions(eng.dec[:-1])
        kk, _ = t.seats()
        players = kk.cpu().numpy()[eng.dec.cpu().numpy() // 6]
        assert eng.D > 8 and eng.D % 4 and players.min() == 2 and players.max() == 6  # absent seats on the list
        assert eng.fused_rollouts == (form == "fused") and eng.sync_net().fused() is not None
        search_and_compare(env, eng, 10, polarity, players, model, ("league", polarity, form))
        t.close()
