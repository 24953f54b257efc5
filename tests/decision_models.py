"""Host models of the decision kernels' Philox draws, and the inputs the tests feed those kernels.

Every stochastic choice a net agent makes on the device is drawn from one stream layout (csrc/sechs_decide.h,
dec_stream; its host owner is rl_6_nimmt/engine.py: dec_stream_host, decision_words_host).  The models here restate
what each consumer does with its words, so a test can predict every single draw instead of a frequency:

  select_model   k_dqn_select / k_dqn_select_duel: explore or not, and the explored hand index.  Exact.
  sample_model   sample_softmax / sample_row (k_policy_sample, the rollout step kernels) in float64.  The device
                 uses __expf and float32 sums, so a decision whose target lies within BAND of a boundary of the
                 cumulative sum may fall on either side of that boundary; every other decision is exact.
  deal_model     deal_one (k_puct_deal, k_puct_deal_batch): the opponents' hands of a rollout.  Exact.
  step_model     the policy sample of seat q of a rollout game at rollout step t.  The band of sample_model.

BAND = 2^-14 (6.1e-5, relative to the sum) is about 20 times an estimated device deviation of 3e-6: ten float32
additions at 2^-24 each, __expf's argument rounding |x - m| log2(e) 2^-24 for |x - m| <= 16, and one ulp on the
result.  That estimate is not a measurement; a mismatch outside the band is a finding to explain, never a reason
to widen it.  Test logits stay within |x| <= 8 so that |x - m| <= 16 holds, and at most MAX_AMBIGUOUS (1 %) of a
test's decisions may lie in the band: test_decision_models_cpu.py asserts that share from the model alone for the
inputs below, which are the very arrays the GPU tests upload (tests/test_gpu_decision_streams.py).
"""
import numpy as np

from rl_6_nimmt.engine import SAMPLE_TAG, SELECT_TAG, dec_stream_host, decision_words_host

BAND = 2.0 ** -14
MAX_AMBIGUOUS = 0.01
LOGIT_MAX = 8.0


# ---------------------------------------------------------------- the models
def uniform24(word):
    """the kernels' 24-bit uniform of a Philox word: f32(word >> 8) * 2^-24, in numpy float32 (exact)"""
    return (np.asarray(word, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def select_model(words, eps, n):
    """dqn_select's draws: words [..., 4] -> (explore [...] bool, explore index [...] int64).  u1 = word 0, u2 =
    word 1; a seat explores iff not (eps <= 0 or (eps < 1 and float64(u1) > eps)); the explored index is
    min(int(u2 * f32(n)), n - 1) with the product in float32.  A seat that does not explore plays greedily."""
    words = np.asarray(words, dtype=np.uint32)
    u1, u2 = uniform24(words[..., 0]), uniform24(words[..., 1])
    eps = float(eps)
    if eps <= 0.0:
        greedy = np.ones(u1.shape, dtype=bool)
    elif eps < 1.0:
        greedy = u1.astype(np.float64) > eps
    else:
        greedy = np.zeros(u1.shape, dtype=bool)
    prod = u2 * np.float32(n)
    assert prod.dtype == np.float32
    return ~greedy, np.minimum(prod.astype(np.int64), n - 1)


def sample_model(logits, u):
    """Categorical(softmax(logits)).sample() by inversion, float64: logits [..., n], u [...] ->
    (index, dist, near).  e = exp(x - max), target = u * sum, index = the first k < n - 1 with cumsum[k] > target,
    else n - 1.  dist = min_k |cumsum[k] - target| / sum and near = that k: the boundary between the indices near
    and near + 1 is the one the target is closest to."""
    x = np.asarray(logits, dtype=np.float64)
    n = x.shape[-1]
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    total, cs = e.sum(axis=-1), np.cumsum(e, axis=-1)
    target = np.asarray(u, dtype=np.float64) * total
    hit = cs > target[..., None]
    hit[..., n - 1] = True  # no k < n - 1 exceeds the target: n - 1, whatever cumsum[n - 1] is
    index = hit.argmax(axis=-1)
    gap = np.abs(cs - target[..., None])
    return index, gap.min(axis=-1) / total, gap.argmin(axis=-1)


def sample_allowed(logits, u):
    """the band rule: (index, ambiguous, lo, hi).  A decision with dist < BAND is ambiguous and the device may
    return lo or hi, the indices on either side of the nearest boundary; every other decision returns index."""
    index, dist, near = sample_model(logits, u)
    n = np.asarray(logits).shape[-1]
    amb = dist < BAND
    return index, amb, np.where(amb, near, index), np.where(amb, np.minimum(near + 1, n - 1), index)


def check_sample(got, logits, u, what):
    """hold sampled indices `got` to sample_model under the band rule (check_allowed)"""
    return check_allowed(got, *sample_allowed(logits, u), what)


def check_allowed(got, index, amb, lo, hi, what):
    """hold sampled indices `got` to sample_allowed's result; returns and prints the three numbers a sampling
    test reports: decisions compared, decisions in the band, and how many of those differ from the float64
    model's index"""
    got = np.asarray(got, dtype=np.int64)
    assert got.shape == index.shape, (what, got.shape, index.shape)
    differ = int((amb & (got != index)).sum())
    print(f"[decision-streams] {what}: compared {got.size}, in the band {int(amb.sum())}, of those differing {differ}")
    assert amb.mean() <= MAX_AMBIGUOUS, (what, "ambiguous share", float(amb.mean()))
    bad = np.nonzero(~((got == lo) | (got == hi)))
    assert bad[0].size == 0, (what, "decisions", [b[:8] for b in bad], "got", got[bad][:8], "model", index[bad][:8],
                              "band", amb[bad][:8])
    return got.size, int(amb.sum()), differ


def deal_from_draws(draw, avail_cards, n, players, seats=None):
    """deal_one's order: for each opponent seat q = 1 .. players - 1, n draws k = draw(left - 1), each removing the
    k-th smallest card of the memory, until the memory is empty; hands sorted (hand_from_set); the seats from
    `players` up to `seats` get empty hands.  Returns the hands of seats 1 .. seats - 1."""
    mem = sorted(int(c) for c in avail_cards)
    hands = []
    for q in range(1, players if seats is None else seats):
        hand = []
        for _ in range(n):
            if not mem or q >= players:
                break
            hand.append(mem.pop(int(draw(len(mem) - 1))))
        hands.append(sorted(hand))
    return hands


def deal_model(seed, step, gid, seat, rollout, avail_cards, n, players, seats=None):
    """the opponents' hands rollout `rollout` deals for the decision of (global game gid, seat): the oracle's
    numpy-legacy interval draws on the Philox stream dec_stream_host(gid, seat, rollout) keyed seed ^ step"""
    from oracle import oracle as O

    key = (int(seed) & (2**64 - 1)) ^ (int(step) & 0xFFFFFFFF)
    rng = O.Rng(O.RNG_PHILOX, key, int(dec_stream_host(gid, seat, rollout)))
    return deal_from_draws(rng.interval, avail_cards, n, players, seats)


def step_uniforms(seed, step, gid, seat, rollout, t, num_seats):
    """the uniform of every seat q < num_seats of the rollout games of decisions (gid [D], seat [D]) at rollout
    step t: word 0 at the counter q on the stream with the tag `rollout` and the low byte 1 + t -> [D, num_seats]"""
    gid, seat = np.asarray(gid, dtype=np.uint64)[:, None], np.asarray(seat, dtype=np.uint64)[:, None]
    w = decision_words_host(seed, step, gid, seat, rollout, 1 + t, np.arange(num_seats)[None, :])
    return uniform24(w[..., 0])


def step_model(seed, step, gid, seat, rollout, t, logits):
    """sample_allowed for every seat of every rollout game: logits [D, num_seats, n_cur]"""
    return sample_allowed(logits, step_uniforms(seed, step, gid, seat, rollout, t, np.asarray(logits).shape[1]))


def sample_uniforms(seed, step, gid, seat):
    """k_policy_sample's uniform: word 0 at the counter 0 under SAMPLE_TAG"""
    return uniform24(decision_words_host(seed, step, gid, seat, SAMPLE_TAG, 0, 0)[..., 0])


def select_words(seed, step, gid, seat):
    """dqn_select's words: the counter 0 under SELECT_TAG"""
    return decision_words_host(seed, step, gid, seat, SELECT_TAG, 0, 0)


# ---------------------------------------------------------------- the tests' inputs
B, N, MASK = 130, 4, 0b0101  # 260 decisions: past a wave and a block, a ragged tail (test_gpu_dqn_batched.py's size)
SEED = 0x1234567890ABCDEF    # both key words carry bits
SAMPLE_STEPS = 16            # 16 x 260 = 4 160 decisions per sampling case
SELECT_STEPS = 4
SCALES = (1.5, 4.0)


def deciders(num_games, num_seats, mask, game_offset=0):
    """(gid [D], seat [D]) of a seats-mask handle in decision order; gid = game_offset + g in uint64"""
    seats = [p for p in range(num_seats) if (mask >> p) & 1]
    gid = (np.uint64(game_offset) + np.repeat(np.arange(num_games, dtype=np.uint64), len(seats)))
    return gid, np.tile(np.array(seats, dtype=np.uint64), num_games)


def normal_logits(key, shape, scale):
    """float32 N(0, scale^2) clipped to |x| <= LOGIT_MAX; `key`: a tuple of ints naming the case"""
    rng = np.random.default_rng([int(k) for k in key])
    return np.clip(rng.normal(0.0, scale, size=shape), -LOGIT_MAX, LOGIT_MAX).astype(np.float32)


def sample_case(n, scale):
    """sn_policy_sample on the 260 decisions at SAMPLE_STEPS decision counters: logits [steps, D, n], u [steps, D]"""
    gid, seat = deciders(B, N, MASK)
    logits = normal_logits((1, n, int(scale * 10)), (SAMPLE_STEPS, gid.size, n), scale)
    u = np.stack([sample_uniforms(SEED, s, gid, seat) for s in range(SAMPLE_STEPS)])
    return logits, u


KEY_CASES = [  # (seed, step, game_offset): every value of each field, a handful of combinations
    (3, 0, 0),
    (2**32 + 3, 1, 1000),
    (2**64 - 1, 2**31, 2**32 - 3),  # the game id's low 32 bits wrap inside the 8-game handle
    (3, 2**32 - 1, 2**32 - 3),
    (2**32 + 3, 2**31, 0),
    (2**64 - 1, 2**32 - 1, 1000),
]
KEY_GAMES = 8


def key_case(i):
    """the 8-game handle of KEY_CASES[i]: (gid, seat, logits [D, 10], u [D])"""
    seed, step, offset = KEY_CASES[i]
    gid, seat = deciders(KEY_GAMES, N, MASK, offset)
    return gid, seat, normal_logits((2, i), (gid.size, 10), 1.5), sample_uniforms(seed, step, gid, seat)


def offset_case():
    """16 games at game_offset 0, whose games 8..15 a handle of 8 games at game_offset 8 repeats"""
    gid, seat = deciders(16, N, MASK)
    return gid, seat, normal_logits((3,), (gid.size, 10), 1.5), sample_uniforms(SEED, 7, gid, seat)


LIST_SLOTS, LIST_STEP = 256, 5


def list_case():
    """the decision-list form: logits [256 * 4, 10] and u by flat g * N + p; the test uses the rows of the seats
    the tournament's seat draw gave its agent, a subset of these"""
    gid, seat = deciders(LIST_SLOTS, N, (1 << N) - 1)
    return gid, seat, normal_logits((4,), (gid.size, 10), 1.5), sample_uniforms(SEED, LIST_STEP, gid, seat)


ENGINE_SEED, ENGINE_STEP0, ENGINE_CALLS = 2**32 + 3, 2**32 - 2, 3  # the 32-bit counter wraps at the third call


def engine_case():
    """three consecutive BatchedReinforce.decide calls: logits [3, D, 10] handed in for the net's, u [3, D]"""
    gid, seat = deciders(B, N, MASK)
    logits = normal_logits((5,), (ENGINE_CALLS, gid.size, 10), 1.5)
    u = np.stack([sample_uniforms(ENGINE_SEED, (ENGINE_STEP0 + i) & 0xFFFFFFFF, gid, seat)
                  for i in range(ENGINE_CALLS)])
    return logits, u


STEP_ROLLOUT, STEP_SEED, STEP_STEP = 2, SEED, 3
STEP_SHAPES = {4: (130, 0b0101), 10: (130, 0b1000000001)}  # seats 0 and N - 1 decide


def step_case(num_seats):
    """sn_puct_step at t = 0 (n_cur = 10, N(0, 1.5^2)) and t = 1 (n_cur = 9, N(0, 4^2)) of rollout 2:
    [(logits [D, num_seats, n_cur], u [D, num_seats])] per step"""
    games, mask = STEP_SHAPES[num_seats]
    gid, seat = deciders(games, num_seats, mask)
    return [(normal_logits((6, num_seats, t), (gid.size, num_seats, 10 - t), SCALES[t]),
             step_uniforms(STEP_SEED, STEP_STEP, gid, seat, STEP_ROLLOUT, t, num_seats)) for t in (0, 1)]


def sampling_inputs():
    """(name, logits, u) of every set of sampling decisions a GPU test compares: the share of ambiguous ones is
    asserted on the CPU for each"""
    for n in (10, 7, 2, 1):
        for scale in SCALES:
            yield (f"sample n={n} scale={scale}",) + sample_case(n, scale)
    for i in range(len(KEY_CASES)):
        yield (f"key fields {i}",) + key_case(i)[2:]
    yield ("game offset",) + offset_case()[2:]
    yield ("decision list",) + list_case()[2:]
    yield ("engine",) + engine_case()
    for num_seats in STEP_SHAPES:
        for t, (logits, u) in enumerate(step_case(num_seats)):
            yield (f"step N={num_seats} t={t}", logits, u)
