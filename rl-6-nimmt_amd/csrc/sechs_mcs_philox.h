// sechs_mcs_philox.h -- the MCSAgent search (agents/mcts.py:91-172) on Philox streams, one lane per
// playout: shared by the league's search kernel (k_league_mcs_philox, sechs_league.hip) and the test
// hook (sn_mcs_decide_philox, sechs_mcs.hip).
//
// The stream law (include/sechs.h at sn_league_step).  A decision is given a Philox key
// and a stream word whose 20-bit tag field (bits 8..27, dec_stream's layout) is zero.  Playout j draws
// from the stream  word | j << 8  of that key, from word 0 on, in the order of mcs_decide_exact's loop
// body (sechs_mcs.h): the numpy shuffle of the ascending card memory, then per step and seat
// random_interval(n - t - 1).  No playout shares a stream, so the lanes of a wave run 64 of them at a
// time with no order among them, and the per-move (sum, count) pairs -- integers -- are added across
// the wave.
#pragma once
#include "sechs_state.h"

namespace sechs {

constexpr uint32_t kMcsPhiloxKey = 0x4D435331u;  // "MCS1", xored into key word 1: never the slot's main key
constexpr int kMcsPhiloxMaxPlayouts = 1 << 20;   // the playout number is the stream word's 20-bit tag
constexpr uint32_t kMcsNoDeal = 0xFFFFFFFFu;     // the card memory cannot deal (K - 1) n cards

// the key of the decisions of a step that began with the slot's main counter at c0
__device__ __forceinline__ void mcs_philox_key(uint64_t seed, uint64_t c0, uint32_t& k0, uint32_t& k1) {
    k0 = (uint32_t)seed ^ (uint32_t)c0;
    k1 = (uint32_t)(seed >> 32) ^ (uint32_t)(c0 >> 32) ^ kMcsPhiloxKey;
}

// stream word (playout 0) of seat p of game `gid` deciding at a hand of n cards
__device__ __forceinline__ uint64_t mcs_philox_stream(uint64_t gid, uint32_t p, uint32_t n) {
    return ((uint64_t)(uint32_t)gid << 32) | ((uint64_t)p << 28) | (uint64_t)n;
}

// One wave's LDS: a deck scratch per lane (kDeckStride is the odd dword stride: lanes never meet on a
// bank) and the decision's card memory as the ascending list every playout shuffles.
struct __attribute__((aligned(16))) McsPhiloxLds {
    uint8_t deck[64 * kDeckStride];
    uint8_t cards[kDeckStride];
};

// board [4][6] int8 (-1 pad) in the device form (as k_reset_to reads it)
__device__ __forceinline__ Board board_from_i8(const int8_t* rows) {
    uint32_t lo[4], hi[4];
#pragma unroll
    for (int r = 0; r < kRows; r++) {
        uint32_t l = 0, card4 = 0, len = 0, heads = 0, end = 0;
        for (int i = 0; i < kThreshold; i++) {
            const int c = rows[r * kThreshold + i];
            if (c < 0) continue;
            if (len < 4) l |= (uint32_t)c << (8 * len);
            else card4 = (uint32_t)c;
            heads += heads_of((uint32_t)c);
            end = (uint32_t)c;
            len++;
        }
        lo[r] = l, hi[r] = (card4 & 0xFFu) | (len << 8) | (heads << 16) | (end << 24);
    }
    Board b;
    b.lo = u32x4{lo[0], lo[1], lo[2], lo[3]};
    b.hi = u32x4{hi[0], hi[1], hi[2], hi[3]};
    return b;
}

// MCSAgent._mcts for one decision of a K-player game, by the whole wave (a one-wave workgroup: every
// lane calls it with the same arguments but `lane`).  n >= 2 cards in `me`.  Returns the chosen card in
// every lane, sum / cnt = the wave's totals per first move, *q6 = a legal move got no playout (quirk
// Q6: the best sampled move is returned); kMcsNoDeal with zeroed totals where the memory holds fewer
// than (K - 1) n cards (or more than a deck).
template <int K>
__device__ uint32_t mcs_decide_philox(McsPhiloxLds& L, const Board& root, const Hand& me, uint32_t n, u32x4 avail,
                                      int mc_per_card, int mc_max, uint32_t key0, uint32_t key1, uint64_t stream0,
                                      uint32_t lane, int32_t (&sum)[kHand], int32_t (&cnt)[kHand], bool* q6) {
#pragma unroll
    for (int i = 0; i < kHand; i++) sum[i] = 0, cnt[i] = 0;
    *q6 = false;
    const uint32_t A = set_count(avail);
    if (A < (uint32_t)(K - 1) * n || A > (uint32_t)kMaxCards) return kMcsNoDeal;
    int64_t fact = 1;
    for (uint32_t i = 2; i <= n; i++) fact *= i;
    const uint32_t n_mc = (uint32_t)min((int64_t)min(mc_max, kMcsPhiloxMaxPlayouts), (int64_t)mc_per_card * fact);
    // _deal_hands: cards = available.copy(), ascending -- once for all playouts
    for (uint32_t i = lane; i < A; i += 64u) L.cards[i] = (uint8_t)set_select(avail, i);
    __syncthreads();
    uint8_t* deck = L.deck + lane * kDeckStride;
    for (uint32_t j = lane; j < n_mc; j += 64u) {
        PhiloxGen gen;
        ByteBuf buf;
        gen.load(key0, key1, stream0 | ((uint64_t)j << 8), 0ull, buf);
        // np.random.shuffle(cards): the permutation of the positions 0 .. A-1, then the cards through it
        deck_shuffle(gen, buf, deck, (int)A);
        Game<K> R;
        R.hand[0] = me;
        R.b = root;
#pragma unroll
        for (int q = 1; q < K; q++) {
            u32x4 set = {0u, 0u, 0u, 0u};
            for (uint32_t i = 0; i < n; i++) set = set_bit(set, L.cards[deck[(q - 1) * n + i]]);
            R.hand[q] = hand_from_set(set);
        }
        // _play_out with uniform moves for every seat (mcts.py:129-154, :187-188)
        uint32_t first = 0;
        int32_t outcome = 0;
        for (uint32_t t = 0; t < n; t++) {
            uint32_t idx[K], card[K], pen[K];
            rng_draws<K>(gen, buf, n - t - 1u, idx);  // K random_interval(n - t - 1) in seat order
            if (t == 0u) first = idx[0];
#pragma unroll
            for (int q = 0; q < K; q++) {
                card[q] = hand_get(R.hand[q], idx[q]);
                hand_del(R.hand[q], idx[q]);
            }
            resolve<K>(R.b, card, pen);
            outcome -= (int32_t)pen[0];
        }
#pragma unroll
        for (int i = 0; i < kHand; i++) {
            const bool hit = (uint32_t)i == first;
            sum[i] += hit ? outcome : 0;
            cnt[i] += hit ? 1 : 0;
        }
    }
    // the wave's totals in every lane: integer adds, so no order among the playouts shows
#pragma unroll
    for (int i = 0; i < kHand; i++) {
        if ((uint32_t)i >= n) continue;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            sum[i] += __shfl_xor(sum[i], off);
            cnt[i] += __shfl_xor(cnt[i], off);
        }
    }
    // _choose_action_from_outcomes: best mean in legal order, strict '>' (means compared as fractions)
    uint32_t best = 0;
    int64_t bs = 0, bc = 0;  // bc == 0: no move sampled yet
    bool missing = false;
#pragma unroll
    for (int i = 0; i < kHand; i++) {
        if ((uint32_t)i >= n) continue;
        if (cnt[i] == 0) {
            missing = true;  // np.mean([]) is NaN: never '>'
            continue;
        }
        if (bc == 0 || (int64_t)sum[i] * bc > bs * (int64_t)cnt[i]) best = (uint32_t)i, bs = sum[i], bc = cnt[i];
    }
    *q6 = missing;
    return hand_get(me, best);
}

}  // namespace sechs
