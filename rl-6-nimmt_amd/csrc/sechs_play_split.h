// sechs_play_split.h -- the role-split k_play: SplitSrc, produce_draws, split_lds, k_play_split.  Part of
// sechs_env.hip's one translation unit: needs sechs_play.h (play_steps, load_results / store_results) first.
#pragma once

// ============================================================================
// Role-split k_play (SN_OPT_PLAY_SPLIT, the default for aligned rollouts).
// Every random decision of the DrunkHamster self-play depends on the word
// stream only, never on the cards: the hand size at each step is fixed (the
// games of a handle stay in lockstep after a reset: `phase`), so the
// policy draws' maxima are known, and the deal is a function of the words.
// A block is 4 PLAY waves + 4 PRODUCER waves on the same 256 games (two
// waves per SIMD, where one game per lane leaves one: a single wave issues
// a VALU instruction at most every 4 cycles, two every 2).  Producers decode
// the launch's policy indices into LDS (nibbles), barrier B1, then shuffle
// and deal the next episode and decode the steps after it while the play
// waves play up to the episode's end; barrier B2; play waves install the
// dealt hands and go on.  The play waves issue no RNG work at all.  Philox
// handles only (numpy-compat variants over the pipelined ring were measured
// slower than k_play + k_mt_ahead and removed).
// Same words, same order, same results: every parity test runs this path.
// ============================================================================
template <int N>
struct SplitSrc {
    const uint16_t* idx;  // this lane's column of the producer's [t][64] index words
    __device__ __forceinline__ void draws(const Game<N>&, int t, uint32_t, bool, uint32_t (&out)[N]) {
        const uint32_t v = idx[t * 64];
#pragma unroll
        for (int p = 0; p < N; p++) out[p] = (v >> (4 * p)) & 15u;
    }
    __device__ __forceinline__ uint32_t league(const DevState&) { return 0u; }
    __device__ __forceinline__ void deal(const DevState&, Game<N>&, PhaseProf&) {}  // installed after B2
};

// the policy indices of steps [t_from, t_to): hand size m_first at t_from,
// one less each step (the game's n), N seats in seat order (play.py:38-41)
template <int N, class R>
__device__ __forceinline__ void produce_draws(R& rng, ByteBuf& buf, uint16_t* idx, int t_from, int t_to, int m_first) {
    for (int t = t_from; t < t_to; t++) {
        const int m = m_first - (t - t_from);
        uint32_t v = 0u;
        if (m >= 2) {
            uint32_t d[N];
            rng_draws<N>(rng, buf, (uint32_t)(m - 1), d);
#pragma unroll
            for (int p = 0; p < N; p++) v |= d[p] << (4 * p);
        }
        idx[t * 64] = (uint16_t)v;
    }
}

// LDS of a k_play_split block: play staging | decks | index words | dealt games
__host__ __device__ __forceinline__ int split_deal_words(int N) { return 3 * N + 1; }
__host__ __device__ __forceinline__ size_t split_lds(int N, int steps) {
    return (size_t)4 * 64 * obs_stage_pieces(N) * 16 + (size_t)4 * 64 * kDealStride + (size_t)4 * steps * 64 * 2 +
           (size_t)4 * split_deal_words(N) * 64 * 4;
}

template <int N, int MODE>
__global__ __launch_bounds__(2 * kBlock) void k_play_split(DevState s, PlayArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_dyn[];
    // the role is wave-uniform: readfirstlane makes it a scalar branch, so each
    // wave runs only its role's code -- and exactly its role's two barriers
    const int tid = (int)threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, w = wave & 3;
    const int64_t g = ((int64_t)blockIdx.x * 4 + w) * 64 + lane;
    const bool live = g < s.B;
    uint8_t* staging = lds_dyn + (size_t)w * 64 * obs_stage_pieces(N) * 16;
    uint8_t* decks = lds_dyn + (size_t)4 * 64 * obs_stage_pieces(N) * 16;
    uint16_t* idx = (uint16_t*)(decks + (size_t)4 * 64 * kDealStride) + (size_t)w * a.steps * 64 + lane;
    uint32_t* dealt = (uint32_t*)((uint8_t*)((uint16_t*)(decks + (size_t)4 * 64 * kDealStride) + (size_t)4 * a.steps * 64)) +
                      (size_t)w * split_deal_words(N) * 64 + lane;
    const int n0 = a.n0;
    const bool deal_in = n0 >= 1 && n0 <= a.steps;  // the episode ends at step n0 - 1 of this launch
    const int tA = deal_in ? n0 : a.steps;
    // B0 hands the play waves the first kSplitEarly steps' indices at once, so
    // they start playing while the producers decode the rest (B1)
    const int tE = min(tA, kSplitEarly);
    if (wave >= 4) {  // ---------------- producer (the critical path: issue priority over the play waves)
        __builtin_amdgcn_s_setprio(1);
        static_assert(MODE == RNG_PHILOX, "k_play_split decodes Philox streams only");
        PhiloxGen rng;
        ByteBuf buf;
        PhaseProf pq;
        pq.start();
        if (live) {
            RngOf<MODE, 2>::load(s, g, rng, buf);
            produce_draws<N>(rng, buf, idx, 0, tE, n0);
        }
        __syncthreads();  // B0: the first steps' indices are in LDS
        if (live) produce_draws<N>(rng, buf, idx, tE, tA, n0 - tE);
        pq.mark(PR_DRAWS);
        __syncthreads();  // B1: every index before the deal is in LDS
        pq.mark(PR_B1);
        if (live && deal_in) {
            uint8_t* deck = decks + (size_t)(w * 64 + lane) * kDealStride;
            Game<N> D;
            shuffle_targets(rng, buf, deck + kDeckStride, s.C);
            pq.mark(PR_TARGETS);
            for (int i = 0; i < s.C; i += 4) *(uint32_t*)(deck + i) = (uint32_t)i * 0x01010101u + 0x03020100u;
            shuffle_apply(deck, deck + kDeckStride, s.C);
            pq.mark(PR_APPLY);
            deal_from_deck<N>(deck, s.C, D);
#pragma unroll
            for (int p = 0; p < N; p++) {
                dealt[(3 * p + 0) * 64] = (uint32_t)D.hand[p].lo;
                dealt[(3 * p + 1) * 64] = (uint32_t)(D.hand[p].lo >> 32);
                dealt[(3 * p + 2) * 64] = D.hand[p].hi;
            }
            dealt[3 * N * 64] = (D.b.lo.x & 0xFFu) | ((D.b.lo.y & 0xFFu) << 8) | ((D.b.lo.z & 0xFFu) << 16) | (D.b.lo.w << 24);
            pq.mark(PR_HANDS);
            produce_draws<N>(rng, buf, idx, tA, a.steps, kHand);
            pq.mark(PR_DRAWS2);
        }
        __syncthreads();  // B2: the deal and the later indices are in LDS
        pq.mark(PR_B2);
        if (live) RngOf<MODE, 2>::store(s, g, rng, buf);
        pq.mark(PR_STORE);
        pq.flush(lane, 1);
        return;
    }
    // -------------------------------------------------------- play
    PhaseProf pp;
    pp.start();
    Game<N> G;
    int32_t sum_res[N], episodes = 0;
    uint32_t lg = 0u;
    if (live) {
        load_game<N>(s, g, G);
        load_results<N>(s, g, a.flags, sum_res, episodes);
    }
    pp.mark(PH_PROLOGUE);
    SplitSrc<N> src{idx};
    __syncthreads();  // B0
    pp.mark(PH_B1);
    if (live) play_steps<N, SplitSrc<N>, 64, false>(s, a, g, lane, staging, G, src, sum_res, episodes, pp, lg, 0, tE);
    __syncthreads();  // B1
    pp.mark(PH_B1);
    if (live) play_steps<N, SplitSrc<N>, 64, false>(s, a, g, lane, staging, G, src, sum_res, episodes, pp, lg, tE, tA);
    pp.mark(PH_EPILOGUE);
    __syncthreads();  // B2
    pp.mark(PH_B2);
    if (live) {
        if (deal_in) {  // the next episode's deal (env.py:99-112), decoded by the producer
#pragma unroll
            for (int p = 0; p < N; p++) {
                G.hand[p].lo = (uint64_t)dealt[(3 * p + 0) * 64] | ((uint64_t)dealt[(3 * p + 1) * 64] << 32);
                G.hand[p].hi = dealt[(3 * p + 2) * 64];
                G.score[p] = 0;
            }
            const uint32_t rw = dealt[3 * N * 64];
            const uint32_t r0 = rw & 0xFFu, r1 = (rw >> 8) & 0xFFu, r2 = (rw >> 16) & 0xFFu, r3 = rw >> 24;
            G.b.lo = u32x4{r0, r1, r2, r3};
            G.b.hi = u32x4{meta_row(r0), meta_row(r1), meta_row(r2), meta_row(r3)};
            G.n = kHand;
        }
        pp.mark(PH_DEAL);
        play_steps<N, SplitSrc<N>, 64, false>(s, a, g, lane, staging, G, src, sum_res, episodes, pp, lg, tA, a.steps);
        store_game<N>(s, g, G);
        store_results<N>(s, g, a.flags, sum_res, episodes);
    }
    pp.mark(PH_EPILOGUE);
    pp.flush(lane);
}
