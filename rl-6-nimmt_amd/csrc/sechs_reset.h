// sechs_reset.h -- seeding and the batched resets: k_seed, k_reset (numpy or Philox deal, league seats),
// k_reset_to (a given board and hands).  Part of sechs_env.hip's one translation unit: needs sechs_state.h and
// `using namespace sechs` first.
#pragma once

__global__ void k_seed(DevState s) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= s.B) return;
    if (s.rng_mode == RNG_NUMPY_MT) {
        // np.random.seed(seed + gid): init_genrand; numpy pos 624 == lazy code 0
        uint32_t* st = s.mt + g * kMtN;
        uint32_t v = (uint32_t)(s.seed + s.game_offset + (uint64_t)g);
        st[0] = v;
        for (int i = 1; i < kMtN; i++) {
            v = 1812433253u * (v ^ (v >> 30)) + (uint32_t)i;
            st[i] = v;
        }
        s.mt_pos[g] = 0u;
    } else {
        s.ctr[g] = 0u;
    }
    for (int p = 0; p < s.N; p++) s.sum_res[(int64_t)p * s.B + g] = 0;
    s.episodes[g] = 0;
}

template <int N, int MODE, bool LG = false>
__global__ __launch_bounds__(kBlock) void k_reset(DevState s, const uint8_t* decks) {
    __shared__ uint8_t lds_deck[kBlock * kDealStride];
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= s.B) return;
    Game<N> G;
    if (decks) {
        const uint8_t* d = decks + g * s.C;
        deal_from<N>([&](int i) -> uint32_t { return d[i]; }, s.C, G);
    } else {
        typename RngOf<MODE>::T rng;
        ByteBuf buf;
        RngOf<MODE>::load(s, g, rng, buf);
        uint32_t lg = 0u;
        if (LG) lg = league_draw(rng, buf, s.lg_K, s.lg_lo, s.lg_hi);  // Tournament.play_game: seats, then the deal
        uint8_t* slot = lds_deck + threadIdx.x * kDealStride;
        deck_shuffle2(rng, buf, slot, s.C);
        deal_from_deck<N>(slot, s.C, G);
        if (LG) {
#pragma unroll
            for (int p = 0; p < N; p++)
                if ((uint32_t)p >= (lg & 15u)) G.hand[p].lo = ~0ull, G.hand[p].hi = ~0u;
            s.lgs[g] = lg;
        }
        RngOf<MODE>::store(s, g, rng, buf);
    }
    store_game<N>(s, g, G);
}

template <int N>
__global__ __launch_bounds__(kBlock) void k_reset_to(DevState s, const int8_t* board, const int8_t* hands) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= s.B) return;
    Game<N> G;
#pragma unroll
    for (int p = 0; p < N; p++) {
        u32x4 set = {0u, 0u, 0u, 0u};
        for (int k = 0; k < kHand; k++) {
            const int c = hands[(g * N + p) * kHand + k];
            if (c >= 0) set = set_bit(set, (uint32_t)c);
        }
        G.hand[p] = hand_from_set(set);
        G.score[p] = 0;
    }
    uint32_t lo[4], hi[4];
#pragma unroll
    for (int r = 0; r < kRows; r++) {
        uint32_t l = 0, card4 = 0, len = 0, heads = 0, end = 0;
        for (int i = 0; i < kThreshold; i++) {
            const int c = board[(g * kRows + r) * kThreshold + i];
            if (c < 0) continue;
            if (len < 4) l |= (uint32_t)c << (8 * len);
            else card4 = (uint32_t)c;
            heads += heads_of((uint32_t)c);
            end = (uint32_t)c;
            len++;
        }
        lo[r] = l;
        hi[r] = (card4 & 0xFFu) | (len << 8) | (heads << 16) | (end << 24);
    }
    G.b.lo = u32x4{lo[0], lo[1], lo[2], lo[3]};
    G.b.hi = u32x4{hi[0], hi[1], hi[2], hi[3]};
    store_game<N>(s, g, G);
}
