// sechs_env1.h -- the one-game fast path of the scalar drop-in env: the kH1* exchange layout, Acts1, out1_game,
// k_step1, k_reset1.  Part of sechs_env.hip's one translation unit: needs sechs_state.h, `using namespace sechs`
// and sechs_play.h (PhaseProf) first.
#pragma once

// ---- one-game fast path (the scalar drop-in SechsNimmtEnv, B == 1) -------
// One launch per env.step / env.reset: the actions arrive as kernel
// arguments, the results (invalid seat, done, rewards, scores, int8 obs rows)
// -- and for a reset the numpy MT19937 state in and out -- go through pinned,
// device-mapped host words, so a call is one launch + one stream sync
// instead of a chain of blocking copies.  Words of hbuf:
constexpr int kH1In = 0;      // [624] key, [624] numpy pos        (sn_reset1 in)
constexpr int kH1Out = 1024;  // [0] invalid, [1] done, [2, 2+N) rewards, [2+N, 2+2N) scores, obs bytes N x 48,
                              // [kH1Trace, +N) per seat: row | undercut << 2 | scored << 3 | penalty << 8 (sn_step1)
constexpr int kH1Trace = 160;  // words into the out block (past 2 + 14 N for N <= 10)
constexpr int kH1Mt = 2048;   // [624] key, [624] code, [625] mt0  (sn_reset1 out)
constexpr int kH1Words = 4096;

struct Acts1 {
    int32_t a[kMaxPlayers];
};

template <int N>
__device__ __forceinline__ void out1_game(const DevState& s, const Game<N>& G, uint32_t* out, int summ) {
#pragma unroll
    for (int p = 0; p < N; p++) out[2 + N + p] = (uint32_t)G.score[p];
    uint32_t w2hi;
    const GameWords gw = summ ? game_words<true>(N, G.b, w2hi) : game_words<false>(N, G.b, w2hi);
    uint32_t* ob = out + 2 + 2 * N;
#pragma unroll
    for (int p = 0; p < N; p++) {
        const Hand& h = G.hand[p];
        const uint32_t row[12] = {(uint32_t)h.lo, (uint32_t)(h.lo >> 32), (h.hi & 0xFFFFu) | w2hi, gw.w0, gw.a.x, gw.a.y,
                                  gw.a.z, gw.a.w, gw.b.x, gw.b.y, gw.b.z, gw.b.w};
#pragma unroll
        for (int i = 0; i < 12; i++) ob[12 * p + i] = row[i];
    }
}

template <int N>
__global__ void k_step1(DevState s, Acts1 acts, uint32_t* hb, int summ) {
    if (threadIdx.x != 0) return;
    uint32_t* out = hb + kH1Out;
    Game<N> G;
    load_game<N>(s, 0, G);
    uint32_t card[N], pen[N], idx[N];
    int bad = -1;
#pragma unroll
    for (int p = N - 1; p >= 0; p--) {  // env.py:114-118 in seat order: the first illegal seat
        const int32_t c = acts.a[p];
        const int k = (G.n > 0u && c >= 0 && c < s.C) ? hand_find(G.hand[p], (uint32_t)c) : -1;
        card[p] = (uint32_t)c;
        idx[p] = (uint32_t)k;
        bad = (k >= 0) ? bad : p;
    }
#pragma unroll
    for (int p = 0; p < N; p++) pen[p] = 0u;
    if (bad < 0) {
#pragma unroll
        for (int p = 0; p < N; p++) hand_del(G.hand[p], idx[p]);
        uint32_t trace[N];
        resolve<N>(G.b, card, pen, trace);
#pragma unroll
        for (int p = 0; p < N; p++) G.score[p] += (int32_t)pen[p];
        G.n -= 1u;
        store_game<N>(s, 0, G);
#pragma unroll
        for (int p = 0; p < N; p++) out[kH1Trace + p] = trace[p];
    } else {  // nothing played: the trace words are 0 (sechs.h), not the previous step's
#pragma unroll
        for (int p = 0; p < N; p++) out[kH1Trace + p] = 0u;
    }
    out[0] = (uint32_t)bad;
    out[1] = (G.n == 0u) ? 1u : 0u;
#pragma unroll
    for (int p = 0; p < N; p++) out[2 + p] = (uint32_t)(-(int32_t)pen[p]);
    out1_game<N>(s, G, out, summ);
}

// sn_reset1, one wave: numpy's (key, pos) arrives in pinned words and is
// imported by all 64 lanes at once into LDS; the 103 Fisher-Yates targets of
// env.py:99-112 (np.random.shuffle: j = random_interval(i), i = C-1 .. 1,
// masked rejection) are decoded 64 stream words per instruction -- a word's
// draw index is its prefix count of accepted words, iterated acceptance ->
// ballot -> v_mbcnt to the fixed point -- with whole 624-word blocks twisted
// in LDS when the stream crosses one (as numpy does); the swaps run on the
// deck held in the wave's registers, one lane deals.  The state goes back in
// numpy's own form (the block holding the consumer + pos): the host
// converts nothing.
template <int N>
__global__ __launch_bounds__(64) void k_reset1(DevState s, uint32_t* hb, int summ) {
    constexpr uint32_t D = kMtN - kMtM;  // 227
    __shared__ uint32_t blk[2 * kMtN];   // the consumer's block, then the next one
    __shared__ __attribute__((aligned(16))) uint8_t slot[kDealStride];
    const uint32_t lane = threadIdx.x;
    const uint32_t C = (uint32_t)s.C, C1 = C - 1u;
    PhaseProf prof;  // libsechs_prof.so only: import / twist / decode / shuffle / deal / out (tools/reset1_prof.py)
    prof.start();
    uint32_t kv[(kMtN + 63) / 64];
#pragma unroll
    for (int q = 0; q < (kMtN + 63) / 64; q++) {  // every lane's host loads in flight at once
        const uint32_t i = 64u * q + lane;
        kv[q] = (i < (uint32_t)kMtN) ? hb[kH1In + i] : 0u;
    }
    const uint32_t pos = __builtin_amdgcn_readfirstlane(hb[kH1In + kMtN]);
#pragma unroll
    for (int q = 0; q < (kMtN + 63) / 64; q++) {
        const uint32_t i = 64u * q + lane;
        if (i < (uint32_t)kMtN) blk[i] = kv[q];
    }
    __syncthreads();
    prof.mark(PR_DRAWS);
    // numpy's twist of blk[0, 624) into blk[624, 1248), in its own order:
    // word j reads old j, j + 1 and j + 397 (j < 227) or new j - 227
    auto twist_next = [&]() {
        for (uint32_t j = lane; j < D; j += 64u) blk[kMtN + j] = mt_mix(blk[j], blk[j + 1u], blk[j + kMtM]);
        __syncthreads();
        for (uint32_t j = D + lane; j < 2u * D; j += 64u) blk[kMtN + j] = mt_mix(blk[j], blk[j + 1u], blk[kMtN + j - D]);
        __syncthreads();
        for (uint32_t j = 2u * D + lane; j < (uint32_t)kMtN - 1u; j += 64u)
            blk[kMtN + j] = mt_mix(blk[j], blk[j + 1u], blk[kMtN + j - D]);
        __syncthreads();
        if (lane == 0u) blk[2 * kMtN - 1] = mt_mix(blk[kMtN - 1], blk[kMtN], blk[kMtN + kMtN - 1 - D]);
        __syncthreads();
    };
    uint32_t dw = pos, o0 = 0u, avail = (uint32_t)kMtN;  // word cursor (from blk[0]), draws done, words in blk
    uint8_t* jslot = slot + kDeckStride;
    while (o0 < C1) {
        while (dw + 64u > avail) {  // the next 64 words: twist (a third block: slide the window first)
            if (avail == 2u * kMtN) {
                uint32_t t[(kMtN + 63) / 64];
#pragma unroll
                for (int q = 0; q < (kMtN + 63) / 64; q++) {
                    const uint32_t i = 64u * q + lane;
                    t[q] = (i < (uint32_t)kMtN) ? blk[kMtN + i] : 0u;
                }
                __syncthreads();
#pragma unroll
                for (int q = 0; q < (kMtN + 63) / 64; q++) {
                    const uint32_t i = 64u * q + lane;
                    if (i < (uint32_t)kMtN) blk[i] = t[q];
                }
                __syncthreads();
                dw -= kMtN;
            }
            prof.mark(PR_TARGETS);
            twist_next();
            prof.mark(PR_SPARE);
            avail = 2u * kMtN;
        }
        const uint32_t x = mt_temper(blk[dw + lane]) & 0xFFu;
        auto eval = [&](uint32_t pre, uint32_t& m) -> bool {
            const uint32_t o = o0 + pre;
            m = (o < C1) ? C1 - o : 1u;  // step o shuffles position i = C-1-o: random_interval(i)
            return o < C1 && (x & (0xFFFFFFFFu >> __builtin_clz(m))) <= m;
        };
        uint32_t m;
        uint64_t Acc = __ballot(eval((lane * 3u) >> 2, m));
        while (true) {
            const uint32_t pre = __builtin_amdgcn_mbcnt_hi((uint32_t)(Acc >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)Acc, 0u));
            const uint64_t A2 = __ballot(eval(pre, m));
            if (A2 == Acc) break;
            Acc = A2;
        }
        const uint32_t pre = __builtin_amdgcn_mbcnt_hi((uint32_t)(Acc >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)Acc, 0u));
        if ((Acc >> lane) & 1ull) {
            (void)eval(pre, m);
            jslot[o0 + pre] = (uint8_t)(x & (0xFFFFFFFFu >> __builtin_clz(m)));
        }
        const uint32_t na = (uint32_t)__popcll(Acc);
        if (o0 + na >= C1) {  // the last draw is in this batch: the consumer stops past its word
            dw += 64u - (uint32_t)__builtin_clzll(Acc);
            break;
        }
        o0 += na;
        dw += 64u;
    }
    __syncthreads();
    prof.mark(PR_TARGETS);
    // the swaps, in numpy's order (step o swaps position i_o = C-1-o with
    // its target j_o), resolved in parallel: v(o), the card step o moves from
    // i_o to j_o, is what an earlier step last moved onto i_o (the latest
    // o' < o with j_o' = i_o), else the card i_o itself -- a chain over
    // earlier steps, resolved by pointer jumping; the final card at i_o is
    // what sat on j_o before step o (the same rule), at position 0 v of the
    // last step targeting 0.  Lane l holds steps l and 64 + l.
    {
        __shared__ int32_t val[128], ptr[128], tail[128];
        __shared__ unsigned long long msk[128];
        const uint32_t oa = lane, ob = 64u + lane;
        const bool va = oa < C1, vb = ob < C1;
        const int32_t ia = (int32_t)(C1 - oa), ib = (int32_t)C1 - (int32_t)ob;
        const int32_t ja = va ? jslot[oa] : -1, jb = vb ? jslot[ob] : -1;
        // the latest earlier step with a given target: per 64-step chunk a
        // mask of the lanes targeting each position (LDS atomic or), the
        // highest lane below mine, else the last one of the chunk before
        tail[lane] = -1, tail[64u + lane] = -1;
        msk[lane] = 0ull, msk[64u + lane] = 0ull;
        __syncthreads();
        const uint64_t below = (1ull << lane) - 1ull;
        if (va) atomicOr(&msk[ja], 1ull << lane);
        __syncthreads();
        uint64_t mj = va ? msk[ja] & below : 0ull, mi = va ? msk[ia] & below : 0ull;
        const int32_t pja = mj ? 63 - (int32_t)__builtin_clzll(mj) : -1;
        const int32_t pia = mi ? 63 - (int32_t)__builtin_clzll(mi) : -1;
        if (va && (msk[ja] >> lane) == 1ull) tail[ja] = (int32_t)lane;  // the chunk's last step onto ja
        __syncthreads();
        if (va) msk[ja] = 0ull;
        __syncthreads();
        if (vb) atomicOr(&msk[jb], 1ull << lane);
        __syncthreads();
        mj = vb ? msk[jb] & below : 0ull, mi = vb ? msk[ib] & below : 0ull;
        const int32_t pjb = mj ? 127 - (int32_t)__builtin_clzll(mj) : (vb ? tail[jb] : -1);
        const int32_t pib = mi ? 127 - (int32_t)__builtin_clzll(mi) : (vb ? tail[ib] : -1);
        const uint64_t z1 = __ballot(vb && jb == 0), z0 = __ballot(va && ja == 0);
        const int32_t last0 = z1 ? 127 - (int32_t)__builtin_clzll(z1) : (z0 ? 63 - (int32_t)__builtin_clzll(z0) : -1);
        // v: resolved values (>= 0) or pointers to earlier steps
        int32_t pa = pia, pb = pib;
        int32_t xa = (pa < 0) ? ia : -1, xb = (pb < 0) ? ib : -1;
        val[oa] = xa, ptr[oa] = pa, val[ob] = xb, ptr[ob] = pb;
        __syncthreads();
        while (__ballot((va && xa < 0) || (vb && xb < 0))) {
            int32_t na = xa, nb = xb, qa = pa, qb = pb;
            if (va && xa < 0) {
                const int32_t w = val[pa];
                if (w >= 0) na = w;
                else qa = ptr[pa];
            }
            if (vb && xb < 0) {
                const int32_t w = val[pb];
                if (w >= 0) nb = w;
                else qb = ptr[pb];
            }
            __syncthreads();
            xa = na, xb = nb, pa = qa, pb = qb;
            val[oa] = xa, ptr[oa] = pa, val[ob] = xb, ptr[ob] = pb;
            __syncthreads();
        }
        const int32_t fa = (pja < 0) ? ja : val[max(pja, 0)], fb = (pjb < 0) ? jb : val[max(pjb, 0)];
        const int32_t f0 = (last0 < 0) ? 0 : val[last0];
        __syncthreads();
        if (va) slot[ia] = (uint8_t)fa;
        if (vb) slot[ib] = (uint8_t)fb;
        if (lane == 0u) slot[0] = (uint8_t)f0;
    }
    __syncthreads();
    prof.mark(PR_APPLY);
    // numpy's state after the deal: the block holding the consumer, pos in 1..624
    const uint32_t b0 = (dw > (uint32_t)kMtN) ? (uint32_t)kMtN : 0u, npos = dw - b0;
    for (uint32_t i = lane; i < (uint32_t)kMtN; i += 64u) {
        const uint32_t v = blk[b0 + i];
        s.mt[i] = v;
        hb[kH1Mt + i] = v;
    }
    if (lane == 0u) {
        prof.mark(PR_STORE);
        Game<N> G;
        deal_from_deck<N>(slot, (int)C, G);
        prof.mark(PR_HANDS);
        store_game<N>(s, 0, G);
        const uint32_t code = mt_code_from_numpy((int)npos);
        s.mt_pos[0] = code;
        uint32_t* out = hb + kH1Out;
        out[0] = 0xFFFFFFFFu;
        out[1] = 0u;
#pragma unroll
        for (int p = 0; p < N; p++) out[2 + p] = 0u;
        out1_game<N>(s, G, out, summ);
        hb[kH1Mt + kMtN] = code;
        hb[kH1Mt + kMtN + 1] = 0u;
        prof.mark(PR_B2);
        prof.flush(0, 1);
    }
}
