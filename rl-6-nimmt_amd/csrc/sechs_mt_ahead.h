// sechs_mt_ahead.h -- the numpy-MT twist-ahead: k_mt_prep (the per-launch ring), the streaming-store helper
// st_nt, AheadArgs, the whole-round twist pieces, k_mt_ahead (the pipelined ring) and k_pipe_code (back to the
// MtGen state code).  Part of sechs_env.hip's one translation unit: needs sechs_state.h and `using namespace
// sechs` first.
#pragma once

// numpy-MT twist-ahead for a k_play launch: one wave per game twists, in
// place and 64 consecutive words per instruction (every load and store one
// contiguous run), the game's stream far enough that ring_w words lie
// twisted and unconsumed, and writes their tempered low bytes to the ring
// (RingGen).  numpy's in-place twist order makes any 227 consecutive words
// independent: word i reads mt[i], mt[i+1] (both still the previous round's)
// and mt[i+397] (previous round, i < 227) or mt[i-227] (this round, twisted
// 227 words earlier).  So the words this launch twists first (j < 227) have
// every input in memory already: all their loads are issued before any
// store (the wave keeps 3 * (NB + 1) loads in flight), and only words j >=
// 227 (a nearly empty ring, or 512-word rings) wait for those stores.  The
// twist pointer stays a multiple of 8 (MtGen's chunking).  Twisting word 0
// of a new round while old words are unconsumed makes the code straddle;
// the overwritten old mt[0] goes to mt0[g] so sn_mt_get can still export
// numpy's key.
constexpr int kPrepGamesPerWave = 4;

template <int NB, int GPW>  // ring_w / 64, games per wave
__global__ __launch_bounds__(kBlock) void k_mt_prep(DevState s) {
    constexpr uint32_t W = 64u * NB;
    constexpr uint32_t D = kMtN - kMtM;  // 227
    const int64_t g0 = ((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * GPW;
    if (g0 >= s.B) return;  // whole waves
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t rem[GPW], KT[GPW], T0[GPW], base[GPW];
    uint32_t A[GPW][NB + 1], C[GPW][NB + 1];
    // Word k of game q (k = 0 .. KT) sits at twist index base + k (mod 624):
    // the first rem are twisted and unconsumed (re-tempered into the ring),
    // the rest are twisted now.  All loads of all GPW games go out first.
    // one load for the GPW state codes (lane q holds game g0 + q's): a
    // per-game load here would make each game's wait drain the previous
    // game's loads (vmcnt counts in order)
    const uint32_t codes = (lane < (uint32_t)GPW) ? s.mt_pos[min(g0 + (int64_t)lane, s.B - 1)] : 0u;
#pragma unroll
    for (int q = 0; q < GPW; q++) {
        const int64_t g = min(g0 + q, s.B - 1);  // a short last wave repeats its last game (loads only)
        const uint32_t code = __builtin_amdgcn_readlane(codes, q);
        const uint32_t T = code & 0x7FFu;
        rem[q] = (code >> 16) & kMtCntMask;
        const uint32_t add = (rem[q] >= W) ? 0u : ((W - rem[q] + 7u) & ~7u);
        KT[q] = rem[q] + add;
        T0[q] = (T == (uint32_t)kMtN) ? 0u : T;
        base[q] = T0[q] + kMtN - rem[q];  // + k, mod 624
        const uint32_t* st = s.mt + g * kMtN;
#pragma unroll
        for (int b = 0; b <= NB; b++) {
            const uint32_t k = 64u * b + lane;
            uint32_t idx = base[q] + k;
            idx = (idx >= (uint32_t)kMtN) ? idx - kMtN : idx;
            idx = (idx >= (uint32_t)kMtN) ? idx - kMtN : idx;
            if (k <= KT[q]) A[q][b] = st[idx];
            if (k >= rem[q] && k < KT[q] && k - rem[q] < D) C[q][b] = st[(idx < D) ? idx + kMtM : idx - D];
        }
    }
    uint32_t* ring = (uint32_t*)s.ring;
#pragma unroll
    for (int q = 0; q < GPW; q++) {
        const int64_t g = g0 + q;
        if (g >= s.B) break;
        uint32_t* st = s.mt + g * kMtN;
        const uint32_t r = rem[q], kt = KT[q];
#pragma unroll
        for (int b = 0; b <= NB; b++) {
            if (b == NB && kt <= W) break;
            const uint32_t k = 64u * b + lane;
            uint32_t idx = base[q] + k;
            idx = (idx >= (uint32_t)kMtN) ? idx - kMtN : idx;
            idx = (idx >= (uint32_t)kMtN) ? idx - kMtN : idx;
            // mt[idx + 1] = word k + 1 = the next lane's A (lane 63: lane 0 of the next batch)
            const uint32_t nxt = (b < NB) ? __shfl(A[q][b < NB ? b + 1 : b], 0) : 0u;
            uint32_t bb = __shfl_down(A[q][b], 1);
            bb = (lane == 63u) ? nxt : bb;
            uint32_t v = A[q][b];
            if (k >= r && k < kt && k - r < D) {
                v = mt_mix(A[q][b], bb, C[q][b]);
                st[idx] = v;
                if (idx == 0u) s.mt0[g * kMt0Levels] = A[q][b];
            }
            if (b < NB) {  // ring bytes: 4 words per dword (lanes 4m..4m+3)
                const uint32_t y = mt_temper(v) & 0xFFu;
                const uint32_t d = y | (__shfl_down(y, 1) << 8) | (__shfl_down(y, 2) << 16) | (__shfl_down(y, 3) << 24);
                if ((lane & 3u) == 0u) ring[(((int64_t)(k >> 4)) * s.B + g) * 4 + ((k >> 2) & 3u)] = d;
            }
        }
        // words j >= 227 read words twisted just above: in order, after those stores
        if (kt > r + D) {
            for (uint32_t k0 = ((r + D) & ~63u); k0 < kt; k0 += 64u) {
                const uint32_t k = k0 + lane;
                uint32_t v = 0u;
                if (k >= r + D && k < kt) {
                    uint32_t idx = base[q] + k;
                    idx = (idx >= (uint32_t)kMtN) ? idx - kMtN : idx;
                    idx = (idx >= (uint32_t)kMtN) ? idx - kMtN : idx;
                    const uint32_t a = st[idx];
                    v = mt_mix(a, st[(idx + 1u == (uint32_t)kMtN) ? 0u : idx + 1u], st[(idx < D) ? idx + kMtM : idx - D]);
                    st[idx] = v;
                    if (idx == 0u) s.mt0[g * kMt0Levels] = a;
                }
                const uint32_t y = mt_temper(v) & 0xFFu;
                const uint32_t d = y | (__shfl_down(y, 1) << 8) | (__shfl_down(y, 2) << 16) | (__shfl_down(y, 3) << 24);
                if ((lane & 3u) == 0u && k < W && k + 3u >= r + D) {
                    uint32_t* dst = ring + (((int64_t)(k >> 4)) * s.B + g) * 4 + ((k >> 2) & 3u);
                    if (k >= r + D) {
                        *dst = d;
                    } else {  // dword shared with words stored above: merge the new bytes
                        const uint32_t keep = (1u << (8u * (r + D - k))) - 1u;
                        *dst = (*dst & keep) | (d & ~keep);
                    }
                }
            }
        }
        if (lane == 0u && kt > r) {
            const uint32_t Tn = T0[q] + (kt - r);
            s.mt_pos[g] = ((Tn > (uint32_t)kMtN) ? Tn - kMtN : Tn) | (kt << 16);
        }
    }
}

// ============================================================================
// Pipelined numpy-MT twist-ahead (SN_OPT_PIPELINE, the default for numpy-mode
// DrunkHamster rollouts).  k_mt_ahead keeps each game's stream twisted
// kPipeLead words past the consumer position of the play launch before last,
// writing the tempered low bytes into a per-game circular ring indexed by
// absolute stream position (pring).  It reads only state no running kernel
// writes (pabsc of the launch before last, its own ptend / ptp), and the
// ring slots it fills are never the ones the running k_play reads (lead +
// one launch < kPipeRing), so it runs on a side stream CONCURRENTLY with
// k_play (launch i+1's twist beside launch i's game loop: memory-bound work
// beside latency-bound work, on the same CUs).  One wave per game; 64
// consecutive words per instruction; the first 224 words have all inputs in
// memory (loads first), later ones follow in order (word j reads j - 227).
// INIT: start from the MtGen state code (re-temper its twisted-unconsumed
// words into the ring first).
// ============================================================================
#ifndef SECHS_NT_OBS
#define SECHS_NT_OBS 1
#endif
#ifndef SECHS_NT_MORE
#define SECHS_NT_MORE 1
#endif
// streaming (non-temporal) stores for what no later kernel finds in L2
// anyway (the 155 MB of trajectory outputs and the MT words / ring bytes a
// launch writes): measured 5.77 -> 6.4 G env-steps/s.  Non-temporal LOADS
// of the MT state were measured slower (5.5 G/s: consecutive lanes share
// lines through L2), so loads stay normal.
template <class T>
__device__ __forceinline__ void st_nt(T* p, T v, bool nt) {
    if (nt) __builtin_nontemporal_store(v, p);
    else *p = v;
}

struct AheadArgs {
    int cin;   // pabsc parity holding the consumer position to lead (INIT: written)
    int tin;   // ptend parity of the previous prep (steady)
    int tout;  // ptend parity written
    int lead;  // words to keep twisted past the consumer (kPipeLead; smaller only to test the overrun path)
    uint32_t* perr_mirror;  // host-mapped copy of *perr, refreshed at launch start (off the play stream)
    int cin_copy;  // INIT: also write the start position to this pabsc slot (-1: none; decode-ahead: the play slot)
    int depth;     // ROUND: whole rounds a refilling game twists past `lead` (SN_OPT_TWIST_DEPTH, 0 .. kTwistDepthMax)
};

// One whole MT19937 round of game G, twisted by the whole wave in LDS (w:
// 624 words; k_mt_ahead's whole-round twists), in three pieces: the state is
// loaded once (mt_round_load, mt_round_to_lds), then every round of a refill
// is twisted in place in LDS (mt_twist_lds) and its tempered low bytes go to
// the ring at stream positions te .. te + 623 (mt_round_emit; te is
// 8-aligned: rounds are 624 = 78 x 8 words), and the state goes back to HBM
// once, after the refill's last round (mt_round_store) -- one HBM read and
// one write of the state per REFILL, however many rounds it chains, plus one
// ring byte per word.  numpy's in-place order in three dependency-free
// phases: words 0..226 read old words only (mt[i+1], mt[i+397]); 227..453
// read old mt[i+1] and the new mt[i-227] of phase 1; 454..623 the new
// mt[i-227] of phase 2 (and mt[623] the new mt[0]).  (k_mt_ahead's partial
// twists read the i+397 input a second time.)  mt_twist_lds returns the old
// mt[0] (the one word the sync-time untwist cannot recover, mt0).
// v: the state's words (word 64k + lane in v[k])
__device__ __forceinline__ void mt_round_load(const DevState& s, int64_t G, uint32_t lane, uint32_t (&v)[10]) {
    const uint32_t* st = s.mt + G * kMtN;
#pragma unroll
    for (int k = 0; k < 10; k++) {
        const uint32_t i = 64u * k + lane;
        v[k] = (i < (uint32_t)kMtN) ? st[i] : 0u;
    }
}

__device__ __forceinline__ void mt_round_to_lds(uint32_t lane, uint32_t* w, const uint32_t (&v)[10]) {
#pragma unroll
    for (int k = 0; k < 10; k++) {
        const uint32_t i = 64u * k + lane;
        if (i < (uint32_t)kMtN) w[i] = v[k];
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

// w holds the round's old words (mt_round_to_lds)
__device__ __forceinline__ uint32_t mt_twist_lds(uint32_t lane, uint32_t* w) {
    constexpr uint32_t D = kMtN - kMtM;  // 227
    const uint32_t old0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)w[0]);
    uint32_t nv[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {  // phase 1: i < 227
        const uint32_t i = 64u * k + lane;
        nv[k] = (i < D) ? mt_mix(w[i], w[i + 1u], w[i + kMtM]) : 0u;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t i = 64u * k + lane;
        if (i < D) w[i] = nv[k];
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
    for (int k = 0; k < 4; k++) {  // phase 2: 227 <= i < 454
        const uint32_t i = D + 64u * k + lane;
        nv[k] = (i < 2u * D) ? mt_mix(w[i], w[i + 1u], w[i - D]) : 0u;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t i = D + 64u * k + lane;
        if (i < 2u * D) w[i] = nv[k];
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
    for (int k = 0; k < 3; k++) {  // phase 3: 454 <= i < 624
        const uint32_t i = 2u * D + 64u * k + lane;
        nv[k] = (i < (uint32_t)kMtN) ? mt_mix(w[i], w[(i + 1u == (uint32_t)kMtN) ? 0u : i + 1u], w[i - D]) : 0u;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint32_t i = 2u * D + 64u * k + lane;
        if (i < (uint32_t)kMtN) w[i] = nv[k];
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    return old0;
}

// the tempered low bytes of the round in w to the ring (4 per dword: dword d
// holds stream positions te + 4d .. te + 4d + 3)
__device__ __forceinline__ void mt_round_emit(const DevState& s, int64_t G, uint32_t lane, const uint32_t* w,
                                              uint32_t te) {
    uint8_t* ring = (uint8_t*)s.pring;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint32_t d = 64u * k + lane;
        if (d < (uint32_t)kMtN / 4u) {
            const u32x4 x = *(const u32x4*)(w + 4u * d);
            const uint32_t y = (mt_temper(x.x) & 0xFFu) | ((mt_temper(x.y) & 0xFFu) << 8) |
                               ((mt_temper(x.z) & 0xFFu) << 16) | ((mt_temper(x.w) & 0xFFu) << 24);
            const uint32_t ri = (te + 4u * d) & (uint32_t)(kPipeRing - 1);
            st_nt((uint32_t*)(ring + ring_byte(ri, G, s.B)), y, SECHS_NT_MORE);  // ri is 4-aligned
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // the LDS reads before the next round's writes
}

// the state in w back to HBM (after the last round of a refill)
__device__ __forceinline__ void mt_round_store(const DevState& s, int64_t G, uint32_t lane, const uint32_t* w) {
    uint32_t* st = s.mt + G * kMtN;
#pragma unroll
    for (int k = 0; k < 10; k++) {
        const uint32_t i = 64u * k + lane;
        if (i < (uint32_t)kMtN) st_nt(&st[i], w[i], SECHS_NT_MORE);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // the LDS reads before the area's next use
}

// ROUND (SN_OPT_TWIST_ROUND): twist whole MT rounds instead of exactly the
// words the lead needs.  A twist that is due first completes the current
// round (the per-64-word form below, at start-up only: afterwards the twist
// pointer rests on a round boundary), then -- if the lead is still short --
// twists whole rounds of 624 words in LDS: the state is read once, every
// input of numpy's in-place order (mt[i+1], mt[i+397] / the new mt[i-227])
// comes from LDS, and the state is written once after the last round.
// Refill with hysteresis (SN_OPT_TWIST_DEPTH = a.depth): a game whose lead
// is at least a.lead twists nothing in this dispatch; one below it twists
// until the lead reaches a.lead + 624 depth, so the 2 x 2 496 B of state
// traffic are shared by depth + 1 rounds and most games skip most
// dispatches.  INIT staggers the games (lead a.lead + 624 (g mod (depth +
// 1))) so that they do not all refill in the same dispatch.  The lead ranges
// up to kPipeSpanMax words (sechs_state.h), which the ring of kPipeRing =
// 8192 bytes per game holds; a handle synchronised while the array is rounds
// ahead of its consumer is untwisted (k_pipe_code, up to kMt0Levels rounds).
template <bool INIT, bool ROUND = false>
__global__ __launch_bounds__(kBlock) void k_mt_ahead(DevState s, AheadArgs a) {
    constexpr uint32_t D = kMtN - kMtM;  // 227
    constexpr uint32_t P1 = 224;          // words twisted before any store (all inputs already in memory)
    const int64_t g = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (g >= s.B) return;  // whole waves
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t B = s.B;
    // publish the overrun count so far (every k_play before the running one)
    // to the host without a sync; sn_rollout reads it at entry
    if (g == 0 && lane == 0u && a.perr_mirror)
        __hip_atomic_store(a.perr_mirror, __hip_atomic_load(s.perr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    uint32_t* st = s.mt + g * kMtN;
    uint8_t* ring = (uint8_t*)s.pring;
    uint32_t Tp, t0, c;
    if (INIT) {
        const uint32_t code = s.mt_pos[g];
        Tp = code & 0x7FFu;
        const uint32_t rem = (code >> 16) & kMtCntMask;
        t0 = 0u;
        c = 0u - rem;
        for (uint32_t k0 = 0; k0 < rem; k0 += 64u) {  // twisted, unconsumed: stream index Tp - rem + k (mod 624)
            const uint32_t k = k0 + lane;
            if (k < rem) {
                const uint32_t v = st[(Tp + kMtN - rem + k) % (uint32_t)kMtN];
                const uint32_t ri = (c + k) & (uint32_t)(kPipeRing - 1);
                ring[ring_byte(ri, g, B)] = (uint8_t)(mt_temper(v) & 0xFFu);
            }
        }
        if (lane == 0u) {
            s.pabsc[(int64_t)a.cin * B + g] = c;
            if (a.cin_copy >= 0) s.pabsc[(int64_t)a.cin_copy * B + g] = c;
        }
    } else {
        Tp = s.ptp[g];
        t0 = s.ptend[(int64_t)a.tin * B + g];
        c = s.pabsc[(int64_t)a.cin * B + g];
    }
    // signed: a consumer past the twisted end means a play lane overran
    // (counted there too); twist nothing rather than underflow the lead
    const int32_t lead = (int32_t)(t0 - c);
    if (lead < 0 && lane == 0u) atomicAdd(s.perr, 1u);
    const uint32_t T0 = (Tp == (uint32_t)kMtN) ? 0u : Tp;
    // ROUND: a game refills when its lead is below lo, up to hi (the hysteresis; INIT: the staggered start-up lead)
    const int32_t lo = a.lead + ((ROUND && INIT) ? kMtN * (int32_t)(g % (int64_t)(a.depth + 1)) : 0);
    const int32_t hi = (ROUND && !INIT) ? a.lead + kMtN * a.depth : lo;
    const bool refill = lead >= 0 && lead < lo;
    // ROUND: the words completing the current round (none at a round boundary)
    const uint32_t n = ROUND ? ((refill && T0 != 0u) ? (uint32_t)kMtN - T0 : 0u)
                             : ((lead >= 0 && lead < a.lead) ? (((uint32_t)(a.lead - lead)) & ~7u) : 0u);
    auto ring_dword = [&](uint32_t j, uint32_t v) {  // t0 is 8-aligned: lanes 4m..4m+3 share one dword
        const uint32_t y = mt_temper(v) & 0xFFu;
        const uint32_t d = y | (__shfl_down(y, 1) << 8) | (__shfl_down(y, 2) << 16) | (__shfl_down(y, 3) << 24);
        const uint32_t ri = (t0 + j) & (uint32_t)(kPipeRing - 1);
        if ((lane & 3u) == 0u && j < n) st_nt((uint32_t*)(ring + ring_byte(ri, g, B)), d, SECHS_NT_MORE);  // ri 4-aligned
    };
    // Word-0 crossings of this launch (wave-uniform count): the overwritten
    // old mt[0] of each.  k_pipe_code's untwist needs one per round the array
    // runs ahead of the consumer -- up to three with SN_OPT_TWIST_EVERY = 3
    // (a lead of 1 800 words) -- so mt0[g][k] keeps the k-th newest; kept
    // in a register here (lane k: the k-th), so no load follows a store of this launch.
    uint32_t ncross = 0u, old0 = 0u;  // lane k: this launch's k-th newest crossing
    auto cross = [&](bool hit, uint32_t old) {
        const uint64_t m = __ballot(hit);
        if (m) {
            const uint32_t v = __shfl(old, (int)__builtin_ctzll(m));
            const uint32_t up = __shfl_up(old0, 1);  // newest first
            old0 = lane ? up : v;
            ncross++;
        }
    };
    // phase 1: words 0 .. min(n, 224)
    uint32_t A[4] = {0u, 0u, 0u, 0u}, Bv[4], Cv[4], IX[4];
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const uint32_t j = 64u * b + lane;
        IX[b] = 0xFFFFu;
        if (j < n && j < P1) {
            const uint32_t idx = (T0 + j) % (uint32_t)kMtN;
            IX[b] = idx;
            A[b] = st[idx];
            Bv[b] = st[(idx + 1u == (uint32_t)kMtN) ? 0u : idx + 1u];
            Cv[b] = st[(idx < D) ? idx + kMtM : idx - D];
        }
    }
#pragma unroll
    for (int b = 0; b < 4; b++) {
        if (64u * b >= min(n, P1)) break;
        const uint32_t j = 64u * b + lane;
        uint32_t v = 0u;
        if (IX[b] != 0xFFFFu) {
            v = mt_mix(A[b], Bv[b], Cv[b]);
            st_nt(&st[IX[b]], v, SECHS_NT_MORE);
        }
        cross(IX[b] == 0u, A[b]);
        ring_dword(j, v);
    }
    // phase 2: words 224 .. n, in order (their inputs include words just twisted)
    for (uint32_t j0 = P1; j0 < n; j0 += 64u) {
        const uint32_t j = j0 + lane;
        uint32_t v = 0u, aa = 0u;
        bool at0 = false;
        if (j < n) {
            const uint32_t idx = (T0 + j) % (uint32_t)kMtN;
            aa = st[idx];
            v = mt_mix(aa, st[(idx + 1u == (uint32_t)kMtN) ? 0u : idx + 1u], st[(idx < D) ? idx + kMtM : idx - D]);
            st[idx] = v;
            at0 = idx == 0u;
        }
        cross(at0, aa);
        ring_dword(j, v);
    }
    uint32_t Tn = Tp, te = t0 + n;
    if (n) {
        Tn = T0 + n;
        while (Tn > (uint32_t)kMtN) Tn -= kMtN;
    }
    if constexpr (ROUND) {
        // whole rounds, chained in the wave's LDS area, until the lead reaches hi (at most kMt0Levels - 1:
        // the start-up lead is fewer, sechs_state.h): one state load before, one state store after
        if (refill && lead + (int32_t)(te - t0) < hi) {
            __shared__ __attribute__((aligned(16))) uint32_t wround[kBlock / 64][kMtN];
            uint32_t* w = wround[threadIdx.x >> 6];
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // the words twisted before: stored first
            uint32_t v[10];
            mt_round_load(s, g, lane, v);  // all ten loads in flight at once
            mt_round_to_lds(lane, w, v);
            for (int rr = 0; rr < kMt0Levels - 1 && lead + (int32_t)(te - t0) < hi; rr++) {
                // three dependency-free phases; old mt[0]: the one word the untwist cannot recover
                cross(true, mt_twist_lds(lane, w));
                mt_round_emit(s, g, lane, w, te);
                te += kMtN;
            }
            mt_round_store(s, g, lane, w);
            Tn = kMtN;
        }
    }
    SN_DASSERT(ncross <= (uint32_t)kMt0Levels);
    // the span the ring holds: the twisted end leads the consumer followed by at most kPipeSpanMax words
    // (a lowered test lead included), and a game that did not refill had the low threshold already
    SN_DASSERT(lead < 0 || te - c <= (uint32_t)kPipeSpanMax);
    SN_DASSERT(!ROUND || lead < 0 || te == t0 || (int32_t)(te - c) >= hi);
    SN_DASSERT(!ROUND || te == t0 || Tn == (uint32_t)kMtN);
    if (lane == 0u) {
        s.ptp[g] = Tn;
        s.ptend[(int64_t)a.tout * B + g] = te;
    }
    if (ncross) {  // the stack of crossings, newest first: this launch's, then the older ones (one 64-B line)
        const uint32_t stk = (lane < (uint32_t)kMt0Levels) ? s.mt0[g * kMt0Levels + lane] : 0u;
        const uint32_t older = __shfl(stk, (int)((lane - ncross) & 63u));
        if (lane < (uint32_t)kMt0Levels) s.mt0[g * kMt0Levels + lane] = (lane < ncross) ? old0 : older;
    }
}

// state code of a pipelined handle (for MtGen users and sn_mt_get):
// twist pointer | (twisted end - consumer) << 16
__device__ __forceinline__ uint32_t mt_untwist_y_dev(uint32_t t) {
    const uint32_t lsb = t >> 31;  // the twist constant's top bit is set, y >> 1's is not
    return (((lsb ? (t ^ 0x9908b0dfu) : t)) << 1) | lsb;
}

__global__ __launch_bounds__(kBlock) void k_pipe_code(DevState s, int cin, int tin) {
    const int64_t g = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);  // one wave per game
    if (g >= s.B) return;  // whole waves
    const uint32_t lane = threadIdx.x & 63u;
    int32_t rem = (int32_t)(s.ptend[(int64_t)tin * s.B + g] - s.pabsc[(int64_t)cin * s.B + g]);
    if (rem < 0 && lane == 0u) atomicAdd(s.perr, 1u);  // an overrun (already counted): the stream is lost
    uint32_t tp = s.ptp[g];
    // The array ran ahead of the consumer's round (whole-round twists, or
    // the K-group lead of SN_OPT_TWIST_EVERY): undo its newest round's
    // twisted words [0, tp) in place (new -> old), the host mt_unstraddle,
    // until fewer than 624 words are unconsumed (below).  With y[j] the twist's
    // intermediate (top(old[j]) | low(old[j+1])): y[j] = U(new[j] ^ X[j]),
    // X[j] = new[j-227] for j >= 227 -- all from new words, in parallel --
    // and old[j+397] for j < 227, whose y[j+396], y[j+397] the first phase
    // gave (or the word was never twisted: j + 397 >= tp); then old[j] =
    // top(y[j]) | low(y[j-1]), old[0]'s low half from mt0 (newest crossing
    // first, then the ones before).  One wave per game, in LDS.
    __shared__ uint32_t sw[kBlock / 64][kMtN], sy[kBlock / 64][kMtN];
    uint32_t* w = sw[threadIdx.x >> 6];
    uint32_t* y = sy[threadIdx.x >> 6];
    uint32_t* a = s.mt + g * kMtN;
    constexpr uint32_t D = kMtN - kMtM;
    int lvl = 0;
    // Rounds are undone while a whole array or more is unconsumed (>=): a consumer exactly one array behind has
    // drawn its round's last word and is still in that round, numpy's pos 624 -- left alone, its code
    // 624 | 624 << 16 would read as an imported pos 0 of the round after.  The one state that IS that import
    // stays: mt_pos still holds the code the pipeline started from (nothing writes it in between), the
    // start-up put the consumer rem0 words before stream index 0 (k_mt_ahead INIT), so pabsc + rem0 words
    // were drawn since; a start from 624 | 624 << 16 with none drawn keeps its last round (no mt0 level
    // belongs to it: a load clears them, sn_mt_set leaves them stale).
    const uint32_t code0 = s.mt_pos[g];
    const bool at0 = code0 == ((uint32_t)kMtN | ((uint32_t)kMtN << 16)) &&
                     s.pabsc[(int64_t)cin * s.B + g] + (uint32_t)kMtN == 0u;
    const int32_t keep = at0 ? kMtN + 1 : kMtN;  // undo while rem >= keep
    if (rem >= keep) {
        for (uint32_t j = lane; j < (uint32_t)kMtN; j += 64u) w[j] = a[j];
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
    for (; rem >= keep && lvl < kMt0Levels; lvl++) {
        SN_DASSERT(tp >= 1u && tp <= (uint32_t)kMtN);
        if (tp < 1u || tp > (uint32_t)kMtN) break;
        for (uint32_t j = D + lane; j < tp; j += 64u) y[j] = mt_untwist_y_dev(w[j] ^ w[j - D]);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        for (uint32_t j = lane; j < min(D, tp); j += 64u) {
            const uint32_t k = j + kMtM;  // 397 .. 623
            const uint32_t old_k = (k < tp) ? ((y[k] & 0x80000000u) | (y[k - 1u] & 0x7fffffffu)) : w[k];
            y[j] = mt_untwist_y_dev(w[j] ^ old_k);
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        const uint32_t m0 = s.mt0[g * kMt0Levels + lvl];
        for (uint32_t j = lane; j < tp; j += 64u)
            w[j] = (y[j] & 0x80000000u) | ((j ? y[j - 1u] : m0) & 0x7fffffffu);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        rem -= (int32_t)tp;
        tp = kMtN;
    }
    if (lvl) {
        for (uint32_t j = lane; j < (uint32_t)kMtN; j += 64u) a[j] = w[j];
        if (lane < (uint32_t)kMt0Levels) {  // the crossings not undone are the newest now (lane k: level k)
            const uint32_t k = lane + (uint32_t)lvl;
            const uint32_t v = (k < (uint32_t)kMt0Levels) ? s.mt0[g * kMt0Levels + k] : 0u;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // every lane's load before any store
            s.mt0[g * kMt0Levels + lane] = v;
        }
    }
    SN_DASSERT(rem < keep);
    if (lane == 0u) s.mt_pos[g] = tp | ((uint32_t)max(rem, 0) << 16);
}
