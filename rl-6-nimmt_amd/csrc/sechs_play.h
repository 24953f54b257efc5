// sechs_play.h -- the env-step loop: PhaseProf (and g_phase), PlayArgs, StreamSrc, obs_stage_pieces, play_steps,
// load_results / store_results, play_body, k_play.  Part of sechs_env.hip's one translation unit: needs
// sechs_state.h, `using namespace sechs` and sechs_mt_ahead.h (st_nt, SECHS_NT_*) first; sechs_decode.h, included
// after it, completes DecSrc.
#pragma once

// ---- k_play phase profiler (diagnostics; built only with -DSECHS_PHASE_PROF,
// the libsechs_prof.so variant).  Each wave accumulates shader-clock cycles
// per phase of its step loop and adds them to g_phase at exit; the clock
// reads add lgkmcnt waits at the phase marks, so the split is indicative.
// PH_B1 / PH_B2: a k_play_split play wave waiting at its barriers; PR_*: the
// producer waves' phases.  g_phase[PH_N] counts play waves, [PH_N + 1] producers.
enum {
    PH_PROLOGUE = 0, PH_OBS, PH_DRAW, PH_RESOLVE, PH_STORE, PH_DEAL, PH_EPILOGUE, PH_HANDS, PH_APPLY, PH_B1, PH_B2,
    PR_DRAWS, PR_B1, PR_TARGETS, PR_APPLY, PR_HANDS, PR_DRAWS2, PR_B2, PR_STORE, PR_SPARE, PH_N
};
#ifdef SECHS_PHASE_PROF
__device__ unsigned long long g_phase[PH_N + 2];
struct PhaseProf {
    uint64_t t, acc[PH_N];
    __device__ __forceinline__ void start() {
        t = __builtin_readcyclecounter();
#pragma unroll
        for (int k = 0; k < PH_N; k++) acc[k] = 0ull;
    }
    __device__ __forceinline__ void mark(int k) {
        const uint64_t n = __builtin_readcyclecounter();
        acc[k] += n - t;
        t = n;
    }
    __device__ __forceinline__ void flush(int lane, int role = 0) {
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < PH_N; k++)
                if (acc[k]) atomicAdd(&g_phase[k], (unsigned long long)acc[k]);
            atomicAdd(&g_phase[PH_N + role], 1ull);
        }
    }
};
#else
struct PhaseProf {
    __device__ __forceinline__ void start() {}
    __device__ __forceinline__ void mark(int) {}
    __device__ __forceinline__ void flush(int, int = 0) {}
};
#endif

// MT19937 chunks (8 words) twisted per refill in k_play: 2 doubles the
// lookahead of the refill's loads (one wave per SIMD: nothing else hides them)
constexpr int kPlayPrefetch = 2;

struct PlayArgs {
    int steps, flags, obs_stride, wave_lds;  // wave_lds: bytes of LDS per wave (dynamic)
    int ring_lds;            // bytes of that per lane for the LDS ring copy (RNG_NUMPY_RING/PIPE), at the region's end
    int pipe_cin, pipe_cout, pipe_t;  // RNG_NUMPY_PIPE: pabsc parity read / written, ptend parity read
    int vec_out;             // rewards 16-B and actions 4-B aligned: one store per lane each (N == 4)
    const int32_t* actions;  // [B][N] (steps == 1) or NULL = DrunkHamster
    int32_t* rewards;        // [steps][B][N]
    uint8_t* done;           // [steps][B]
    uint8_t* actions_out;    // [steps][B][N]
    int8_t* obs;             // [steps][B][N][obs_stride]
    int32_t* invalid;        // [B]
    int32_t* league_rec;     // league: [episodes][B][1 + N] per finished game: seats word, results
    int step0;               // league: env-steps of this rollout before this launch (episode index of a record)
    int n0;                  // k_play_split: every game's hand size at the launch's start (aligned handle);
                             // RNG_NUMPY_DEC: the launch's first step within its episode (0..9)
    int drec0;               // RNG_NUMPY_DEC: record slot of the launch's first episode (the next ones follow, mod kDecRecords)
};

// The env-step loop of one lane (game g).  R supplies the random words
// (topup/force, sechs_device.h).  Each wave
// owns a private LDS region: the lanes' deal decks, and -- when the
// observation rows are 48 bytes -- a staging area where the wave's 64 rows
// are assembled so that they leave as 1-KB contiguous stores instead of 64
// scattered 16-B pieces per instruction.  (Both uses never overlap in time
// within a step: observations first, the deal at the very end.)
// Where a step's random decisions come from.  StreamSrc: the game's own
// word stream, in the play loop (DrunkHamster draws, tournament seat draws,
// the deal).  SplitSrc: decisions a producer wave decoded into LDS
// (k_play_split): the indices of every step, the next deal's hands/rows.
template <int N, class R>
struct StreamSrc {
    R& rng;
    ByteBuf& buf;
    uint8_t* deck;  // kDealStride bytes of LDS: deck + swap targets
    __device__ __forceinline__ void draws(const Game<N>& G, int, uint32_t kp, bool lg, uint32_t (&idx)[N]) {
        // DrunkHamster for every seat in seat order (play.py:38-41):
        // legal[random_interval(n-1)], agents/random.py:9
        if (lg && !__all(kp == (uint32_t)N)) {  // a tournament game with fewer players
#pragma unroll
            for (int p = 0; p < N; p++) idx[p] = ((uint32_t)p < kp) ? rng_interval(rng, buf, G.n - 1u) : 0u;
        } else {
            rng_draws<N>(rng, buf, G.n - 1u, idx);
        }
    }
    __device__ __forceinline__ uint32_t league(const DevState& s) { return league_draw(rng, buf, s.lg_K, s.lg_lo, s.lg_hi); }
    __device__ __forceinline__ void deal(const DevState& s, Game<N>& G, PhaseProf& pp) {
        // deck_shuffle2 in its two phases (marked apart for the profiler)
        shuffle_targets(rng, buf, deck + kDeckStride, s.C);
        pp.mark(PH_DEAL);
        for (int i = 0; i < s.C; i += 4) *(uint32_t*)(deck + i) = (uint32_t)i * 0x01010101u + 0x03020100u;
        shuffle_apply(deck, deck + kDeckStride, s.C);
        pp.mark(PH_APPLY);
        deal_from_deck<N>(deck, s.C, G);
#pragma unroll
        for (int p = 0; p < N; p++) SN_DASSERT(hand_strict(G.hand[p]) && hand_len(G.hand[p]) == (uint32_t)kHand);
    }
};

// 16-B pieces per lane in the obs staging rows: 3N padded to an odd count, so
// the 64 lanes' ds_write_b128 at a common piece index spread over all banks
// (an even stride -- 12 pieces = 192 B at N = 4 -- serialised them)
__host__ __device__ constexpr int obs_stage_pieces(int N) { return 3 * N + ((N & 1) ? 0 : 1); }

// Observation rows of 48 bytes are staged: play_steps assembles a wave's rows
// in LDS and stores them as 16-byte pieces.  The one predicate for the kernel
// (whether it stages) and the host (whether the launch holds a staging area,
// lds_plan's callers, and needs the rows 16-byte aligned, check_obs_align).
__host__ __device__ __forceinline__ constexpr bool obs_staged(const void* obs, int stride) { return obs && stride == 48; }

template <int N, class Src, int GPW = 64, bool LG = false>
__device__ __forceinline__ void play_steps(const DevState& s, const PlayArgs& a, int64_t g, int lane, uint8_t* wave_lds,
                                           Game<N>& G, Src& src, int32_t (&sum_res)[N], int32_t& episodes,
                                           PhaseProf& pp, uint32_t& lg, int t_begin, int t_end) {
    const int64_t B = s.B;
    const bool staged = obs_staged(a.obs, a.obs_stride);
    const int64_t g0 = g - lane;                           // first game of this wave
    const int wave_games = (int)min((int64_t)GPW, B - g0);  // = active lanes (lanes past B left)
    const bool auto_reset = (a.flags & SN_AUTO_RESET) != 0;
    const bool summ = !(a.flags & SN_NO_SUMMARIES);
    int32_t* rew = a.rewards ? a.rewards + ((int64_t)t_begin * B + g) * N : nullptr;
    uint8_t* act = a.actions_out ? a.actions_out + ((int64_t)t_begin * B + g) * N : nullptr;
    uint8_t* dn = a.done ? a.done + (int64_t)t_begin * B + g : nullptr;
    int8_t* ob = a.obs ? a.obs + ((int64_t)t_begin * B + g) * N * a.obs_stride : nullptr;
    for (int t = t_begin; t < t_end; t++) {
        const uint32_t kp = LG ? (lg & 15u) : (uint32_t)N;  // players of this game
        if (ob) {
            uint32_t w2hi;
            const int nobs = LG ? (int)kp : N;
            const GameWords gw = summ ? game_words<true>(nobs, G.b, w2hi) : game_words<false>(nobs, G.b, w2hi);
            if (staged) {
                constexpr int P = obs_stage_pieces(N);  // odd: lanes' rows land on distinct bank groups
                u32x4* row = (u32x4*)wave_lds + lane * P;
#pragma unroll
                for (int p = 0; p < N; p++) {
                    const Hand& h = G.hand[p];
                    row[3 * p + 0] = u32x4{(uint32_t)h.lo, (uint32_t)(h.lo >> 32), (h.hi & 0xFFFFu) | w2hi, gw.w0};
                    row[3 * p + 1] = gw.a;
                    row[3 * p + 2] = gw.b;
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                const u32x4* src = (const u32x4*)wave_lds;
                u32x4* dst = (u32x4*)(a.obs + ((int64_t)t * B + g0) * N * 48);
                if (wave_games == GPW) {  // all reads, one wait, all stores
                    u32x4 pc[3 * N];
#pragma unroll
                    for (int j = 0; j < 3 * N; j++) {
                        const int c = lane + GPW * j;  // piece c of the wave's contiguous obs block
                        pc[j] = src[(c / (3 * N)) * P + c % (3 * N)];
                    }
#pragma unroll
                    for (int j = 0; j < 3 * N; j++) {
                        if (SECHS_NT_OBS) __builtin_nontemporal_store(pc[j], &dst[lane + GPW * j]);
                        else dst[lane + GPW * j] = pc[j];
                    }
                } else {
                    const int pieces = wave_games * N * 3;
                    for (int i = lane; i < pieces; i += wave_games) dst[i] = src[(i / (3 * N)) * P + i % (3 * N)];
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            } else {
#pragma unroll
                for (int p = 0; p < N; p++) store_obs_row(ob + p * a.obs_stride, G.hand[p], w2hi, gw, a.obs_stride);
            }
            ob += B * N * a.obs_stride;
        }
        pp.mark(PH_OBS);
        uint32_t card[N], pen[N], idx[N];
        int bad = -1;
        if (G.n == 0u) {
            bad = 0;  // finished game stepped without auto-reset: nothing to play
        } else if (a.actions) {
#pragma unroll
            for (int p = N - 1; p >= 0; p--) {
                const int32_t c = a.actions[g * N + p];
                const int k = (c >= 0 && c < s.C) ? hand_find(G.hand[p], (uint32_t)c) : -1;
                card[p] = (uint32_t)c;
                idx[p] = (uint32_t)k;
                bad = (k >= 0) ? bad : p;
            }
        } else {
            src.draws(G, t, kp, LG, idx);
#pragma unroll
            for (int p = 0; p < N; p++) {
                card[p] = hand_get(G.hand[p], idx[p]);
                SN_DASSERT((LG && (uint32_t)p >= kp) || (idx[p] < G.n && card[p] < (uint32_t)s.C));  // the hand holds it
            }
        }
        pp.mark(PH_DRAW);
        if (a.invalid) a.invalid[g] = bad;
        if (bad >= 0) {
            if (rew) {
#pragma unroll
                for (int p = 0; p < N; p++) rew[p] = 0;
                rew += B * N;
            }
            if (act) act += B * N;
            if (dn) {
                *dn = (G.n == 0u) ? 1 : 0;
                dn += B;
            }
            continue;
        }
#pragma unroll
        for (int p = 0; p < N; p++) hand_del(G.hand[p], idx[p]);
        resolve<N, LG>(G.b, card, pen);  // absent seats' cards are 0xFF (empty hands)
#pragma unroll
        for (int p = 0; p < N; p++) G.score[p] += (int32_t)pen[p];
        G.n -= 1u;
        const bool done = (G.n == 0u);  // env.py:246-249
        pp.mark(PH_RESOLVE);
        if (rew) {
            if (N == 4 && a.vec_out) {  // one 16-B store per lane: 1 KB contiguous per wave
                st_nt((u32x4*)rew, u32x4{-pen[0], -pen[1 % N], -pen[2 % N], -pen[3 % N]}, SECHS_NT_MORE);
            } else {
#pragma unroll
                for (int p = 0; p < N; p++) rew[p] = -(int32_t)pen[p];
            }
            rew += B * N;
        }
        if (act) {
            if (N == 4 && a.vec_out) {
                st_nt((uint32_t*)act, (uint32_t)(card[0] | (card[1 % N] << 8) | (card[2 % N] << 16) | (card[3 % N] << 24)),
                      SECHS_NT_MORE);
            } else {
#pragma unroll
                for (int p = 0; p < N; p++) act[p] = (uint8_t)card[p];
            }
            act += B * N;
        }
        if (dn) {
            st_nt(dn, (uint8_t)(done ? 1 : 0), SECHS_NT_MORE);
            dn += B;
        }
        pp.mark(PH_STORE);
        if (LG && done && a.league_rec) {  // the finished game's record: seats word, results (-penalty)
            int32_t* rec = a.league_rec + ((int64_t)((a.step0 + t) / kHand) * B + g) * (1 + N);
            rec[0] = (int32_t)lg;
#pragma unroll
            for (int p = 0; p < N; p++) rec[1 + p] = -G.score[p];
        }
        if (done && auto_reset) {
            // GameSession.results.append(scores) then the next play_game()
#pragma unroll
            for (int p = 0; p < N; p++) sum_res[p] -= G.score[p];
            episodes += 1;
            if (LG) lg = src.league(s);  // Tournament.play_game: seats first
            src.deal(s, G, pp);
            if (LG) {  // a k-player env deals k hands (env.py:108)
                const uint32_t k2 = lg & 15u;
#pragma unroll
                for (int p = 0; p < N; p++)
                    if ((uint32_t)p >= k2) G.hand[p].lo = ~0ull, G.hand[p].hi = ~0u;
            }
            pp.mark(PH_HANDS);
        }
    }
}

// episode results stay in registers for the launch (one load, one store)
template <int N>
__device__ __forceinline__ void load_results(const DevState& s, int64_t g, int flags, int32_t (&sum_res)[N], int32_t& episodes) {
#pragma unroll
    for (int p = 0; p < N; p++) sum_res[p] = 0;
    episodes = 0;
    if (flags & SN_AUTO_RESET) {
#pragma unroll
        for (int p = 0; p < N; p++) sum_res[p] = s.sum_res[(int64_t)p * s.B + g];
        episodes = s.episodes[g];
    }
}

template <int N>
__device__ __forceinline__ void store_results(const DevState& s, int64_t g, int flags, const int32_t (&sum_res)[N],
                                              int32_t episodes) {
    if (flags & SN_AUTO_RESET) {
#pragma unroll
        for (int p = 0; p < N; p++) s.sum_res[(int64_t)p * s.B + g] = sum_res[p];
        s.episodes[g] = episodes;
    }
}

template <int N>
struct DecSrc;  // play_body's source on the decode-ahead path: sechs_decode.h

// GPW = games per wave: 64 (one game per lane), or 32 for the pipelined
// path (lanes 32..63 idle) -- half the LDS per wave, so two blocks fit a CU
// and a SIMD holds two waves to hide each other's latency
template <int N, int MODE, int GPW, bool LG = false>
__device__ __forceinline__ void play_body(const DevState& s, const PlayArgs& a, uint8_t* lds_dyn, int tid) {
    const int lane = tid & 63;
    if (GPW < 64 && lane >= GPW) return;
    // issue priority over the co-resident k_mt_ahead waves: the game loop
    // is one latency-bound wave per SIMD (measured +1.7 %)
    __builtin_amdgcn_s_setprio(1);
    const int64_t g = ((int64_t)blockIdx.x * (kBlock / 64) + (tid >> 6)) * GPW + lane;
    if (g >= s.B) return;
    uint8_t* wave_lds = lds_dyn + (tid >> 6) * a.wave_lds;
    PhaseProf pp;
    pp.start();
    Game<N> G;
    load_game<N>(s, g, G);
    int32_t sum_res[N], episodes;
    load_results<N>(s, g, a.flags, sum_res, episodes);
    uint32_t lg = LG ? s.lgs[g] : 0u;
    ByteBuf buf;
    if constexpr (MODE == RNG_NUMPY_DEC) {
        DecSrc<N> src;
        src.load(s, a, g);
        pp.mark(PH_PROLOGUE);
        play_steps<N, DecSrc<N>, 64, false>(s, a, g, lane, wave_lds, G, src, sum_res, episodes, pp, lg, 0, a.steps);
        s.pabsc[(int64_t)a.pipe_cout * s.B + g] = src.position();  // the consumer position (sn_pipe_sync)
    } else if constexpr (MODE == RNG_NUMPY_PIPE) {
        RingPipe rng;
        rng.load(s, g, buf, wave_lds + a.wave_lds - GPW * a.ring_lds + lane * a.ring_lds, a.pipe_cin, a.pipe_t);
        pp.mark(PH_PROLOGUE);
        StreamSrc<N, RingPipe> src{rng, buf, wave_lds + lane * kDealStride};
        play_steps<N, StreamSrc<N, RingPipe>, GPW, LG>(s, a, g, lane, wave_lds, G, src, sum_res, episodes, pp, lg, 0,
                                                       a.steps);
        s.pabsc[(int64_t)a.pipe_cout * s.B + g] = rng.consumed(buf);  // read by k_mt_ahead on the other queue
    } else {
        typename RngOf<MODE, kPlayPrefetch>::T rng;
        if constexpr (MODE == RNG_NUMPY_RING || MODE == RNG_NUMPY_RING_HBM) {
            uint8_t* slot = wave_lds + a.wave_lds - 64 * a.ring_lds + lane * a.ring_lds;
            RngOf<MODE, kPlayPrefetch>::load(s, g, rng, buf, slot);
        } else {
            RngOf<MODE, kPlayPrefetch>::load(s, g, rng, buf);
        }
        pp.mark(PH_PROLOGUE);
        using Gen = typename RngOf<MODE, kPlayPrefetch>::T;
        StreamSrc<N, Gen> src{rng, buf, wave_lds + lane * kDealStride};
        play_steps<N, StreamSrc<N, Gen>, 64, LG>(s, a, g, lane, wave_lds, G, src, sum_res, episodes, pp, lg, 0, a.steps);
        RngOf<MODE, kPlayPrefetch>::store(s, g, rng, buf);
    }
    store_game<N>(s, g, G);
    store_results<N>(s, g, a.flags, sum_res, episodes);
    if (LG) s.lgs[g] = lg;
    pp.mark(PH_EPILOGUE);
    pp.flush(lane);
}

// Decode-ahead at N = 4 (251 VGPRs; 259 before the launch could span a twist group): at most
// one wave per SIMD as ever -- the allocation is padded past half the file -- so that no CU
// takes two of the launch's 53-KB blocks (one per CU at 65 536 games) while another holds none:
// without the bound the 10-step launch measured 12 % slower.
template <int N, int MODE, int GPW = 64, bool LG = false>
__global__ __launch_bounds__(kBlock)
__attribute__((amdgpu_waves_per_eu(1, (MODE == RNG_NUMPY_DEC && N == kSplitMaxPlayers) ? 1 : 8)))
void k_play(DevState s, PlayArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_dyn[];
    play_body<N, MODE, GPW, LG>(s, a, lds_dyn, (int)threadIdx.x);
}
