// sechs_decode.h -- the decode-ahead records, reader and writer side by side: the record layout, dec_u16, DecSrc
// (k_play<RNG_NUMPY_DEC> plays from the records), DecArgs, dec_draws_slow, k_decode (writes them).  Part of
// sechs_env.hip's one translation unit: needs sechs_play.h (PhaseProf, PlayArgs) first.
#pragma once

// ---- decode-ahead records (SN_OPT_PIPE_DEC, the default for lockstep
// DrunkHamster rollouts of a numpy-compat handle, N <= 4) -----------------
// Every random decision of such a rollout depends on the word stream only
// (the draw maxima are n - 1 for the known hand size n, the deal's are
// 103..1), so k_decode, on the side stream beside the play launches, walks
// each game's pipelined ring a group of launches ahead and writes one record
// per game and episode; k_play<RNG_NUMPY_DEC> then plays from the records
// and issues no RNG work: no draws, no swap targets, no Fisher-Yates swaps,
// no hand sorting.  Record of an episode, 24 dwords as kDecQuads u32x4
// pieces at drec[(slot * kDecQuads + q) * B + g] (a wave's piece q of 64
// games is one 1-KB run):
//   w0       stream position where the record starts (the first decoded
//            step: step phi0 of the pipeline's first episode, else step 0)
//   w1..w5   off[t], t = 0..9 (u16 pairs): words consumed from w0 through
//            step t's draws (t = 9: through the deal that ends the episode)
//   w6..w10  step t's draws, t = 0..8 (u16 each: seat p's index at bits 4p;
//            step 9 holds one card, numpy draws nothing)
//   w11      the next deal's row cards r0..r3 (bytes, env.py:108-110)
//   w12..w23 the next deal's hands, seat p at w12 + 3p: the sorted legal list
//            as lo32, hi32, hi (bytes 8, 9 | 0xFFFF0000), env.py:104-107
constexpr int kDecWords = 4 * kDecQuads;

__device__ __forceinline__ uint32_t dec_u16(const uint32_t (&w)[kDecWords], int base, int t) {
    // u16 t of the u16 array at dword `base` (t wave-uniform, 0..9)
    uint32_t v = 0u;
#pragma unroll
    for (int k = 0; k < 5; k++) v = (t >> 1 == k) ? w[base + k] : v;
    return (t & 1) ? (v >> 16) : (v & 0xFFFFu);
}

template <int N>
struct DecSrc {
    uint32_t A[kDecWords];  // the current episode's record
    const u32x4* rec;       // drec + g: this game's piece 0 of record slot 0
    int64_t B;
    int slot;               // record slot of the current episode
    int base;               // the launch step that is the current episode's step 0 (at load: minus the launch's first step
                            // within its episode, -9 .. 0)
    int end;                // the launch's steps

    __device__ __forceinline__ void fetch() {
        const u32x4* ra = rec + (int64_t)slot * kDecQuads * B;
#pragma unroll
        for (int q = 0; q < kDecQuads; q++) {
            const u32x4 v = ra[(int64_t)q * B];
            A[4 * q] = v.x, A[4 * q + 1] = v.y, A[4 * q + 2] = v.z, A[4 * q + 3] = v.w;
        }
    }
    __device__ __forceinline__ void load(const DevState& s, const PlayArgs& a, int64_t g) {
        rec = s.drec + g, B = s.B;
        slot = a.drec0, base = -a.n0, end = a.steps;
        fetch();
    }
    __device__ __forceinline__ void draws(const Game<N>&, int t, uint32_t, bool, uint32_t (&idx)[N]) {
        const int tau = t - base;  // wave-uniform: the step within the episode
        SN_DASSERT(tau >= 0 && tau < kHand);
        const uint32_t v = (tau < kHand - 1) ? dec_u16(A, 6, tau) : 0u;
#pragma unroll
        for (int p = 0; p < N; p++) idx[p] = (v >> (4 * p)) & 15u;
    }
    __device__ __forceinline__ uint32_t league(const DevState&) { return 0u; }
    // The next episode's deal, then -- a launch that plays on (up to a whole twist group of
    // launches, K deals) -- the next episode's record: the one place where the step loop
    // loads, once per episode, waited for here behind this step's few small stores and not
    // at the first draw behind the next step's observation stores (vmcnt counts in order).
    __device__ __forceinline__ void deal(const DevState&, Game<N>& G, PhaseProf&) {
        install_deal<N>(A + 12, A[11], G);
        if (base + kHand < end) {  // wave-uniform (lockstep games)
            base += kHand;
            slot = (slot + 1 == kDecRecords) ? 0 : slot + 1;
            fetch();
#pragma unroll
            for (int k = 0; k < kDecWords; k++) asm volatile("" : "+v"(A[k]));
        }
    }
    // the stream position after the launch's last step (what sn_pipe_sync exports)
    __device__ __forceinline__ uint32_t position() const {
        const int last = end - 1 - base;  // 0 .. 9: a launch that ends on a deal keeps that episode's record
        SN_DASSERT(last >= 0 && last < kHand);
        return A[0] + dec_u16(A, 1, last);
    }
};

// k_decode: the decode-ahead producer.  One lane per game walks its
// pipelined ring from the decoder position (pabsc[kDecSlot]) and writes the
// records of episodes e0 .. e0 + ne - 1 (slots mod kDecRecords): per step
// the N DrunkHamster draws legal[random_interval(n - 1)] in seat order
// (agents/random.py:9, play.py:38-41; n = 10 - t), after step 9 the next
// deal -- np.random.shuffle(arange(C)) as Fisher-Yates from the end
// (env.py:99-112: j = random_interval(i), i = C-1 .. 1), the swaps in the
// lane's LDS deck, the hands sorted -- and the stream offsets after every
// step.  The same words in the same order as k_play's own draws and deals
// (StreamSrc), so the games are the same.  phi0: the first episode starts at
// that step (a pipeline started mid-episode).  The twist before it on the
// same stream (ptend[tpar]) leads the decoder position by the lead.
struct DecArgs {
    int e0, ne, phi0, tpar;
    int cin, cout;  // pabsc slots of the decoder position read / written
};

// One lane per game.  Per episode the lane copies a RingPipe window of its
// ring (kPipeWin bytes from the decoder position, all loads in flight at
// once) to LDS and reads the words from there -- the draws through the byte
// buffer, the shuffle targets straight from the window by position -- as
// the play kernel's own RingPipe path does.  (Reading the ring from HBM unit
// by unit was twice as slow: the loop's loads waited one by one.)  Per lane
// kPipeSlot bytes (an odd 8-B stride): the window; the swap targets overlay
// its first 104 bytes (target k lands on window byte k while the reads are
// past stream offset 36 + k: every earlier draw took >= 1 word), and the
// deck its bytes 112..219 once the targets are drawn.
constexpr int kDecBlock = 64;  // one wave per workgroup: packs beside the play blocks
constexpr int kDecLane = kPipeSlot;
static_assert(kDecLane % 8 == 0 && (kDecLane / 8) % 2 == 1 && kDecLane >= 112 + 108, "decoder LDS lane");

// A step of the WALK form whose window is too short (walk_draws returned false): rng_draws on an
// empty byte buffer from stream offset t, which reads on past the window byte by byte, stops at the
// twisted end and counts an overrun, as in the other form.  The buffer lives in this branch only, so
// it does not count in the decoder's allocation: 85 VGPRs and no scratch at N = 4, the other form
// 90 (out of line, as pipe_slow is, the call cost 103 VGPRs and a 16-byte frame).  Returns the
// offset after the step and the draws, a nibble each.
struct DecSlow {
    uint32_t t, idx;
};

template <int N>
static __device__ __forceinline__ DecSlow dec_draws_slow(RingPipe rng, uint32_t t, uint32_t max) {
    ByteBuf buf;
    buf.clear();
    rng.take = t;
    uint32_t idx[N];
    rng_draws<N>(rng, buf, max, idx);
    DecSlow r;
    r.t = rng.take - buf.cnt;  // buffered bytes are re-read from the window, as shuffle_targets does
    r.idx = 0u;
#pragma unroll
    for (int p = 0; p < N; p++) r.idx |= idx[p] << (4 * p);
    return r;
}

// WALK (SN_OPT_DEC_WALK, the default): the draws too are read by window position (walk_draws); a
// step the window is too short for goes through the byte buffer as in the other form.
//
// TOUCH (SN_OPT_DEC_EARLY, the default): the next episode's window is touched (RingPipe::touch_at, one dword of each
// of its ring chunks) as soon as its position is known, right behind the swap targets: a deck's work later the
// window's own loads find their lines in L2.  The touches' bytes are dropped behind the swaps; they feed nothing, count
// nothing, and the dispatch's last episode issues none.  The same records either way.
template <int N, bool WALK, bool TOUCH>
__global__ __launch_bounds__(kDecBlock) void k_decode(DevState s, DecArgs d) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kDecBlock * kDecLane];
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * kDecBlock + threadIdx.x;
    if (g >= s.B) return;
    const int64_t B = s.B;
    uint8_t* win = lds + threadIdx.x * kDecLane;  // the ring window
    uint8_t* jslot = win;                         // the swap targets, over the window's consumed head
    uint8_t* deck = win + 112;                    // the deck, once the window is dead
    uint32_t pos = s.pabsc[(int64_t)d.cin * B + g];
    const uint32_t tend = s.ptend[(int64_t)d.tpar * B + g];
    PhaseProf pq;
    pq.start();
    for (int i = 0; i < d.ne; i++) {
        const int phi = (i == 0) ? d.phi0 : 0;
        RingPipe rng;
        ByteBuf buf;
        rng.load_at(s, g, buf, win, pos, tend);  // an overrun (pos past tend) counts perr there
        const uint32_t start = pos;
        uint32_t off[5] = {0u, 0u, 0u, 0u, 0u}, dr[5] = {0u, 0u, 0u, 0u, 0u};
        bool big = false;
        uint32_t wt = 0u;  // WALK: the next unconsumed byte of the window (the buffer stays empty)
#pragma unroll
        for (int t = 0; t < kHand - 1; t++) {  // steps 0..8: hand size n = 10 - t, draws random_interval(n - 1)
            if (t >= phi) {
                uint32_t idx[N];
                if constexpr (WALK) {
                    if (!walk_draws<N>(rng, wt, (uint32_t)(kHand - 1 - t), idx)) {
                        // max as a run-time value here: with it constant, the nine copies' 64-bit masks are
                        // hoisted out of the episode loop and sit in VGPRs beside the window load
                        uint32_t mx = (uint32_t)(kHand - 1 - t);
                        asm volatile("" : "+v"(mx));
                        const DecSlow r = dec_draws_slow<N>(rng, wt, mx);
                        wt = r.t;
#pragma unroll
                        for (int p = 0; p < N; p++) idx[p] = (r.idx >> (4 * p)) & 15u;
                    }
                } else {
                    rng_draws<N>(rng, buf, (uint32_t)(kHand - 1 - t), idx);
                }
                uint32_t v = 0u;
#pragma unroll
                for (int p = 0; p < N; p++) v |= idx[p] << (4 * p);
                dr[t >> 1] |= v << (16 * (t & 1));
                const uint32_t o = WALK ? wt : rng.consumed(buf) - start;  // the window starts at `start`
                big = big || o > 0xFFFFu;
                off[t >> 1] |= (o & 0xFFFFu) << (16 * (t & 1));
            }
        }
        pq.mark(PR_DRAWS);
        // step 9 plays each seat's last card (no draw), then the auto-reset deal
        if constexpr (WALK) rng.take = wt;
        shuffle_targets(rng, buf, jslot, s.C, kDecLane - 1);  // the window's own form (by position), dummy past it
        pos = rng.consumed(buf);
        const bool more = i + 1 < d.ne;  // wave-uniform
        uint32_t tv[RingPipe::kPipeTouch] = {};
        if constexpr (TOUCH) {
            if (more) RingPipe::touch_at(s, g, pos, tv);
        }
        pq.mark(PR_TARGETS);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // the window reads before the deck's writes
        for (int k = 0; k < s.C; k += 4) *(uint32_t*)(deck + k) = (uint32_t)k * 0x01010101u + 0x03020100u;
        shuffle_apply(deck, jslot, s.C);
        if constexpr (TOUCH) {
            if (more) {  // the touches' bytes end here: long back by now (nothing else is in flight: load_at drained)
#pragma unroll
                for (int k = 0; k < RingPipe::kPipeTouch; k++) asm volatile("" ::"v"(tv[k]));
            }
        }
        pq.mark(PR_APPLY);
        Game<N> G;
        deal_from_deck<N>(deck, s.C, G);
        pq.mark(PR_HANDS);
        {
            const uint32_t o = pos - start;
            big = big || o > 0xFFFFu;
            off[4] |= (o & 0xFFFFu) << 16;
        }
        if (big) atomicAdd(s.perr, 1u);  // cannot happen (an episode draws ~200 words); fail loudly
        uint32_t hw[12] = {};  // seats past N: zeros
        const uint32_t rows = pack_deal<N>(G, hw);
        u32x4* rec = s.drec + (int64_t)((d.e0 + i) % kDecRecords) * kDecQuads * B + g;
        rec[0 * B] = u32x4{start, off[0], off[1], off[2]};
        rec[1 * B] = u32x4{off[3], off[4], dr[0], dr[1]};
        rec[2 * B] = u32x4{dr[2], dr[3], dr[4], rows};
        rec[3 * B] = u32x4{hw[0], hw[1], hw[2], hw[3]};
        rec[4 * B] = u32x4{hw[4], hw[5], hw[6], hw[7]};
        rec[5 * B] = u32x4{hw[8], hw[9], hw[10], hw[11]};
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // the deck reads before the next window's writes
        pq.mark(PR_STORE);
    }
    pq.flush(lane, 1);
    s.pabsc[(int64_t)d.cout * B + g] = pos;
}
