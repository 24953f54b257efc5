// sechs_env.hip -- vectorised SechsNimmtEnv for gfx950 + the C ABI (include/sechs.h).
//
// Device state layout: sechs_state.h.
// A launch loads each game into VGPRs, plays `steps` env-steps and stores it
// back; per step the only HBM traffic is the caller's outputs and, in
// numpy-compat mode, the MT19937 words (8 per refill, 16-B accesses).
//
// This file is the host side and the small read-out kernels.  The other
// kernels are in headers that only this file includes (one translation unit:
// the dev, devprof, debug and prof variants recompile it alone):
//   sechs_reset.h       k_seed, k_reset, k_reset_to
//   sechs_mt_ahead.h    k_mt_prep, st_nt, AheadArgs, k_mt_ahead, k_pipe_code
//   sechs_play.h        PhaseProf / g_phase, PlayArgs, StreamSrc, play_steps, play_body, k_play
//   sechs_decode.h      the decode-ahead records: DecSrc (reader), DecArgs, k_decode (writer)
//   sechs_env1.h        the one-game fast path: the kH1* exchange layout, k_step1, k_reset1
//   sechs_play_split.h  SplitSrc, produce_draws, split_lds, k_play_split
// Host sections below, in order: errors and launch templates; handle
// lifecycle and options; the k_play launch plan; the pipeline schedule;
// rollout and step entry points; league entry points; state read-out; MT
// import and export; the one-game path; timing and debug.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>

#define SECHS_DEBUG_HERE  // SN_DASSERT is live in this file's kernels (libsechs_debug.so only)
#include "sechs_state.h"

using namespace sechs;

// The device half.  The order matters: each header names what it needs first.
#include "sechs_reset.h"
#include "sechs_mt_ahead.h"
#include "sechs_play.h"
#include "sechs_decode.h"
#include "sechs_env1.h"
#include "sechs_play_split.h"

// ============================================================================
// read-out kernels
// ============================================================================
// obs in any dtype, one thread per (game, seat)
template <typename T>
__global__ void k_obs(DevState s, T* out, int stride, int summ) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= s.B * s.N) return;
    const int64_t g = i / s.N;
    const int p = (int)(i - g * s.N);
    const Hand h = load_hand(s, p, g);
    const Board b = load_board(s, g);
    uint32_t w2hi;
    const GameWords gwv = summ ? game_words<true>(s.N, b, w2hi) : game_words<false>(s.N, b, w2hi);
    const uint32_t gw[9] = {gwv.w0, gwv.a.x, gwv.a.y, gwv.a.z, gwv.a.w, gwv.b.x, gwv.b.y, gwv.b.z, gwv.b.w};
    const uint32_t all[12] = {(uint32_t)h.lo, (uint32_t)(h.lo >> 32), (h.hi & 0xFFFFu) | w2hi,
                              gw[0], gw[1], gw[2], gw[3], gw[4], gw[5], gw[6], gw[7], gw[8]};
    T* dst = out + i * stride;
    const int L = summ ? 47 : 35;
#pragma unroll
    for (int wi = 0; wi < 12; wi++)
#pragma unroll
        for (int bi = 0; bi < 4; bi++) {
            const int k = 4 * wi + bi;
            if (k < stride) dst[k] = (k < L) ? (T)(int8_t)((all[wi] >> (8 * bi)) & 0xFFu) : (T)0;
        }
    for (int k = 48; k < stride; k++) dst[k] = (T)0;
}

__global__ void k_hands(DevState s, int8_t* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= s.B * s.N) return;
    const int64_t g = i / s.N;
    const int p = (int)(i - g * s.N);
    const Hand h = load_hand(s, p, g);
#pragma unroll
    for (int k = 0; k < kHand; k++) out[i * kHand + k] = (int8_t)hand_get(h, (uint32_t)k);
}

__global__ void k_board(DevState s, int8_t* out) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= s.B) return;
    const Board b = load_board(s, g);
    const uint32_t lo[4] = {b.lo.x, b.lo.y, b.lo.z, b.lo.w};
    const uint32_t hi[4] = {b.hi.x, b.hi.y, b.hi.z, b.hi.w};
#pragma unroll
    for (int r = 0; r < kRows; r++)
#pragma unroll
        for (int i = 0; i < kThreshold; i++)
            out[(g * kRows + r) * kThreshold + i] =
                (i < 5 && (uint32_t)i < len_of(hi[r])) ? (int8_t)card_at(lo[r], hi[r], i < 5 ? i : 0) : (int8_t)-1;
}

__global__ void k_scores(DevState s, int32_t* scores, int32_t* sum_res, int32_t* episodes) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= s.B) return;
    for (int p = 0; p < s.N; p++) {
        if (scores) scores[g * s.N + p] = s.score[(int64_t)p * s.B + g];
        if (sum_res) sum_res[g * s.N + p] = s.sum_res[(int64_t)p * s.B + g];
    }
    if (episodes) episodes[g] = s.episodes[g];
}

__global__ void k_clear_results(DevState s) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= s.B) return;
    for (int p = 0; p < s.N; p++) s.sum_res[(int64_t)p * s.B + g] = 0;
    s.episodes[g] = 0;
}

// ============================================================================
// host side / C ABI
// ============================================================================
static thread_local std::string g_err;

namespace sechs {
sn_status set_error(sn_status st, const std::string& msg) {
    g_err = msg;
    return st;
}
}  // namespace sechs

static sn_status fail(sn_status st, const std::string& msg) { return set_error(st, msg); }

// ---------------------------------------------------------------- errors and launch templates
// launch templates (C++ linkage: ahead of the C ABI block)
// One k_play launch.  The instantiations that exist: league seats for 2 .. 6 players, decode-ahead for N <= 4
// (no handle reaches the others: sn_league_config, dec_ok).
template <int NN, int MODE, int GPW = 64, bool LG = false>
static sn_status launch_k_play(const DevState& s, const PlayArgs& a, unsigned grid, size_t shmem, hipStream_t st) {
    if constexpr ((!LG || (NN >= 2 && NN <= kLeagueMaxPlayers)) && (MODE != RNG_NUMPY_DEC || NN <= kSplitMaxPlayers)) {
        HIP_TRY(hipFuncSetAttribute((const void*)k_play<NN, MODE, GPW, LG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
        hipLaunchKernelGGL((k_play<NN, MODE, GPW, LG>), dim3(grid), dim3(kBlock), shmem, st, s, a);
        HIP_TRY(hipGetLastError());
    }
    return SN_OK;
}

// k_mt_prep<ring_w / 64> for the ring sizes sn_set_option admits (64 .. 512 words)
template <int NB = 1>
static sn_status launch_mt_prep(const DevState& s, hipStream_t st) {
    if constexpr (NB <= 8) {
        if (s.ring_w / 64 != NB) return launch_mt_prep<NB + 1>(s, st);
        constexpr int GPW = kPrepGamesPerWave;
        const dim3 pg((unsigned)((s.B + GPW * (kBlock / 64) - 1) / (GPW * (kBlock / 64))));
        hipLaunchKernelGGL((k_mt_prep<NB, GPW>), pg, dim3(kBlock), 0, st, s);
        return SN_OK;
    } else {
        return fail(SN_EINVAL, "bad ring size");
    }
}

// ---------------------------------------------------------------- handle lifecycle, options, resets
// A default overridden from the environment (A/B runs of whole legs): taken when the whole value is one decimal
// integer in [lo, hi] (0 <= lo), ignored otherwise.
static void env_default(const char* name, int lo, int hi, int& field) {
    const char* v = getenv(name);
    if (!v || !*v) return;
    int x = 0;
    for (; *v >= '0' && *v <= '9' && x <= hi; v++) x = 10 * x + (*v - '0');
    if (!*v && x >= lo && x <= hi) field = x;
}

extern "C" {

const char* sn_last_error(void) { return g_err.c_str(); }
const char* sn_version(void) { return "sechs-mi355x 0.1 (gfx950)"; }

sn_status sn_create(sn_env** out, int device, int64_t num_games, int num_players, int num_cards, uint64_t seed,
                    uint64_t game_offset, int rng_mode) {
    if (!out) return fail(SN_EINVAL, "out is NULL");
    *out = nullptr;
    if (num_games <= 0) return fail(SN_EINVAL, "num_games must be > 0");
    if (num_players < 1 || num_players > kMaxPlayers) return fail(SN_EINVAL, "num_players must be in 1..10");
    if (num_cards < kHand * num_players + kRows) return fail(SN_EINVAL, "num_cards must be >= 10*num_players + 4");
    if (num_cards > kMaxCards) return fail(SN_EUNSUPPORTED, "num_cards > 104 (the reference's _card_value asserts card < 104)");
    if (rng_mode != SN_RNG_PHILOX && rng_mode != SN_RNG_NUMPY_MT) return fail(SN_EINVAL, "unknown rng_mode");
    HIP_TRY(hipSetDevice(device));
    sn_env* e = new (std::nothrow) sn_env();
    if (!e) return fail(SN_ENOMEM, "host allocation failed");
    e->device = device;
    if (hipDeviceGetAttribute(&e->cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || e->cus < 1) {
        delete e;
        return fail(SN_EHIP, "cannot query the device's CU count");
    }
    DevState& s = e->s;
    s.B = num_games, s.N = num_players, s.C = num_cards, s.rng_mode = rng_mode;
    s.seed = seed, s.game_offset = game_offset;
    const int64_t B = num_games, N = num_players;
    struct {
        void** p;
        size_t bytes;
    } allocs[] = {
        {(void**)&s.hand, sizeof(uint32_t) * N * 3 * B},   {(void**)&s.row_lo, sizeof(uint32_t) * kRows * B},
        {(void**)&s.row_hi, sizeof(uint32_t) * kRows * B}, {(void**)&s.score, sizeof(int32_t) * N * B},
        {(void**)&s.sum_res, sizeof(int32_t) * N * B},     {(void**)&s.episodes, sizeof(int32_t) * B},
        {(void**)&s.mt_pos, sizeof(uint32_t) * B},         {(void**)&s.ctr, sizeof(uint64_t) * B},
        {(void**)&s.mt, rng_mode == SN_RNG_NUMPY_MT ? sizeof(uint32_t) * kMtN * B : 4},
        {(void**)&s.mt0, sizeof(uint32_t) * kMt0Levels * B},  // per game: [0] newest crossing, then the ones before
    };
    for (auto& a : allocs) {
        if (hipMalloc(a.p, a.bytes) != hipSuccess) {
            sn_destroy(e);
            return fail(SN_ENOMEM, "hipMalloc of device state failed");
        }
        (void)hipMemset(*a.p, 0, a.bytes);
    }
    e->opt.chunk_steps = 10;
    e->opt.pipe = 1;
    e->opt.pipe_gpw = 64;
    e->opt.pipe_lead = kPipeLead;
    e->phase = -1;
    e->opt.play_split = 1;
    // measured: three-phase whole-round twists, the
    // ring in 64-B chunks and one twist per four play launches: 0.0861 ->
    // 0.0775 ms per step same box (K = 1 -> 4; K = 2: 0.0792, 3: 0.0783)
    e->opt.twist_round = 1;
    e->opt.twist_every = 4;
    env_default("SECHS_TWIST_EVERY", 1, kTwistEveryMax, e->opt.twist_every);
    e->opt.twist_depth = 3;  // measured: the fastest of 0 .. 3 on both bench commands
    env_default("SECHS_TWIST_DEPTH", 0, kTwistDepthMax, e->opt.twist_depth);
    e->opt.pipe_serial = 0;
    env_default("SECHS_PIPE_SERIAL", 0, 1, e->opt.pipe_serial);
    e->opt.play_group = 1;  // one k_play launch per twist group where a call spans it
    env_default("SECHS_PLAY_GROUP", 0, 1, e->opt.play_group);
    e->opt.dec_walk = 1;  // k_decode's draws by window position
    env_default("SECHS_DEC_WALK", 0, 1, e->opt.dec_walk);
    e->opt.dec_early = 1;  // k_decode touches the next window behind the swap targets
    env_default("SECHS_DEC_EARLY", 0, 1, e->opt.dec_early);
    e->opt.pipe_dec = 1;  // decode-ahead where it applies: 0.0776 -> 0.069 ms per step same box
    env_default("SECHS_PIPE_DEC", 0, 1, e->opt.pipe_dec);
    if (rng_mode == SN_RNG_NUMPY_MT) {
        struct {
            void** p;
            size_t bytes;
        } pal[] = {{(void**)&s.pring, (size_t)kPipeRing * B},
                   {(void**)&s.pabsc, sizeof(uint32_t) * (kPipeSlots + 2) * B},  // + the decoder's two slots
                   {(void**)&s.ptend, sizeof(uint32_t) * kPipeSlots * B}, {(void**)&s.ptp, sizeof(uint32_t) * B},
                   {(void**)&s.perr, sizeof(uint32_t)},
                   {(void**)&s.drec, N <= kSplitMaxPlayers ? sizeof(u32x4) * kDecRecords * kDecQuads * B : 16}};
        for (auto& a : pal) {
            if (hipMalloc(a.p, a.bytes) != hipSuccess) {
                sn_destroy(e);
                return fail(SN_ENOMEM, "hipMalloc of the MT pipeline failed");
            }
            (void)hipMemset(*a.p, 0, a.bytes);
        }
        // the pipeline's events order kernels on one device only: a device-scope
        // release is enough (the default system-scope one writes L2 back at
        // every record; SECHS_EV_SYSFENCE=1 restores it for A/B runs)
        int sysfence = 0;
        env_default("SECHS_EV_SYSFENCE", 0, 1, sysfence);
        const unsigned evf = hipEventDisableTiming | (sysfence ? 0u : (unsigned)hipEventDisableSystemFence);
        if (hipStreamCreateWithFlags(&e->pl.side, hipStreamNonBlocking) != hipSuccess ||
            hipStreamCreateWithFlags(&e->pl.side2, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&e->pl.ev_prep2, evf) != hipSuccess ||
            hipEventCreateWithFlags(&e->pl.ev_prep, evf) != hipSuccess ||
            hipEventCreateWithFlags(&e->pl.ev_main, evf) != hipSuccess ||
            hipEventCreateWithFlags(&e->pl.ev_play, evf) != hipSuccess) {
            sn_destroy(e);
            return fail(SN_EHIP, "stream/event creation failed");
        }
        for (int k = 0; k < 2; k++)
            if (hipEventCreateWithFlags(&e->pl.evt[k], evf) != hipSuccess ||
                hipEventCreateWithFlags(&e->pl.evd[k], evf) != hipSuccess) {
                sn_destroy(e);
                return fail(SN_EHIP, "stream/event creation failed");
            }
        if (hipHostMalloc((void**)&e->perr_host, sizeof(uint32_t), hipHostMallocMapped) != hipSuccess ||
            hipHostGetDevicePointer((void**)&e->perr_host_dev, e->perr_host, 0) != hipSuccess) {
            sn_destroy(e);
            return fail(SN_ENOMEM, "pinned overrun mirror allocation failed");
        }
        *e->perr_host = 0u;
    }
    if (rng_mode == SN_RNG_NUMPY_MT) {
        const sn_status r = sn_set_option(e, SN_OPT_RING_WORDS, N <= 4 ? 256 : 512);
        if (r != SN_OK) {
            sn_destroy(e);
            return r;
        }
    }
    hipLaunchKernelGGL(k_seed, dim3(grid_for(B)), dim3(kBlock), 0, 0, s);
    hipError_t err = hipDeviceSynchronize();
    if (err == hipSuccess) err = hipGetLastError();
    if (err != hipSuccess) {
        sn_destroy(e);
        return fail(SN_EHIP, std::string("seeding failed: ") + hipGetErrorString(err));
    }
    *out = e;
    return SN_OK;
}

static void free_timing(sn_env* e);

sn_status sn_destroy(sn_env* e) {
    if (!e) return SN_OK;
    (void)hipSetDevice(e->device);
    DevState& s = e->s;
    (void)hipDeviceSynchronize();  // no k_mt_ahead may still be in flight
    if (e->pl.ev_prep) (void)hipEventDestroy(e->pl.ev_prep);
    if (e->pl.ev_main) (void)hipEventDestroy(e->pl.ev_main);
    if (e->pl.ev_play) (void)hipEventDestroy(e->pl.ev_play);
    for (int k = 0; k < 2; k++) {
        if (e->pl.evt[k]) (void)hipEventDestroy(e->pl.evt[k]);
        if (e->pl.evd[k]) (void)hipEventDestroy(e->pl.evd[k]);
    }
    if (e->pl.ev_prep2) (void)hipEventDestroy(e->pl.ev_prep2);
    if (e->pl.side2) (void)hipStreamDestroy(e->pl.side2);
    if (e->perr_host) (void)hipHostFree(e->perr_host);
    if (e->hbuf) (void)hipHostFree(e->hbuf);
    if (e->pl.side) (void)hipStreamDestroy(e->pl.side);
    free_timing(e);
    void* ps[] = {s.hand, s.row_lo, s.row_hi, s.score, s.sum_res, s.episodes, s.mt_pos, s.ctr, s.mt, s.mt0, s.ring,
                  s.pring, s.pabsc, s.ptend, s.ptp, s.perr, s.lgs, s.lmem, s.drec};
    for (void* p : ps)
        if (p) (void)hipFree(p);
    delete e;
    return SN_OK;
}

static void free_timing(sn_env* e) {
    for (int i = 0; i < kTimingEvents * e->tcap; i++)
        if (e->tev[i]) (void)hipEventDestroy(e->tev[i]);
    delete[] e->tev;
    delete[] e->tev_tw;
    e->tev = nullptr;
    e->tev_tw = nullptr;
    e->tcap = e->tn = 0;
}

sn_status sn_set_option(sn_env* e, int option, int value) {
    if (!e) return fail(SN_EINVAL, "env is NULL");
    DevState& s = e->s;
    if (sn_pipe_sync(e, 0) != SN_OK) return SN_EHIP;
    switch (option) {
        case SN_OPT_RING_WORDS: {
            if (value < 0 || value > 512 || (value % 64)) return fail(SN_EINVAL, "ring words must be a multiple of 64 in 0..512");
            if (value && s.rng_mode != SN_RNG_NUMPY_MT) return fail(SN_EINVAL, "the ring feeds numpy-compat mode only");
            HIP_TRY(hipSetDevice(e->device));
            HIP_TRY(hipDeviceSynchronize());
            if (s.ring) (void)hipFree(s.ring);
            s.ring = nullptr;
            s.ring_w = 0;
            if (value) {
                if (hipMalloc((void**)&s.ring, (size_t)value * (size_t)s.B) != hipSuccess) return fail(SN_ENOMEM, "ring allocation failed");
                s.ring_w = value;
            }
            return SN_OK;
        }
        case SN_OPT_CHUNK_STEPS:
            if (value < 1) return fail(SN_EINVAL, "chunk steps must be >= 1");
            e->opt.chunk_steps = value;
            return SN_OK;
        case SN_OPT_PIPELINE:
            if (value != 0 && value != 1) return fail(SN_EINVAL, "pipeline must be 0 or 1");
            e->opt.pipe = value;
            return SN_OK;
        case SN_OPT_PIPE_GPW:
            if (value != 32 && value != 64) return fail(SN_EINVAL, "games per wave must be 32 or 64");
            e->opt.pipe_gpw = value;
            return SN_OK;
        case SN_OPT_PLAY_SPLIT:
            if (value < 0 || value > 1) return fail(SN_EINVAL, "play split must be 0 or 1");
            e->opt.play_split = value;
            return SN_OK;
        case SN_OPT_TWIST_EVERY:
            if (value < 1 || value > kTwistEveryMax) return fail(SN_EINVAL, "twist every must be 1 .. 5");
            e->opt.twist_every = value;
            return SN_OK;
        case SN_OPT_TWIST_DEPTH:  // thresholds only: takes effect at the next twist, no pipeline restart
            if (value < 0 || value > kTwistDepthMax) return fail(SN_EINVAL, "twist depth must be 0 .. 3");
            e->opt.twist_depth = value;
            return SN_OK;
        case SN_OPT_TWIST_ROUND:
            if (value < 0 || value > 1) return fail(SN_EINVAL, "twist round must be 0 or 1");
            e->opt.twist_round = value;
            return SN_OK;
        case SN_OPT_PLAY_QUAD:
        case SN_OPT_PIPE_FUSED:  // round-5 experiments, measured slower and removed
            return fail(SN_EUNSUPPORTED, "option removed (k_play_quad / the fused twist measured slower)");
        case SN_OPT_PIPE_DEC:
            if (value < 0 || value > 1) return fail(SN_EINVAL, "pipe dec must be 0 or 1");
            e->opt.pipe_dec = value;
            return SN_OK;
        case SN_OPT_PLAY_GROUP:  // the launch form only: the pipeline's bookkeeping is in chunks either way, no restart
            if (value < 0 || value > 1) return fail(SN_EINVAL, "play group must be 0 or 1");
            e->opt.play_group = value;
            return SN_OK;
        case SN_OPT_DEC_WALK:  // the form of k_decode only, read at every dispatch (dec_launch): the same records either
                               // way, so nothing past the pipeline sync every option change begins with (above)
            if (value < 0 || value > 1) return fail(SN_EINVAL, "dec walk must be 0 or 1");
            e->opt.dec_walk = value;
            return SN_OK;
        case SN_OPT_DEC_EARLY:  // as SN_OPT_DEC_WALK: the form of k_decode only, read at every dispatch
            if (value < 0 || value > 1) return fail(SN_EINVAL, "dec early must be 0 or 1");
            e->opt.dec_early = value;
            return SN_OK;
        case SN_OPT_TWIST_SKIP:
            if (value < 0 || value > 1) return fail(SN_EINVAL, "twist skip must be 0 or 1");
            e->opt.twist_skip = value;
            return SN_OK;
        case SN_OPT_PIPE_LEAD:
            if (value < 64 || value > kPipeLead) return fail(SN_EINVAL, "pipe lead must be in 64..600");
            e->opt.pipe_lead = value;
            return SN_OK;
        case SN_OPT_TIMING:
            if (value < 0 || value > 4096) return fail(SN_EINVAL, "timing launches must be in 0..4096");
            HIP_TRY(hipSetDevice(e->device));
            HIP_TRY(hipDeviceSynchronize());
            free_timing(e);
            if (value) {
                e->tev = new hipEvent_t[kTimingEvents * value]();
                e->tev_tw = new int[value]();
                e->tcap = value;
                for (int i = 0; i < kTimingEvents * value; i++) HIP_TRY(hipEventCreate(&e->tev[i]));
            }
            return SN_OK;
        default: return fail(SN_EINVAL, "unknown option");
    }
}

sn_status sn_info(const sn_env* e, int64_t* B, int* N, int* C, int* mode) {
    if (!e) return fail(SN_EINVAL, "env is NULL");
    if (B) *B = e->s.B;
    if (N) *N = e->s.N;
    if (C) *C = e->s.C;
    if (mode) *mode = e->s.rng_mode;
    return SN_OK;
}

sn_status sn_reset(sn_env* e, const uint8_t* decks, void* stream) {
    if (!e) return fail(SN_EINVAL, "env is NULL");
    hipStream_t st = (hipStream_t)stream;
    if (sn_pipe_sync(e, st) != SN_OK) return SN_EHIP;
    const DevState& s = e->s;
    if (s.lg_K) {  // a batched tournament: every game draws its seats, then deals (tournament.py:132-138)
        if (decks) return fail(SN_EINVAL, "a tournament handle deals from its own streams (decks must be NULL)");
        if (s.rng_mode == SN_RNG_NUMPY_MT) {
            SN_DISPATCH_N(s.N, {
                if constexpr (NN >= 2 && NN <= kLeagueMaxPlayers)
                    hipLaunchKernelGGL((k_reset<NN, RNG_NUMPY_MT, true>), dim3(grid_for(s.B)), dim3(kBlock), 0, st, s, decks);
            });
        } else {
            SN_DISPATCH_N(s.N, {
                if constexpr (NN >= 2 && NN <= kLeagueMaxPlayers)
                    hipLaunchKernelGGL((k_reset<NN, RNG_PHILOX, true>), dim3(grid_for(s.B)), dim3(kBlock), 0, st, s, decks);
            });
        }
        e->lg_phase = 0;
        e->phase = -1;
    } else if (s.rng_mode == SN_RNG_NUMPY_MT) {
        SN_DISPATCH_N(s.N, hipLaunchKernelGGL((k_reset<NN, RNG_NUMPY_MT>), dim3(grid_for(s.B)), dim3(kBlock), 0, st, s, decks));
    } else {
        SN_DISPATCH_N(s.N, hipLaunchKernelGGL((k_reset<NN, RNG_PHILOX>), dim3(grid_for(s.B)), dim3(kBlock), 0, st, s, decks));
    }
    if (!s.lg_K) e->phase = 0;  // every game dealt: in lockstep
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

sn_status sn_reset_to(sn_env* e, const int8_t* board, const int8_t* hands, void* stream) {
    if (!e || !board || !hands) return fail(SN_EINVAL, "NULL argument");
    e->phase = -1;
    hipStream_t st = (hipStream_t)stream;
    const DevState& s = e->s;
    SN_DISPATCH_N(s.N, hipLaunchKernelGGL((k_reset_to<NN>), dim3(grid_for(s.B)), dim3(kBlock), 0, st, s, board, hands));
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

// ---------------------------------------------------------------- the k_play launch plan
// LDS per CU (gfx950); a k_play block (4 waves) must fit in it
constexpr int kLdsBytes = 160 * 1024;

// Staged observation rows (obs_staged, sechs_play.h) leave LDS as 16-byte pieces: sn_rollout and
// sn_league_rollout require them 16-byte aligned -- before anything is launched.
static sn_status check_obs_align(const int8_t* obs, int stride) {
    if (obs && (((uintptr_t)obs) & 3)) return fail(SN_EINVAL, "obs must be 4-byte aligned");
    if (obs_staged(obs, stride) && (((uintptr_t)obs) & 15)) return fail(SN_EINVAL, "obs with stride 48 must be 16-byte aligned");
    return SN_OK;
}

// The dynamic LDS of one k_play wave, by the kernel's RngMode: the lanes' deal decks or the obs staging
// area (never live together, play_steps), then -- RNG_NUMPY_PIPE: the lanes' RingPipe windows (gpw = 32 or
// 64 games per wave); RNG_NUMPY_RING: their copies of the k_mt_prep ring if the block still fits, else
// ring_lds = 0 and RNG_NUMPY_RING_HBM plays; RNG_NUMPY_DEC: the staging area alone (no deck either);
// every other mode: nothing more.  (k_play_split sizes its own: split_lds.)
struct LdsPlan {
    int wave;      // bytes per wave (PlayArgs::wave_lds)
    int ring_lds;  // of them per lane for the ring copy / window, at the region's end (PlayArgs::ring_lds)
};
constexpr size_t block_lds(LdsPlan p) { return (size_t)p.wave * (kBlock / 64); }
constexpr LdsPlan lds_plan(int N, bool staged, int mode, int gpw = 64, int ring_w = 0) {
    const int stage = staged ? gpw * obs_stage_pieces(N) * 16 : 0, deal = gpw * kDealStride;
    if (mode == RNG_NUMPY_DEC) return {stage ? stage : 16, 0};
    const LdsPlan direct{deal > stage ? deal : stage, 0};
    if (mode == RNG_NUMPY_PIPE) return {direct.wave + gpw * kPipeSlot, kPipeSlot};
    const LdsPlan ring{direct.wave + 64 * ring_lds_stride(ring_w), ring_lds_stride(ring_w)};
    return (mode == RNG_NUMPY_RING && block_lds(ring) <= (size_t)kLdsBytes) ? ring : direct;
}
// window: 240 + 30 bytes in whole 16-B chunks = 256, + 8 for the funnel's second read
static_assert(kPipeSlot == 264, "RingPipe window per lane");
// decks 64 x 212 = 13 568 (> staging 64 x 13 pieces x 16 = 13 312), windows 64 x 264 = 16 896
static_assert(lds_plan(4, true, RNG_NUMPY_PIPE, 64).wave == 13568 + 16896 && lds_plan(4, true, RNG_NUMPY_PIPE).ring_lds == 264, "");
// staging alone: 64 lanes x 13 pieces x 16 bytes
static_assert(lds_plan(4, true, RNG_NUMPY_DEC).wave == 13312 && lds_plan(4, false, RNG_NUMPY_DEC).wave == 16, "");
// staging 64 x 31 pieces x 16 = 31 744 (> decks 13 568)
static_assert(lds_plan(10, true, RNG_PHILOX).wave == 31744 && lds_plan(10, false, RNG_NUMPY_MT).wave == 13568, "");
// decks 13 568 + ring copies 64 x (256 + 8) = 16 896: 30 464 per wave, 121 856 per block <= 163 840
static_assert(lds_plan(4, true, RNG_NUMPY_RING, 64, 256).wave == 30464 && lds_plan(4, true, RNG_NUMPY_RING, 64, 256).ring_lds == 264, "");
// decks 13 568 + ring copies 64 x 520 = 33 280: 187 392 per block > 163 840, so the ring stays in HBM
static_assert(lds_plan(4, true, RNG_NUMPY_RING, 64, 512).wave == 13568 && lds_plan(4, true, RNG_NUMPY_RING, 64, 512).ring_lds == 0, "");

static void apply_plan(PlayArgs& a, LdsPlan p) { a.wave_lds = p.wave, a.ring_lds = p.ring_lds; }

static PlayArgs rollout_args(int steps, int flags, int obs_stride, int32_t* rewards, uint8_t* done, uint8_t* actions, int8_t* obs) {
    PlayArgs a{};
    a.steps = steps, a.flags = flags, a.obs_stride = obs_stride;
    a.rewards = rewards, a.done = done, a.actions_out = actions, a.obs = obs;
    return a;
}

// env-steps [t0, t0 + n) of a rollout's arguments
static PlayArgs slice_steps(const PlayArgs& a, int t0, int n, int64_t B, int64_t N) {
    PlayArgs c = a;
    c.steps = n;
    c.step0 = a.step0 + t0;
    if (a.rewards) c.rewards = a.rewards + (int64_t)t0 * B * N;
    if (a.done) c.done = a.done + (int64_t)t0 * B;
    if (a.actions_out) c.actions_out = a.actions_out + (int64_t)t0 * B * N;
    if (a.obs) c.obs = a.obs + (int64_t)t0 * B * N * a.obs_stride;
    return c;
}


// The k_play variants: (mode, games per wave, tournament handle) -> instantiation.  32 games per wave exist on
// the pipelined ring only, league seats on it and on Philox.
static sn_status launch_play_mode(const DevState& s, const PlayArgs& a, int mode, int gpw, hipStream_t st) {
    const unsigned grid = (unsigned)((s.B + gpw * (kBlock / 64) - 1) / (gpw * (kBlock / 64)));
    const size_t shmem = (size_t)a.wave_lds * (kBlock / 64);
    const bool lg = s.lg_K != 0;
    SN_DISPATCH_N(s.N, {
        switch (mode) {
            case RNG_NUMPY_MT: return (launch_k_play<NN, RNG_NUMPY_MT>(s, a, grid, shmem, st));
            case RNG_NUMPY_RING: return (launch_k_play<NN, RNG_NUMPY_RING>(s, a, grid, shmem, st));
            case RNG_NUMPY_RING_HBM: return (launch_k_play<NN, RNG_NUMPY_RING_HBM>(s, a, grid, shmem, st));
            case RNG_NUMPY_DEC: return (launch_k_play<NN, RNG_NUMPY_DEC>(s, a, grid, shmem, st));
            case RNG_NUMPY_PIPE:
                if (gpw == 32) return (launch_k_play<NN, RNG_NUMPY_PIPE, 32>(s, a, grid, shmem, st));
                return lg ? (launch_k_play<NN, RNG_NUMPY_PIPE, 64, true>(s, a, grid, shmem, st))
                          : (launch_k_play<NN, RNG_NUMPY_PIPE>(s, a, grid, shmem, st));
            default:
                return lg ? (launch_k_play<NN, RNG_PHILOX, 64, true>(s, a, grid, shmem, st))
                          : (launch_k_play<NN, RNG_PHILOX>(s, a, grid, shmem, st));
        }
    });
    return SN_OK;
}

// k_play_split applies to in-kernel DrunkHamster rollouts of a handle whose
// games are in lockstep (e->phase), with auto-reset, N <= kSplitMaxPlayers
static bool split_ok(const sn_env* e, const PlayArgs& a) {
    return e->opt.play_split && e->phase >= 0 && (a.flags & SN_AUTO_RESET) && !a.actions && !a.invalid && !e->s.lg_K &&
           e->s.N <= kSplitMaxPlayers;
}

// one play launch outside the pipeline (ring-fed: behind its own k_mt_prep)
static sn_status launch_play_one(sn_env* e, PlayArgs a, hipStream_t st) {
    const DevState& s = e->s;
    int mode = RNG_PHILOX;
    if (s.rng_mode == SN_RNG_NUMPY_MT) mode = (!a.actions && s.ring_w > 0) ? RNG_NUMPY_RING : RNG_NUMPY_MT;
    const LdsPlan plan = lds_plan(s.N, obs_staged(a.obs, a.obs_stride), mode, 64, s.ring_w);
    apply_plan(a, plan);
    if (mode == RNG_NUMPY_RING) {
        if (const sn_status r = launch_mt_prep(s, st); r != SN_OK) return r;
        if (!plan.ring_lds) mode = RNG_NUMPY_RING_HBM;
    } else if (mode == RNG_PHILOX && split_ok(e, a) && a.steps <= kHand) {  // at most one deal per launch
        a.n0 = kHand - e->phase;
        SN_DISPATCH_N(s.N, {
            if constexpr (NN <= kSplitMaxPlayers) {
                const size_t sl = split_lds(NN, a.steps);
                HIP_TRY(hipFuncSetAttribute((const void*)k_play_split<NN, RNG_PHILOX>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)sl));
                hipLaunchKernelGGL((k_play_split<NN, RNG_PHILOX>), dim3(grid_for(s.B)), dim3(2 * kBlock), sl, st, s, a);
            }
        });
        HIP_TRY(hipGetLastError());
        return SN_OK;
    }
    return launch_play_mode(s, a, mode, 64, st);
}

// ---------------------------------------------------------------- the pipeline schedule
// Slots by index: play launch p reads the consumer position launch p-1 left
// in pabsc and writes its own; twist G writes its twisted end to ptend, read
// by the launches of group G+1; decode G leaves the decoder's position in the
// two pabsc slots past the play launches'.  The start-up twist and decode
// count as index -1 (kStartUp), its consumer position as launch -1's.
constexpr uint64_t kStartUp = ~0ull;
constexpr uint32_t kSlotMask = (uint32_t)kPipeSlots - 1u;
static inline int pabsc_in(uint64_t p) { return (int)((p + kSlotMask) & kSlotMask); }
static inline int pabsc_out(uint64_t p) { return (int)(p & kSlotMask); }
static inline int ptend_slot(uint64_t G) { return (int)(G & 1u); }
static inline int dec_slot(uint64_t G) { return kDecSlot + (int)(G & 1u); }
static inline int dec_record(int64_t episode) { return (int)(episode % kDecRecords); }  // drec slot of an episode's record

sn_status sn_pipe_sync(sn_env* e, hipStream_t st) {
    if (!e || !e->pl.valid) return SN_OK;
    // k_pipe_code reads the last k_play's consumer position (pabsc) and the
    // last k_mt_ahead's twisted end: wait for both, whatever stream `st` is
    // (the null stream does not order behind a non-blocking caller stream).
    // ev_play was recorded behind the last pipelined k_play when its rollout
    // was enqueued (launch_pipe), on the caller's stream of that call -- so no
    // stream of an earlier call is touched here; ev_prep is recorded now,
    // behind everything enqueued so far on the side stream.
    HIP_TRY(hipStreamWaitEvent(st, e->pl.ev_play, 0));
    HIP_TRY(hipEventRecord(e->pl.ev_prep, e->pl.side));
    HIP_TRY(hipStreamWaitEvent(st, e->pl.ev_prep, 0));
    HIP_TRY(hipEventRecord(e->pl.ev_prep2, e->pl.side2));  // the decodes (their ring reads) are done too
    HIP_TRY(hipStreamWaitEvent(st, e->pl.ev_prep2, 0));
    // the last play launch wrote pabsc[pl_cout]; the last twist ptend[tw_out]
    hipLaunchKernelGGL(k_pipe_code, dim3((unsigned)((e->s.B + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0, st,
                       e->s, e->pl.pl_cout, e->pl.tw_out);
    HIP_TRY(hipGetLastError());
    e->pl.valid = 0;
    return SN_OK;
}

// Longest pipelined launch for N players.  k_mt_ahead leaves 593..600 words
// twisted past the consumer position of the launch BEFORE the running one,
// so two consecutive launches must draw <= 592 words.  With auto-reset, 2c
// consecutive env-steps hold at most ceil(2c/10) deals (103 draws each,
// ~146 words) and each hand size at most that often; the exact tail of the
// summed geometric word counts (tools/pipe_tail.py) gives, per game and
// launch pair, P(> 592 words) = 2e-31 at N = 4 with 10-step launches
// (two episodes) but 1.4e-25 at N = 5 and 4.5e-5 at N = 10; with 5-step
// launches (one episode per pair) it is <= 6.1e-73 for every N <= 10.
static int pipe_max_chunk(int N) { return N <= 4 ? 10 : 5; }

static sn_status launch_ahead(const DevState& s, bool init, bool round_tw, const AheadArgs& aa, hipStream_t st) {
    const dim3 pg((unsigned)((s.B + kBlock / 64 - 1) / (kBlock / 64)));
    if (init && round_tw) hipLaunchKernelGGL((k_mt_ahead<true, true>), pg, dim3(kBlock), 0, st, s, aa);
    else if (init) hipLaunchKernelGGL((k_mt_ahead<true, false>), pg, dim3(kBlock), 0, st, s, aa);
    else if (round_tw) hipLaunchKernelGGL((k_mt_ahead<false, true>), pg, dim3(kBlock), 0, st, s, aa);
    else hipLaunchKernelGGL((k_mt_ahead<false, false>), pg, dim3(kBlock), 0, st, s, aa);
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

// records of episodes [e0, e0 + ne) (global counter since the pipeline start) on stream st
static sn_status dec_launch(sn_env* e, int64_t e0, int ne, int phi0, int tpar, int cin, int cout, hipStream_t st) {
    const DevState& s = e->s;
    const DecArgs d{dec_record(e0), ne, phi0, tpar, cin, cout};
    const dim3 grid((unsigned)((s.B + kDecBlock - 1) / kDecBlock));
    SN_DISPATCH_N(s.N, {
        if constexpr (NN <= kSplitMaxPlayers) {
            const bool walk = e->opt.dec_walk != 0;
            const bool touch = e->opt.dec_early != 0;
            if (walk && touch) hipLaunchKernelGGL((k_decode<NN, true, true>), grid, dim3(kDecBlock), 0, st, s, d);
            else if (walk) hipLaunchKernelGGL((k_decode<NN, true, false>), grid, dim3(kDecBlock), 0, st, s, d);
            else if (touch) hipLaunchKernelGGL((k_decode<NN, false, true>), grid, dim3(kDecBlock), 0, st, s, d);
            else hipLaunchKernelGGL((k_decode<NN, false, false>), grid, dim3(kDecBlock), 0, st, s, d);
        }
    });
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

// Decode-ahead applies to in-kernel DrunkHamster rollouts with auto-reset of
// a plain (non-tournament) handle of N <= 4 whose games are in lockstep
// (e->phase known): every launch's random decisions are then the same
// function of the stream for every game.
static bool dec_ok(const sn_env* e, const PlayArgs& a) {
    return e->opt.pipe_dec && e->phase >= 0 && (a.flags & SN_AUTO_RESET) && !a.actions && !a.invalid && !e->s.lg_K &&
           e->s.N <= kSplitMaxPlayers && e->opt.pipe_gpw == 64 && e->s.drec;
}

// Start the pipeline from mt_pos: twist the lead ahead, synchronously (on the caller's stream).
static sn_status pipe_start(sn_env* e, int K, bool dec, int lead, hipStream_t st) {
    sn_env::Pipeline& pl = e->pl;
    // decode-ahead: the start position to the decoder's input slot of the first decode and
    // the play slot (a sync before any play launch exports it)
    const AheadArgs aa{dec ? dec_slot(kStartUp - 1) : pabsc_out(kStartUp), ptend_slot(kStartUp - 1), ptend_slot(kStartUp), lead,
                       e->perr_host_dev, dec ? pabsc_out(kStartUp) : -1, e->opt.twist_depth};
    pl.tw_out = ptend_slot(kStartUp), pl.pl_cout = pabsc_out(kStartUp), pl.launches = 0;
    if (const sn_status r = launch_ahead(e->s, true, e->opt.twist_round, aa, st); r != SN_OK) return r;
    if (dec) {  // the records of the first group's launches (episodes 0 .. K), from the current step on
        pl.dec_e = 0;
        const sn_status r = dec_launch(e, 0, K + 1, e->phase, ptend_slot(kStartUp), dec_slot(kStartUp - 1), dec_slot(kStartUp), st);
        if (r != SN_OK) return r;
        pl.dec_next = K + 1;
    }
    HIP_TRY(hipEventRecord(pl.ev_prep, st));
    pl.valid = 1, pl.K = K, pl.dec = dec ? 1 : 0;
    return SN_OK;
}

// Twist G on `side` -- and, decode-ahead, decode G on `side2` -- beside play launch p, the first of group G, which
// started in episode e_start.  ti: the launch's SN_OPT_TIMING events (-1: none).
static sn_status pipe_twist(sn_env* e, uint64_t G, uint64_t p, int64_t e_start, int lead, int ti, hipStream_t st) {
    sn_env::Pipeline& pl = e->pl;
    hipEvent_t* tv = (ti >= 0) ? e->tev + kTimingEvents * ti : nullptr;
    // beside this launch (SECHS_PIPE_SERIAL=1, diagnostics: after it -- solo kernel times)
    if (e->opt.pipe_serial) HIP_TRY(hipEventRecord(pl.ev_main, st));
    HIP_TRY(hipStreamWaitEvent(pl.side, pl.ev_main, 0));
    if (tv) HIP_TRY(hipEventRecord(tv[2], pl.side));
    // SN_OPT_TWIST_SKIP (tests only): the overrun detector under the default schedule
    const AheadArgs aa{pl.dec ? dec_slot(G - 1) : pabsc_in(p), ptend_slot(G - 1), ptend_slot(G),
                       (e->opt.twist_skip && G >= 1u) ? 0 : lead, e->perr_host_dev, -1, e->opt.twist_depth};
    if (const sn_status r = launch_ahead(e->s, false, e->opt.twist_round, aa, pl.side); r != SN_OK) return r;
    if (tv) HIP_TRY(hipEventRecord(tv[3], pl.side));
    if (pl.dec) {
        // decode G on side2, concurrent with twist G: the records group G+1 may touch --
        // its launches start at most K episodes past this launch's and touch at most one
        // more each: episodes < e_start + 2K + 1 (the ring of kDecRecords >= 2K + 2
        // slots never overwrites one a running launch reads: the oldest, launch p-K,
        // reads episodes >= e_start - K, 3K + 1 <= kDecRecords).  A fused launch
        // (SN_OPT_PLAY_GROUP) covers chunks of one group only and loads, deal by deal, the
        // records its chunks would have loaded as launches of their own: the same episodes
        // (>= e_start - K for the group before), while it runs in those launches' place on
        // the play stream, so the bound holds unchanged.  It reads the words twist
        // G-1 twisted and waits for that twist only (which waited for launch p-K-1), and
        // its position goes to the decoder slot of decode G, which twist G+1 reads.
        const int64_t target = e_start + 2 * pl.K + 1;
        // (group 0: the start-up twist and decode ran on the play stream, before ev_main)
        if (e->opt.pipe_serial || G == 0u) HIP_TRY(hipStreamWaitEvent(pl.side2, pl.ev_main, 0));
        if (G >= 1u) HIP_TRY(hipStreamWaitEvent(pl.side2, pl.evt[ptend_slot(G - 1)], 0));
        if (tv) HIP_TRY(hipEventRecord(tv[4], pl.side2));
        const int ne = target > pl.dec_next ? (int)(target - pl.dec_next) : 0;
        // ne == 0 (short launches): still a launch, so the position moves to decode G's slot
        const sn_status r = dec_launch(e, pl.dec_next, ne, 0, ptend_slot(G - 1), dec_slot(G - 1), dec_slot(G), pl.side2);
        if (r != SN_OK) return r;
        pl.dec_next = max(pl.dec_next, target);
        if (tv) {
            HIP_TRY(hipEventRecord(tv[5], pl.side2));
            e->tev_tw[ti] |= 2;
        }
        HIP_TRY(hipEventRecord(pl.evd[ptend_slot(G)], pl.side2));
    }
    HIP_TRY(hipEventRecord(pl.evt[ptend_slot(G)], pl.side));
    HIP_TRY(hipEventRecord(pl.ev_prep, pl.side));
    pl.tw_out = ptend_slot(G);
    return SN_OK;
}

// The pipelined numpy-MT rollout: per launch of <= 10 env-steps, k_play (on
// the caller's stream) draws from words k_mt_ahead twisted during the
// previous launch, while the next k_mt_ahead runs on the side stream.
// Hand-off: HIP events both ways -- a wait and a record on the caller's
// stream between play launches.  (Device-flag and in-launch hand-offs were
// built and measured slower on gfx950)
//
// SN_OPT_TWIST_EVERY = K: play launches in groups of K; beside the first
// launch p of group G runs twist G, leading the consumer position of
// launch p-1 by 600 K words -- the 2K launches p .. p+2K-1, i.e. K
// launch pairs of the §4 tail bound -- and launch p waits for twist G-1
// only, which had a whole group of launches to finish.  Per group, one
// record and one wait on the caller's stream (K = 1: the launch before).
// Slots: pabsc by launch index mod kPipeSlots (8 >= K + 3: the next writer
// of launch p-1's slot is launch p+7, in group G+1 or later, which is
// ordered behind twist G -- the reader of that slot), ptend by group
// parity.  The ring holds the lead, the SN_OPT_TWIST_DEPTH rounds a refill
// adds and a round's overshoot for K <= 5 (kPipeSpanMax, sechs_state.h), and
// mt0 the word-0 crossings of that span.
//
// Decode-ahead: twist G runs on `side` CONCURRENTLY with decode G on `side2`,
// so it leads the decoder position after decode G-1 by the words of the
// 2K + 1 episodes decode G+1 may need: 600 (K + 1) words (~200 per episode at
// N <= 4), and the play launches (one launch plan: no deck, no ring window)
// read no ring at all -- so the 10-step limit does not bind them, and one launch plays
// the call's chunks of a whole group (SN_OPT_PLAY_GROUP, the loop below).  Otherwise the
// twists lead the play consumer by 600 K words.
static sn_status launch_pipe(sn_env* e, PlayArgs a, LdsPlan plan, hipStream_t st) {
    const DevState& s = e->s;
    sn_env::Pipeline& pl = e->pl;
    const int gpw = e->opt.pipe_gpw, K = e->opt.twist_every;
    const bool dec = dec_ok(e, a);
    const int mode = dec ? RNG_NUMPY_DEC : RNG_NUMPY_PIPE;
    apply_plan(a, dec ? lds_plan(s.N, obs_staged(a.obs, a.obs_stride), RNG_NUMPY_DEC) : plan);
    if (pl.valid && (pl.K != K || (pl.dec != 0) != dec)) {  // restart with the other group size / form
        if (const sn_status r = sn_pipe_sync(e, st); r != SN_OK) return r;
    }
    const int lead = dec ? min(e->opt.pipe_lead * (K + 1), kPipeRing - kMtN) : e->opt.pipe_lead * K;
    static_assert(kPipeLeadMax <= kPipeRing - kMtN, "the decode-ahead lead is never capped by the ring");
    if (!pl.valid) {
        if (const sn_status r = pipe_start(e, K, dec, lead, st); r != SN_OK) return r;
    } else {
        // order behind the last pipelined k_play (recorded on the stream of
        // that call): always, also on the same stream -- a stream handle's
        // value may be reused by a new stream once the caller destroyed the
        // old one, and a wait on an event already behind costs ~nothing
        HIP_TRY(hipStreamWaitEvent(st, pl.ev_play, 0));
    }
    // a tournament game adds its seat draw (<= K - 1 + 1 draws): 10-step
    // launches keep the pair tail < 1e-26 up to K = 8 agents at N <= 4
    // (tools/pipe_tail.py), beyond that 5-step launches
    const int chunk = min(e->opt.chunk_steps, (s.lg_K > 8) ? 5 : pipe_max_chunk(s.N));
    int phase = dec ? e->phase : 0;  // decode-ahead: the games' step within their episode
    // SN_OPT_PLAY_GROUP, decode-ahead only: one k_play launch for the call's consecutive chunks
    // of one twist group -- the tail bound above limits whoever reads the ring, here k_decode;
    // k_play reads records finished a group earlier.  The bookkeeping stays in chunks.
    const bool fuse = dec && e->opt.play_group;
    for (int t0 = 0, m = 1; t0 < a.steps; t0 += m * chunk) {
        const uint64_t p = pl.launches, G = p / (uint64_t)K;
        const bool first = (p % (uint64_t)K) == 0u;  // twist G beside this launch
        // chunks [p, p + m) in this launch: to the end of the call or of group G, whichever is first
        m = fuse ? (int)min((int64_t)(a.steps - t0 + chunk - 1) / chunk, (int64_t)K - (int64_t)(p % (uint64_t)K)) : 1;
        PlayArgs c = slice_steps(a, t0, min(m * chunk, a.steps - t0), s.B, s.N);
        c.pipe_cin = pabsc_in(p), c.pipe_cout = pabsc_out(p + (uint64_t)m - 1u);
        c.pipe_t = ptend_slot(G - 1);  // twist G-1's end (the start-up's for group 0)
        if (dec) {  // the launch's records: its first episode's, then (past each deal) the next one's
            c.n0 = phase;
            c.drec0 = dec_record(pl.dec_e);
        }
        // twist G-1 (decode-ahead: decode G-1, which waited for twist G-1 itself)
        if (first && G >= 1u) HIP_TRY(hipStreamWaitEvent(st, (dec ? pl.evd : pl.evt)[ptend_slot(G - 1)], 0));
        if (first && !e->opt.pipe_serial) HIP_TRY(hipEventRecord(pl.ev_main, st));  // launch p-1's consumption is final
        const int ti = (e->tn < e->tcap) ? e->tn++ : -1;  // SN_OPT_TIMING: this launch's events
        hipEvent_t* tv = (ti >= 0) ? e->tev + kTimingEvents * ti : nullptr;
        if (tv) e->tev_tw[ti] = first ? 1 : 0;
        if (tv) HIP_TRY(hipEventRecord(tv[0], st));
        if (const sn_status r = launch_play_mode(s, c, mode, gpw, st); r != SN_OK) return r;  // decode-ahead: gpw == 64
        const int64_t e_start = pl.dec_e;  // the episode this launch started in
        if (dec) {
            phase += c.steps;  // as if the chunks had been launched one by one
            pl.dec_e += phase / kHand, phase %= kHand;
        }
        if (tv) HIP_TRY(hipEventRecord(tv[1], st));
        if (first) {
            if (const sn_status r = pipe_twist(e, G, p, e_start, lead, ti, st); r != SN_OK) return r;
        }
        pl.pl_cout = c.pipe_cout;
        pl.launches += (uint64_t)m;
    }
    // behind this rollout's last k_play, on the caller's stream of THIS call:
    // the next call (or sn_pipe_sync) orders behind it without touching a
    // stream the caller may have destroyed since (one record per rollout)
    HIP_TRY(hipEventRecord(pl.ev_play, st));
    return SN_OK;
}

// ---------------------------------------------------------------- rollout and step entry points
// Every rollout and step goes through here.  Pipelined where it applies; else a
// ring-fed (numpy-MT, in-kernel DrunkHamster) rollout runs in launches of
// at most chunk_steps env-steps, each behind its own k_mt_prep, so that one
// ring covers a launch's draws (a 4-player episode: 193.5 +- 9.3 words).
static sn_status launch_play(sn_env* e, PlayArgs a, hipStream_t st) {
    const DevState& s = e->s;
    const bool numpy = s.rng_mode == SN_RNG_NUMPY_MT;
    a.vec_out = ((((uintptr_t)a.rewards) & 15) == 0) && ((((uintptr_t)a.actions_out) & 3) == 0);
    if (s.lg_K) {  // tournament handles: in-kernel DrunkHamster seats, pipelined numpy-MT or philox
        if (a.actions) return fail(SN_EUNSUPPORTED, "a tournament handle plays in-kernel DrunkHamster seats only (sn_rollout)");
        if (!(a.flags & SN_AUTO_RESET)) return fail(SN_EINVAL, "a tournament handle rolls out with SN_AUTO_RESET");
    }
    if (numpy && !a.actions && (e->opt.pipe || s.lg_K)) {
        const LdsPlan plan = lds_plan(s.N, obs_staged(a.obs, a.obs_stride), RNG_NUMPY_PIPE, e->opt.pipe_gpw);
        const bool fits = block_lds(plan) <= (size_t)kLdsBytes;
        if (s.lg_K && (!e->opt.pipe || e->opt.pipe_gpw != 64 || !fits))
            return fail(SN_EUNSUPPORTED, "tournament rollouts need the pipelined numpy-MT path (64 games per wave)");
        if (fits) return launch_pipe(e, a, plan, st);
    }
    if (const sn_status r = sn_pipe_sync(e, st); r != SN_OK) return r;
    const bool ring = numpy && !a.actions && s.ring_w > 0;
    const int chunk = ring ? e->opt.chunk_steps : a.steps;  // only a ring limits a launch's draws
    for (int t0 = 0; t0 < a.steps; t0 += chunk) {
        const sn_status r = launch_play_one(e, slice_steps(a, t0, min(chunk, a.steps - t0), s.B, s.N), st);
        if (r != SN_OK) return r;
    }
    return SN_OK;
}


sn_status sn_step(sn_env* e, const int32_t* actions, int32_t* rewards, uint8_t* done, int32_t* invalid, int flags,
                  void* stream) {
    if (!e) return fail(SN_EINVAL, "env is NULL");
    if (e->s.lg_K) return fail(SN_EUNSUPPORTED, "a tournament handle plays whole games with sn_league_rollout");
    e->phase = -1;  // external actions may be refused per game
    PlayArgs a{};
    a.steps = 1;
    a.flags = flags;
    a.actions = actions;
    a.rewards = rewards;
    a.done = done;
    a.invalid = invalid;
    return launch_play(e, a, (hipStream_t)stream);
}

sn_status sn_rollout(sn_env* e, int steps, int32_t* rewards, uint8_t* done, uint8_t* actions, int8_t* obs,
                     int obs_stride, int flags, void* stream) {
    if (!e) return fail(SN_EINVAL, "env is NULL");
    if (steps < 0) return fail(SN_EINVAL, "steps must be >= 0");
    const int L = (flags & SN_NO_SUMMARIES) ? 35 : 47;
    if (obs && (obs_stride < L || (obs_stride & 3))) return fail(SN_EINVAL, "obs_stride must be a multiple of 4 and >= obs length");
    if (check_obs_align(obs, obs_stride) != SN_OK) return SN_EINVAL;
    if (steps == 0) return SN_OK;
    if (e->perr_host && __atomic_load_n(e->perr_host, __ATOMIC_RELAXED))
        return fail(SN_ERNG, "a pipelined numpy-MT draw ran past the twisted words; this handle's rollouts are invalid "
                             "from that launch on (sn_pipe_errors)");
    const sn_status r = launch_play(e, rollout_args(steps, flags, obs_stride, rewards, done, actions, obs), (hipStream_t)stream);
    if (r == SN_OK && e->s.lg_K) e->lg_phase = (e->lg_phase + steps) % kHand;
    e->phase = (r == SN_OK && e->phase >= 0 && (flags & SN_AUTO_RESET)) ? (e->phase + steps) % kHand : -1;
    return r;
}

// ---------------------------------------------------------------- league entry points
sn_status sn_league_config(sn_env* e, int num_agents, int min_players, int max_players) {
    if (!e) return fail(SN_EINVAL, "env is NULL");
    DevState& s = e->s;
    HIP_TRY(hipSetDevice(e->device));
    if (num_agents == 0) {
        HIP_TRY(hipDeviceSynchronize());
        if (s.lgs) (void)hipFree(s.lgs);
        s.lgs = nullptr;
        s.lg_K = s.lg_lo = s.lg_hi = 0;
        return SN_OK;
    }
    if (max_players != s.N) return fail(SN_EINVAL, "max_players must equal the handle's num_players");
    if (min_players < 2 || min_players > max_players || max_players > kLeagueMaxPlayers)
        return fail(SN_EINVAL, "need 2 <= min_players <= max_players <= 6");
    if (num_agents < max_players || num_agents > kLeagueMaxAgents)
        return fail(SN_EINVAL, "need max_players <= num_agents <= 16 (tournament.py:170 asserts len(self) >= num_players)");
    if (!s.lgs && hipMalloc((void**)&s.lgs, sizeof(uint32_t) * s.B) != hipSuccess) return fail(SN_ENOMEM, "league state");
    HIP_TRY(hipMemset(s.lgs, 0, sizeof(uint32_t) * s.B));
    s.lg_K = num_agents, s.lg_lo = min_players, s.lg_hi = max_players;
    for (int i = 0; i < kLeagueMaxAgents; i++) e->lg_kind[i] = SN_AGENT_RANDOM, e->lg_mpc[i] = 10, e->lg_mmax[i] = 100;
    e->lg_phase = -1;  // sn_reset deals the first games
    return SN_OK;
}

sn_status sn_league_rollout(sn_env* e, int steps, int32_t* rewards, uint8_t* done, uint8_t* actions, int8_t* obs,
                            int obs_stride, int32_t* records, void* stream) {
    if (!e) return fail(SN_EINVAL, "env is NULL");
    if (!e->s.lg_K) return fail(SN_EINVAL, "not a tournament handle (sn_league_config)");
    for (int i = 0; i < e->s.lg_K; i++)
        if (e->lg_kind[i] != SN_AGENT_RANDOM)
            return fail(SN_EUNSUPPORTED, "sn_league_rollout plays DrunkHamster agents in-kernel; mixed leagues use sn_league_step");
    if (e->lg_phase != 0) return fail(SN_EINVAL, "tournament rollouts start right after sn_reset or a whole number of games");
    if (steps % kHand) return fail(SN_EINVAL, "tournament rollouts play whole games (steps a multiple of 10)");
    if (steps < 0) return fail(SN_EINVAL, "steps must be >= 0");
    if (obs && (obs_stride < 47 || (obs_stride & 3))) return fail(SN_EINVAL, "obs_stride must be a multiple of 4 and >= 47");
    if (check_obs_align(obs, obs_stride) != SN_OK) return SN_EINVAL;
    if (steps == 0) return SN_OK;
    if (e->perr_host && __atomic_load_n(e->perr_host, __ATOMIC_RELAXED))
        return fail(SN_ERNG, "a pipelined numpy-MT draw ran past the twisted words (sn_pipe_errors)");
    PlayArgs a = rollout_args(steps, SN_AUTO_RESET, obs_stride, rewards, done, actions, obs);
    a.league_rec = records;
    return launch_play(e, a, (hipStream_t)stream);
}

// Host replay (no GPU): the reference scores a tournament game's Elo right
// after it (tournament.py:157-164), one game at a time; rl_6_nimmt/elo.py
// restates multi_elo's multiplayer Elo (parity unpinned).  Same operation
// order as elo.calc_elo, so the doubles match the Python replay bit for bit.
sn_status sn_elo_replay(const int32_t* rec, int64_t G, int NP, int K, double elo_k, double* elos) {
    if ((!rec && G > 0) || !elos) return fail(SN_EINVAL, "NULL argument");
    if (NP < 2 || NP > kLeagueMaxPlayers || K < 1 || K > kLeagueMaxAgents) return fail(SN_EINVAL, "bad sizes");
    for (int64_t i = 0; i < G; i++) {
        const int32_t* r = rec + i * (1 + NP);
        const uint32_t w = (uint32_t)r[0];
        const int k = (int)(w & 15u);
        if (k < 2 || k > NP) return fail(SN_EINVAL, "record " + std::to_string(i) + ": bad player count");
        int a[kLeagueMaxPlayers];
        double place[kLeagueMaxPlayers], old[kLeagueMaxPlayers], nw[kLeagueMaxPlayers];
        for (int p = 0; p < k; p++) {
            a[p] = (int)((w >> (4 + 4 * p)) & 15u);
            if (a[p] >= K) return fail(SN_EINVAL, "record " + std::to_string(i) + ": agent id out of range");
            old[p] = elos[a[p]];
        }
        for (int p = 0; p < k; p++) {  // Tournament._compute_absolute_positions: 1-based, ties averaged
            int greater = 0, equal = 0;
            for (int q = 0; q < k; q++) {
                greater += r[1 + q] > r[1 + p];
                equal += r[1 + q] == r[1 + p];
            }
            place[p] = (double)greater + 0.5 * (double)(1 + equal);
        }
        const double kk = elo_k / (double)(k - 1);
        for (int p = 0; p < k; p++) {
            double delta = 0.0;
            for (int q = 0; q < k; q++) {
                if (q == p) continue;
                const double actual = place[p] < place[q] ? 1.0 : (place[p] == place[q] ? 0.5 : 0.0);
                const double expected = 1.0 / (1.0 + std::pow(10.0, (old[q] - old[p]) / 400.0));
                delta += kk * (actual - expected);
            }
            nw[p] = old[p] + delta;
        }
        for (int p = 0; p < k; p++) elos[a[p]] = nw[p];
    }
    return SN_OK;
}

sn_status sn_league_seats(sn_env* e, uint32_t* out, void* stream) {
    if (!e || !out) return fail(SN_EINVAL, "NULL argument");
    if (!e->s.lg_K) return fail(SN_EINVAL, "not a tournament handle (sn_league_config)");
    HIP_TRY(hipMemcpyAsync(out, e->s.lgs, sizeof(uint32_t) * e->s.B, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return SN_OK;
}

// ---------------------------------------------------------------- state read-out
sn_status sn_obs(sn_env* e, void* out, int dtype, int stride, int flags, void* stream) {
    if (!e || !out) return fail(SN_EINVAL, "NULL argument");
    const int L = (flags & SN_NO_SUMMARIES) ? 35 : 47;
    if (stride < L) return fail(SN_EINVAL, "obs stride shorter than the observation");
    const DevState& s = e->s;
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = grid_for(s.B * s.N);
    const int summ = !(flags & SN_NO_SUMMARIES);
    switch (dtype) {
        case SN_I8: hipLaunchKernelGGL(k_obs<int8_t>, dim3(grid), dim3(kBlock), 0, st, s, (int8_t*)out, stride, summ); break;
        case SN_I16: hipLaunchKernelGGL(k_obs<int16_t>, dim3(grid), dim3(kBlock), 0, st, s, (int16_t*)out, stride, summ); break;
        case SN_I32: hipLaunchKernelGGL(k_obs<int32_t>, dim3(grid), dim3(kBlock), 0, st, s, (int32_t*)out, stride, summ); break;
        case SN_I64: hipLaunchKernelGGL(k_obs<int64_t>, dim3(grid), dim3(kBlock), 0, st, s, (int64_t*)out, stride, summ); break;
        case SN_F32: hipLaunchKernelGGL(k_obs<float>, dim3(grid), dim3(kBlock), 0, st, s, (float*)out, stride, summ); break;
        default: return fail(SN_EINVAL, "unknown obs dtype");
    }
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

sn_status sn_hands(sn_env* e, int8_t* out, void* stream) {
    if (!e || !out) return fail(SN_EINVAL, "NULL argument");
    hipLaunchKernelGGL(k_hands, dim3(grid_for(e->s.B * e->s.N)), dim3(kBlock), 0, (hipStream_t)stream, e->s, out);
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

sn_status sn_board(sn_env* e, int8_t* out, void* stream) {
    if (!e || !out) return fail(SN_EINVAL, "NULL argument");
    hipLaunchKernelGGL(k_board, dim3(grid_for(e->s.B)), dim3(kBlock), 0, (hipStream_t)stream, e->s, out);
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

sn_status sn_scores(sn_env* e, int32_t* out, void* stream) {
    if (!e || !out) return fail(SN_EINVAL, "NULL argument");
    hipLaunchKernelGGL(k_scores, dim3(grid_for(e->s.B)), dim3(kBlock), 0, (hipStream_t)stream, e->s, out,
                       (int32_t*)nullptr, (int32_t*)nullptr);
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

sn_status sn_results(sn_env* e, int32_t* sum_results, int32_t* episodes, void* stream) {
    if (!e) return fail(SN_EINVAL, "NULL argument");
    hipLaunchKernelGGL(k_scores, dim3(grid_for(e->s.B)), dim3(kBlock), 0, (hipStream_t)stream, e->s,
                       (int32_t*)nullptr, sum_results, episodes);
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

sn_status sn_clear_results(sn_env* e, void* stream) {
    if (!e) return fail(SN_EINVAL, "NULL argument");
    hipLaunchKernelGGL(k_clear_results, dim3(grid_for(e->s.B)), dim3(kBlock), 0, (hipStream_t)stream, e->s);
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

// ---------------------------------------------------------------- MT import and export
// lazy -> numpy form: finish the current round for words [p, 624)
static void mt_finish_round(uint32_t* a, int p) {
    for (int i = p; i < kMtN; i++) {
        uint32_t y = (a[i] & 0x80000000u) | (a[(i + 1) % kMtN] & 0x7fffffffu);
        a[i] = a[(i + kMtM) % kMtN] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
    }
}

// Undo the twist of the new round's words [0, T): new[j] = src ^ (y >> 1) ^
// (y & 1 ? A : 0) with y = (old[j] & UPPER) | (old[j+1] & LOWER) and src =
// new[j-227] (j >= 227) or old[j+397] (j < 227: still in place, or itself
// restored from the j >= 227 words when T > 397).  A's top bit is set and
// y >> 1's is not, so the top bit of new[j] ^ src is y & 1 and y follows.
// old[0]'s low 31 bits never enter the twist; they come from mt0.
static uint32_t mt_untwist_y(uint32_t t) {
    const uint32_t lsb = t >> 31;
    if (lsb) t ^= 0x9908b0dfu;
    return (t << 1) | lsb;
}

static void mt_unstraddle(uint32_t* a, int T, uint32_t old0) {
    constexpr int D = kMtN - kMtM;  // 227
    uint32_t y[kMtN];
    for (int j = D; j < T; j++) y[j] = mt_untwist_y(a[j] ^ a[j - D]);
    auto old_at = [&](int m) -> uint32_t {  // m >= 397
        return (m < T) ? ((y[m] & 0x80000000u) | (y[m - 1] & 0x7fffffffu)) : a[m];
    };
    for (int j = 0; j < T && j < D; j++) y[j] = mt_untwist_y(a[j] ^ old_at(j + kMtM));
    for (int j = 0; j < T; j++) a[j] = (y[j] & 0x80000000u) | ((j == 0 ? old0 : y[j - 1]) & 0x7fffffffu);
}

// The lazy form (sechs_device.h MtGenT: the array `key` with state code `code`, words [pos - cnt, pos) twisted and
// unconsumed) to numpy's (key, pos), in place; old0: the newest word-0 crossing's old mt[0] (mt0).  Returns pos.
static int32_t mt_to_numpy(uint32_t* key, uint32_t code, uint32_t old0) {
    const int p = (int)(code & 0x7FFu);
    // still in the previous round, whose head [0, p) was overwritten
    if (mt_code_straddles(code)) mt_unstraddle(key, p, old0);
    else if (p > 0 && p < kMtN) mt_finish_round(key, p);  // twist the rest of this round in place
    return (int32_t)mt_numpy_pos(code);
}

sn_status sn_mt_get(sn_env* e, int64_t game, uint32_t* key, int32_t* pos) {
    if (!e || !key || !pos) return fail(SN_EINVAL, "NULL argument");
    if (e->s.rng_mode != SN_RNG_NUMPY_MT) return fail(SN_EINVAL, "env is not in numpy-compat RNG mode");
    if (game < 0 || game >= e->s.B) return fail(SN_EINVAL, "game out of range");
    HIP_TRY(hipSetDevice(e->device));
    if (sn_pipe_sync(e, 0) != SN_OK) return SN_EHIP;
    HIP_TRY(hipDeviceSynchronize());
    uint32_t code = 0, old0 = 0;
    HIP_TRY(hipMemcpy(key, e->s.mt + game * kMtN, sizeof(uint32_t) * kMtN, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&code, e->s.mt_pos + game, sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&old0, e->s.mt0 + game * kMt0Levels, sizeof(uint32_t), hipMemcpyDeviceToHost));
    *pos = mt_to_numpy(key, code, old0);
    return SN_OK;
}

sn_status sn_mt_set(sn_env* e, int64_t game, const uint32_t* key, int32_t pos) {
    if (!e || !key) return fail(SN_EINVAL, "NULL argument");
    if (e->s.rng_mode != SN_RNG_NUMPY_MT) return fail(SN_EINVAL, "env is not in numpy-compat RNG mode");
    if (game < 0 || game >= e->s.B) return fail(SN_EINVAL, "game out of range");
    if (pos < 0 || pos > kMtN) return fail(SN_EINVAL, "pos must be in 0..624");
    HIP_TRY(hipSetDevice(e->device));
    if (sn_pipe_sync(e, 0) != SN_OK) return SN_EHIP;
    HIP_TRY(hipDeviceSynchronize());
    const uint32_t code = mt_code_from_numpy(pos);
    HIP_TRY(hipMemcpy(e->s.mt + game * kMtN, key, sizeof(uint32_t) * kMtN, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->s.mt_pos + game, &code, sizeof(uint32_t), hipMemcpyHostToDevice));
    return SN_OK;
}

// ---------------------------------------------------------------- the one-game path
static sn_status h1_ready(sn_env* e) {
    if (e->s.B != 1) return fail(SN_EINVAL, "the one-game fast path needs a one-game handle");
    if (!e->hbuf) {
        if (hipHostMalloc((void**)&e->hbuf, sizeof(uint32_t) * kH1Words, hipHostMallocMapped) != hipSuccess ||
            hipHostGetDevicePointer((void**)&e->hbuf_dev, e->hbuf, 0) != hipSuccess)
            return fail(SN_ENOMEM, "pinned exchange buffer");
    }
    return SN_OK;
}

// out_host: the 2 + 14 N result words, then N trace words (sn_step1; zeros for a reset)
static void h1_copy_out(const sn_env* e, int32_t* out, bool trace) {
    const int N = e->s.N;
    std::memcpy(out, e->hbuf + kH1Out, sizeof(uint32_t) * (2 + 2 * N + 12 * N));
    if (trace) std::memcpy(out + 2 + 14 * N, e->hbuf + kH1Out + kH1Trace, sizeof(uint32_t) * N);
    else std::memset(out + 2 + 14 * N, 0, sizeof(uint32_t) * N);
}

sn_status sn_step1(sn_env* e, const int32_t* actions_host, int32_t* out_host, int flags) {
    if (!e || !actions_host || !out_host) return fail(SN_EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(e->device));
    if (h1_ready(e) != SN_OK) return SN_ENOMEM;
    if (e->s.lg_K) return fail(SN_EUNSUPPORTED, "a tournament handle plays whole games with sn_league_rollout");
    e->phase = -1;
    Acts1 a{};
    for (int p = 0; p < e->s.N; p++) a.a[p] = actions_host[p];
    const int summ = !(flags & SN_NO_SUMMARIES);
    SN_DISPATCH_N(e->s.N, hipLaunchKernelGGL((k_step1<NN>), dim3(1), dim3(64), 0, 0, e->s, a, e->hbuf_dev, summ));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    h1_copy_out(e, out_host, true);
    return SN_OK;
}

sn_status sn_reset1(sn_env* e, const uint32_t* key_host, int32_t pos, uint32_t* key_out_host, int32_t* pos_out,
                    int32_t* out_host, int flags) {
    if (!e || !key_host || !key_out_host || !pos_out || !out_host) return fail(SN_EINVAL, "NULL argument");
    if (e->s.rng_mode != SN_RNG_NUMPY_MT) return fail(SN_EINVAL, "env is not in numpy-compat RNG mode");
    if (pos < 0 || pos > kMtN) return fail(SN_EINVAL, "pos must be in 0..624");
    HIP_TRY(hipSetDevice(e->device));
    if (h1_ready(e) != SN_OK) return SN_ENOMEM;
    if (e->s.lg_K) return fail(SN_EUNSUPPORTED, "a tournament handle deals with sn_reset");
    if (sn_pipe_sync(e, 0) != SN_OK) return SN_EHIP;
    std::memcpy(e->hbuf + kH1In, key_host, sizeof(uint32_t) * kMtN);
    e->hbuf[kH1In + kMtN] = (uint32_t)pos;
    const int summ = !(flags & SN_NO_SUMMARIES);
    SN_DISPATCH_N(e->s.N, hipLaunchKernelGGL((k_reset1<NN>), dim3(1), dim3(64), 0, 0, e->s, e->hbuf_dev, summ));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    e->phase = 0;  // one game, just dealt
    h1_copy_out(e, out_host, false);
    // the advanced state in numpy's (key, pos) form, as sn_mt_get
    std::memcpy(key_out_host, e->hbuf + kH1Mt, sizeof(uint32_t) * kMtN);
    *pos_out = mt_to_numpy(key_out_host, e->hbuf[kH1Mt + kMtN], e->hbuf[kH1Mt + kMtN + 1]);
    return SN_OK;
}

// ---------------------------------------------------------------- timing and debug
sn_status sn_kernel_times(sn_env* e, float* play_ms, float* ahead_ms, int32_t* n) {
    return sn_kernel_times_dec(e, play_ms, ahead_ms, nullptr, n);
}

sn_status sn_kernel_times_dec(sn_env* e, float* play_ms, float* ahead_ms, float* decode_ms, int32_t* n) {
    if (!e || !play_ms || !ahead_ms || !n) return fail(SN_EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    double sp = 0.0, sa = 0.0, sd = 0.0;
    int na = 0, nd = 0;
    for (int i = 0; i < e->tn; i++) {
        const hipEvent_t* tv = e->tev + kTimingEvents * i;
        float a = 0.f, b = 0.f, c = 0.f;
        HIP_TRY(hipEventElapsedTime(&a, tv[0], tv[1]));
        sp += a;
        if (e->tev_tw[i] & 1) {  // a twist ran beside this launch (the first of its group)
            HIP_TRY(hipEventElapsedTime(&b, tv[2], tv[3]));
            sa += b, na++;
        }
        if (e->tev_tw[i] & 2) {  // and a decode-ahead launch after it
            HIP_TRY(hipEventElapsedTime(&c, tv[4], tv[5]));
            sd += c, nd++;
        }
    }
    *n = e->tn;
    *play_ms = e->tn ? (float)(sp / e->tn) : 0.f;
    *ahead_ms = na ? (float)(sa / na) : 0.f;
    if (decode_ms) *decode_ms = nd ? (float)(sd / nd) : 0.f;
    return SN_OK;
}

sn_status sn_debug_phases(uint64_t* out, int n) {
    if (!out || n < 1) return fail(SN_EINVAL, "NULL argument");
#ifdef SECHS_PHASE_PROF
    unsigned long long h[PH_N + 2];
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_phase), sizeof(h)));
    for (int k = 0; k < n; k++) out[k] = (k <= PH_N + 1) ? (uint64_t)h[k] : 0ull;
    const unsigned long long z[PH_N + 2] = {};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_phase), z, sizeof(z)));
    return SN_OK;
#else
    for (int k = 0; k < n; k++) out[k] = 0ull;
    return fail(SN_EUNSUPPORTED, "built without SECHS_PHASE_PROF (make libsechs_prof.so)");
#endif
}

#if defined(SECHS_DEBUG)
__global__ void k_debug_selftest(int fail) { SN_DASSERT(fail == 0); }
#endif

sn_status sn_debug_failures(uint32_t* count, uint32_t* first_line, int selftest) {
    if (!count || !first_line) return fail(SN_EINVAL, "NULL argument");
    *count = 0u, *first_line = 0u;
#if defined(SECHS_DEBUG)
    if (selftest) {  // one deliberately violated assertion: proves the counter is live
        hipLaunchKernelGGL(k_debug_selftest, dim3(1), dim3(1), 0, 0, 1);
        HIP_TRY(hipGetLastError());
    }
    unsigned int h[2];
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_sn_dbg), sizeof(h)));
    *count = h[0], *first_line = h[1];
    const unsigned int z[2] = {0u, 0xFFFFFFFFu};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_sn_dbg), z, sizeof(z)));
    return SN_OK;
#else
    (void)selftest;
    return fail(SN_EUNSUPPORTED, "built without SECHS_DEBUG (make libsechs_debug.so)");
#endif
}

sn_status sn_pipe_errors(sn_env* e, uint32_t* count) {
    if (!e || !count) return fail(SN_EINVAL, "NULL argument");
    *count = 0;
    if (!e->s.perr) return SN_OK;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(count, e->s.perr, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (e->perr_host && *count) __atomic_store_n(e->perr_host, *count, __ATOMIC_RELAXED);
    return SN_OK;
}

sn_status sn_debug_pipe_words(sn_env* e, int what, int slot, uint32_t* out) {
    if (!e || !out) return fail(SN_EINVAL, "NULL argument");
    if (!e->s.pabsc) return fail(SN_EUNSUPPORTED, "no pipeline (numpy-compat handles only)");
    const int64_t B = e->s.B;
    const void* src = nullptr;
    size_t bytes = 0;
    if (what == 0 && slot >= 0 && slot < kPipeSlots + 2) src = e->s.pabsc + (int64_t)slot * B, bytes = 4 * B;
    else if (what == 1 && slot >= 0 && slot < 2) src = e->s.ptend + (int64_t)slot * B, bytes = 4 * B;
    else if (what == 2 && slot >= 0 && slot < kDecRecords && e->s.drec)
        src = e->s.drec + (int64_t)slot * kDecQuads * B, bytes = sizeof(u32x4) * kDecQuads * B;
    else if (what == 3 && slot == 0 && e->s.mt_pos)  // as they stand: no pipeline sync
        src = e->s.mt_pos, bytes = 4 * B;
    else return fail(SN_EINVAL, "what / slot out of range");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
    return SN_OK;
}

sn_status sn_philox_counter(sn_env* e, int64_t game, uint64_t* ctr) {
    if (!e || !ctr) return fail(SN_EINVAL, "NULL argument");
    if (game < 0 || game >= e->s.B) return fail(SN_EINVAL, "game out of range");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(ctr, e->s.ctr + game, sizeof(uint64_t), hipMemcpyDeviceToHost));
    return SN_OK;
}

}  // extern "C"
