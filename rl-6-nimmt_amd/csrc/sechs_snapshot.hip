// sechs_snapshot.hip -- whole-handle device snapshots (sn_state_bytes / sn_state_save / sn_state_load).
//
// The format is sechs_snapshot.h's.  k_snapshot_save gathers one game per wave into its record: the small SoA
// fields word by word, and the numpy-MT state brought to np.random.get_state() form in LDS -- the device
// counterpart of sn_mt_get's host conversion (mt_to_numpy, sechs_env.hip) -- so the live handle is only read.
// k_snapshot_load is the inverse scatter; it leaves the plain state (mt, mt_pos, a zero mt0) from which the next
// rollout starts its pipeline.  Nothing a restarted pipeline or the next launch rebuilds is saved.
#include "sechs_state.h"
#include "sechs_snapshot.h"

#include <cstring>

using namespace sechs;

namespace {

constexpr int kSnapWaves = kBlock / 64;  // games per block: one wave each

__device__ __forceinline__ uint32_t snap_untwist_y(uint32_t t) {
    const uint32_t lsb = t >> 31;  // the twist constant's top bit is set, y >> 1's is not
    return ((lsb ? (t ^ 0x9908b0dfu) : t) << 1) | lsb;
}

// the small fields of game g as record dword i (i < L.small)
__device__ __forceinline__ uint32_t snap_small_get(const DevState& s, const SnapLayout& L, int64_t g, int i) {
    const int64_t B = s.B;
    const int N = s.N;
    if (i < L.row_lo) return s.hand[(int64_t)i * B + g];  // record order p * 3 + k is the SoA plane index
    if (i < L.row_hi) return s.row_lo[(int64_t)(i - L.row_lo) * B + g];
    if (i < L.score) return s.row_hi[(int64_t)(i - L.row_hi) * B + g];
    if (i < L.sum_res) return (uint32_t)s.score[(int64_t)(i - L.score) * B + g];
    if (i < L.episodes) return (uint32_t)s.sum_res[(int64_t)(i - L.sum_res) * B + g];
    if (i == L.episodes) return (uint32_t)s.episodes[g];
    if (i == L.lgs) return s.lgs ? s.lgs[g] : 0u;
    const int k = i - L.lmem, p = k >> 2, w = k & 3;  // four words per seat; lmem is [4][B * N], word-major
    return s.lmem ? s.lmem[(int64_t)w * B * N + g * N + p] : 0u;
}

__device__ __forceinline__ void snap_small_put(const DevState& s, const SnapLayout& L, int64_t g, int i, uint32_t v) {
    const int64_t B = s.B;
    const int N = s.N;
    if (i < L.row_lo) s.hand[(int64_t)i * B + g] = v;
    else if (i < L.row_hi) s.row_lo[(int64_t)(i - L.row_lo) * B + g] = v;
    else if (i < L.score) s.row_hi[(int64_t)(i - L.row_hi) * B + g] = v;
    else if (i < L.sum_res) s.score[(int64_t)(i - L.score) * B + g] = (int32_t)v;
    else if (i < L.episodes) s.sum_res[(int64_t)(i - L.sum_res) * B + g] = (int32_t)v;
    else if (i == L.episodes) s.episodes[g] = (int32_t)v;
    else if (i == L.lgs) {
        if (s.lgs) s.lgs[g] = v;
    } else if (s.lmem) {
        const int k = i - L.lmem, p = k >> 2, w = k & 3;
        s.lmem[(int64_t)w * B * N + g * N + p] = v;
    }
}

// One wave per game, the grid sized from B as k_pipe_code's.  MT: the 624 state words go through LDS, where the
// lazy form (state code in mt_pos: sechs_device.h, at MtGenT) becomes numpy's:
//   straddled (cnt > pos > 0)  the array's head [0, pos) is a round ahead of the consumer: untwisted with the
//                              newest mt0 level, as k_pipe_code undoes a round (cnt == pos < 624 too: the
//                              consumer has drawn its round's last word, numpy shows that round at 624);
//   mid-round (0 < pos < 624)  words [pos, 624) twisted in place, in chunks of 224 <= 227 words: word i reads
//                              old i + 1 and old i + 397 (i < 227; neither written before this chunk ends) or
//                              new i - 227 (written by an earlier chunk, or before pos), so a chunk's reads
//                              all precede its writes;
//   complete (pos 0 or 624)    copied.
template <bool MT>
__global__ __launch_bounds__(kBlock) void k_snapshot_save(DevState s, SnapHeader hdr, uint32_t* blob) {
    __shared__ __attribute__((aligned(16))) uint32_t sw[MT ? kSnapWaves : 1][MT ? kMtN : 4];
    __shared__ uint32_t sy[MT ? kSnapWaves : 1][MT ? kMtN : 4];
    const int64_t g = (int64_t)blockIdx.x * kSnapWaves + (threadIdx.x >> 6);
    if (g >= s.B) return;  // whole waves
    const uint32_t lane = threadIdx.x & 63u;
    const SnapLayout L = snap_layout(s.N, s.rng_mode, hdr.league);
    if (g == 0) {  // the header travels as a kernel argument: no host copy, no synchronisation
        const uint32_t* h = (const uint32_t*)&hdr;
        // ... but for the overrun count: what perr holds now, behind k_pipe_code on this stream (which counts too)
        const uint32_t over = s.perr ? *s.perr : 0u;
        for (uint32_t i = lane; i < (uint32_t)(kSnapHeaderBytes / 4); i += 64u)
            blob[i] = (i == (uint32_t)(offsetof(SnapHeader, overruns) / 4)) ? over : h[i];
    }
    uint32_t* rec = blob + kSnapHeaderBytes / 4 + g * (int64_t)L.dwords;
    for (int i = (int)lane; i < L.small; i += 64) rec[i] = snap_small_get(s, L, g, i);
    if constexpr (MT) {
        constexpr uint32_t D = kMtN - kMtM;  // 227
        constexpr uint32_t NV = kMtN / 4;    // 156 16-byte pieces
        uint32_t* w = sw[threadIdx.x >> 6];
        uint32_t* y = sy[threadIdx.x >> 6];
        const u32x4* src = (const u32x4*)(s.mt + g * kMtN);  // 2 496 bytes per game: 16-byte aligned
        for (uint32_t q = lane; q < NV; q += 64u) *(u32x4*)(w + 4u * q) = src[q];
        const uint32_t code = s.mt_pos[g];
        const uint32_t p = code & 0x7FFu;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        if (mt_code_straddles(code)) {
            const uint32_t tp = min(p, (uint32_t)kMtN);
            for (uint32_t j = D + lane; j < tp; j += 64u) y[j] = snap_untwist_y(w[j] ^ w[j - D]);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            for (uint32_t j = lane; j < min(D, tp); j += 64u) {
                const uint32_t k = j + kMtM;  // 397 .. 623
                const uint32_t old_k = (k < tp) ? ((y[k] & 0x80000000u) | (y[k - 1u] & 0x7fffffffu)) : w[k];
                y[j] = snap_untwist_y(w[j] ^ old_k);
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            const uint32_t m0 = s.mt0[g * kMt0Levels];
            for (uint32_t j = lane; j < tp; j += 64u) w[j] = (y[j] & 0x80000000u) | ((j ? y[j - 1u] : m0) & 0x7fffffffu);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        } else if (p > 0u && p < (uint32_t)kMtN) {
            for (uint32_t s0 = p; s0 < (uint32_t)kMtN; s0 += 224u) {
                const uint32_t e = min(s0 + 224u, (uint32_t)kMtN);
                uint32_t v[4];
#pragma unroll
                for (uint32_t b = 0; b < 4u; b++) {
                    const uint32_t i = s0 + 64u * b + lane;
                    v[b] = 0u;
                    if (i < e) v[b] = mt_mix(w[i], w[(i + 1u == (uint32_t)kMtN) ? 0u : i + 1u], w[(i < D) ? i + kMtM : i - D]);
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
                for (uint32_t b = 0; b < 4u; b++) {
                    const uint32_t i = s0 + 64u * b + lane;
                    if (i < e) w[i] = v[b];
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            }
        }
        for (int i = L.small + (int)lane; i < L.pos; i += 64) rec[i] = 0u;  // the padding in front of pos
        if (lane == 0u) rec[L.pos] = (uint32_t)mt_numpy_pos(code);
        u32x4* dst = (u32x4*)(rec + L.key);
        for (uint32_t q = lane; q < NV; q += 64u) dst[q] = *(const u32x4*)(w + 4u * q);
        for (int i = L.key + kMtN + (int)lane; i < L.dwords; i += 64) rec[i] = 0u;
    } else {
        for (int i = L.small + (int)lane; i < L.ctr; i += 64) rec[i] = 0u;
        if (lane == 0u) {
            const uint64_t c = s.ctr[g];
            rec[L.ctr] = (uint32_t)c, rec[L.ctr + 1] = (uint32_t)(c >> 32);
        }
        for (int i = L.ctr + 2 + (int)lane; i < L.dwords; i += 64) rec[i] = 0u;
    }
}

// the inverse: game g of the handle takes record first + g
template <bool MT>
__global__ __launch_bounds__(kBlock) void k_snapshot_load(DevState s, int league, const uint32_t* blob, int64_t first) {
    const int64_t g = (int64_t)blockIdx.x * kSnapWaves + (threadIdx.x >> 6);
    if (g >= s.B) return;  // whole waves
    const uint32_t lane = threadIdx.x & 63u;
    const SnapLayout L = snap_layout(s.N, s.rng_mode, league);
    const uint32_t* rec = blob + kSnapHeaderBytes / 4 + (first + g) * (int64_t)L.dwords;
    for (int i = (int)lane; i < L.small; i += 64) snap_small_put(s, L, g, i, rec[i]);
    if constexpr (MT) {
        constexpr uint32_t NV = kMtN / 4;
        const u32x4* src = (const u32x4*)(rec + L.key);
        u32x4* dst = (u32x4*)(s.mt + g * kMtN);
        for (uint32_t q = lane; q < NV; q += 64u) dst[q] = src[q];
        if (lane == 0u) s.mt_pos[g] = mt_code_from_numpy((int)min(rec[L.pos], (uint32_t)kMtN));
        if (lane < (uint32_t)kMt0Levels) s.mt0[g * kMt0Levels + lane] = 0u;  // a numpy-form state straddles nothing
        if (g == 0 && lane == 0u) *s.perr = 0u;
    } else {
        if (lane == 0u) s.ctr[g] = (uint64_t)rec[L.ctr] | ((uint64_t)rec[L.ctr + 1] << 32);
    }
}

sn_status snap_fail(const std::string& msg) { return set_error(SN_EINVAL, msg); }

SnapHeader header_of(const sn_env* e) {
    const DevState& s = e->s;
    const SnapLayout L = snap_layout(s.N, s.rng_mode, s.lg_K > 0);
    SnapHeader h;
    std::memset(&h, 0, sizeof(h));
    h.magic = kSnapMagic, h.version = kSnapVersion, h.header_bytes = kSnapHeaderBytes, h.record_bytes = 4u * (uint32_t)L.dwords;
    h.B = s.B, h.N = s.N, h.C = s.C, h.rng_mode = s.rng_mode, h.league = s.lg_K > 0;
    h.seed = s.seed, h.game_offset = s.game_offset;
    h.lg_K = s.lg_K, h.lg_lo = s.lg_lo, h.lg_hi = s.lg_hi;
    h.phase = e->phase, h.lg_phase = s.lg_K > 0 ? e->lg_phase : 0;
    for (int i = 0; i < s.lg_K && i < kSnapAgents; i++)
        h.lg_kind[i] = e->lg_kind[i], h.lg_mpc[i] = e->lg_mpc[i], h.lg_mmax[i] = e->lg_mmax[i];
    return h;
}

}  // namespace

extern "C" {

int64_t sn_state_bytes(int64_t num_games, int num_players, int rng_mode, int league, int64_t* header_bytes,
                       int64_t* record_bytes) {
    if (num_games < 0 || num_players < 1 || num_players > kMaxPlayers ||
        (rng_mode != SN_RNG_PHILOX && rng_mode != SN_RNG_NUMPY_MT)) {
        set_error(SN_EINVAL, "sn_state_bytes: num_games >= 0, num_players 1..10, a known rng_mode");
        return -1;
    }
    const SnapLayout L = snap_layout(num_players, rng_mode, league != 0);
    if (header_bytes) *header_bytes = kSnapHeaderBytes;
    if (record_bytes) *record_bytes = 4 * (int64_t)L.dwords;
    return kSnapHeaderBytes + num_games * 4 * (int64_t)L.dwords;
}

int64_t sn_state_size(const sn_env* e) {
    if (!e) {
        set_error(SN_EINVAL, "env is NULL");
        return -1;
    }
    return sn_state_bytes(e->s.B, e->s.N, e->s.rng_mode, e->s.lg_K > 0, nullptr, nullptr);
}

sn_status sn_state_save(sn_env* e, void* blob, int64_t blob_bytes, void* stream) {
    if (!e || !blob) return snap_fail("NULL argument");
    if ((uintptr_t)blob & 15u) return snap_fail("the snapshot blob must be 16-byte aligned");
    if (blob_bytes < sn_state_size(e)) return snap_fail("the snapshot blob is smaller than sn_state_bytes");
    if (e->perr_host && __atomic_load_n(e->perr_host, __ATOMIC_RELAXED))
        return set_error(SN_ERNG, "a pipelined numpy-MT draw ran past the twisted words: this handle's streams are lost "
                                  "and are not saved (sn_pipe_errors)");
    const DevState& s = e->s;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(e->device));
    if (const sn_status r = sn_pipe_sync(e, st); r != SN_OK) return r;  // the pipelines back into (mt, mt_pos, mt0)
    const SnapHeader h = header_of(e);
    const dim3 grid((unsigned)((s.B + kSnapWaves - 1) / kSnapWaves));
    if (s.rng_mode == SN_RNG_NUMPY_MT) hipLaunchKernelGGL((k_snapshot_save<true>), grid, dim3(kBlock), 0, st, s, h, (uint32_t*)blob);
    else hipLaunchKernelGGL((k_snapshot_save<false>), grid, dim3(kBlock), 0, st, s, h, (uint32_t*)blob);
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

sn_status sn_state_load(sn_env* e, const void* blob, int64_t blob_bytes, int64_t first, void* stream) {
    if (!e || !blob) return snap_fail("NULL argument");
    if ((uintptr_t)blob & 15u) return snap_fail("the snapshot blob must be 16-byte aligned");
    if (blob_bytes < kSnapHeaderBytes) return snap_fail("the snapshot blob is shorter than its header");
    DevState& s = e->s;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(e->device));
    SnapHeader h;
    HIP_TRY(hipMemcpyAsync(&h, blob, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const SnapLayout L = snap_layout(s.N, s.rng_mode, s.lg_K > 0);
    if (h.magic != kSnapMagic) return snap_fail("not a snapshot (magic)");
    if (h.version != kSnapVersion) return snap_fail("snapshot format version " + std::to_string(h.version) + ", this library reads " + std::to_string(kSnapVersion));
    if (h.overruns) return snap_fail("the snapshot is of a handle that had run past its twisted words (" + std::to_string(h.overruns) + " overruns): its streams were lost before the save");
    if (h.N != s.N || h.C != s.C) return snap_fail("the snapshot's num_players / num_cards differ from the handle's");
    if (h.rng_mode != s.rng_mode) return snap_fail("the snapshot's rng_mode differs from the handle's");
    if (h.seed != s.seed) return snap_fail("the snapshot's seed differs from the handle's");
    if (h.lg_K != s.lg_K || h.lg_lo != s.lg_lo || h.lg_hi != s.lg_hi || h.league != (s.lg_K > 0))
        return snap_fail("the snapshot's league configuration differs from the handle's (sn_league_config)");
    for (int i = 0; i < s.lg_K && i < kSnapAgents; i++)
        if (h.lg_kind[i] != e->lg_kind[i] || h.lg_mpc[i] != e->lg_mpc[i] || h.lg_mmax[i] != e->lg_mmax[i])
            return snap_fail("the snapshot's league agents differ from the handle's (sn_league_agents)");
    if (h.header_bytes != (uint32_t)kSnapHeaderBytes || h.record_bytes != 4u * (uint32_t)L.dwords)
        return snap_fail("the snapshot's header / record size is not this format's");
    if (first < 0 || h.B < 0 || first > h.B || s.B > h.B - first) return snap_fail("first + num_games runs past the snapshot's records");
    if (h.game_offset + (uint64_t)first != s.game_offset)
        return snap_fail("record `first` has another global game id than the handle's game 0 (every stream is keyed by it)");
    // by division: no product of header fields can overflow
    if ((blob_bytes - kSnapHeaderBytes) / (int64_t)h.record_bytes < h.B) return snap_fail("the snapshot blob is shorter than its header says");
    if (const sn_status r = sn_pipe_sync(e, st); r != SN_OK) return r;
    const dim3 grid((unsigned)((s.B + kSnapWaves - 1) / kSnapWaves));
    if (s.rng_mode == SN_RNG_NUMPY_MT) hipLaunchKernelGGL((k_snapshot_load<true>), grid, dim3(kBlock), 0, st, s, (int)(s.lg_K > 0), (const uint32_t*)blob, first);
    else hipLaunchKernelGGL((k_snapshot_load<false>), grid, dim3(kBlock), 0, st, s, (int)(s.lg_K > 0), (const uint32_t*)blob, first);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));  // [sync]: the pipeline's side streams are behind st too (sn_pipe_sync)
    if (e->perr_host) __atomic_store_n(e->perr_host, 0u, __ATOMIC_RELAXED);
    e->phase = h.phase;
    if (s.lg_K) e->lg_phase = h.lg_phase;
    return SN_OK;
}

}  // extern "C"
