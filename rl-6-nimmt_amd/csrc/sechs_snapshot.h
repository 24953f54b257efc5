// sechs_snapshot.h -- the snapshot format of a handle (sn_state_save / sn_state_load, sechs_snapshot.hip).
// This header is the format's one owner; rl_6_nimmt/snapshot.py is its host model (tests/test_snapshot_cpu.py
// holds the two together through sn_state_bytes).
//
// A snapshot is one contiguous blob: a SnapHeader (kSnapHeaderBytes, a multiple of 64 B), then one record per
// game, game-major: game g at header + g * record_bytes.  A record is dwords, in this order (SnapLayout):
//   hand     3 N   seat p's sorted hand words lo.lo32, lo.hi32, hi (DevState::hand)
//   row_lo   4     cards 0..3 of each row
//   row_hi   4     card4 | len << 8 | heads << 16 | end << 24
//   score    N     penalties this episode
//   sum_res  N     sum of the finished episodes' results
//   episodes 1
//   lgs      1     tournament handles only: the seat word of the slot's current game
//   lmem     4 N   tournament handles only: the MCS card memory, four words per seat (zero without MCS agents)
//   the RNG in canonical form:
//     numpy-MT  pos (0..624) in the dword right before key, key[624] 16-byte aligned in the record: exactly
//               np.random.get_state()[1:3] at the play consumer's position
//     Philox    the 64-bit word counter, 8-byte aligned
//   zero padding to a multiple of 16 B.
// Records depend on (N, rng_mode, tournament or not) only: not on the SN_OPT_* settings, the pipeline's phase
// or the SoA strides, so a range of records is the state of a shard and a numpy state can be handed to numpy.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sechs.h"

namespace sechs {

constexpr uint32_t kSnapMagic = 0x50534E53u;  // "SNSP"
constexpr uint32_t kSnapVersion = 1u;
constexpr int kSnapAgents = 16;  // kLeagueMaxAgents

struct SnapHeader {
    uint32_t magic, version, header_bytes, record_bytes;
    int64_t B;  // records in the blob
    int32_t N, C, rng_mode, league;  // league: 1 = the records carry lgs and lmem
    uint64_t seed, game_offset;      // game_offset: the global id of record 0
    int32_t lg_K, lg_lo, lg_hi;
    int32_t phase, lg_phase;  // sn_env::phase, sn_env::lg_phase: read by the next rollout / league call
    uint32_t overruns;  // DevState::perr behind the save's pipeline sync, written by k_snapshot_save: a blob of a
                        // handle that had overrun its twisted words (its streams are lost) is refused at a load
    int32_t lg_kind[kSnapAgents], lg_mpc[kSnapAgents], lg_mmax[kSnapAgents];  // agents < lg_K; 0 past them
    uint32_t pad1[12];
};
constexpr int kSnapHeaderBytes = 320;
static_assert(sizeof(SnapHeader) == kSnapHeaderBytes && kSnapHeaderBytes % 64 == 0, "the header is a fixed 320 bytes");
static_assert(offsetof(SnapHeader, overruns) % 4 == 0, "k_snapshot_save writes the overrun count as one dword");

// dword offsets inside a record
struct SnapLayout {
    int hand, row_lo, row_hi, score, sum_res, episodes, lgs, lmem;  // lgs, lmem: -1 on plain handles
    int small;                                                        // dwords before the RNG part
    int pos, key, ctr;                                                // numpy-MT: pos, key; Philox: ctr; else -1
    int dwords;                                                       // record size, a multiple of 4
};

__host__ __device__ inline SnapLayout snap_layout(int N, int rng_mode, int league) {
    SnapLayout L;
    int o = 0;
    L.hand = o, o += 3 * N;
    L.row_lo = o, o += 4;
    L.row_hi = o, o += 4;
    L.score = o, o += N;
    L.sum_res = o, o += N;
    L.episodes = o, o += 1;
    L.lgs = L.lmem = -1;
    if (league) {
        L.lgs = o, o += 1;
        L.lmem = o, o += 4 * N;
    }
    L.small = o;
    L.pos = L.key = L.ctr = -1;
    if (rng_mode == SN_RNG_NUMPY_MT) {
        L.key = (o + 1 + 3) & ~3;  // room for pos, then 16-byte aligned
        L.pos = L.key - 1;
        o = L.key + 624;
    } else {
        L.ctr = (o + 1) & ~1;
        o = L.ctr + 2;
    }
    L.dwords = (o + 3) & ~3;
    return L;
}

}  // namespace sechs
