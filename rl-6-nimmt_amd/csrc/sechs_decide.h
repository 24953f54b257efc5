// sechs_decide.h -- what every kernel over a batch of decisions shares: the
// launch arguments built from an sn_puct (PuctArgs, puct_args), the
// decision -> (game, seat) addressing, the candidate-row normalisation, and
// the Philox stream word of a decision with the table of its reserved tags.
// Included by the PUCT search (sechs_puct.hip) and by the entry points an
// engine without a search calls (sechs_agents.hip).  PuctArgs stays in the
// global namespace: it is part of every kernel's mangled name.
#pragma once
#include <hip/hip_bf16.h>

#include "sechs_state.h"

using namespace sechs;

constexpr int kRowLen = 48;      // 1 (action) + 47 (observation)

struct PuctArgs {
    int64_t D;                // decisions = B * popcount(seats_mask), or num_dec of a decision list
    uint32_t seats_mask, M;   // deciding seats, M = popcount
    const int32_t* dec;       // decision list (g * N + p per decision) or NULL (seats_mask)
    const uint32_t* lgs;      // tournament handle: per game k | agents..., the rollouts seat k players; NULL: N
    int N;                    // the handle's seats
    int n;                    // root hand size (all decisions in lockstep)
    int flags;                // 1: PUCT at the root (PUCTAgent), 0: sample it (PolicyMCSAgent)
    double c_puct;
    uint32_t seed_lo, seed_hi, step, rollout;
    const uint32_t* avail;    // [4][B*N] card memory (sn_mcs_memorize)
    int32_t* ro;              // [D][48] rollout games
    int32_t* stats;           // [D][24]
    int32_t* hist;            // [D][172]
    float* root_probs;        // [D][10]
    const uint32_t* step_dev; // decision counter in device memory (graph replays), else `step`
};

// the decision counter mixed into every Philox key of a decision: from
// device memory when the launches were captured into a graph (one capture
// replayed for every decision), else the launch argument
__device__ __forceinline__ uint32_t puct_step_of(const PuctArgs& a) { return a.step_dev ? *a.step_dev : a.step; }

__device__ __forceinline__ void dec_to_gp(const PuctArgs& a, int64_t d, int64_t& g, int& p) {
    if (a.dec) {  // a tournament agent's seats (sn_puct.dec_list)
        const int32_t gp = a.dec[d];
        g = gp / a.N;
        p = gp - (int)g * a.N;
        return;
    }
    g = d / a.M;
    uint32_t k = (uint32_t)(d - g * a.M), m = a.seats_mask;
    for (uint32_t i = 0; i < k; i++) m &= m - 1u;  // drop the k lowest deciding seats
    p = __builtin_ctz(m);
}

// players of game g: the agent's num_players = state[10] (mcts.py:62-64); a
// tournament game seats k <= N of the handle's N seats
__device__ __forceinline__ int players_of(const PuctArgs& a, int64_t g) { return a.lgs ? (int)(a.lgs[g] & 15u) : a.N; }

// ---------------------------------------------------------------- Philox streams
// Every random word of a decision is Philox keyed (seed ^ step) on the stream
// word  game id << 32 | seat << 28 | tag << 8 | low byte.  The 20-bit tag is
// the rollout number inside the search; the kernels that draw outside a
// rollout take theirs from the top of the range, so their streams never meet
// each other's or a rollout's:
constexpr uint32_t kNoisyTag0 = 0xFFF00u;    // + 2 * layer + side: a noisy layer's noise vectors (k_noisy_*)
constexpr uint32_t kNoisyLayers = 64u;
constexpr uint32_t kSelectTag = 0xFFFFEu;    // the epsilon-greedy draws (k_dqn_select, k_dqn_select_duel)
constexpr uint32_t kSampleTag = 0xFFFFFu;    // the policy sample (k_policy_sample)
constexpr uint32_t kRolloutTagEnd = kNoisyTag0;  // a rollout number stays below this (rollout_tags_ok: the search refuses a larger one)
static_assert(kRolloutTagEnd <= kNoisyTag0 && kNoisyTag0 + 2u * kNoisyLayers <= kSelectTag && kSelectTag < kSampleTag &&
                  kSampleTag < (1u << 20),
              "rollout numbers, then the noise tags, the select tag, the sample tag: disjoint 20-bit ranges in this order");

// the stream word of seat p of game g (the low 32 bits of this handle's game_offset + g)
// with the low byte 0; the search's step kernels OR theirs in (1 + the rollout step)
__device__ __forceinline__ uint64_t dec_stream(const DevState& s, int64_t g, int p, uint32_t tag) {
    const uint64_t gid = s.game_offset + (uint64_t)g;
    return ((uint64_t)(uint32_t)gid << 32) | ((uint64_t)p << 28) | ((uint64_t)tag << 8);
}

// ---------------------------------------------------------------- candidate rows
// utils/preprocessing.py:55-57 in float32, same operation order as torch
__device__ __forceinline__ float nrm(float x, float lo, float hi) {
    float t = x - lo;
    t = 2.0f * t;
    t = t / (hi - lo);
    return -1.0f + t;
}

template <typename T>
__device__ __forceinline__ T to_out(float v);
template <>
__device__ __forceinline__ float to_out<float>(float v) { return v; }
template <>
__device__ __forceinline__ __hip_bfloat16 to_out<__hip_bfloat16>(float v) { return __float2bfloat16(v); }

// one candidate row: [card, observation of a seat holding `h` on board `b`]
template <typename T>
__device__ __forceinline__ void write_row(T* dst, uint32_t card, const Hand& h, int N, const Board& b, int64_t st = 1) {
    dst[0] = to_out<T>(nrm((float)card, 0.f, 103.f));
#pragma unroll
    for (int k = 0; k < kHand; k++) {
        const uint32_t c = hand_get(h, (uint32_t)k);
        dst[(1 + k) * st] = to_out<T>(nrm(c == 0xFFu ? -1.f : (float)c, 0.f, 103.f));
    }
    dst[11 * st] = to_out<T>(nrm((float)N, 0.f, 6.f));
    const uint32_t lo[4] = {b.lo.x, b.lo.y, b.lo.z, b.lo.w};
    const uint32_t hi[4] = {b.hi.x, b.hi.y, b.hi.z, b.hi.w};
#pragma unroll
    for (int r = 0; r < kRows; r++) {
        dst[(12 + r) * st] = to_out<T>(nrm((float)len_of(hi[r]), 1.f, 5.f));
        dst[(16 + r) * st] = to_out<T>(nrm((float)end_of(hi[r]), 0.f, 103.f));
        dst[(20 + r) * st] = to_out<T>(nrm((float)heads_in(hi[r]), 1.f, 10.f));
#pragma unroll
        for (int i = 0; i < kThreshold; i++) {
            const float v = (i < 5 && (uint32_t)i < len_of(hi[r])) ? (float)card_at(lo[r], hi[r], i < 5 ? i : 0) : -1.f;
            dst[(24 + r * kThreshold + i) * st] = to_out<T>(nrm(v, 0.f, 103.f));
        }
    }
}

// ---------------------------------------------------------------- host
// the search buffers of sn_puct an entry point's kernels dereference (include/sechs.h, at sn_puct):
// checked on the host before anything is launched
enum : unsigned { kNeedAvail = 1, kNeedRo = 2, kNeedStats = 4, kNeedHist = 8, kNeedProbs = 16 };
inline sn_status puct_need(const sn_puct* q, unsigned need) {
    const struct {
        unsigned bit;
        const void* p;
        const char* name;
    } fields[] = {{kNeedAvail, q->avail, "avail"},
                  {kNeedRo, q->rollouts, "rollouts"},
                  {kNeedStats, q->stats, "stats"},
                  {kNeedHist, q->hist, "hist"},
                  {kNeedProbs, q->root_probs, "root_probs"}};
    for (const auto& f : fields)
        if ((need & f.bit) && !f.p)
            return set_error(SN_EINVAL, std::string("sn_puct.") + f.name + " is NULL: this call reads or writes it");
    return SN_OK;
}

// rollouts r0 .. r0 + nr - 1 are stream tags: one at or past kRolloutTagEnd would draw from the stream of a
// noise, select or sample tag, so the entry points that deal or step a rollout refuse it before they launch
inline sn_status rollout_tags_ok(int64_t r0, int64_t nr, const char* what) {
    if (r0 + nr > (int64_t)kRolloutTagEnd)
        return set_error(SN_EINVAL, std::string(what) + ": rollout number " + std::to_string(r0 + nr - 1) +
                                        " reaches the reserved stream tags (rollouts stay below 0xFFF00)");
    return SN_OK;
}

inline sn_status puct_args(sn_env* e, const sn_puct* q, PuctArgs& a, unsigned need = 0) {
    if (!e || !q) return set_error(SN_EINVAL, "NULL argument");
    if (sn_status st = puct_need(q, need); st != SN_OK) return st;
    if (q->n < 1 || q->n > kHand) return set_error(SN_EINVAL, "hand size out of range");
    a.N = e->s.N;
    a.lgs = e->s.lg_K ? e->s.lgs : nullptr;
    if (q->dec_list) {
        if (q->num_dec < 1 || q->num_dec > e->s.B * e->s.N) return set_error(SN_EINVAL, "num_dec out of range");
        a.dec = q->dec_list;
        a.D = q->num_dec;
        a.M = 1u;
        a.seats_mask = 0u;
    } else {
        if (a.lgs) return set_error(SN_EINVAL, "a tournament handle's engines take decision lists (dec_list)");
        const uint32_t mask = q->seats_mask & ((1u << e->s.N) - 1u);
        if (!mask) return set_error(SN_EINVAL, "seats_mask selects no seat");
        a.M = (uint32_t)__builtin_popcount(mask);
        a.seats_mask = mask;
        a.D = e->s.B * a.M;
    }
    a.n = q->n;
    a.flags = q->puct_root ? 1 : 0;
    a.c_puct = q->c_puct;
    a.seed_lo = (uint32_t)q->seed, a.seed_hi = (uint32_t)(q->seed >> 32), a.step = q->step;
    a.rollout = q->rollout;
    a.step_dev = q->step_dev;
    a.avail = q->avail;
    a.ro = q->rollouts;
    a.stats = q->stats;
    a.hist = q->hist;
    a.root_probs = q->root_probs;
    return SN_OK;
}
