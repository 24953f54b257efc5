// sechs_agents.hip -- the per-decision kernels of the net-agent engines: what
// a batched engine without a search calls between the env's steps and its
// PyTorch-ROCm net, for every deciding seat at once on gfx950.
//   the net's input     k_puct_root_rows (the normalised candidate rows of the
//                       policy agents), k_dqn_obs (the raw observation of the
//                       DQN family)
//   the move            k_policy_sample (REINFORCE / ACER), k_pcv_choose
//                       (PUCTCustomedAgent), k_dqn_select / k_dqn_select_duel
//                       (epsilon-greedy over Q)
//   the noisy nets      k_noisy_eps / _scale / _combine
//   replay and targets  k_dqn_pack / _pack_nstep / _unpack, k_dqn_target
// None of them reads a search buffer of sn_puct.  The decision addressing, the
// launch arguments and the Philox stream words are sechs_decide.h's, shared
// with the PUCT search (sechs_puct.hip).
#include <type_traits>

#include "sechs_decide.h"

// ---------------------------------------------------------------- policy agents
// the root candidates' rows, one per card held: [D * n][48], row d * n + k
template <typename T>
__global__ void k_puct_root_rows(DevState s, PuctArgs a, T* rows) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.D * a.n) return;
    const int64_t d = i / a.n;
    const uint32_t k = (uint32_t)(i - d * a.n);
    int64_t g;
    int p;
    dec_to_gp(a, d, g, p);
    const Hand h = load_hand(s, p, g);
    write_row<T>(rows + i * kRowLen, hand_get(h, k), h, players_of(a, g), load_board(s, g));
}

// Categorical(probs).sample() with u from Philox: the first k whose
// running sum of the float32 softmax exceeds u
__device__ __forceinline__ int sample_softmax(const float* x, int n, float u) {
    float m = x[0];
    for (int k = 1; k < n; k++) m = fmaxf(m, x[k]);
    float sum = 0.f;
    for (int k = 0; k < n; k++) sum += __expf(x[k] - m);
    const float target = u * sum;
    float acc = 0.f;
    for (int k = 0; k < n - 1; k++) {
        acc += __expf(x[k] - m);
        if (acc > target) return k;
    }
    return n - 1;
}

// PUCTCustomedAgent (mcts.py:325-451): no rollouts; the 2-head net's value
// head picks the move (_choose_action_mc_func, mcts.py:385-395: the first
// argmax of the values over the legal list), its policy head gives the
// move's log-probability (Categorical(softmax(policy)).log_prob) and the
// chosen value is the step's "outcome".  heads = [D*n][2] f32 (policy, value)
// in sn_puct_root_rows order.  One lane per decision.
__global__ void k_pcv_choose(DevState s, PuctArgs a, const float* heads, int32_t* actions, int32_t* best_index,
                             float* log_prob, float* value) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= a.D) return;
    int64_t g;
    int p;
    dec_to_gp(a, d, g, p);
    const Hand h = load_hand(s, p, g);
    const float2* x = (const float2*)heads + d * a.n;
    float bv = x[0].y, m = x[0].x;
    int best = 0;
    for (int k = 1; k < a.n; k++) {
        const float2 v = x[k];
        if (v.y > bv) bv = v.y, best = k;
        m = fmaxf(m, v.x);
    }
    float sum = 0.f;
    for (int k = 0; k < a.n; k++) sum += expf(x[k].x - m);
    actions[g * s.N + p] = (int32_t)hand_get(h, (uint32_t)best);
    if (best_index) best_index[d] = best;
    if (log_prob) log_prob[d] = (x[best].x - m) - logf(sum);
    if (value) value[d] = bv;
}

// BatchedReinforceAgent.forward (agents/policy.py:137-156) for every
// deciding seat: Categorical(softmax(logits)).sample() with a Philox uniform
// keyed (seed ^ step, game, seat; the tag kSampleTag, never a PUCT
// rollout's), plus log_prob and entropy of the distribution.  logits
// [D*n] f32 in sn_puct_root_rows order.  One lane per decision.
__global__ void k_policy_sample(DevState s, PuctArgs a, const float* logits, int32_t* actions, int32_t* index,
                                float* log_prob, float* entropy) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= a.D) return;
    int64_t g;
    int p;
    dec_to_gp(a, d, g, p);
    const Hand h = load_hand(s, p, g);
    const float* x = logits + d * a.n;
    const uint64_t stream = dec_stream(s, g, p, kSampleTag);
    const int k = sample_softmax(x, a.n, philox_uniform(a.seed_lo ^ puct_step_of(a), a.seed_hi, stream, 0u));
    float m = x[0];
    for (int j = 1; j < a.n; j++) m = fmaxf(m, x[j]);
    float sum = 0.f, sx = 0.f;
    for (int j = 0; j < a.n; j++) {
        const float e = expf(x[j] - m);
        sum += e;
        sx += e * (x[j] - m);
    }
    const float lse = logf(sum);
    actions[g * s.N + p] = (int32_t)hand_get(h, (uint32_t)k);
    if (index) index[d] = k;
    if (log_prob) log_prob[d] = (x[k] - m) - lse;
    if (entropy) entropy[d] = lse - sx / sum;  // -sum p log p
}

// ---------------------------------------------------------------- batched DQN (rl_6_nimmt/dqn.py)
constexpr int kDqnObs = 48;       // observation bytes per row: 47 values + one zero pad
constexpr int kDqnActions = 104;  // the Q head: one value per card
constexpr int kDqnRow = 112;      // replay payload row (the layout at sn_dqn_pack, include/sechs.h)
constexpr int kDqnPieces = kDqnRow / 16;

// byte i (0..15) of a 16-byte piece as the int8 it holds
__device__ __forceinline__ float piece_val(const u32x4& v, int i) {
    const uint32_t w = (i >> 2) == 0 ? v.x : (i >> 2) == 1 ? v.y : (i >> 2) == 2 ? v.z : v.w;
    return (float)(int8_t)((w >> (8 * (i & 3))) & 0xFFu);
}
__device__ __forceinline__ void piece_to_f32(const u32x4& v, float* dst) {
#pragma unroll
    for (int j = 0; j < 4; j++)
        reinterpret_cast<float4*>(dst)[j] =
            float4{piece_val(v, 4 * j), piece_val(v, 4 * j + 1), piece_val(v, 4 * j + 2), piece_val(v, 4 * j + 3)};
}
// the values are integers in -1..104: their bf16 is the upper half of the f32, exactly
__device__ __forceinline__ uint32_t bf16_pair(float a, float b) {
    return (__float_as_uint(a) >> 16) | (__float_as_uint(b) & 0xFFFF0000u);
}
__device__ __forceinline__ void piece_to_bf16(const u32x4& v, uint16_t* dst) {
#pragma unroll
    for (int j = 0; j < 2; j++)
        reinterpret_cast<u32x4*>(dst)[j] = u32x4{bf16_pair(piece_val(v, 8 * j), piece_val(v, 8 * j + 1)),
                                                 bf16_pair(piece_val(v, 8 * j + 2), piece_val(v, 8 * j + 3)),
                                                 bf16_pair(piece_val(v, 8 * j + 4), piece_val(v, 8 * j + 5)),
                                                 bf16_pair(piece_val(v, 8 * j + 6), piece_val(v, 8 * j + 7))};
}

// The observation a DQN agent acts on: the raw _create_states row
// (env.py:174-212) of every deciding seat, un-normalised, as the int8
// replay form and as the Q net's float input (column 47 zero).  One lane
// per decision; an empty hand (after the last step) is the terminal
// next_state: ten -1 bytes.
template <bool BF16>
__global__ void k_dqn_obs(DevState s, PuctArgs a, u32x4* obs_i8, void* states) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= a.D) return;
    int64_t g;
    int p;
    dec_to_gp(a, d, g, p);
    const Hand h = load_hand(s, p, g);
    uint32_t w2hi;
    const GameWords gw = game_words<true>(players_of(a, g), load_board(s, g), w2hi);
    const u32x4 row[3] = {u32x4{(uint32_t)h.lo, (uint32_t)(h.lo >> 32), (h.hi & 0xFFFFu) | w2hi, gw.w0}, gw.a, gw.b};
    if (obs_i8) {
#pragma unroll
        for (int c = 0; c < 3; c++) obs_i8[d * 3 + c] = row[c];
    }
    if (states) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            if (BF16)
                piece_to_bf16(row[c], (uint16_t*)states + d * kDqnObs + 16 * c);
            else
                piece_to_f32(row[c], (float*)states + d * kDqnObs + 16 * c);
        }
    }
}

// _action_selection (agents/dqn.py:85-101) for every deciding seat: epsilon-
// greedy over the hand, one lane per decision.  Two Philox uniforms keyed as
// k_policy_sample's (seed ^ step, game, seat) with the tag kSelectTag, so the
// streams never meet that kernel's or a PUCT rollout's.  Greedy: the first
// maximum of Q[legal[j]] over the ascending legal list = numpy's first
// arg-max of the -1e8-masked vector (any Q > -1e8).  q_row(d) is called on
// the greedy branch only and returns the callable q(c) = Q of card c of
// decision d.
template <class QRow>
__device__ __forceinline__ void dqn_select(const DevState& s, const PuctArgs& a, double eps, int32_t* actions,
                                           int32_t* index, float* value, QRow q_row) {
#pragma clang fp contract(off)
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= a.D) return;
    int64_t g;
    int p;
    dec_to_gp(a, d, g, p);
    const Hand h = load_hand(s, p, g);
    const uint64_t stream = dec_stream(s, g, p, kSelectTag);
    const u32x4 o = philox4x32_10(0u, 0u, (uint32_t)stream, (uint32_t)(stream >> 32), a.seed_lo ^ puct_step_of(a),
                                  a.seed_hi);
    const float u1 = (float)(o.x >> 8) * (1.0f / 16777216.0f), u2 = (float)(o.y >> 8) * (1.0f / 16777216.0f);
    int k;
    float v;
    if (eps <= 0.0 || (eps < 1.0 && (double)u1 > eps)) {  // random.random() > eps; the ends never / always explore
        const auto q_of = q_row(d);
        k = 0;
        v = -1.f;
        for (int j = 0; j < a.n; j++) {
            const uint32_t c = hand_get(h, (uint32_t)j);
            if (c >= (uint32_t)kDqnActions) break;  // a hand shorter than q->n: no load past the Q row
            const float q = q_of(c);
            if (j == 0 || q > v) v = q, k = j;
        }
    } else {  // random.choice(legal)
        k = (int)(u2 * (float)a.n);
        k = k < a.n ? k : a.n - 1;
        v = -1.f;
    }
    actions[g * s.N + p] = (int32_t)hand_get(h, (uint32_t)k);
    if (index) index[d] = k;
    if (value) value[d] = v;
}

// qvals [D][q_stride] f32, the Q head over all 104 cards
__global__ void k_dqn_select(DevState s, PuctArgs a, const float* qvals, int64_t q_stride, double eps, int32_t* actions,
                             int32_t* index, float* value) {
    dqn_select(s, a, eps, actions, index, value, [&](int64_t d) {
        const float* x = qvals + d * q_stride;
        return [x](uint32_t c) { return x[c]; };
    });
}

// k_dqn_select over a duelling net's head output read in place: heads
// [D][stride] f32 with V in column v_col and A in the 104 columns from a_off.
// Q_c = V + (A_c - mean A) as torch evaluates DuellingDQNNet.forward in fp32,
// unfused; mean = sum / 104.0f with the sum taken in this fixed order: four
// partial sums s_k over the columns c = k (mod 4), each ascending in c, then
// (s_0 + s_1) + (s_2 + s_3).  VEC: every row's A starts 16-byte aligned and
// is read as 26 float4; else scalar loads, the same order.
template <bool VEC>
__global__ void k_dqn_select_duel(DevState s, PuctArgs a, const float* heads, int64_t stride, int v_col, int a_off,
                                  double eps, int32_t* actions, int32_t* index, float* value) {
#pragma clang fp contract(off)
    dqn_select(s, a, eps, actions, index, value, [&](int64_t d) {
        const float* x = heads + d * stride;
        const float* adv = x + a_off;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll 2
        for (int j = 0; j < kDqnActions / 4; j++) {
            float4 w;
            if (VEC)
                w = reinterpret_cast<const float4*>(adv)[j];
            else
                w = float4{adv[4 * j], adv[4 * j + 1], adv[4 * j + 2], adv[4 * j + 3]};
            s0 = s0 + w.x;
            s1 = s1 + w.y;
            s2 = s2 + w.z;
            s3 = s3 + w.w;
        }
        const float sum = (s0 + s1) + (s2 + s3);
        const float mean = sum / (float)kDqnActions;
        const float V = x[v_col];
        return [adv, mean, V](uint32_t c) {
            const float centred = adv[c] - mean;
            return V + centred;
        };
    });
}

// ---- the noisy DQN nets (utils/nets.py NoisyFactorizedLinear; rl_6_nimmt/dqn.py) ----
// Every decision row has its own factorised noise: per linear layer l (forward
// order) one vector over the layer's inputs (side 0) and one over its outputs
// (side 1).  Philox keyed as k_dqn_select's (seed ^ step, game, seat) with the
// tag kNoisyTag0 + 2 l + side, l < kNoisyLayers: below the select and sample
// tags and above any PUCT rollout's (the table in sechs_decide.h).  Counter
// word 0 is the pair index i: block i gives the units 2 i and 2 i + 1 by
// Box-Muller in fp32 with the accurate logf / cosf / sinf; u1 in (0, 1], so
// |normal| <= sqrt(48 ln 2).  The value used is e = sign(normal) * sqrt|normal|.

__device__ __forceinline__ float in_f32(float v) { return v; }
__device__ __forceinline__ float in_f32(__hip_bfloat16 v) { return __bfloat162float(v); }
__device__ __forceinline__ float noisy_shape(float n) { return copysignf(sqrtf(fabsf(n)), n); }

__device__ __forceinline__ float2 noisy_pair(const DevState& s, const PuctArgs& a, int64_t d, uint32_t tag, uint32_t i) {
    int64_t g;
    int p;
    dec_to_gp(a, d, g, p);
    const uint64_t stream = dec_stream(s, g, p, tag);
    const u32x4 o = philox4x32_10(i, 0u, (uint32_t)stream, (uint32_t)(stream >> 32), a.seed_lo ^ puct_step_of(a),
                                  a.seed_hi);
    const float u1 = (float)((o.x >> 8) + 1u) * (1.0f / 16777216.0f), u2 = (float)(o.y >> 8) * (1.0f / 16777216.0f);
    const float r = sqrtf(-2.0f * logf(u1));
    const float t = 6.283185307179586f * u2;
    return float2{noisy_shape(r * cosf(t)), noisy_shape(r * sinf(t))};
}

// One lane per (decision row, unit pair), adjacent lanes on adjacent pairs of
// a row; an odd width uses half of its last pair.
#define SN_NOISY_LANE(width)                                                   \
    const int P = ((width) + 1) >> 1;                                          \
    const int64_t lane_id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;    \
    if (lane_id >= a.D * P) return;                                            \
    const int64_t d = lane_id / P;                                             \
    const int i = (int)(lane_id - d * P);                                      \
    const bool both = 2 * i + 1 < (width)

__global__ void k_noisy_eps(DevState s, PuctArgs a, uint32_t tag, int width, float* __restrict__ out) {
    SN_NOISY_LANE(width);
    const float2 e = noisy_pair(s, a, d, tag, (uint32_t)i);
    float* o = out + d * width + 2 * i;
    o[0] = e.x;
    if (both) o[1] = e.y;
}

// out[d][k] = x[d][k] * e_k, the product in fp32 rounded once to T.  VEC: both
// rows start pair-aligned (base pointers and strides), a pair is one access.
template <typename T, bool VEC>
__global__ void k_noisy_scale(DevState s, PuctArgs a, uint32_t tag, const T* __restrict__ x, int64_t x_stride,
                              int width, T* __restrict__ out, int64_t out_stride) {
    SN_NOISY_LANE(width);
    const float2 e = noisy_pair(s, a, d, tag, (uint32_t)i);
    const T* src = x + d * x_stride + 2 * i;
    T* dst = out + d * out_stride + 2 * i;
    if (VEC && both) {
        if constexpr (std::is_same<T, float>::value) {
            const float2 v = *reinterpret_cast<const float2*>(src);
            *reinterpret_cast<float2*>(dst) = float2{v.x * e.x, v.y * e.y};
        } else {
            const uint32_t v = *reinterpret_cast<const uint32_t*>(src);
            const float lo = __uint_as_float(v << 16) * e.x, hi = __uint_as_float(v & 0xFFFF0000u) * e.y;
            *reinterpret_cast<uint32_t*>(dst) = (uint32_t)__bfloat16_as_ushort(__float2bfloat16(lo)) |
                                                ((uint32_t)__bfloat16_as_ushort(__float2bfloat16(hi)) << 16);
        }
        return;
    }
    dst[0] = to_out<T>(in_f32(src[0]) * e.x);
    if (both) dst[1] = to_out<T>(in_f32(src[1]) * e.y);
}

// out[d][j] = mu[d][j] + e_{j - col0} * (sg[d][j] + sigma_b[j]) over the columns
// col0 .. col0 + width - 1, fp32 in that order, every operation rounded (no
// fma), then max(., 0) if relu.  out may be mu.  VEC: col0, the stride and the
// pointers are pair-aligned.
template <bool VEC>
__global__ void k_noisy_combine(DevState s, PuctArgs a, uint32_t tag, const float* mu, const float* sg, int64_t stride,
                                int col0, int width, const float* __restrict__ sigma_b, int relu, float* out) {
#pragma clang fp contract(off)
    SN_NOISY_LANE(width);
    const float2 e = noisy_pair(s, a, d, tag, (uint32_t)i);
    const int j = col0 + 2 * i;
    const int64_t at = d * stride + j;
    if (VEC && both) {
        const float2 m = *reinterpret_cast<const float2*>(mu + at), g = *reinterpret_cast<const float2*>(sg + at);
        const float2 b = *reinterpret_cast<const float2*>(sigma_b + j);
        const float s0 = g.x + b.x, s1 = g.y + b.y;
        const float n0 = e.x * s0, n1 = e.y * s1;
        float v0 = m.x + n0, v1 = m.y + n1;
        if (relu) v0 = fmaxf(v0, 0.f), v1 = fmaxf(v1, 0.f);
        *reinterpret_cast<float2*>(out + at) = float2{v0, v1};
        return;
    }
    {
        const float s0 = sg[at] + sigma_b[j];
        const float n0 = e.x * s0;
        const float v0 = mu[at] + n0;
        out[at] = relu ? fmaxf(v0, 0.f) : v0;
    }
    if (both) {
        const float s1 = sg[at + 1] + sigma_b[j + 1];
        const float n1 = e.y * s1;
        const float v1 = mu[at + 1] + n1;
        out[at + 1] = relu ? fmaxf(v1, 0.f) : v1;
    }
}
#undef SN_NOISY_LANE

// the hand size of an observation from its first piece: hand bytes 0..9, the
// cards held are >= 0 and the empty slots -1, so it is 10 - the sign bits set
__device__ __forceinline__ uint32_t dqn_hand_size(const u32x4& h) {
    const uint32_t neg = (h.x & 0x80808080u) | ((h.y & 0x80808080u) >> 1) | ((h.z & 0x00008080u) >> 2);
    return 10u - (uint32_t)__builtin_popcount(neg);
}
// byte 96..99 of a replay row: action | done << 8 | hand size << 16 | m << 24
__device__ __forceinline__ uint32_t dqn_control(int32_t action, uint32_t done, uint32_t hand, uint32_t m) {
    return ((uint32_t)action & 0xFFu) | (done << 8) | (hand << 16) | (m << 24);
}

// Replay rows of one episode: row (t, d) = [obs[t][d] | obs[t+1][d] | action,
// done, hand size, 0 | reward i32 | 0, 0].  One lane per 16-byte piece,
// consecutive lanes on consecutive pieces of a row (as k_per_store).
__global__ void k_dqn_pack(int64_t T, int64_t D, const u32x4* __restrict__ obs, const int32_t* __restrict__ actions,
                           const int32_t* __restrict__ rewards_seen, u32x4* __restrict__ rows) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= T * D * kDqnPieces) return;
    const int64_t r = e / kDqnPieces;
    const int c = (int)(e - r * kDqnPieces);
    const int64_t t = r / D;
    u32x4 v;
    if (c < 6) {
        v = obs[(r + (c < 3 ? 0 : D)) * 3 + (c < 3 ? c : c - 3)];  // obs[t + 1][d] lies D rows on
    } else {
        const uint32_t hand = dqn_hand_size(obs[r * 3]);
        const uint32_t done = t == T - 1 ? 1u : 0u;
        v = u32x4{dqn_control(actions[r], done, hand, 0u), (uint32_t)rewards_seen[r], 0u, 0u};
    }
    rows[e] = v;
}

// The n-step rows of one episode (DQN_NStep_Agent._store / _finish_episode,
// agents/dqn.py:264-301): row (s, d) = [obs[s][d] | obs[min(s + n, T)][d] |
// action, done, hand size, m | r_s i32 | n-step return f32 | 0] with
// m = min(n, T - s) rewards summed and done = s + n > T, or the last step's
// own flag when n = 1.  The return accumulates in f64 from 0.0, left to
// right, acc = acc + (double)r_{s+i} * gpow[i] unfused (Python's sum of
// r * gamma ** i; gpow holds the host's gamma ** i), and is rounded to f32
// once.  One lane per 16-byte piece.
struct DqnGpow {
    double v[SN_DQN_T_STEPS];
};
__global__ void k_dqn_pack_nstep(int64_t T, int64_t D, int n, DqnGpow gpow, const u32x4* __restrict__ obs,
                                 const int32_t* __restrict__ actions, const int32_t* __restrict__ rewards_seen,
                                 u32x4* __restrict__ rows) {
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= T * D * kDqnPieces) return;
    const int64_t r = e / kDqnPieces;
    const int c = (int)(e - r * kDqnPieces);
    const int64_t t = r / D;
    const int64_t left = T - t;  // 1..T <= SN_DQN_T_STEPS
    const int m = (int64_t)n < left ? n : (int)left;
    u32x4 v;
    if (c < 3) {
        v = obs[r * 3 + c];
    } else if (c < 6) {
        v = obs[(r + (int64_t)m * D) * 3 + (c - 3)];  // obs[min(t + n, T)][d] lies m * D rows on
    } else {
        const uint32_t hand = dqn_hand_size(obs[r * 3]);
        const uint32_t done = ((int64_t)n > left || (n == 1 && left == 1)) ? 1u : 0u;
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < SN_DQN_T_STEPS; i++) {
            if (i < m) {
                const double term = (double)rewards_seen[r + (int64_t)i * D] * gpow.v[i];
                acc = acc + term;
            }
        }
        v = u32x4{dqn_control(actions[r], done, hand, (uint32_t)m), (uint32_t)rewards_seen[r],
                  __float_as_uint((float)acc), 0u};
    }
    rows[e] = v;
}

// the inverse for a sampled minibatch: fp32 states / next_states [n][48],
// action [n] i64, reward [n] f32, not_done [n] f32 = 1 - done.  One lane per
// 16-byte piece of a row.  NSTEP: the reward is the n-step return, the f32 at
// byte 104 (k_dqn_pack_nstep); else the i32 at byte 100.
template <bool NSTEP>
__global__ void k_dqn_unpack(int64_t n, const u32x4* __restrict__ rows, float* __restrict__ states,
                             float* __restrict__ next_states, int64_t* __restrict__ action, float* __restrict__ reward,
                             float* __restrict__ not_done) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * kDqnPieces) return;
    const int64_t r = e / kDqnPieces;
    const int c = (int)(e - r * kDqnPieces);
    const u32x4 v = rows[e];
    if (c < 3) {
        if (states) piece_to_f32(v, states + r * kDqnObs + 16 * c);
    } else if (c < 6) {
        if (next_states) piece_to_f32(v, next_states + r * kDqnObs + 16 * (c - 3));
    } else {
        if (action) action[r] = (int64_t)(v.x & 0xFFu);
        if (reward) reward[r] = NSTEP ? __uint_as_float(v.z) : (float)(int32_t)v.y;
        if (not_done) not_done[r] = ((v.x >> 8) & 0xFFu) ? 0.f : 1.f;
    }
}

// Bellman targets (agents/dqn.py:136-140 DQNVanilla._calc_reward, :165-174
// DDQNAgent._calc_reward): one wave per row, lanes on consecutive actions,
// an arg-max butterfly that carries the index (lowest index on ties, as
// torch.max / torch.argmax over the unmasked 104 actions).  fp32 in torch's
// operation order -- reward + gamma * (value * not_done) -- unfused.
__global__ __launch_bounds__(kBlock) void k_dqn_target(int64_t n, const float* __restrict__ q_local,
                                                       const float* __restrict__ q_target, int64_t stride,
                                                       const float* __restrict__ reward,
                                                       const float* __restrict__ not_done, float gamma,
                                                       float* __restrict__ target) {
#pragma clang fp contract(off)
    const int lane = (int)(threadIdx.x & 63u);
    const int64_t r = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (r >= n) return;  // whole waves leave together
    const float* x = q_local + r * stride;
    float v = x[lane];
    int i = lane;
    if (lane + 64 < kDqnActions) {
        const float w = x[lane + 64];
        if (w > v) v = w, i = lane + 64;
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const float ov = __shfl_xor(v, m, 64);
        const int oi = __shfl_xor(i, m, 64);
        if (ov > v || (ov == v && oi < i)) v = ov, i = oi;
    }
    if (lane == 0) {
        const float best = q_target ? q_target[r * stride + i] : v;
        const float kept = best * not_done[r];
        const float disc = gamma * kept;
        target[r] = reward[r] + disc;
    }
}

// ============================================================================
// C ABI
// ============================================================================
extern "C" {

sn_status sn_puct_root_rows(sn_env* e, const sn_puct* q, void* rows, int bf16, void* stream) {
    PuctArgs a{};
    sn_status st = puct_args(e, q, a);
    if (st != SN_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    if (bf16)
        hipLaunchKernelGGL(k_puct_root_rows<__hip_bfloat16>, dim3(grid_for(a.D * a.n)), dim3(kBlock), 0, s, e->s, a,
                           (__hip_bfloat16*)rows);
    else
        hipLaunchKernelGGL(k_puct_root_rows<float>, dim3(grid_for(a.D * a.n)), dim3(kBlock), 0, s, e->s, a, (float*)rows);
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

sn_status sn_pcv_choose(sn_env* e, const sn_puct* q, const float* heads, int32_t* actions, int32_t* best_index,
                        float* log_prob, float* value, void* stream) {
    if (!heads || !actions) return set_error(SN_EINVAL, "NULL argument");
    PuctArgs a{};
    sn_status st = puct_args(e, q, a);
    if (st != SN_OK) return st;
    if (a.n < 1) return set_error(SN_EINVAL, "hand size must be >= 1");
    hipLaunchKernelGGL(k_pcv_choose, dim3(grid_for(a.D)), dim3(kBlock), 0, (hipStream_t)stream, e->s, a, heads,
                       actions, best_index, log_prob, value);
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

sn_status sn_policy_sample(sn_env* e, const sn_puct* q, const float* logits, int32_t* actions, int32_t* index,
                           float* log_prob, float* entropy, void* stream) {
    if (!logits || !actions) return set_error(SN_EINVAL, "NULL argument");
    PuctArgs a{};
    sn_status st = puct_args(e, q, a);
    if (st != SN_OK) return st;
    hipLaunchKernelGGL(k_policy_sample, dim3(grid_for(a.D)), dim3(kBlock), 0, (hipStream_t)stream, e->s, a, logits,
                       actions, index, log_prob, entropy);
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

sn_status sn_dqn_obs(sn_env* e, const sn_puct* q, void* obs_i8, void* states, int bf16, void* stream) {
    if (!q) return set_error(SN_EINVAL, "NULL argument");
    if ((((uintptr_t)obs_i8 | (uintptr_t)states) & 15) != 0) return set_error(SN_EINVAL, "outputs must be 16-byte aligned");
    sn_puct qq = *q;
    if (qq.n == 0) qq.n = 1;  // the hand size is not used: after the last step it is 0
    PuctArgs a{};
    sn_status st = puct_args(e, &qq, a);
    if (st != SN_OK) return st;
    if (!obs_i8 && !states) return SN_OK;
    if (bf16)
        hipLaunchKernelGGL(k_dqn_obs<true>, dim3(grid_for(a.D)), dim3(kBlock), 0, (hipStream_t)stream, e->s, a,
                           (u32x4*)obs_i8, states);
    else
        hipLaunchKernelGGL(k_dqn_obs<false>, dim3(grid_for(a.D)), dim3(kBlock), 0, (hipStream_t)stream, e->s, a,
                           (u32x4*)obs_i8, states);
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

sn_status sn_dqn_select(sn_env* e, const sn_puct* q, const float* qvals, int64_t q_stride, double eps, int32_t* actions,
                        int32_t* index, float* value, void* stream) {
    if (!qvals || !actions) return set_error(SN_EINVAL, "NULL argument");
    if (q_stride < kDqnActions) return set_error(SN_EINVAL, "q_stride must be >= 104");
    if (!(eps == eps)) return set_error(SN_EINVAL, "eps is NaN");
    PuctArgs a{};
    sn_status st = puct_args(e, q, a);
    if (st != SN_OK) return st;
    hipLaunchKernelGGL(k_dqn_select, dim3(grid_for(a.D)), dim3(kBlock), 0, (hipStream_t)stream, e->s, a, qvals,
                       q_stride, eps, actions, index, value);
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

sn_status sn_dqn_pack(int64_t T, int64_t D, const void* obs_i8, const int32_t* actions, const int32_t* rewards_seen,
                      void* rows, void* stream) {
    if (!obs_i8 || !actions || !rewards_seen || !rows) return set_error(SN_EINVAL, "NULL argument");
    if (T < 1 || D < 1 || T > 0x7FFFFFFF / D) return set_error(SN_EINVAL, "T x D must be in 1..2^31-1");
    if ((((uintptr_t)obs_i8 | (uintptr_t)rows) & 15) != 0) return set_error(SN_EINVAL, "obs_i8 and rows must be 16-byte aligned");
    hipLaunchKernelGGL(k_dqn_pack, dim3(grid_for(T * D * kDqnPieces)), dim3(kBlock), 0, (hipStream_t)stream, T, D,
                       (const u32x4*)obs_i8, actions, rewards_seen, (u32x4*)rows);
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

sn_status sn_dqn_unpack(int64_t n, const void* rows, float* states, float* next_states, int64_t* action, float* reward,
                        float* not_done, void* stream) {
    if (!rows) return set_error(SN_EINVAL, "NULL argument");
    if (n < 1 || n > 0x7FFFFFFF) return set_error(SN_EINVAL, "n must be in 1..2^31-1");
    if ((((uintptr_t)rows | (uintptr_t)states | (uintptr_t)next_states) & 15) != 0)
        return set_error(SN_EINVAL, "rows, states and next_states must be 16-byte aligned");
    hipLaunchKernelGGL(k_dqn_unpack<false>, dim3(grid_for(n * kDqnPieces)), dim3(kBlock), 0, (hipStream_t)stream, n,
                       (const u32x4*)rows, states, next_states, action, reward, not_done);
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

sn_status sn_dqn_select_duel(sn_env* e, const sn_puct* q, const float* heads, int64_t stride, int64_t v_col,
                             int64_t a_off, double eps, int32_t* actions, int32_t* index, float* value, void* stream) {
    if (!heads || !actions) return set_error(SN_EINVAL, "NULL argument");
    if (a_off < 0 || v_col < 0 || a_off > stride - kDqnActions || v_col >= stride ||
        (v_col >= a_off && v_col < a_off + kDqnActions))
        return set_error(SN_EINVAL, "V and the 104 A columns must lie apart inside a row of `stride` floats");
    if (stride > 0x7FFFFFFF) return set_error(SN_EINVAL, "stride must be < 2^31");
    if (!(eps == eps)) return set_error(SN_EINVAL, "eps is NaN");
    PuctArgs a{};
    sn_status st = puct_args(e, q, a);
    if (st != SN_OK) return st;
    const bool vec = ((uintptr_t)(heads + a_off) & 15) == 0 && (stride & 3) == 0;
    if (vec)
        hipLaunchKernelGGL(k_dqn_select_duel<true>, dim3(grid_for(a.D)), dim3(kBlock), 0, (hipStream_t)stream, e->s, a,
                           heads, stride, (int)v_col, (int)a_off, eps, actions, index, value);
    else
        hipLaunchKernelGGL(k_dqn_select_duel<false>, dim3(grid_for(a.D)), dim3(kBlock), 0, (hipStream_t)stream, e->s, a,
                           heads, stride, (int)v_col, (int)a_off, eps, actions, index, value);
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

sn_status sn_dqn_pack_nstep(int64_t T, int64_t D, int64_t n, sn_dqn_gpow gpow, const void* obs_i8,
                            const int32_t* actions, const int32_t* rewards_seen, void* rows, void* stream) {
    if (!obs_i8 || !actions || !rewards_seen || !rows) return set_error(SN_EINVAL, "NULL argument");
    if (T < 1 || T > SN_DQN_T_STEPS) return set_error(SN_EINVAL, "T must be in 1..10");
    if (n < 1 || n > 0x7FFFFFFF) return set_error(SN_EINVAL, "n must be in 1..2^31-1");
    if (D < 1 || T > 0x7FFFFFFF / D) return set_error(SN_EINVAL, "T x D must be in 1..2^31-1");
    if ((((uintptr_t)obs_i8 | (uintptr_t)rows) & 15) != 0) return set_error(SN_EINVAL, "obs_i8 and rows must be 16-byte aligned");
    DqnGpow gp;
    for (int i = 0; i < SN_DQN_T_STEPS; i++) gp.v[i] = gpow.v[i];
    hipLaunchKernelGGL(k_dqn_pack_nstep, dim3(grid_for(T * D * kDqnPieces)), dim3(kBlock), 0, (hipStream_t)stream, T, D,
                       (int)n, gp, (const u32x4*)obs_i8, actions, rewards_seen, (u32x4*)rows);
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

sn_status sn_dqn_unpack_nstep(int64_t n, const void* rows, float* states, float* next_states, int64_t* action,
                              float* reward, float* not_done, void* stream) {
    if (!rows) return set_error(SN_EINVAL, "NULL argument");
    if (n < 1 || n > 0x7FFFFFFF) return set_error(SN_EINVAL, "n must be in 1..2^31-1");
    if ((((uintptr_t)rows | (uintptr_t)states | (uintptr_t)next_states) & 15) != 0)
        return set_error(SN_EINVAL, "rows, states and next_states must be 16-byte aligned");
    hipLaunchKernelGGL(k_dqn_unpack<true>, dim3(grid_for(n * kDqnPieces)), dim3(kBlock), 0, (hipStream_t)stream, n,
                       (const u32x4*)rows, states, next_states, action, reward, not_done);
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

sn_status sn_dqn_target(int64_t n, const float* q_next_local, const float* q_next_target, int64_t stride,
                        const float* reward, const float* not_done, double gamma, float* target, void* stream) {
    if (!q_next_local || !reward || !not_done || !target) return set_error(SN_EINVAL, "NULL argument");
    if (n < 1 || n > 0x7FFFFFFF) return set_error(SN_EINVAL, "n must be in 1..2^31-1");
    if (stride < kDqnActions) return set_error(SN_EINVAL, "stride must be >= 104");
    hipLaunchKernelGGL(k_dqn_target, dim3((unsigned)((n + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0,
                       (hipStream_t)stream, n, q_next_local, q_next_target, stride, reward, not_done, (float)gamma,
                       target);
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

// the noise kernels' shared argument checks: the decider arguments, a tag of layer < 64, a width
static sn_status noisy_args(sn_env* e, const sn_puct* q, PuctArgs& a, int64_t tag, int64_t width) {
    sn_status st = puct_args(e, q, a);
    if (st != SN_OK) return st;
    if (tag < kNoisyTag0 || tag >= kNoisyTag0 + 2 * kNoisyLayers)
        return set_error(SN_EINVAL, "tag must be 0xFFF00 + 2 * layer + side with layer < 64");
    if (width < 1 || width > 0x3FFFFFFF) return set_error(SN_EINVAL, "width must be >= 1");
    return SN_OK;
}
static unsigned noisy_grid(const PuctArgs& a, int64_t width) { return grid_for(a.D * ((width + 1) / 2)); }

sn_status sn_noisy_eps(sn_env* e, const sn_puct* q, int64_t tag, int64_t width, float* out, void* stream) {
    if (!out) return set_error(SN_EINVAL, "NULL argument");
    PuctArgs a{};
    sn_status st = noisy_args(e, q, a, tag, width);
    if (st != SN_OK) return st;
    hipLaunchKernelGGL(k_noisy_eps, dim3(noisy_grid(a, width)), dim3(kBlock), 0, (hipStream_t)stream, e->s, a,
                       (uint32_t)tag, (int)width, out);
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

sn_status sn_noisy_scale(sn_env* e, const sn_puct* q, int64_t tag, const void* x, int64_t x_stride, int64_t width,
                         int bf16, void* out, int64_t out_stride, void* stream) {
    if (!x || !out) return set_error(SN_EINVAL, "NULL argument");
    PuctArgs a{};
    sn_status st = noisy_args(e, q, a, tag, width);
    if (st != SN_OK) return st;
    if (x_stride < width || out_stride < width) return set_error(SN_EINVAL, "a row stride is shorter than the width");
    const uintptr_t pair = bf16 ? 3 : 7;  // a pair's bytes - 1
    const bool vec = (((uintptr_t)x | (uintptr_t)out) & pair) == 0 && ((x_stride | out_stride) & 1) == 0;
    const dim3 grid(noisy_grid(a, width)), block(kBlock);
    hipStream_t hs = (hipStream_t)stream;
#define SN_SCALE(T, V)                                                                                              \
    hipLaunchKernelGGL((k_noisy_scale<T, V>), grid, block, 0, hs, e->s, a, (uint32_t)tag, (const T*)x, x_stride, \
                       (int)width, (T*)out, out_stride)
    if (bf16) {
        if (vec) SN_SCALE(__hip_bfloat16, true); else SN_SCALE(__hip_bfloat16, false);
    } else {
        if (vec) SN_SCALE(float, true); else SN_SCALE(float, false);
    }
#undef SN_SCALE
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

sn_status sn_noisy_combine(sn_env* e, const sn_puct* q, int64_t tag, const float* mu, const float* sg, int64_t stride,
                           int64_t col0, int64_t width, const float* sigma_b, int relu, float* out, void* stream) {
    if (!mu || !sg || !sigma_b || !out) return set_error(SN_EINVAL, "NULL argument");
    PuctArgs a{};
    sn_status st = noisy_args(e, q, a, tag, width);
    if (st != SN_OK) return st;
    if (col0 < 0 || stride > 0x7FFFFFFF || col0 > stride - width)
        return set_error(SN_EINVAL, "the columns col0 .. col0 + width - 1 must lie inside a row of `stride` floats");
    const bool vec = (((uintptr_t)mu | (uintptr_t)sg | (uintptr_t)sigma_b | (uintptr_t)out) & 7) == 0 &&
                     ((stride | col0) & 1) == 0;
    if (vec)
        hipLaunchKernelGGL(k_noisy_combine<true>, dim3(noisy_grid(a, width)), dim3(kBlock), 0, (hipStream_t)stream, e->s,
                           a, (uint32_t)tag, mu, sg, stride, (int)col0, (int)width, sigma_b, relu, out);
    else
        hipLaunchKernelGGL(k_noisy_combine<false>, dim3(noisy_grid(a, width)), dim3(kBlock), 0, (hipStream_t)stream, e->s,
                           a, (uint32_t)tag, mu, sg, stride, (int)col0, (int)width, sigma_b, relu, out);
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

}  // extern "C"
