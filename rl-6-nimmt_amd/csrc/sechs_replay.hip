// sechs_replay.hip -- prioritised experience replay on gfx950: the SumTree and
// PriorityReplayBuffer of the reference (utils/replay_buffer.py:15-203) behind
// the sn_per_* entry points; include/sechs.h states the contract (the heap
// layout, the two kept quirks of the reference's counters).
//
// Where the reference walks `+= change` up from one leaf per store / update
// (replay_buffer.py:16-27), the kernels write all leaves of a call and then
// recompute every internal node as left + right, pairwise from the leaves
// (k_per_rebuild): deterministic, no atomics on the tree, and equal to the
// incremental tree up to that tree's own rounding drift (~1e-14 relative).
// Sampling keeps the reference's operation order in f64; FP contraction is off
// for the whole file: a fused seg * i + u * seg is a different number.
#include <new>

#include "sechs_state.h"

#pragma clang fp contract(off)

using namespace sechs;

namespace {

constexpr int kPerBlock = 256;      // threads per workgroup of every kernel here
constexpr int kPerPartials = 256;   // most workgroups of a leaf reduction
constexpr int kPerLevels = 11;      // tree levels one workgroup rebuilds in LDS (2^11 - 1 f64 = 16 KiB)
constexpr int64_t kPerMaxCapacity = (int64_t)1 << 30;  // 2*capacity-1 fits the u32 tree indices

// every thread of the workgroup gets the (min, max) over the workgroup's (lo, hi)
__device__ inline void per_block_minmax(double& lo, double& hi) {
    __shared__ double smin[kPerBlock], smax[kPerBlock];
    smin[threadIdx.x] = lo, smax[threadIdx.x] = hi;
    __syncthreads();
    for (int s = kPerBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const double a = smin[threadIdx.x + s], b = smax[threadIdx.x + s];
            if (a < smin[threadIdx.x]) smin[threadIdx.x] = a;
            if (b > smax[threadIdx.x]) smax[threadIdx.x] = b;
        }
        __syncthreads();
    }
    lo = smin[0], hi = smax[0];
}

// min and max over `count` leaves, one (min, max) pair per workgroup into
// part[2b], part[2b+1]; the consumers reduce the <= kPerPartials pairs again
__global__ void __launch_bounds__(kPerBlock) k_per_reduce(const double* __restrict__ leaves, int64_t count,
                                                          double* __restrict__ part) {
    double lo = INFINITY, hi = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * kPerBlock + threadIdx.x; i < count; i += (int64_t)gridDim.x * kPerBlock) {
        const double x = leaves[i];
        lo = x < lo ? x : lo;
        hi = x > hi ? x : hi;
    }
    per_block_minmax(lo, hi);
    if (threadIdx.x == 0) part[2 * blockIdx.x] = lo, part[2 * blockIdx.x + 1] = hi;
}

__device__ inline void per_partials(const double* __restrict__ part, int nparts, double& lo, double& hi) {
    lo = INFINITY, hi = -INFINITY;
    if ((int)threadIdx.x < nparts) lo = part[2 * threadIdx.x], hi = part[2 * threadIdx.x + 1];
    per_block_minmax(lo, hi);
}

// PriorityReplayBuffer.store x m (replay_buffer.py:150-158): slots pointer ..
// pointer+m-1 (mod capacity) get the priority M = max leaf before the call
// (1.0 if that is 0), and their payload rows.  One thread per 16-byte piece
// of a row (one per row without payload).
__global__ void __launch_bounds__(kPerBlock) k_per_store(double* __restrict__ tree, uint8_t* __restrict__ ring,
                                                         const uint8_t* __restrict__ rows, int64_t cap, int64_t pointer,
                                                         int64_t m, int chunks, const double* __restrict__ part,
                                                         int nparts) {
    double lo, hi;
    per_partials(part, nparts, lo, hi);
    const double prio = hi == 0.0 ? 1.0 : hi;
    const int per_row = chunks > 0 ? chunks : 1;
    const int64_t e = (int64_t)blockIdx.x * kPerBlock + threadIdx.x;
    if (e >= m * per_row) return;
    const int64_t j = e / per_row;
    const int c = (int)(e - j * per_row);
    int64_t slot = pointer + j;
    if (slot >= cap) slot -= cap;
    if (c == 0) tree[cap - 1 + slot] = prio;
    if (chunks > 0 && rows)
        reinterpret_cast<uint4*>(ring)[slot * chunks + c] = reinterpret_cast<const uint4*>(rows)[j * chunks + c];
}

// Internal nodes of depths d0 .. d0+k-1 (k <= kPerLevels): workgroup b owns
// the subtree rooted at r = 2^d0 - 1 + b, whose relative level j is the
// contiguous range [(r+1)*2^j - 1, (r+1)*2^j - 1 + 2^j) for any capacity.
// The deepest level reads its children from memory (already final: leaves or
// an earlier pass), the levels above read what this workgroup just computed
// from LDS -- except children that are leaves (index >= cap-1: a capacity
// that is no power of two has leaves at two depths), read from memory.
__global__ void __launch_bounds__(kPerBlock) k_per_rebuild(double* __restrict__ tree, int64_t cap, int d0, int k) {
    __shared__ double lvl[(1 << kPerLevels)];  // level j at [2^j, 2^(j+1))
    const int64_t r = (((int64_t)1 << d0) - 1) + blockIdx.x;
    const int64_t internal = cap - 1;
    for (int j = k - 1; j >= 0; j--) {
        const int64_t first = ((r + 1) << j) - 1;
        for (int t = threadIdx.x; t < (1 << j); t += kPerBlock) {
            const int64_t node = first + t;
            if (node >= internal) continue;
            const int64_t c = 2 * node + 1;
            const bool mem = j == k - 1;
            const double left = (mem || c >= internal) ? tree[c] : lvl[(2 << j) + 2 * t];
            const double right = (mem || c + 1 >= internal) ? tree[c + 1] : lvl[(2 << j) + 2 * t + 1];
            const double sum = left + right;
            lvl[(1 << j) + t] = sum;
            tree[node] = sum;
        }
        __syncthreads();
    }
}

// PriorityReplayBuffer.sample / get_samples (replay_buffer.py:160-186): one
// lane per sample walks the tree (_get_leaf_index, :43-60; the loop ends at
// the array length, so every load is in bounds), then the workgroup copies
// the sampled payload rows, 16 bytes per lane, consecutive lanes on
// consecutive pieces of a row.
__global__ void __launch_bounds__(kPerBlock) k_per_sample(const double* __restrict__ tree,
                                                          const uint8_t* __restrict__ ring, int64_t cap, int64_t n,
                                                          const double* __restrict__ u, double beta,
                                                          uint32_t* __restrict__ tree_idx, double* __restrict__ priority,
                                                          double* __restrict__ is_weight, uint8_t* __restrict__ rows_out,
                                                          int chunks, const double* __restrict__ part, int nparts) {
    __shared__ int64_t slot_of[kPerBlock];
    double min_leaf, hi;
    per_partials(part, nparts, min_leaf, hi);
    const int64_t base = (int64_t)blockIdx.x * kPerBlock;
    const int64_t i = base + threadIdx.x;
    const int64_t len = 2 * cap - 1;
    if (i < n) {
        const double total = tree[0];
        const double seg = total / (double)n;
        const double a = seg * (double)i;
        const double b = u[i] * seg;
        double v = a + b;
        int64_t node = 0;
        for (;;) {
            const int64_t left = 2 * node + 1;
            if (left >= len) break;
            const double l = tree[left];
            if (v <= l) {
                node = left;
            } else {
                v -= l;
                node = left + 1;
            }
        }
        const double p = tree[node];
        const double min_prob = min_leaf / total;
        const double prob = p / total;
        tree_idx[i] = (uint32_t)node;
        if (priority) priority[i] = p;
        if (is_weight) is_weight[i] = pow(prob / min_prob, -beta);
        slot_of[threadIdx.x] = node - (cap - 1);
    }
    if (!rows_out || chunks == 0) return;
    __syncthreads();
    const int64_t here = n - base < kPerBlock ? n - base : kPerBlock;
    for (int64_t e = threadIdx.x; e < here * chunks; e += kPerBlock) {
        const int64_t s = e / chunks;
        const int c = (int)(e - s * chunks);
        reinterpret_cast<uint4*>(rows_out)[(base + s) * chunks + c] =
            reinterpret_cast<const uint4*>(ring)[slot_of[s] * chunks + c];
    }
}

// The payload rows of n given data slots: k_per_sample's gather without the
// tree walk (History.sample, replay_buffer.py: random.sample(range(len))
// picks the slots).  A slot outside [0, cap) gives a zero row.
__global__ void __launch_bounds__(kPerBlock) k_per_gather(const uint8_t* __restrict__ ring, int64_t cap, int64_t n,
                                                          const int32_t* __restrict__ slots,
                                                          uint8_t* __restrict__ rows_out, int chunks) {
    const int64_t e = (int64_t)blockIdx.x * kPerBlock + threadIdx.x;
    if (e >= n * chunks) return;
    const int64_t s = e / chunks;
    const int c = (int)(e - s * chunks);
    const int64_t slot = slots[s];
    uint4 v = uint4{0u, 0u, 0u, 0u};
    if (slot >= 0 && slot < cap) v = reinterpret_cast<const uint4*>(ring)[slot * chunks + c];
    reinterpret_cast<uint4*>(rows_out)[e] = v;
}

// batch_update (replay_buffer.py:188-200) is a sequential loop: where a tree
// index repeats, the last position wins.  k_per_claim records per leaf the
// highest position + 1 that names it (integer max: the result does not depend
// on the order), k_per_write lets only that position write and clears the
// claim for the next call.  Indices outside the leaf range are skipped.
__global__ void __launch_bounds__(kPerBlock) k_per_claim(uint32_t* __restrict__ owner, int64_t cap, int64_t n,
                                                         const uint32_t* __restrict__ tree_idx) {
    const int64_t i = (int64_t)blockIdx.x * kPerBlock + threadIdx.x;
    if (i >= n) return;
    const int64_t node = tree_idx[i];
    if (node < cap - 1 || node > 2 * cap - 2) return;
    atomicMax(&owner[node - (cap - 1)], (uint32_t)(i + 1));
}

__global__ void __launch_bounds__(kPerBlock) k_per_write(double* __restrict__ tree, uint32_t* __restrict__ owner,
                                                         int64_t cap, int64_t n, const uint32_t* __restrict__ tree_idx,
                                                         const double* __restrict__ abs_err, double eps, double upper,
                                                         double alpha) {
    const int64_t i = (int64_t)blockIdx.x * kPerBlock + threadIdx.x;
    if (i >= n) return;
    const int64_t node = tree_idx[i];
    if (node < cap - 1 || node > 2 * cap - 2) return;
    if (owner[node - (cap - 1)] != (uint32_t)(i + 1)) return;
    owner[node - (cap - 1)] = 0;
    const double e = abs_err[i] + eps;
    const double clipped = e < upper ? e : upper;  // np.minimum
    tree[node] = alpha == 1.0 ? clipped : pow(clipped, alpha);
}

// sn_per_inherit / sn_per_import: every destination slot is written, so
// nothing stale survives.  Slot k < h takes the leaf and the payload row of
// source slot (src_first + k) mod cap_src, slot k >= h a zero leaf and a zero
// row.  One thread per 16-byte piece of a destination row (one per row
// without payload), the layout of k_per_store.  src_first < cap_src, h <=
// min(cap_src, cap_dst); per_rebuild follows.
__global__ void __launch_bounds__(kPerBlock) k_per_inherit(double* __restrict__ tree, uint8_t* __restrict__ ring,
                                                           int64_t cap, const double* __restrict__ src_leaves,
                                                           const uint8_t* __restrict__ src_ring, int64_t cap_src,
                                                           int64_t src_first, int64_t h, int chunks) {
    const int per_row = chunks > 0 ? chunks : 1;
    const int64_t e = (int64_t)blockIdx.x * kPerBlock + threadIdx.x;
    if (e >= cap * per_row) return;
    const int64_t k = e / per_row;
    const int c = (int)(e - k * per_row);
    double leaf = 0.0;
    uint4 v = uint4{0u, 0u, 0u, 0u};
    if (k < h) {
        int64_t s = src_first + k;
        if (s >= cap_src) s -= cap_src;
        leaf = src_leaves[s];
        if (chunks > 0) v = reinterpret_cast<const uint4*>(src_ring)[s * chunks + c];
    }
    if (c == 0) tree[cap - 1 + k] = leaf;
    if (chunks > 0) reinterpret_cast<uint4*>(ring)[k * chunks + c] = v;
}

inline unsigned per_grid(int64_t n) { return (unsigned)((n + kPerBlock - 1) / kPerBlock); }

}  // namespace

struct sn_per {
    int device;
    int64_t cap;
    int64_t row_bytes;
    int64_t pointer;    // SumTree.data_pointer
    int64_t num_items;  // SumTree.num_items (stores minus wraps)
    double* tree;       // [2*cap - 1]
    uint8_t* ring;      // [cap][row_bytes] or NULL
    uint32_t* owner;    // [cap] update claims, all 0 between calls
    double* part;       // [kPerPartials][2] leaf (min, max) per workgroup
};

namespace {

// (min, max) over the first `count` leaves into per->part; returns the pairs written
int per_reduce(sn_per* per, int64_t count, hipStream_t st) {
    int64_t nb = (count + 4 * kPerBlock - 1) / (4 * kPerBlock);
    nb = nb < 1 ? 1 : (nb > kPerPartials ? kPerPartials : nb);
    k_per_reduce<<<(unsigned)nb, kPerBlock, 0, st>>>(per->tree + (per->cap - 1), count, per->part);
    return (int)nb;
}

// every internal node = left + right, bottom levels first
void per_rebuild(sn_per* per, hipStream_t st) {
    int levels = 0;  // internal nodes 0 .. cap-2 span depths 0 .. levels-1
    while ((((int64_t)1 << levels) - 1) < per->cap - 1) levels++;
    int hi = levels;
    while (hi > 0) {
        const int d0 = hi > kPerLevels ? hi - kPerLevels : 0;
        const int64_t first = ((int64_t)1 << d0) - 1;
        int64_t roots = (int64_t)1 << d0;
        if (roots > per->cap - 1 - first) roots = per->cap - 1 - first;
        k_per_rebuild<<<(unsigned)roots, kPerBlock, 0, st>>>(per->tree, per->cap, d0, hi - d0);
        hi = d0;
    }
}

// all of per's slots from h source slots starting at src_first (k_per_inherit), then the internal nodes
sn_status per_load(sn_per* per, const double* src_leaves, const uint8_t* src_ring, int64_t cap_src,
                   int64_t src_first, int64_t h, hipStream_t st) {
    const int chunks = (int)(per->row_bytes / 16);
    const int64_t blocks = (per->cap * (chunks > 0 ? chunks : 1) + kPerBlock - 1) / kPerBlock;
    if (blocks > 0x7FFFFFFF) return set_error(SN_EUNSUPPORTED, "capacity x row pieces exceeds one launch");
    k_per_inherit<<<(unsigned)blocks, kPerBlock, 0, st>>>(per->tree, per->ring, per->cap, src_leaves, src_ring, cap_src,
                                                          src_first, h, chunks);
    per_rebuild(per, st);
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

}  // namespace

extern "C" {

sn_status sn_per_create(sn_per** out, int64_t capacity, int64_t row_bytes, int device) {
    if (!out) return set_error(SN_EINVAL, "out is NULL");
    *out = nullptr;
    if (capacity < 2) return set_error(SN_EINVAL, "capacity must be >= 2 (the reference cannot sample from one slot)");
    if (capacity > kPerMaxCapacity) return set_error(SN_EUNSUPPORTED, "capacity > 2^30");
    if (row_bytes < 0 || row_bytes % 16 != 0) return set_error(SN_EINVAL, "row_bytes must be 0 or a multiple of 16");
    if (row_bytes > (1 << 20)) return set_error(SN_EUNSUPPORTED, "row_bytes > 2^20");
    HIP_TRY(hipSetDevice(device));
    sn_per* p = new (std::nothrow) sn_per();
    if (!p) return set_error(SN_ENOMEM, "host allocation failed");
    p->device = device, p->cap = capacity, p->row_bytes = row_bytes;
    const size_t tree_bytes = sizeof(double) * (size_t)(2 * capacity - 1);
    bool ok = hipMalloc((void**)&p->tree, tree_bytes) == hipSuccess &&
              hipMalloc((void**)&p->owner, sizeof(uint32_t) * (size_t)capacity) == hipSuccess &&
              hipMalloc((void**)&p->part, sizeof(double) * 2 * kPerPartials) == hipSuccess &&
              (row_bytes == 0 || hipMalloc((void**)&p->ring, (size_t)capacity * (size_t)row_bytes) == hipSuccess);
    ok = ok && hipMemset(p->tree, 0, tree_bytes) == hipSuccess &&
         hipMemset(p->owner, 0, sizeof(uint32_t) * (size_t)capacity) == hipSuccess &&
         (row_bytes == 0 || hipMemset(p->ring, 0, (size_t)capacity * (size_t)row_bytes) == hipSuccess);
    if (!ok) {
        (void)hipGetLastError();
        sn_per_destroy(p);
        return set_error(SN_ENOMEM, "device allocation of the replay failed");
    }
    *out = p;
    return SN_OK;
}

sn_status sn_per_destroy(sn_per* per) {
    if (!per) return SN_OK;
    (void)hipSetDevice(per->device);
    if (per->tree) (void)hipFree(per->tree);
    if (per->owner) (void)hipFree(per->owner);
    if (per->part) (void)hipFree(per->part);
    if (per->ring) (void)hipFree(per->ring);
    delete per;
    return SN_OK;
}

sn_status sn_per_info(const sn_per* per, int64_t* capacity, int64_t* pointer, int64_t* num_items) {
    if (!per) return set_error(SN_EINVAL, "NULL argument");
    if (capacity) *capacity = per->cap;
    if (pointer) *pointer = per->pointer;
    if (num_items) *num_items = per->num_items;
    return SN_OK;
}

sn_status sn_per_store(sn_per* per, int64_t m, const void* rows, void* stream) {
    if (!per) return set_error(SN_EINVAL, "NULL argument");
    if (m < 1 || m > per->cap) return set_error(SN_EINVAL, "m must be in 1..capacity");
    if (rows && per->row_bytes == 0) return set_error(SN_EINVAL, "rows given to a replay without payload");
    if (((uintptr_t)rows & 15) != 0) return set_error(SN_EINVAL, "rows must be 16-byte aligned");
    HIP_TRY(hipSetDevice(per->device));
    hipStream_t st = (hipStream_t)stream;
    const int chunks = rows ? (int)(per->row_bytes / 16) : 0;
    const int nparts = per_reduce(per, per->cap, st);
    k_per_store<<<per_grid(m * (chunks > 0 ? chunks : 1)), kPerBlock, 0, st>>>(
        per->tree, per->ring, (const uint8_t*)rows, per->cap, per->pointer, m, chunks, per->part, nparts);
    per_rebuild(per, st);
    HIP_TRY(hipGetLastError());
    // SumTree.add x m (replay_buffer.py:98-104): a store that wraps the pointer does not count
    const int64_t end = per->pointer + m;
    const int64_t wraps = end >= per->cap ? 1 : 0;
    per->pointer = wraps ? end - per->cap : end;
    per->num_items += m - wraps;
    return SN_OK;
}

sn_status sn_per_sample(sn_per* per, int64_t n, const double* u, double beta, uint32_t* tree_idx, double* priority,
                        double* is_weight, void* rows_out, void* stream) {
    if (!per || !u || !tree_idx) return set_error(SN_EINVAL, "NULL argument");
    if (n < 1 || n > 0x7FFFFFFF) return set_error(SN_EINVAL, "n must be in 1..2^31-1");
    if (per->num_items < 1) return set_error(SN_EINVAL, "sample from an empty replay (the reference's np.min raises)");
    if (rows_out && per->row_bytes == 0) return set_error(SN_EINVAL, "rows_out given to a replay without payload");
    if (((uintptr_t)rows_out & 15) != 0) return set_error(SN_EINVAL, "rows_out must be 16-byte aligned");
    HIP_TRY(hipSetDevice(per->device));
    hipStream_t st = (hipStream_t)stream;
    const int64_t counted = per->num_items < per->cap ? per->num_items : per->cap;
    const int nparts = per_reduce(per, counted, st);
    k_per_sample<<<per_grid(n), kPerBlock, 0, st>>>(per->tree, per->ring, per->cap, n, u, beta, tree_idx, priority,
                                                    is_weight, (uint8_t*)rows_out,
                                                    rows_out ? (int)(per->row_bytes / 16) : 0, per->part, nparts);
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

sn_status sn_per_gather(sn_per* per, int64_t n, const int32_t* slots, void* rows_out, void* stream) {
    if (!per || !slots || !rows_out) return set_error(SN_EINVAL, "NULL argument");
    if (per->row_bytes == 0) return set_error(SN_EINVAL, "gather from a replay without payload");
    if (n < 1 || n > 0x7FFFFFFF) return set_error(SN_EINVAL, "n must be in 1..2^31-1");
    if (((uintptr_t)rows_out & 15) != 0) return set_error(SN_EINVAL, "rows_out must be 16-byte aligned");
    HIP_TRY(hipSetDevice(per->device));
    const int chunks = (int)(per->row_bytes / 16);
    k_per_gather<<<per_grid(n * chunks), kPerBlock, 0, (hipStream_t)stream>>>(per->ring, per->cap, n, slots,
                                                                             (uint8_t*)rows_out, chunks);
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

sn_status sn_per_update(sn_per* per, int64_t n, const uint32_t* tree_idx, const double* abs_err, double eps,
                        double upper, double alpha, void* stream) {
    if (!per || !tree_idx || !abs_err) return set_error(SN_EINVAL, "NULL argument");
    if (n < 1 || n > 0x7FFFFFFF) return set_error(SN_EINVAL, "n must be in 1..2^31-1");
    HIP_TRY(hipSetDevice(per->device));
    hipStream_t st = (hipStream_t)stream;
    k_per_claim<<<per_grid(n), kPerBlock, 0, st>>>(per->owner, per->cap, n, tree_idx);
    k_per_write<<<per_grid(n), kPerBlock, 0, st>>>(per->tree, per->owner, per->cap, n, tree_idx, abs_err, eps, upper,
                                                   alpha);
    per_rebuild(per, st);
    HIP_TRY(hipGetLastError());
    return SN_OK;
}

sn_status sn_per_tree(sn_per* per, double* tree_out, void* stream) {
    if (!per || !tree_out) return set_error(SN_EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(per->device));
    HIP_TRY(hipMemcpyAsync(tree_out, per->tree, sizeof(double) * (size_t)(2 * per->cap - 1), hipMemcpyDeviceToDevice,
                           (hipStream_t)stream));
    return SN_OK;
}

sn_status sn_per_inherit(sn_per* dst, const sn_per* src, void* stream) {
    if (!dst || !src) return set_error(SN_EINVAL, "NULL argument");
    if (dst == src) return set_error(SN_EINVAL, "a replay cannot inherit from itself");
    if (dst->row_bytes != src->row_bytes) return set_error(SN_EINVAL, "row_bytes of parent and child differ");
    if (dst->device != src->device) return set_error(SN_EINVAL, "parent and child live on different devices");
    HIP_TRY(hipSetDevice(dst->device));
    const double* leaves = src->tree + (src->cap - 1);
    if (dst->cap == src->cap) {  // verbatim: every slot stays where it is, and so do the counters
        const sn_status s = per_load(dst, leaves, src->ring, src->cap, 0, src->cap, (hipStream_t)stream);
        if (s != SN_OK) return s;
        dst->pointer = src->pointer, dst->num_items = src->num_items;
        return SN_OK;
    }
    // re-home the newest rows, oldest first.  The ring has wrapped exactly when num_items != pointer:
    // before the first wrap both count the stores, from then on they differ by (capacity - 1) x wraps.
    const int64_t held = src->num_items != src->pointer ? src->cap : src->pointer;
    const int64_t h = held < dst->cap ? held : dst->cap;
    int64_t first = src->pointer - h;
    if (first < 0) first += src->cap;
    const sn_status s = per_load(dst, leaves, src->ring, src->cap, first, h, (hipStream_t)stream);
    if (s != SN_OK) return s;
    // the counters of h stores into an empty ring (sn_per_store)
    dst->pointer = h == dst->cap ? 0 : h;
    dst->num_items = h - (h == dst->cap ? 1 : 0);
    return SN_OK;
}

sn_status sn_per_import(sn_per* dst, const double* leaves, const void* rows, int64_t pointer, int64_t num_items,
                        void* stream) {
    if (!dst || !leaves) return set_error(SN_EINVAL, "NULL argument");
    if ((rows == nullptr) != (dst->row_bytes == 0))
        return set_error(SN_EINVAL, "rows must be NULL exactly for a replay without payload");
    if (((uintptr_t)rows & 15) != 0) return set_error(SN_EINVAL, "rows must be 16-byte aligned");
    if (((uintptr_t)leaves & 7) != 0) return set_error(SN_EINVAL, "leaves must be 8-byte aligned");
    if (pointer < 0 || pointer >= dst->cap) return set_error(SN_EINVAL, "pointer must be in 0..capacity-1");
    if (num_items < 0) return set_error(SN_EINVAL, "num_items must be >= 0");
    HIP_TRY(hipSetDevice(dst->device));
    const sn_status s = per_load(dst, leaves, (const uint8_t*)rows, dst->cap, 0, dst->cap, (hipStream_t)stream);
    if (s != SN_OK) return s;
    dst->pointer = pointer, dst->num_items = num_items;
    return SN_OK;
}

}  // extern "C"
