// dca_hcache.hip — device-resident heuristic cache of the AVI update step (include/dca.h "heuristic cache"): an open-addressed
// table keyed by the uint8 network-input row, so that the target network evaluates every distinct child state once.
//
// Reference behaviour restated (paths relative to forestagostinelli/DeepCubeA): updaters/updater.py:11-54 hands ALL n x moves
// children of a batch to the heuristic queues (utils/search_utils.py:16-32 bellman); many are the same state.  A heuristic
// that is a function of the row alone (the fp32 parity network: same bits in any batch, row or chunking) may be memoised
// without changing a single target.
//
// Table (caller-owned, 16-byte aligned, dca_hcache_bytes() bytes; all zero = empty):
//   [0, 64)    header: word 0 = slots in use (uint32)
//   tags       uint64 [slots]          dca_hash64 of the slot's row, 0 = empty
//   claim      uint64 [slots]          id of the lookup call that claimed the slot
//   vals       uint64 [slots]          bit 32 = "a value was stored", low word = the float's bits
//   keys       uint64 [slots][kw]      the row itself, kw = ceil(row_bytes / 8) little-endian words, zero padded
//
// No thread ever waits for another thread's write: a lookup is two launches (claim, then resolve — the key bytes a claim
// writes are read only after the kernel boundary), a finish is two launches (store, then fill the duplicates).  Every loop has
// a fixed bound; the only atomics are the 64-bit compare-and-swap on a tag and the 32-bit add on the fill count.
#include "dca_common.h"

#include <atomic>

namespace dca {

constexpr int kHcThreads = 256;
constexpr int kHcProbes = 32;
constexpr int kHcMaxBlocks = 8192;
constexpr uint64_t kHcValid = 1ull << 32;
constexpr int64_t kHcHeader = 64;

struct HcTable {
    uint32_t* used;
    uint64_t* tags;
    uint64_t* claim;
    uint64_t* vals;
    uint64_t* keys;
    int kw;
};

static HcTable hc_view(void* table, int row_bytes, int64_t slots) {
    HcTable t;
    uint8_t* p = (uint8_t*)table;
    t.kw = (row_bytes + 7) / 8;
    t.used = (uint32_t*)p;
    t.tags = (uint64_t*)(p + kHcHeader);
    t.claim = t.tags + slots;
    t.vals = t.claim + slots;
    t.keys = t.vals + slots;
    return t;
}

// the row as 8 little-endian words, zero padded: W-byte loads (W = what the base pointer and the row stride are both
// multiples of) for the whole units, single bytes for the tail — the tail lies inside one word because W divides 8
template <int W>
__device__ __forceinline__ void hc_load_row(const uint8_t* __restrict__ p, int rb, uint64_t (&w)[8]) {
    const int full = rb / W * W;
#pragma unroll
    for (int q = 0; q < 8; q++) w[q] = 0;
#pragma unroll
    for (int k = 0; k < 64; k += W) {
        if (k + W <= rb) {
            uint64_t v;
            if constexpr (W == 8) v = *(const uint64_t*)(p + k);
            else if constexpr (W == 4) v = *(const uint32_t*)(p + k);
            else if constexpr (W == 2) v = *(const uint16_t*)(p + k);
            else v = p[k];
            w[k >> 3] |= v << (8 * (k & 7));
        }
    }
    if constexpr (W > 1) {
        uint64_t tail = 0;
#pragma unroll
        for (int j = 0; j < W - 1; j++) {
            const int k = full + j;
            if (k < rb) tail |= (uint64_t)p[k] << (8 * (k & 7));
        }
        const int tw = full >> 3;
#pragma unroll
        for (int q = 0; q < 8; q++)
            if (q == tw) w[q] |= tail;
    }
}

__device__ __forceinline__ uint64_t hc_hash(const uint64_t (&w)[8], int rb, int kw) {
    uint64_t h = hash_init(rb);
#pragma unroll
    for (int q = 0; q < 8; q++)
        if (q < kw) h = hash_word(h, w[q]);
    return hash_final(h);
}

// launch 1 of a lookup: find the row's slot by its tag, or claim an empty one.  Leaves status = EVAL_STORE (this row claimed
// the slot and wrote the key), DUP (a slot with the row's tag exists: resolved by launch 2) or EVAL_ONLY.
template <int W>
__global__ __launch_bounds__(kHcThreads) void hc_claim_kernel(HcTable t, int rb, int64_t slots, const uint8_t* __restrict__ rows,
                                                              int64_t n, int64_t ld, uint64_t call, int32_t* __restrict__ slot,
                                                              uint8_t* __restrict__ status) {
    const uint64_t mask = (uint64_t)slots - 1;
    const uint32_t limit = (uint32_t)(slots / 2);
    const int64_t stride = (int64_t)gridDim.x * kHcThreads;
    for (int64_t i = (int64_t)blockIdx.x * kHcThreads + threadIdx.x; i < n; i += stride) {
        uint64_t w[8];
        hc_load_row<W>(rows + i * ld, rb, w);
        const uint64_t h = hc_hash(w, rb, t.kw);
        int32_t found = -1;
        uint8_t st = DCA_HCACHE_EVAL_ONLY;
        if (h != 0) {  // 0 marks an empty slot: a row that hashes to it is never cached
            uint64_t s = h & mask;
            for (int p = 0; p < kHcProbes; p++) {
                uint64_t tg = __hip_atomic_load(t.tags + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (tg == 0) {
                    // fill limit: a place in the count is taken BEFORE the compare-and-swap and given back by a loser, so the
                    // count never passes slots / 2
                    if (__hip_atomic_load(t.used, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= limit) break;
                    if (atomicAdd(t.used, 1u) >= limit) {
                        atomicSub(t.used, 1u);
                        break;
                    }
                    tg = atomicCAS((unsigned long long*)(t.tags + s), 0ull, (unsigned long long)h);
                    if (tg == 0) {
                        uint64_t* key = t.keys + s * (uint64_t)t.kw;
#pragma unroll
                        for (int q = 0; q < 8; q++)
                            if (q < t.kw) key[q] = w[q];
                        t.claim[s] = call;
                        found = (int32_t)s;
                        st = DCA_HCACHE_EVAL_STORE;
                        break;
                    }
                    atomicSub(t.used, 1u);
                }
                if (tg == h) {
                    found = (int32_t)s;
                    st = DCA_HCACHE_DUP;
                    break;
                }
                s = (s + 1) & mask;
            }
        }
        slot[i] = found;
        status[i] = st;
    }
}

// launch 2 of a lookup: the rows that found their tag compare their bytes with the slot's key and read its value
template <int W>
__global__ __launch_bounds__(kHcThreads) void hc_resolve_kernel(HcTable t, int rb, int64_t slots, const uint8_t* __restrict__ rows,
                                                                int64_t n, int64_t ld, uint64_t call, float* __restrict__ h,
                                                                int32_t* __restrict__ slot, uint8_t* __restrict__ status) {
    const int64_t stride = (int64_t)gridDim.x * kHcThreads;
    for (int64_t i = (int64_t)blockIdx.x * kHcThreads + threadIdx.x; i < n; i += stride) {
        if (status[i] != DCA_HCACHE_DUP) continue;
        const int64_t s = slot[i];
        bool same = s >= 0 && s < slots;
        if (same) {
            uint64_t w[8];
            hc_load_row<W>(rows + i * ld, rb, w);
            const uint64_t* key = t.keys + s * t.kw;
#pragma unroll
            for (int q = 0; q < 8; q++)
                if (q < t.kw) same = same && key[q] == w[q];
        }
        if (same) {
            const uint64_t v = t.vals[s];
            if (v & kHcValid) {
                h[i] = __uint_as_float((uint32_t)v);
                status[i] = DCA_HCACHE_HIT;
                continue;
            }
            if (t.claim[s] == call) continue;  // DUP of an EVAL_STORE row of this call
        }
        // other bytes under the same tag, or a key an earlier call claimed and never stored
        slot[i] = -1;
        status[i] = DCA_HCACHE_EVAL_ONLY;
    }
}

__global__ __launch_bounds__(kHcThreads) void hc_store_kernel(HcTable t, int64_t slots, int64_t n, const int32_t* __restrict__ slot,
                                                              const uint8_t* __restrict__ status, const float* __restrict__ h) {
    const int64_t stride = (int64_t)gridDim.x * kHcThreads;
    for (int64_t i = (int64_t)blockIdx.x * kHcThreads + threadIdx.x; i < n; i += stride) {
        if (status[i] != DCA_HCACHE_EVAL_STORE) continue;
        const int64_t s = slot[i];
        if (s < 0 || s >= slots) continue;
        if (t.tags[s] == 0) continue;  // not a claimed slot: nothing a lookup handed out
        t.vals[s] = kHcValid | (uint64_t)__float_as_uint(h[i]);
    }
}

__global__ __launch_bounds__(kHcThreads) void hc_fill_kernel(HcTable t, int64_t slots, int64_t n, const int32_t* __restrict__ slot,
                                                             const uint8_t* __restrict__ status, float* __restrict__ h) {
    const int64_t stride = (int64_t)gridDim.x * kHcThreads;
    for (int64_t i = (int64_t)blockIdx.x * kHcThreads + threadIdx.x; i < n; i += stride) {
        if (status[i] != DCA_HCACHE_DUP) continue;
        const int64_t s = slot[i];
        uint64_t v = 0;
        if (s >= 0 && s < slots) v = t.vals[s];
        h[i] = (v & kHcValid) ? __uint_as_float((uint32_t)v) : __uint_as_float(0x7FC00000u);  // never stored: NaN, loudly
    }
}

static std::atomic<uint64_t> g_hc_call{1};

static int hc_check_table(const void* table, int row_bytes, int64_t slots) {
    DCA_ARG(row_bytes >= 1 && row_bytes <= 64);
    DCA_ARG(slots >= 2 && slots <= ((int64_t)1 << 30) && (slots & (slots - 1)) == 0);
    DCA_ARG(table != nullptr && ((uintptr_t)table & 15) == 0);
    return 0;
}

static unsigned hc_blocks(int64_t n) {
    const int64_t b = (n + kHcThreads - 1) / kHcThreads;
    return (unsigned)(b < kHcMaxBlocks ? b : kHcMaxBlocks);
}

template <int W>
static int hc_lookup_launch(const HcTable& t, int rb, int64_t slots, const uint8_t* rows, int64_t n, int64_t ld, uint64_t call,
                            float* h, int32_t* slot, uint8_t* status, hipStream_t st) {
    hipLaunchKernelGGL(hc_claim_kernel<W>, dim3(hc_blocks(n)), dim3(kHcThreads), 0, st, t, rb, slots, rows, n, ld, call, slot, status);
    if (int rc = launch_check("hc_claim_kernel")) return rc;
    hipLaunchKernelGGL(hc_resolve_kernel<W>, dim3(hc_blocks(n)), dim3(kHcThreads), 0, st, t, rb, slots, rows, n, ld, call, h, slot,
                       status);
    return launch_check("hc_resolve_kernel");
}

}  // namespace dca

using namespace dca;

extern "C" {

int64_t dca_hcache_bytes(int row_bytes, int64_t slots) {
    if (row_bytes < 1 || row_bytes > 64 || slots < 2 || slots > ((int64_t)1 << 30) || (slots & (slots - 1)) != 0) {
        set_error("dca_hcache_bytes: row_bytes %d not in 1..64 or slots %lld not a power of two in 2..2^30", row_bytes, (long long)slots);
        return DCA_E_BADARG;
    }
    return kHcHeader + slots * (int64_t)(24 + 8 * ((row_bytes + 7) / 8));
}

int dca_hcache_clear(void* table, int row_bytes, int64_t slots, void* stream) {
    if (int rc = hc_check_table(table, row_bytes, slots)) return rc;
    DCA_HIP(hipMemsetAsync(table, 0, (size_t)dca_hcache_bytes(row_bytes, slots), (hipStream_t)stream));
    return 0;
}

int dca_hcache_lookup(void* table, int row_bytes, int64_t slots, const uint8_t* rows, int64_t n, int64_t ld, float* h, int32_t* slot,
                      uint8_t* status, void* stream) {
    DCA_ARG(row_bytes >= 1 && row_bytes <= 64);
    DCA_ARG(slots >= 2 && slots <= ((int64_t)1 << 30) && (slots & (slots - 1)) == 0);
    DCA_ARG(n >= 0 && n < ((int64_t)1 << 31));
    DCA_ARG(ld >= row_bytes);
    if (int rc = hc_check_table(table, row_bytes, slots)) return rc;
    if (n == 0) return 0;
    DCA_ARG(rows && h && slot && status);
    DCA_ARG(((uintptr_t)h & 3) == 0 && ((uintptr_t)slot & 3) == 0);
    const HcTable t = hc_view(table, row_bytes, slots);
    const uint64_t call = g_hc_call.fetch_add(1);
    const uintptr_t al = (uintptr_t)rows | (uintptr_t)ld;
    hipStream_t st = (hipStream_t)stream;
    if ((al & 7) == 0) return hc_lookup_launch<8>(t, row_bytes, slots, rows, n, ld, call, h, slot, status, st);
    if ((al & 3) == 0) return hc_lookup_launch<4>(t, row_bytes, slots, rows, n, ld, call, h, slot, status, st);
    if ((al & 1) == 0) return hc_lookup_launch<2>(t, row_bytes, slots, rows, n, ld, call, h, slot, status, st);
    return hc_lookup_launch<1>(t, row_bytes, slots, rows, n, ld, call, h, slot, status, st);
}

int dca_hcache_finish(void* table, int row_bytes, int64_t slots, int64_t n, const int32_t* slot, const uint8_t* status, float* h,
                      void* stream) {
    DCA_ARG(row_bytes >= 1 && row_bytes <= 64);
    DCA_ARG(slots >= 2 && slots <= ((int64_t)1 << 30) && (slots & (slots - 1)) == 0);
    DCA_ARG(n >= 0 && n < ((int64_t)1 << 31));
    if (int rc = hc_check_table(table, row_bytes, slots)) return rc;
    if (n == 0) return 0;
    DCA_ARG(slot && status && h);
    DCA_ARG(((uintptr_t)h & 3) == 0 && ((uintptr_t)slot & 3) == 0);
    const HcTable t = hc_view(table, row_bytes, slots);
    hipLaunchKernelGGL(hc_store_kernel, dim3(hc_blocks(n)), dim3(kHcThreads), 0, (hipStream_t)stream, t, slots, n, slot, status, h);
    if (int rc = launch_check("hc_store_kernel")) return rc;
    hipLaunchKernelGGL(hc_fill_kernel, dim3(hc_blocks(n)), dim3(kHcThreads), 0, (hipStream_t)stream, t, slots, n, slot, status, h);
    return launch_check("hc_fill_kernel");
}

}  // extern "C"
