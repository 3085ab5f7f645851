// dca_pdb.hip — additive disjoint pattern databases for the sliding puzzles (include/dca.h "pattern databases"): the exact
// admissible, consistent heuristic the DeepCubeA paper measures its network against.  Two kernels:
//
//   build   fills one pattern's dense table [N^(k+1)] bytes with exact distances by relaxation sweeps.  One thread owns an entry:
//           it decodes the entry's digits (blank, then the k tile positions; the divisions are by the compile-time N) and PULLS
//           from the up-to-four entries one blank move away — a move that swaps the blank with a pattern tile costs 1, with an
//           invisible tile 0 — and writes only its own byte.  No read-modify-write atomics, no write race.  Sweeps update in
//           place: a value a neighbour lowered in the same sweep may or may not be seen, which changes how many sweeps it takes,
//           never the result — every value is an upper bound of the true distance at all times and only ever falls, and a sweep
//           that changes nothing has read a constant table, so every entry satisfies its Bellman equation: the unique fixed
//           point.  The host reads one "changed" word per sweep (this synchronises the stream).
//   eval    one thread per state row: the row's bytes in registers, then for every pattern tile t the LAST position p with
//           row[p] == t (0 if none; bytes >= N match no tile) by a compare sweep over the N positions — no array indexed by a
//           row byte, so nothing a row holds can form an address: every digit is < N and every index < N^(k+1) for ANY bytes.
//           One byte gather per pattern (up to four in flight), summed, written as fp32.
//
// What bounds either kernel has not been measured (profiles/pdb_probe.txt holds only wall-clock rates).
#include "dca_common.h"
#include "dca_pdb_row.h"

namespace dca {

constexpr int kPdbThreads = 256;
constexpr int kPdbMaxPatterns = 24;
constexpr int kPdbMaxK = 8;            // N^(k+1) <= 2^34 allows k = 8 on puzzle8 (all tiles), fewer on every larger board
constexpr int kPdbMaxBuildBlocks = 1 << 16;
constexpr int kPdbMaxEvalBlocks = 1 << 14;
constexpr int kPdbMaxSweeps = 1 << 16;
constexpr uint8_t kPdbNoState = 0xFF;  // two digits equal
constexpr uint8_t kPdbInf = 0xFE;      // a state the goal cannot be reached from (or: not reached yet, during the build)
constexpr int64_t kPdbMaxBytes = (int64_t)1 << 34;

struct PdbPattern {
    uint8_t tiles[kPdbMaxK];
};

struct PdbSet {
    const uint8_t* table[kPdbMaxPatterns];
    PdbPattern pat[kPdbMaxPatterns];
    uint8_t k[kPdbMaxPatterns];
    int np;
};

// ---------------------------------------------------------------------------------------------------------------- build
// entry -> 0xFF (two digits equal), 0 (the goal: tile t at t - 1, blank at N - 1) or "not reached yet"
template <int DIM>
__host__ __device__ inline uint8_t pdb_init_value(uint64_t e, int k, const PdbPattern& pat) {
    constexpr uint64_t N = DIM * DIM;
    uint64_t r = e;
    const uint32_t blank = (uint32_t)(r % N);
    r /= N;
    uint64_t seen = 1ull << blank;
    bool distinct = true, goal = blank == N - 1;
#pragma unroll
    for (int j = 0; j < kPdbMaxK; j++)
        if (j < k) {
            const uint32_t p = (uint32_t)(r % N);
            r /= N;
            distinct = distinct && !((seen >> p) & 1);
            seen |= 1ull << p;
            goal = goal && p == (uint32_t)pat.tiles[j] - 1u;
        }
    return !distinct ? kPdbNoState : goal ? (uint8_t)0 : kPdbInf;
}

template <int DIM>
__global__ __launch_bounds__(kPdbThreads) void pdb_init_kernel(uint8_t* __restrict__ table, uint64_t total, int k, PdbPattern pat) {
    const uint64_t stride = (uint64_t)gridDim.x * kPdbThreads;
    for (uint64_t e = (uint64_t)blockIdx.x * kPdbThreads + threadIdx.x; e < total; e += stride) table[e] = pdb_init_value<DIM>(e, k, pat);
}

// One entry's relaxation: the smallest of its own value `cur` and its blank-move neighbours' values plus the move's cost.
// Neighbour bytes are read while other threads may lower them: relaxed byte loads / stores (a byte never tears), see the file
// comment for why the fixed point does not depend on what a racing read returns.
template <int DIM>
__host__ __device__ inline uint32_t pdb_relax(const uint8_t* table, uint64_t e, int k, uint32_t cur) {
    constexpr uint64_t N = DIM * DIM;
    uint64_t r = e;
    const int blank = (int)(r % N);
    r /= N;
    uint32_t pos[kPdbMaxK];
#pragma unroll
    for (int j = 0; j < kPdbMaxK; j++) {
        pos[j] = 0xFFFFFFFFu;
        if (j < k) {
            pos[j] = (uint32_t)(r % N);
            r /= N;
        }
    }
    uint32_t best = cur;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const int nb = npuzzle_swap(DIM, blank, a);
        if (nb == blank) continue;
        // the neighbour: blank digit blank -> nb; if pattern tile j stands on nb its digit goes nb -> blank, and the move costs 1
        int64_t delta = (int64_t)nb - blank;
        uint32_t cost = 0;
        uint64_t w = N;
#pragma unroll
        for (int j = 0; j < kPdbMaxK; j++) {
            if (pos[j] == (uint32_t)nb) {
                delta += (int64_t)w * ((int64_t)blank - nb);
                cost = 1;
            }
            w *= N;
        }
        const uint64_t ne = (uint64_t)((int64_t)e + delta);  // the entry's digits, two of them exchanged: every digit < N, ne < N^(k+1)
        const uint32_t v = __hip_atomic_load(table + ne, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v < kPdbInf && v + cost < best) best = v + cost;
    }
    return best;
}

template <int DIM>
__global__ __launch_bounds__(kPdbThreads) void pdb_sweep_kernel(uint8_t* table, uint64_t total, int k, uint32_t* __restrict__ changed) {
    const uint64_t stride = (uint64_t)gridDim.x * kPdbThreads;
    bool any = false;
    for (uint64_t e = (uint64_t)blockIdx.x * kPdbThreads + threadIdx.x; e < total; e += stride) {
        const uint32_t cur = __hip_atomic_load(table + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kPdbNoState || cur == 0) continue;
        const uint32_t best = pdb_relax<DIM>(table, e, k, cur);
        if (best < cur) {
            __hip_atomic_store(table + e, (uint8_t)best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            any = true;
        }
    }
    if (any) __hip_atomic_store(changed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

static unsigned pdb_blocks(uint64_t n, int cap) {
    const uint64_t b = (n + kPdbThreads - 1) / kPdbThreads;
    return (unsigned)(b < (uint64_t)cap ? b : (uint64_t)cap);
}

template <int DIM>
static int pdb_build_launch(uint8_t* table, uint64_t total, int k, const PdbPattern& pat, int* sweeps, hipStream_t st) {
    uint32_t* changed = nullptr;
    DCA_HIP(hipMalloc((void**)&changed, sizeof(uint32_t)));
    const unsigned blocks = pdb_blocks(total, kPdbMaxBuildBlocks);
    int rc = 0, done = 0;
    hipLaunchKernelGGL(pdb_init_kernel<DIM>, dim3(blocks), dim3(kPdbThreads), 0, st, table, total, k, pat);
    rc = launch_check("pdb_init_kernel");
    bool fixed = false;
    while (rc == 0 && !fixed && done < kPdbMaxSweeps) {
        uint32_t flag = 0;
        hipError_t e = hipMemsetAsync(changed, 0, sizeof(uint32_t), st);
        if (e != hipSuccess) {
            rc = hip_fail(e, "hipMemsetAsync(pdb changed flag)");
            break;
        }
        hipLaunchKernelGGL(pdb_sweep_kernel<DIM>, dim3(blocks), dim3(kPdbThreads), 0, st, table, total, k, changed);
        if ((rc = launch_check("pdb_sweep_kernel")) != 0) break;
        e = hipMemcpyAsync(&flag, changed, sizeof(uint32_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            rc = hip_fail(e, "pdb changed flag read-back");
            break;
        }
        done++;
        fixed = flag == 0;
    }
    (void)hipFree(changed);
    if (rc == 0 && !fixed) {
        set_error("dca_pdb_build: no fixed point after %d sweeps", done);
        return DCA_E_STATE;
    }
    if (rc == 0 && sweeps) *sweeps = done;
    return rc;
}

// ---------------------------------------------------------------------------------------------------------------- eval
// (the row load, pdb_load_row, is shared with the cube3 tables: dca_pdb_row.h)
// last position whose byte equals t, 0 if none (t < N is wave-uniform; a byte >= N equals no tile)
template <int N>
__host__ __device__ inline uint32_t pdb_find(const uint32_t (&w)[(N + 3) / 4], uint32_t t) {
    uint32_t pos = 0;
#pragma unroll
    for (int i = 0; i < N; i++) pos = ((w[i >> 2] >> (8 * (i & 3))) & 0xFFu) == t ? (uint32_t)i : pos;
    return pos;
}

// one row's value: the sum over the set's patterns of table[blank + N (pos(tile 0) + N (pos(tile 1) + ...))]
template <int N>
__host__ __device__ inline uint32_t pdb_row_value(const uint32_t (&w)[(N + 3) / 4], const PdbSet& set) {
    const uint64_t blank = pdb_find<N>(w, 0u);
    uint32_t sum = 0;
    for (int p0 = 0; p0 < set.np; p0 += 4) {  // four independent gathers in flight
        uint32_t v[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            v[q] = 0;
            const int pi = p0 + q;
            if (pi < set.np) {
                const int k = set.k[pi];
                uint64_t idx = 0;
                for (int j = k - 1; j >= 0; j--) idx = idx * N + pdb_find<N>(w, set.pat[pi].tiles[j]);  // every digit < N
                idx = idx * N + blank;                                                                    // < N^(k+1)
                v[q] = set.table[pi][idx];
            }
        }
        sum += v[0] + v[1] + v[2] + v[3];
    }
    return sum;
}

template <int DIM, int W>
__global__ __launch_bounds__(kPdbThreads) void pdb_eval_kernel(const uint8_t* __restrict__ states, int64_t n, int64_t ld, PdbSet set,
                                                               float* __restrict__ out) {
    constexpr int N = DIM * DIM;
    const int64_t stride = (int64_t)gridDim.x * kPdbThreads;
    for (int64_t i = (int64_t)blockIdx.x * kPdbThreads + threadIdx.x; i < n; i += stride) {
        uint32_t w[(N + 3) / 4];
        pdb_load_row<N, W>(states + i * ld, w);
        out[i] = (float)pdb_row_value<N>(w, set);  // <= 24 * 255: exact
    }
}

template <int DIM>
static int pdb_eval_launch(const uint8_t* states, int64_t n, int64_t ld, const PdbSet& set, float* out, hipStream_t st) {
    const unsigned blocks = pdb_blocks((uint64_t)n, kPdbMaxEvalBlocks);
    if ((((uintptr_t)states | (uintptr_t)ld) & 3) == 0)
        hipLaunchKernelGGL((pdb_eval_kernel<DIM, 4>), dim3(blocks), dim3(kPdbThreads), 0, st, states, n, ld, set, out);
    else
        hipLaunchKernelGGL((pdb_eval_kernel<DIM, 1>), dim3(blocks), dim3(kPdbThreads), 0, st, states, n, ld, set, out);
    return launch_check("pdb_eval_kernel");
}

// N^(k+1), or a negative code with the message set
static int64_t pdb_bytes_checked(const char* who, int dim, int k) {
    if (dim < 3 || dim > 7) {
        set_error("bad argument: %s: dim: unsupported puzzle dim %d (3..7)", who, dim);
        return DCA_E_BADARG;
    }
    const int N = dim * dim;
    if (k < 1 || k > N - 1) {
        set_error("bad argument: %s: k = %d is not in 1..%d", who, k, N - 1);
        return DCA_E_BADARG;
    }
    int64_t b = N;
    for (int j = 0; j < k; j++) {
        b *= N;
        if (b > kPdbMaxBytes) {
            set_error("bad argument: %s: k = %d: a table of %d^%d bytes is over the 2^34 limit", who, k, N, k + 1);
            return DCA_E_BADARG;
        }
    }
    return b;
}

static int pdb_check_tiles(const char* who, int N, const uint8_t* tiles, int k, uint64_t& seen) {
    for (int j = 0; j < k; j++) {
        const int t = tiles[j];
        if (t < 1 || t > N - 1) {
            set_error("bad argument: %s: tiles: tile %d is not in 1..%d", who, t, N - 1);
            return DCA_E_BADARG;
        }
        if ((seen >> t) & 1) {
            set_error("bad argument: %s: tiles: tile %d appears twice", who, t);
            return DCA_E_BADARG;
        }
        seen |= 1ull << t;
    }
    return 0;
}

}  // namespace dca

using namespace dca;

extern "C" {

int64_t dca_pdb_bytes(int dim, int k) { return pdb_bytes_checked("dca_pdb_bytes", dim, k); }

int dca_pdb_build(int dim, const uint8_t* tiles, int k, uint8_t* table, int* sweeps, void* stream) {
    const int64_t total = pdb_bytes_checked(__func__, dim, k);
    if (total < 0) return (int)total;
    DCA_ARG(k <= kPdbMaxK);
    DCA_ARG(tiles != nullptr);
    DCA_ARG(table != nullptr);
    uint64_t seen = 0;
    if (int rc = pdb_check_tiles(__func__, dim * dim, tiles, k, seen)) return rc;
    PdbPattern pat{};
    for (int j = 0; j < k; j++) pat.tiles[j] = tiles[j];
    hipStream_t st = (hipStream_t)stream;
    switch (dim) {
        case 3: return pdb_build_launch<3>(table, (uint64_t)total, k, pat, sweeps, st);
        case 4: return pdb_build_launch<4>(table, (uint64_t)total, k, pat, sweeps, st);
        case 5: return pdb_build_launch<5>(table, (uint64_t)total, k, pat, sweeps, st);
        case 6: return pdb_build_launch<6>(table, (uint64_t)total, k, pat, sweeps, st);
        default: return pdb_build_launch<7>(table, (uint64_t)total, k, pat, sweeps, st);
    }
}

int dca_pdb_eval(int dim, const uint8_t* states, int64_t n, int64_t ld, int num_patterns, const uint8_t* tiles, const int* ks,
                 const uint8_t* const* tables, float* out, void* stream) {
    if (dim < 3 || dim > 7) {
        set_error("bad argument: %s: dim: unsupported puzzle dim %d (3..7)", __func__, dim);
        return DCA_E_BADARG;
    }
    const int N = dim * dim;
    DCA_ARG(n >= 0 && n < ((int64_t)1 << 31));
    DCA_ARG(ld >= N);
    DCA_ARG(num_patterns >= 1 && num_patterns <= 24);
    DCA_ARG(tiles != nullptr && ks != nullptr && tables != nullptr);
    PdbSet set{};
    set.np = num_patterns;
    uint64_t seen = 0;
    const uint8_t* t = tiles;
    for (int p = 0; p < num_patterns; p++) {
        const int64_t b = pdb_bytes_checked(__func__, dim, ks[p]);
        if (b < 0) return (int)b;
        if (int rc = pdb_check_tiles(__func__, N, t, ks[p], seen)) return rc;
        if (tables[p] == nullptr) {
            set_error("bad argument: %s: tables: table %d is NULL", __func__, p);
            return DCA_E_BADARG;
        }
        set.table[p] = tables[p];
        set.k[p] = (uint8_t)ks[p];
        for (int j = 0; j < ks[p]; j++) set.pat[p].tiles[j] = t[j];
        t += ks[p];
    }
    if (n == 0) return 0;
    DCA_ARG(states != nullptr && out != nullptr);
    DCA_ARG(((uintptr_t)out & 3) == 0);
    hipStream_t st = (hipStream_t)stream;
    switch (dim) {
        case 3: return pdb_eval_launch<3>(states, n, ld, set, out, st);
        case 4: return pdb_eval_launch<4>(states, n, ld, set, out, st);
        case 5: return pdb_eval_launch<5>(states, n, ld, set, out, st);
        case 6: return pdb_eval_launch<6>(states, n, ld, set, out, st);
        default: return pdb_eval_launch<7>(states, n, ld, set, out, st);
    }
}

}  // extern "C"
