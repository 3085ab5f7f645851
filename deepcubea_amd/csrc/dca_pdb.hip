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
//           The reflected family (PdbEvalReflect, dca_pdb_eval_reflected) reads the same tables at the row and at its mirror
//           image in the main diagonal and writes the larger sum; it derives every tile's position once, in one pass over the row.
//
// What bounds either kernel has not been measured (profiles/pdb_probe.txt and profiles/pdb_reflect_probe.txt hold only wall-clock rates).
#include "dca_pdb_puzzle.h"

namespace dca {

constexpr int kPdbMaxSweeps = 1 << 16;
constexpr uint8_t kPdbNoState = 0xFF;  // two digits equal

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
            goal = goal && p == (uint32_t)pat.id[j] - 1u;
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

template <int DIM>
static int pdb_build_launch(uint8_t* table, uint64_t total, int k, const PdbPattern& pat, int* sweeps, hipStream_t st) {
    const unsigned blocks = pdb_blocks(total, kPdbMaxBuildBlocks);
    hipLaunchKernelGGL(pdb_init_kernel<DIM>, dim3(blocks), dim3(kPdbThreads), 0, st, table, total, k, pat);
    int done = 0, rc = launch_check("pdb_init_kernel");
    if (rc == 0)
        rc = pdb_sweep_until_quiet(st, kPdbMaxSweeps, "dca_pdb_build", [&](int, uint32_t* changed) {
            hipLaunchKernelGGL(pdb_sweep_kernel<DIM>, dim3(blocks), dim3(kPdbThreads), 0, st, table, total, k, changed);
            return launch_check("pdb_sweep_kernel");
        }, done);
    if (rc == DCA_E_STATE) set_error("dca_pdb_build: no fixed point after %d sweeps", done);
    if (rc == 0 && sweeps) *sweeps = done;
    return rc;
}

// ---------------------------------------------------------------------------------------------------------------- eval
template <int DIM>
static int pdb_eval_run(const uint8_t* states, int64_t n, int64_t ld, const PdbSet& set, float* out, bool reflect, bool host, hipStream_t st) {
    if (host) {
        if (reflect)
            pdb_eval_rows_host<PdbEvalReflect<DIM>>(states, n, ld, set, out);
        else
            pdb_eval_rows_host<PdbEval<DIM>>(states, n, ld, set, out);
        return 0;
    }
    return reflect ? pdb_eval_launch<PdbEvalReflect<DIM>>(states, n, ld, set, out, st) : pdb_eval_launch<PdbEval<DIM>>(states, n, ld, set, out, st);
}

#define DCA_PDB_ARG(cond)                                      \
    do {                                                       \
        if (!(cond)) {                                         \
            set_error("bad argument: %s: %s", who, #cond);     \
            return DCA_E_BADARG;                               \
        }                                                      \
    } while (0)

// what the three eval entry points share: every refusal, before any HIP call, then the family's kernels or the host loop
static int pdb_eval_entry(const char* who, int dim, const uint8_t* states, int64_t n, int64_t ld, int num_patterns, const uint8_t* tiles,
                          const int* ks, const uint8_t* const* tables, float* out, bool reflect, bool host, hipStream_t st) {
    if (dim < 3 || dim > 7) {
        set_error("bad argument: %s: dim: unsupported puzzle dim %d (3..7)", who, dim);
        return DCA_E_BADARG;
    }
    const int N = dim * dim;
    DCA_PDB_ARG(n >= 0 && n < ((int64_t)1 << 31));
    DCA_PDB_ARG(ld >= N);
    DCA_PDB_ARG(num_patterns >= 1 && num_patterns <= 24);
    DCA_PDB_ARG(tiles != nullptr && ks != nullptr && tables != nullptr);
    PdbSet set{};
    uint64_t seen = 0;  // across the whole set: the patterns are disjoint
    if (int rc = pdb_fill_set(
            who, set, num_patterns, tiles, ks, tables, [&](int p) { return pdb_bytes_checked(who, dim, ks[p]); },
            [&](int p, const uint8_t* t) { return pdb_check_tiles(who, N, t, ks[p], seen); }))
        return rc;
    if (n == 0) return 0;
    DCA_PDB_ARG(states != nullptr && out != nullptr);
    DCA_PDB_ARG(((uintptr_t)out & 3) == 0);
    switch (dim) {
        case 3: return pdb_eval_run<3>(states, n, ld, set, out, reflect, host, st);
        case 4: return pdb_eval_run<4>(states, n, ld, set, out, reflect, host, st);
        case 5: return pdb_eval_run<5>(states, n, ld, set, out, reflect, host, st);
        case 6: return pdb_eval_run<6>(states, n, ld, set, out, reflect, host, st);
        default: return pdb_eval_run<7>(states, n, ld, set, out, reflect, host, st);
    }
}
#undef DCA_PDB_ARG

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
    const PdbPattern pat = pdb_pattern(tiles, k);
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
    return pdb_eval_entry(__func__, dim, states, n, ld, num_patterns, tiles, ks, tables, out, false, false, (hipStream_t)stream);
}

int dca_pdb_eval_reflected(int dim, const uint8_t* states, int64_t n, int64_t ld, int num_patterns, const uint8_t* tiles, const int* ks,
                           const uint8_t* const* tables, float* out, void* stream) {
    return pdb_eval_entry(__func__, dim, states, n, ld, num_patterns, tiles, ks, tables, out, true, false, (hipStream_t)stream);
}

int dca_pdb_eval_host(int dim, const uint8_t* states, int64_t n, int64_t ld, int num_patterns, const uint8_t* tiles, const int* ks,
                      const uint8_t* const* tables, int reflect, float* out) {
    return pdb_eval_entry(__func__, dim, states, n, ld, num_patterns, tiles, ks, tables, out, reflect != 0, true, nullptr);
}

}  // extern "C"
