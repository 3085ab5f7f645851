// dca_pdb_puzzle.h — what the sliding-puzzle pattern-database code shares between dca_pdb.hip (build and eval kernels) and
// dca_idastar.hip (the IDA* search): the position compare sweep, the eval frame's row value and the entry points' checks.
// Header-only: every translation unit compiles its own copy, no device symbol crosses a translation unit.
#pragma once
#include "dca_pdb_shared.h"

namespace dca {

// ---------------------------------------------------------------------------------------------------------------- eval
// last position whose byte equals t, 0 if none (t < N is wave-uniform; a byte >= N equals no tile)
template <int N>
__host__ __device__ inline uint32_t pdb_find(const uint32_t (&w)[(N + 3) / 4], uint32_t t) {
    uint32_t pos = 0;
#pragma unroll
    for (int i = 0; i < N; i++) pos = ((w[i >> 2] >> (8 * (i & 3))) & 0xFFu) == t ? (uint32_t)i : pos;
    return pos;
}

// what pdb_eval_kernel / pdb_eval_launch (dca_pdb_shared.h) take for a DIM x DIM board
template <int DIM>
struct PdbEval {
    static constexpr int N = DIM * DIM;
    using Set = PdbSet;
    static constexpr const char* kernel_name = "pdb_eval_kernel";

    // one row's value: the sum over the set's patterns of table[blank + N (pos(tile 0) + N (pos(tile 1) + ...))]
    __host__ __device__ static inline uint32_t row_value(const uint32_t (&w)[(N + 3) / 4], const PdbSet& set) {
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
                    for (int j = k - 1; j >= 0; j--) idx = idx * N + pdb_find<N>(w, set.pat[pi].id[j]);  // every digit < N
                    idx = idx * N + blank;                                                               // < N^(k+1)
                    v[q] = set.table[pi][idx];
                }
            }
            sum += v[0] + v[1] + v[2] + v[3];
        }
        return sum;
    }
};

// ------------------------------------------------------------------------------------------------------ reflected eval
// The mirror in the main diagonal (include/dca.h "reflected look-up"): refl on positions, phi on tiles; both are involutions.
template <int DIM>
__host__ __device__ constexpr uint32_t pdb_refl(uint32_t p) {
    return (p % DIM) * DIM + p / DIM;
}
template <int DIM>
__host__ __device__ constexpr uint32_t pdb_phi(uint32_t t) {
    return t == 0u ? 0u : pdb_refl<DIM>(t - 1u) + 1u;
}

// Every tile's position at once, byte t of `pos` = pdb_find<N>(w, t): one pass over the row in ascending position, a later
// position overwriting an earlier one (the LAST position wins; 0 where no position holds t).  The word a byte goes to is picked
// by compares against constants, so `pos` stays in registers and no row byte forms an address; a byte >= N lands in no word or
// in the last word's padding, which nothing reads.
template <int N>
__host__ __device__ inline void pdb_positions(const uint32_t (&w)[(N + 3) / 4], uint32_t (&pos)[(N + 3) / 4]) {
    constexpr int NW = (N + 3) / 4;
#pragma unroll
    for (int q = 0; q < NW; q++) pos[q] = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
        const uint32_t b = (w[i >> 2] >> (8 * (i & 3))) & 0xFFu, sh = 8u * (b & 3u);
        const uint32_t keep = ~(0xFFu << sh), put = (uint32_t)i << sh;
#pragma unroll
        for (int q = 0; q < NW; q++) pos[q] = (b >> 2) == (uint32_t)q ? (pos[q] & keep) | put : pos[q];
    }
}

// byte t of `pos` (t < N is wave-uniform: the word is picked by uniform compares, not by an index into the registers)
template <int N>
__host__ __device__ inline uint32_t pdb_pos_of(const uint32_t (&pos)[(N + 3) / 4], uint32_t t) {
    uint32_t byte = 0;
#pragma unroll
    for (int q = 0; q < (N + 3) / 4; q++) byte |= (t >> 2) == (uint32_t)q ? (pos[q] >> (8u * (t & 3u))) & 0xFFu : 0u;
    return byte;
}

// The reflected family: the same tables read at the row and at its mirror image, the larger of the two sums.
template <int DIM>
struct PdbEvalReflect {
    static constexpr int N = DIM * DIM;
    using Set = PdbSet;
    static constexpr const char* kernel_name = "pdb_eval_kernel (reflected)";

    // max(sum_p table_p[index_p], sum_p table_p[reflected index_p]); the mirrored row holds phi(t) at refl(pos(t)), so its
    // digit for tile t is refl(pos(phi(t))) and its blank digit refl(pos(0)): every digit < N for ANY bytes, like the plain one
    __host__ __device__ static inline uint32_t row_value(const uint32_t (&w)[(N + 3) / 4], const PdbSet& set) {
        uint32_t pos[(N + 3) / 4];
        pdb_positions<N>(w, pos);
        const uint64_t blank = pdb_pos_of<N>(pos, 0u), rblank = pdb_refl<DIM>((uint32_t)blank);
        uint32_t sum = 0, rsum = 0;
        for (int p0 = 0; p0 < set.np; p0 += 4) {  // four patterns a trip: their eight gathers are independent, all in flight
            uint32_t v[4], r[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                v[q] = r[q] = 0;
                const int pi = p0 + q;
                if (pi < set.np) {
                    const int k = set.k[pi];
                    uint64_t idx = 0, ridx = 0;
                    for (int j = k - 1; j >= 0; j--) {
                        const uint32_t t = set.pat[pi].id[j];
                        idx = idx * N + pdb_pos_of<N>(pos, t);
                        ridx = ridx * N + pdb_refl<DIM>(pdb_pos_of<N>(pos, pdb_phi<DIM>(t)));
                    }
                    v[q] = set.table[pi][idx * N + blank];  // < N^(k+1)
                    r[q] = set.table[pi][ridx * N + rblank];
                }
            }
            sum += v[0] + v[1] + v[2] + v[3];
            rsum += r[0] + r[1] + r[2] + r[3];
        }
        return sum > rsum ? sum : rsum;
    }
};

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
