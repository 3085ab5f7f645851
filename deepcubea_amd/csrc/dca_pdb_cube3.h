// dca_pdb_cube3.h — what the cube3 pattern-database code shares between dca_pdb_cube3.hip (build and eval kernels) and
// dca_idastar.hip (the IDA* search): the cubies derived at compile time, rank / unrank, the row -> locations rule, the eval
// frame's row value and the entry points' checks.  Header-only: every translation unit compiles its own copy, no device symbol
// crosses a translation unit.
#pragma once
#include "dca_pdb_shared.h"

namespace dca {

constexpr int kC3Locs = 24;       // n * o of either kind: 8 * 3 corners, 12 * 2 edges

template <int KIND>
struct C3Kind {
    static constexpr int n = KIND == DCA_CUBE3_CORNERS ? 8 : 12;
    static constexpr int o = KIND == DCA_CUBE3_CORNERS ? 3 : 2;
};

// ------------------------------------------------------------------------------------------------ cubies, at compile time
struct Cube3Cubies {
    uint8_t pos[2][kC3Locs];       // kind, slot * o + r -> sticker position
    uint8_t loc[54];               // sticker position -> slot * o + r within its kind (centres: 0xFF)
    uint8_t kind[54];              // sticker position -> 0 corner, 1 edge, 2 centre
    uint8_t move[2][12][kC3Locs];  // kind, move, location -> location after the move
    uint8_t colours[2][12];        // kind, cubie -> its colour set, bit c = colour c (position / 9)
    int count[2];
};

constexpr Cube3Cubies make_cube3_cubies() {
    Cube3Cubies c{};
    uint32_t moved[54] = {};
    for (int a = 0; a < 12; a++)
        for (int i = 0; i < 54; i++)
            if (kCube3Perm.p[a][i] != i) moved[i] |= 1u << a;
    bool done[54] = {};
    for (int i = 0; i < 54; i++) {
        if (done[i]) continue;
        int members[6] = {}, m = 0;  // the positions the same moves displace, ascending
        for (int q = i; q < 54; q++)
            if (moved[q] == moved[i]) {
                if (m < 6) members[m] = q;
                m++;
            }
        const int kind = m == 3 ? DCA_CUBE3_CORNERS : m == 2 ? DCA_CUBE3_EDGES : 2;
        const int slot = kind < 2 ? c.count[kind]++ : 0;
        for (int x = 0; x < m && x < 6; x++) {
            const int q = members[x];
            done[q] = true;
            c.kind[q] = (uint8_t)kind;
            c.loc[q] = kind < 2 ? (uint8_t)(slot * m + x) : (uint8_t)0xFF;
            if (kind < 2 && slot < 12) {
                c.pos[kind][slot * m + x] = (uint8_t)q;
                c.colours[kind][slot] |= (uint8_t)(1u << (q / 9));
            }
        }
    }
    // next[i] = cur[perm[a][i]]: the facelet at position perm[a][i] goes to position i
    for (int a = 0; a < 12; a++)
        for (int i = 0; i < 54; i++)
            if (c.kind[i] < 2) c.move[c.kind[i]][a][c.loc[kCube3Perm.p[a][i]]] = c.loc[i];
    return c;
}
inline constexpr Cube3Cubies kC3 = make_cube3_cubies();
static_assert(kC3.count[0] == 8 && kC3.count[1] == 12, "cube3: 8 corner and 12 edge cubies");
static_assert(kC3.pos[0][0] == 0 && kC3.pos[0][1] == 26 && kC3.pos[0][2] == 47 && kC3.pos[0][21] == 17 && kC3.pos[0][23] == 51,
              "corner lists");
static_assert(kC3.pos[1][0] == 1 && kC3.pos[1][1] == 23 && kC3.pos[1][22] == 34 && kC3.pos[1][23] == 37, "edge lists");

struct C3Set : PdbTables {
    uint8_t kind[kPdbMaxPatterns];
    int np;
    int kinds_used;  // bit kind = some pattern is of that kind
};

struct C3MoveTable {
    uint32_t w[12 * kC3Locs / 4];  // move[kind] as words: the kernels stage it in LDS
};

// ------------------------------------------------------------------------------------------------ rank / unrank
// index of k locations (slot * o + r each, < 24): include/dca.h "index rule".  A digit is clamped below its radix, so locations
// that are no partial permutation (any-bytes rule) still give an index inside the table.
template <int KIND>
__host__ __device__ inline uint64_t c3_rank(const uint32_t (&loc)[kPdbMaxK], int k) {
    constexpr int n = C3Kind<KIND>::n, o = C3Kind<KIND>::o;
    uint32_t seen = 0, rank = 0, orient = 0, ok = 1;
#pragma unroll
    for (int j = 0; j < kPdbMaxK; j++)
        if (j < k) {
            const uint32_t s = loc[j] / o, r = loc[j] - s * o;
            uint32_t d = s - (uint32_t)__builtin_popcount(seen & ((1u << s) - 1u));
            d = d < (uint32_t)(n - 1 - j) ? d : (uint32_t)(n - 1 - j);
            seen |= 1u << s;
            rank = rank * (uint32_t)(n - j) + d;  // < P(12, 8) = 19 958 400
            orient = orient * o + r;              // < 3^8
            ok *= o;
        }
    return (uint64_t)rank * ok + orient;
}

// the k locations of table entry e (every entry is a partial permutation with orientations: no invalid indices)
template <int KIND, typename IdxT>
__host__ __device__ inline void c3_unrank(IdxT e, int k, uint32_t (&loc)[kPdbMaxK]) {
    constexpr int n = C3Kind<KIND>::n, o = C3Kind<KIND>::o;
    uint32_t r[kPdbMaxK], s[kPdbMaxK];
#pragma unroll
    for (int j = kPdbMaxK - 1; j >= 0; j--) {
        r[j] = 0;
        if (j < k) {
            r[j] = (uint32_t)(e % (IdxT)o);
            e /= (IdxT)o;
        }
    }
    uint32_t rank = (uint32_t)e;
#pragma unroll
    for (int j = kPdbMaxK - 1; j >= 0; j--) {
        s[j] = 0;
        if (j < k) {
            s[j] = rank % (uint32_t)(n - j);
            rank /= (uint32_t)(n - j);
        }
    }
    // digits -> slots: d_j counts the slots below s_j that are still free after cubies 0 .. j-1 took theirs
#pragma unroll
    for (int i = kPdbMaxK - 2; i >= 0; i--)
#pragma unroll
        for (int j = i + 1; j < kPdbMaxK; j++)
            if (j < k && s[j] >= s[i]) s[j]++;
#pragma unroll
    for (int j = 0; j < kPdbMaxK; j++) loc[j] = j < k ? s[j] * o + r[j] : 0u;
}

// ---------------------------------------------------------------------------------------------------------------- eval
// colour of the byte at position p of a row held as words (p is a compile-time constant wherever this is called)
template <int ROWS>
__host__ __device__ inline uint32_t c3_colour(const uint32_t (&w)[14], int p) {
    const uint32_t b = (w[p >> 2] >> (8 * (p & 3))) & 0xFFu;
    return ROWS == DCA_ROWS_STATE ? (b * 57u) >> 9 : b;  // id / 9 for ids < 64; a byte >= 54 gives a colour >= 6
}

// the locations of all the cubies of one kind, 5 bits per cubie: include/dca.h "colour rule" and "any-bytes rule"
template <int KIND, int ROWS>
__host__ __device__ inline uint64_t c3_row_locs(const uint32_t (&w)[14]) {
    constexpr int n = C3Kind<KIND>::n, o = C3Kind<KIND>::o;
    uint32_t set[n], at[n];  // per slot: the colour set on its positions, and slot * o + r of its smallest colour
#pragma unroll
    for (int s = 0; s < n; s++) {
        uint32_t least = c3_colour<ROWS>(w, kC3.pos[KIND][s * o]), r = 0;
        set[s] = least < 6u ? 1u << least : 0u;
#pragma unroll
        for (int x = 1; x < o; x++) {
            const uint32_t c = c3_colour<ROWS>(w, kC3.pos[KIND][s * o + x]);
            set[s] |= c < 6u ? 1u << c : 0u;
            r = c < least ? (uint32_t)x : r;
            least = c < least ? c : least;
        }
        at[s] = (uint32_t)(s * o) + r;
    }
    uint64_t locs = 0;
#pragma unroll
    for (int q = 0; q < n; q++) {
        uint32_t l = 0;
#pragma unroll
        for (int s = 0; s < n; s++) l = set[s] == (uint32_t)kC3.colours[KIND][q] ? at[s] : l;  // the LAST such slot, 0 if none
        locs |= (uint64_t)l << (5 * q);
    }
    return locs;
}

template <int KIND>
__host__ __device__ inline uint64_t c3_index(uint64_t locs, const PdbPattern& pat, int k) {
    uint32_t loc[kPdbMaxK];
#pragma unroll
    for (int j = 0; j < kPdbMaxK; j++) loc[j] = j < k ? (uint32_t)(locs >> (5 * pat.id[j])) & 31u : 0u;  // cubie < 12, location < 24
    return c3_rank<KIND>(loc, k);
}

// what pdb_eval_kernel / pdb_eval_launch (dca_pdb_shared.h) take for rows of sticker ids or of colours
template <int ROWS>
struct C3Eval {
    static constexpr int N = 54;
    using Set = C3Set;
    static constexpr const char* kernel_name = "c3_eval_kernel";

    // one row's value: the largest of the set's patterns' table bytes
    __host__ __device__ static inline uint32_t row_value(const uint32_t (&w)[14], const C3Set& set) {
        const uint64_t corner = (set.kinds_used & 1) ? c3_row_locs<DCA_CUBE3_CORNERS, ROWS>(w) : 0ull;
        const uint64_t edge = (set.kinds_used & 2) ? c3_row_locs<DCA_CUBE3_EDGES, ROWS>(w) : 0ull;
        uint32_t best = 0;
        for (int p0 = 0; p0 < set.np; p0 += 4) {  // four independent gathers in flight
            uint32_t v[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                v[q] = 0;
                const int pi = p0 + q;
                if (pi < set.np) {
                    const uint64_t idx = set.kind[pi] == DCA_CUBE3_CORNERS ? c3_index<DCA_CUBE3_CORNERS>(corner, set.pat[pi], set.k[pi])
                                                                           : c3_index<DCA_CUBE3_EDGES>(edge, set.pat[pi], set.k[pi]);
                    v[q] = set.table[pi][idx];
                }
            }
            const uint32_t a = v[0] > v[1] ? v[0] : v[1], b = v[2] > v[3] ? v[2] : v[3];
            best = best > a ? best : a;
            best = best > b ? best : b;
        }
        return best;
    }
};

// ---------------------------------------------------------------------------------------------------------------- checks
// P(n, k) * o^k, or a negative code with the message set
static int64_t c3_bytes_checked(const char* who, int kind, int k) {
    if (kind != DCA_CUBE3_CORNERS && kind != DCA_CUBE3_EDGES) {
        set_error("bad argument: %s: kind = %d is neither 0 (corners) nor 1 (edges)", who, kind);
        return DCA_E_BADARG;
    }
    if (k < 1 || k > kPdbMaxK) {
        set_error("bad argument: %s: k = %d is not in 1..%d", who, k, kPdbMaxK);
        return DCA_E_BADARG;
    }
    const int n = kind == DCA_CUBE3_CORNERS ? 8 : 12, o = kind == DCA_CUBE3_CORNERS ? 3 : 2;
    int64_t b = 1;
    for (int j = 0; j < k; j++) b *= (int64_t)(n - j) * o;  // <= 12^8 * 2^8: no overflow
    if (b > kPdbMaxBytes) {
        set_error("bad argument: %s: k = %d: a table of %lld bytes is over the 2^34 limit", who, k, (long long)b);
        return DCA_E_BADARG;
    }
    return b;
}

static int c3_check_cubies(const char* who, int kind, const uint8_t* cubies, int k) {
    const int n = kind == DCA_CUBE3_CORNERS ? 8 : 12;
    uint32_t seen = 0;
    for (int j = 0; j < k; j++) {
        const int c = cubies[j];
        if (c >= n) {
            set_error("bad argument: %s: cubies: cubie %d is not in 0..%d", who, c, n - 1);
            return DCA_E_BADARG;
        }
        if ((seen >> c) & 1) {
            set_error("bad argument: %s: cubies: cubie %d appears twice in its pattern", who, c);
            return DCA_E_BADARG;
        }
        seen |= 1u << c;
    }
    return 0;
}

}  // namespace dca
