// dca_pdb_cube3.hip — pattern databases for cube3 (include/dca.h "pattern databases for cube3"): Korf's distance tables over the
// corner cubies and over subsets of the edge cubies, combined by max.  The cubie lists, the sticker -> location map and the
// 12 x 24 location-move tables are derived at compile time from kCube3Perm.  Two kernels:
//
//   build   level-synchronous pulling.  The table starts as 0xFE with 0 at the goal; sweep d = 1, 2, ... gives every entry that
//           is still 0xFE and has a neighbour at d - 1 the value d.  One thread owns an entry: it unranks the entry into k
//           locations (slot * o + r), maps them through the location-move table of each of the 12 moves (staged in LDS once per
//           workgroup), re-ranks and reads the 12 neighbour bytes, and writes only its own byte.  A neighbour another thread
//           fills in the same sweep reads as 0xFE or as d, never as d - 1, so the result and the number of sweeps (deepest
//           level + 1) do not depend on the order threads run in.  The host reads one "filled" word per sweep (this
//           synchronises the stream).
//   eval    one thread per row: the row's bytes in registers as colours; per slot the colour set and the place of its smallest
//           colour, compared against the cubies' compile-time colour sets — no array indexed by a row byte.  The locations of
//           the 8 corner and 12 edge cubies are packed 5 bits each into one 64-bit word per kind, from which every pattern
//           picks its cubies (wave-uniform shifts).  Every rank digit is clamped below its radix, so any 54 bytes give an
//           index inside the table.  One byte gather per pattern, four in flight, max, written as fp32.
//
// What bounds either kernel has not been measured (profiles/cube3_pdb_probe.txt holds only wall-clock times).
#include "dca_pdb_shared.h"

namespace dca {

constexpr int kC3MaxSweeps = 64;  // far above any pattern's depth, far below the 0xFE byte
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

// ---------------------------------------------------------------------------------------------------------------- build
template <int KIND, typename IdxT>
__global__ __launch_bounds__(kPdbThreads) void c3_sweep_kernel(uint8_t* table, uint64_t total, int k, uint32_t depth, C3MoveTable mt,
                                                              uint32_t* __restrict__ filled) {
    __shared__ uint32_t mvw[12 * kC3Locs / 4];
    if (threadIdx.x == 0) {  // (constant indices into the kernel argument: scalar loads, no private copy of the struct)
#pragma unroll
        for (int q = 0; q < 12 * kC3Locs / 4; q++) mvw[q] = mt.w[q];
    }
    __syncthreads();
    const uint8_t* mv = (const uint8_t*)mvw;
    const uint64_t stride = (uint64_t)gridDim.x * kPdbThreads;
    bool any = false;
    for (uint64_t e = (uint64_t)blockIdx.x * kPdbThreads + threadIdx.x; e < total; e += stride) {
        if (__hip_atomic_load(table + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != kPdbInf) continue;
        uint32_t loc[kPdbMaxK];
        c3_unrank<KIND, IdxT>((IdxT)e, k, loc);
        bool hit = false;
#pragma unroll
        for (int a0 = 0; a0 < 12; a0 += 4) {  // four neighbour reads in flight
            uint32_t v[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                uint32_t nl[kPdbMaxK];
#pragma unroll
                for (int j = 0; j < kPdbMaxK; j++) nl[j] = j < k ? (uint32_t)mv[(a0 + q) * kC3Locs + loc[j]] : 0u;  // loc < 24
                const uint64_t ne = c3_rank<KIND>(nl, k);  // a move permutes locations: distinct slots stay distinct, ne < total
                v[q] = __hip_atomic_load(table + ne, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            hit = hit || v[0] == depth - 1 || v[1] == depth - 1 || v[2] == depth - 1 || v[3] == depth - 1;
        }
        if (hit) {
            __hip_atomic_store(table + e, (uint8_t)depth, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            any = true;
        }
    }
    if (any) __hip_atomic_store(filled, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int KIND>
static int c3_build_launch(uint8_t* table, uint64_t total, int k, const PdbPattern& pat, int* sweeps, hipStream_t st) {
    constexpr int o = C3Kind<KIND>::o;
    uint32_t home[kPdbMaxK] = {};
    for (int j = 0; j < k; j++) home[j] = (uint32_t)pat.id[j] * o;
    const uint64_t goal = c3_rank<KIND>(home, k);
    C3MoveTable mt{};
    for (int a = 0; a < 12; a++)
        for (int l = 0; l < kC3Locs; l++) mt.w[(a * kC3Locs + l) >> 2] |= (uint32_t)kC3.move[KIND][a][l] << (8 * (l & 3));
    const unsigned blocks = pdb_blocks(total, kPdbMaxBuildBlocks);
    hipError_t e = hipMemsetAsync(table, kPdbInf, total, st);
    if (e == hipSuccess) e = hipMemsetAsync(table + goal, 0, 1, st);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(cube3 pdb table)");
    int done = 0;
    const int rc = pdb_sweep_until_quiet(st, kC3MaxSweeps, "dca_cube3_pdb_build", [&](int depth, uint32_t* filled) {
        if (total <= 0xFFFFFFFFull)
            hipLaunchKernelGGL((c3_sweep_kernel<KIND, uint32_t>), dim3(blocks), dim3(kPdbThreads), 0, st, table, total, k, (uint32_t)depth, mt, filled);
        else
            hipLaunchKernelGGL((c3_sweep_kernel<KIND, uint64_t>), dim3(blocks), dim3(kPdbThreads), 0, st, table, total, k, (uint32_t)depth, mt, filled);
        return launch_check("c3_sweep_kernel");
    }, done);
    if (rc == DCA_E_STATE) set_error("dca_cube3_pdb_build: levels still filling after %d sweeps", done);
    if (rc == 0 && sweeps) *sweeps = done;
    return rc;
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

template <int ROWS>
static int64_t c3_host_index(int kind, const PdbPattern& pat, int k, const uint8_t* row) {
    uint32_t w[14];
    pdb_load_row<54, 1>(row, w);
    return kind == DCA_CUBE3_CORNERS ? (int64_t)c3_index<DCA_CUBE3_CORNERS>(c3_row_locs<DCA_CUBE3_CORNERS, ROWS>(w), pat, k)
                                     : (int64_t)c3_index<DCA_CUBE3_EDGES>(c3_row_locs<DCA_CUBE3_EDGES, ROWS>(w), pat, k);
}

}  // namespace dca

using namespace dca;

extern "C" {

int64_t dca_cube3_pdb_bytes(int kind, int k) { return c3_bytes_checked("dca_cube3_pdb_bytes", kind, k); }

int dca_cube3_pdb_cubies(int kind, uint8_t* positions) {
    if (kind != DCA_CUBE3_CORNERS && kind != DCA_CUBE3_EDGES) {
        set_error("bad argument: %s: kind = %d is neither 0 (corners) nor 1 (edges)", __func__, kind);
        return DCA_E_BADARG;
    }
    DCA_ARG(positions != nullptr);
    for (int l = 0; l < kC3Locs; l++) positions[l] = kC3.pos[kind][l];
    return 0;
}

int dca_cube3_pdb_index(int kind, const uint8_t* cubies, int k, const uint8_t* row, int row_kind, int64_t* index) {
    const int64_t total = c3_bytes_checked(__func__, kind, k);
    if (total < 0) return (int)total;
    DCA_ARG(cubies != nullptr);
    DCA_ARG(row != nullptr);
    DCA_ARG(row_kind == DCA_ROWS_STATE || row_kind == DCA_ROWS_NNET);
    DCA_ARG(index != nullptr);
    if (int rc = c3_check_cubies(__func__, kind, cubies, k)) return rc;
    const PdbPattern pat = pdb_pattern(cubies, k);
    *index =row_kind == DCA_ROWS_STATE ? c3_host_index<DCA_ROWS_STATE>(kind, pat, k, row) : c3_host_index<DCA_ROWS_NNET>(kind, pat, k, row);
    return 0;
}

int dca_cube3_pdb_build(int kind, const uint8_t* cubies, int k, uint8_t* table, int* sweeps, void* stream) {
    const int64_t total = c3_bytes_checked(__func__, kind, k);
    if (total < 0) return (int)total;
    DCA_ARG(cubies != nullptr);
    DCA_ARG(table != nullptr);
    if (int rc = c3_check_cubies(__func__, kind, cubies, k)) return rc;
    const PdbPattern pat = pdb_pattern(cubies, k);
    hipStream_t st = (hipStream_t)stream;
    return kind == DCA_CUBE3_CORNERS ? c3_build_launch<DCA_CUBE3_CORNERS>(table, (uint64_t)total, k, pat, sweeps, st)
                                     : c3_build_launch<DCA_CUBE3_EDGES>(table, (uint64_t)total, k, pat, sweeps, st);
}

int dca_cube3_pdb_eval(const uint8_t* states, int64_t n, int64_t ld, int row_kind, int num_patterns, const int* kinds,
                       const uint8_t* cubies, const int* ks, const uint8_t* const* tables, float* out, void* stream) {
    DCA_ARG(n >= 0 && n < ((int64_t)1 << 31));
    DCA_ARG(ld >= 54);
    DCA_ARG(row_kind == DCA_ROWS_STATE || row_kind == DCA_ROWS_NNET);
    DCA_ARG(num_patterns >= 1 && num_patterns <= 24);
    DCA_ARG(kinds != nullptr && cubies != nullptr && ks != nullptr && tables != nullptr);
    C3Set set{};
    const char* who = __func__;
    if (int rc = pdb_fill_set(
            who, set, num_patterns, cubies, ks, tables, [&](int p) { return c3_bytes_checked(who, kinds[p], ks[p]); },
            [&](int p, const uint8_t* c) { return c3_check_cubies(who, kinds[p], c, ks[p]); }))
        return rc;
    for (int p = 0; p < num_patterns; p++) {
        set.kind[p] = (uint8_t)kinds[p];
        set.kinds_used |= 1 << kinds[p];
    }
    if (n == 0) return 0;
    DCA_ARG(states != nullptr && out != nullptr);
    DCA_ARG(((uintptr_t)out & 3) == 0);
    hipStream_t st = (hipStream_t)stream;
    return row_kind == DCA_ROWS_STATE ? pdb_eval_launch<C3Eval<DCA_ROWS_STATE>>(states, n, ld, set, out, st)
                                      : pdb_eval_launch<C3Eval<DCA_ROWS_NNET>>(states, n, ld, set, out, st);
}

}  // extern "C"
