// dca_pdb_cube3.h — what the cube3 pattern-database code shares between dca_pdb_cube3.hip (build and eval kernels) and
// dca_idastar.hip (the IDA* search): the cubies derived at compile time, rank / unrank, the row -> locations rule, the eval
// frame's row value, the cube's 48 symmetries with the look-up list made from them, the inverse state's location words for the
// dual look-ups, and the entry points' checks.
// Header-only: every translation unit compiles its own copy, no device symbol crosses a translation unit.
#pragma once
#include <stddef.h>
#include <string.h>

#include <mutex>

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

// ---------------------------------------------------------------------------------------------------------- symmetries
// The 48 rotations and reflections of the cube (include/dca.h "Symmetric look-ups"), derived once at first use from kCube3Perm
// and kC3: nothing here is typed in.  Host only; a search or an eval is handed the look-up list made from them.
constexpr int kC3Syms = DCA_CUBE3_SYMS;
constexpr int kC3SymMaxLookups = DCA_CUBE3_SYM_MAX_LOOKUPS;

struct Cube3Syms {
    uint8_t face[kC3Syms][6];              // the face maps phi, in lexicographic order of (phi(0) .. phi(5)): the identity first
    uint8_t sticker[kC3Syms][54];          // sigma: position -> position
    uint8_t move[kC3Syms][12];             // pi: sigma o P_a o sigma^-1 = P_pi(a)
    uint8_t cubie[kC3Syms][2][12];         // kind, cubie c -> sigma(c)
    uint8_t source[kC3Syms][2][12];        // kind, cubie q -> sigma^-1(q)
    uint8_t loc[kC3Syms][2][12][kC3Locs];  // kind, cubie c: R_{sigma,c}, location of c -> location of sigma(c) in the conjugate
    const char* broken;                    // nullptr, or which property of the derivation failed
};

static const char* c3_derive_syms(Cube3Syms& t) {
    uint8_t opp[6];
    for (int f = 0; f < 6; f++) {  // two faces are opposite exactly when no cubie carries both colours
        int found = -1, count = 0;
        for (int g = 0; g < 6; g++) {
            if (g == f) continue;
            bool together = false;
            for (int kind = 0; kind < 2; kind++)
                for (int c = 0; c < kC3.count[kind]; c++) {
                    const uint32_t colours = kC3.colours[kind][c];
                    together = together || ((colours >> f) & (colours >> g) & 1u);
                }
            if (!together) {
                found = g;
                count++;
            }
        }
        if (count != 1) return "a face without exactly one opposite face";
        opp[f] = (uint8_t)found;
    }
    int ns = 0;
    uint8_t phi[6];
    for (int code = 0; code < 6 * 6 * 6 * 6 * 6 * 6; code++) {  // ascending code = lexicographic order, phi(0) most significant
        uint32_t seen = 0;
        for (int f = 5, c = code; f >= 0; f--, c /= 6) {
            phi[f] = (uint8_t)(c % 6);
            seen |= 1u << phi[f];
        }
        bool keeps = seen == 63u;
        for (int f = 0; f < 6 && keeps; f++) keeps = phi[opp[f]] == opp[phi[f]];
        if (!keeps) continue;
        if (ns == kC3Syms) return "more than 48 face maps keep the opposite pairs";
        for (int f = 0; f < 6; f++) t.face[ns][f] = phi[f];
        ns++;
    }
    if (ns != kC3Syms) return "fewer than 48 face maps keep the opposite pairs";
    const auto image_set = [](const uint8_t* map, uint32_t set) {
        uint32_t out = 0;
        for (int f = 0; f < 6; f++)
            if ((set >> f) & 1) out |= 1u << map[f];
        return out;
    };
    for (int s = 0; s < kC3Syms; s++) {
        const uint8_t* map = t.face[s];
        for (int kind = 0; kind < 2; kind++)
            for (int c = 0; c < kC3.count[kind]; c++) {
                int to = -1;
                for (int d = 0; d < kC3.count[kind]; d++)
                    if (kC3.colours[kind][d] == image_set(map, kC3.colours[kind][c])) to = d;
                if (to < 0) return "a cubie whose image's colour set belongs to no cubie";
                t.cubie[s][kind][c] = (uint8_t)to;
                t.source[s][kind][to] = (uint8_t)c;
            }
        // the sticker on face f of the cubie with colour set F goes to the sticker on face phi(f) of the cubie with set phi(F)
        uint64_t hit = 0;
        for (int p = 0; p < 54; p++) {
            const int kind = kC3.kind[p], face = map[p / 9];
            int to = -1;
            if (kind == 2) {
                for (int q = 0; q < 54; q++)
                    if (kC3.kind[q] == 2 && q / 9 == face) to = q;
            } else {
                const int o = kind == DCA_CUBE3_CORNERS ? 3 : 2, d = t.cubie[s][kind][kC3.loc[p] / o];
                for (int x = 0; x < o; x++)
                    if (kC3.pos[kind][d * o + x] / 9 == face) to = kC3.pos[kind][d * o + x];
            }
            if (to < 0) return "a sticker without an image";
            t.sticker[s][p] = (uint8_t)to;
            hit |= 1ull << to;
        }
        if (hit != (1ull << 54) - 1) return "a sticker map that is no permutation";
        for (int a = 0; a < 12; a++) {  // gather tables: P_b[sigma(i)] = sigma(P_a[i]) for every i
            int to = -1;
            for (int b = 0; b < 12 && to < 0; b++) {
                bool same = true;
                for (int i = 0; i < 54 && same; i++) same = kCube3Perm.p[b][t.sticker[s][i]] == t.sticker[s][kCube3Perm.p[a][i]];
                if (same) to = b;
            }
            if (to < 0) return "a conjugated move that is no move";
            t.move[s][a] = (uint8_t)to;
        }
        for (int r = 0; r < s; r++) {
            bool same = true;
            for (int a = 0; a < 12; a++) same = same && t.move[r][a] == t.move[s][a];
            if (same) return "two symmetries with the same move map";
        }
        // R[home(c)] = home(sigma(c)); R[move_a(l)] = move_pi(a)(R[l]): a breadth-first fill that must not contradict itself
        for (int kind = 0; kind < 2; kind++) {
            const int o = kind == DCA_CUBE3_CORNERS ? 3 : 2;
            for (int c = 0; c < kC3.count[kind]; c++) {
                uint8_t* R = t.loc[s][kind][c];
                for (int l = 0; l < kC3Locs; l++) R[l] = 0xFF;
                uint8_t queue[kC3Locs];
                int head = 0, tail = 0;
                R[c * o] = (uint8_t)(t.cubie[s][kind][c] * o);
                queue[tail++] = (uint8_t)(c * o);
                while (head < tail) {
                    const int l = queue[head++];
                    for (int a = 0; a < 12; a++) {
                        const int l2 = kC3.move[kind][a][l], v = kC3.move[kind][t.move[s][a]][R[l]];
                        if (R[l2] == 0xFF) {
                            R[l2] = (uint8_t)v;
                            queue[tail++] = (uint8_t)l2;
                        } else if (R[l2] != v) {
                            return "a location map that contradicts itself";
                        }
                    }
                }
                if (tail != kC3Locs) return "a location map that does not cover the 24 locations";
            }
        }
    }
    for (int f = 0; f < 6; f++)
        if (t.face[0][f] != f) return "the first symmetry is not the identity";
    return nullptr;
}

static const Cube3Syms& c3_syms() {
    static const Cube3Syms* const table = [] {
        Cube3Syms* t = new Cube3Syms();
        t->broken = c3_derive_syms(*t);
        return t;
    }();
    return *table;
}

// One look-up: a table read at the rank of k mapped locations.  Its source cubies src[j] = sigma^-1 of the pattern's are held
// as shift[j] = 5 * src[j], where the cubie's location sits in the packed word of its kind; map[j] is R_{sigma,src[j]} with
// the image location already split, slot | r << 4, so that one rank routine serves both kinds with no division.  Rows j >= k
// are zero and are read like the others (no load sits behind a branch).  The identity's look-up is the plain one.
struct C3Lookup {
    const uint8_t* table;
    uint32_t meta;  // kind | k << 8 | symmetry << 16
    uint32_t pad;
    uint8_t shift[kPdbMaxK];
    uint8_t map[kPdbMaxK][kC3Locs];
};

#define DCA_C3_INLINE __host__ __device__ inline __attribute__((always_inline))

// the layout c3_lookup_head's word offsets assume: table in words 0..1, meta in 2, the shifts in 4..5, the maps from byte 24
static_assert(sizeof(C3Lookup) == 216 && offsetof(C3Lookup, table) == 0 && offsetof(C3Lookup, meta) == 8 &&
                  offsetof(C3Lookup, shift) == 16 && offsetof(C3Lookup, map) == 24,
              "C3Lookup layout");

// a look-up's wave-uniform fields (the first 24 bytes) in registers
struct C3LookupHead {
    const uint8_t* table;
    uint32_t meta;
    uint64_t shifts;
};

// What the symmetric kernels read, in device memory (host memory for the host twins): 216 bytes a look-up, 13.8 KB in all.
// A look-up's number is wave-uniform: its head is read through the constant address space (the list is never written while a
// kernel runs), which makes the reads scalar loads; only map[j][location] and the table byte are per-lane reads.  All 64
// entries are valid: those past n repeat entry 0, so a trip of four needs no test against n and changes no maximum.
struct C3SymList {
    C3Lookup lk[kC3SymMaxLookups];
    int n;
    int kinds_used;
};

struct C3SymSet {  // the kernel argument
    const C3SymList* list;
    int n;
    int kinds_used;
};

// the images of one pattern: its distinct source cubie SETS in the symmetries' order, the pattern itself (the identity) first,
// at most max_images of them -> their number, each appended to `out` (room for kC3Syms)
static int c3_pattern_images(int kind, const uint8_t* cubies, int k, int max_images, const uint8_t* table, C3Lookup* out) {
    const Cube3Syms& t = c3_syms();
    uint32_t seen[kC3Syms];
    int n = 0;
    for (int s = 0; s < kC3Syms && n < max_images; s++) {
        uint32_t set = 0;
        for (int j = 0; j < k; j++) set |= 1u << t.source[s][kind][cubies[j]];
        bool fresh = true;
        for (int i = 0; i < n; i++) fresh = fresh && seen[i] != set;
        if (!fresh) continue;
        seen[n] = set;
        C3Lookup& lk = out[n++];
        lk = C3Lookup{};
        lk.table = table;
        lk.meta = (uint32_t)kind | (uint32_t)k << 8 | (uint32_t)s << 16;
        const int o = kind == DCA_CUBE3_CORNERS ? 3 : 2;
        for (int j = 0; j < k; j++) {
            const int src = t.source[s][kind][cubies[j]];
            lk.shift[j] = (uint8_t)(5 * src);
            for (int l = 0; l < kC3Locs; l++) {
                const int to = t.loc[s][kind][src][l];
                lk.map[j][l] = (uint8_t)(to / o | (to % o) << 4);
            }
        }
    }
    return n;
}

// The look-up list of a checked pattern set: pattern 0's images, then pattern 1's, ...  A code and the message where the
// derivation is broken, max_images is outside 1..48 or the list is over its cap.
static int c3_fill_sym_list(const char* who, const C3Set& set, int max_images, C3SymList& list) {
    if (max_images < 1 || max_images > kC3Syms) {
        set_error("bad argument: %s: max_images = %d is not in 1..%d", who, max_images, kC3Syms);
        return DCA_E_BADARG;
    }
    if (c3_syms().broken != nullptr) {
        set_error("%s: the cube's symmetries could not be derived from the move table: %s", who, c3_syms().broken);
        return DCA_E_STATE;
    }
    list = C3SymList{};
    C3Lookup images[kC3Syms];
    int total = 0;
    for (int p = 0; p < set.np; p++) {
        const int n = c3_pattern_images(set.kind[p], set.pat[p].id, set.k[p], max_images, set.table[p], images);
        for (int i = 0; i < n; i++, total++)
            if (total < kC3SymMaxLookups) list.lk[total] = images[i];
    }
    if (total > kC3SymMaxLookups) {
        set_error("bad argument: %s: max_images = %d gives %d look-ups, over the cap DCA_CUBE3_SYM_MAX_LOOKUPS = %d: "
                  "take fewer images of each pattern (pdb:<spec>+sym:N)", who, max_images, total, kC3SymMaxLookups);
        return DCA_E_BADARG;
    }
    for (int i = total; i < kC3SymMaxLookups; i++) list.lk[i] = list.lk[0];
    list.n = total;
    list.kinds_used = set.kinds_used;
    return 0;
}

// The device copy of a look-up list.  A copy is never written again once made: a list seen before (same look-ups, same table
// addresses, same device) gives its copy back with no HIP call; a new one is allocated and copied (the copy blocks the host;
// once per set and tables); the ninth distinct list of a translation unit frees the oldest.  hipFree waits for the device, so
// a kernel already launched on a copy is never disturbed.  NOT covered: a caller that has taken a copy but not launched yet
// while other threads bring in eight more distinct lists — more than eight distinct sets in use at once are not supported
// (include/dca.h says so).  The allocation, copy and free are not stream operations: none of this may run under a stream
// capture, so a set's first call comes before the capture.
struct C3SymDeviceLists {
    static constexpr int kEntries = 8;
    std::mutex mutex;
    C3SymList host[kEntries];
    C3SymList* dev[kEntries] = {};
    int device[kEntries] = {};
    int next = 0;
};

static int c3_sym_device_list(const C3SymList& list, const C3SymList*& out) {
    static C3SymDeviceLists* const cache = new C3SymDeviceLists();
    int device = 0;
    DCA_HIP(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(cache->mutex);
    for (int i = 0; i < C3SymDeviceLists::kEntries; i++)
        if (cache->dev[i] != nullptr && cache->device[i] == device && memcmp(&cache->host[i], &list, sizeof(C3SymList)) == 0) {
            out = cache->dev[i];
            return 0;
        }
    const int slot = cache->next;
    if (cache->dev[slot] != nullptr) {
        (void)hipFree(cache->dev[slot]);
        cache->dev[slot] = nullptr;
    }
    C3SymList* fresh = nullptr;
    DCA_HIP(hipMalloc((void**)&fresh, sizeof(C3SymList)));
    const hipError_t e = hipMemcpy(fresh, &list, sizeof(C3SymList), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(fresh);
        return hip_fail(e, "hipMemcpy(cube3 look-up list)");
    }
    cache->host[slot] = list;
    cache->dev[slot] = fresh;
    cache->device[slot] = device;
    cache->next = (slot + 1) % C3SymDeviceLists::kEntries;
    out = fresh;
    return 0;
}

DCA_C3_INLINE C3LookupHead c3_lookup_head(const C3Lookup* lk) {
#ifdef __HIP_DEVICE_COMPILE__
    typedef const uint32_t __attribute__((address_space(4))) ConstWord;
    ConstWord* w = (ConstWord*)(uintptr_t)lk;
    return C3LookupHead{(const uint8_t*)((uint64_t)w[0] | (uint64_t)w[1] << 32), w[2], (uint64_t)w[4] | (uint64_t)w[5] << 32};
#else
    uint64_t shifts = 0;
    for (int j = 0; j < kPdbMaxK; j++) shifts |= (uint64_t)lk->shift[j] << (8 * j);
    return C3LookupHead{lk->table, lk->meta, shifts};
#endif
}

// The eight map reads of one look-up from the packed locations of both kinds (c3_row_locs, or the search's state), no branch.
// A location is < 24 (c3_row_locs, kC3.move) and a shift <= 55, so every read is inside its row.
DCA_C3_INLINE void c3_sym_maps(const C3Lookup* lk, const C3LookupHead& h, uint64_t corner, uint64_t edge, uint32_t (&m)[kPdbMaxK]) {
    const uint64_t locs = (h.meta & 0xFFu) == (uint32_t)DCA_CUBE3_CORNERS ? corner : edge;
#pragma unroll
    for (int j = 0; j < kPdbMaxK; j++) m[j] = lk->map[j][(uint32_t)(locs >> ((uint32_t)(h.shifts >> (8 * j)) & 63u)) & 31u];
}

// The index from the eight map bytes: c3_rank with n and o as values — digits clamped below their radix, so any locations give
// an index inside the table.
DCA_C3_INLINE uint64_t c3_sym_rank(const C3LookupHead& h, const uint32_t (&m)[kPdbMaxK]) {
    const bool corners = (h.meta & 0xFFu) == (uint32_t)DCA_CUBE3_CORNERS;
    const uint32_t k = (h.meta >> 8) & 0xFFu, n = corners ? 8u : 12u, o = corners ? 3u : 2u;
    uint32_t seen = 0, rank = 0, orient = 0, ok = 1;
#pragma unroll
    for (int j = 0; j < kPdbMaxK; j++) {
        const bool on = (uint32_t)j < k;
        const uint32_t s = m[j] & 15u, r = m[j] >> 4;
        uint32_t d = s - (uint32_t)__builtin_popcount(seen & ((1u << s) - 1u));
        d = d < n - 1u - (uint32_t)j ? d : n - 1u - (uint32_t)j;
        seen |= on ? 1u << s : 0u;
        rank = on ? rank * (n - (uint32_t)j) + d : rank;
        orient = on ? orient * o + r : orient;
        ok = on ? ok * o : ok;
    }
    return (uint64_t)rank * ok + orient;
}

DCA_C3_INLINE uint64_t c3_sym_index(const C3Lookup* lk, const C3LookupHead& h, uint64_t corner, uint64_t edge) {
    uint32_t m[kPdbMaxK];
    c3_sym_maps(lk, h, corner, edge, m);
    return c3_sym_rank(h, m);
}

// Four look-ups of the list, from look-up p0 on (p0 a multiple of 4: all four exist) -> the largest of their bytes.  The four
// heads are scalar, the 32 map reads depend on nothing but the state and the four gathers on nothing but their own maps.  Forced
// inline: left to itself the compiler made it a call in the eval kernels.
DCA_C3_INLINE uint32_t c3_sym_gather4(const C3SymList* list, int p0, uint64_t corner, uint64_t edge) {
    uint64_t idx[4];
    C3LookupHead h[4];
    uint32_t m[4][kPdbMaxK];
#pragma unroll
    for (int q = 0; q < 4; q++) h[q] = c3_lookup_head(&list->lk[p0 + q]);
#pragma unroll
    for (int q = 0; q < 4; q++) c3_sym_maps(&list->lk[p0 + q], h[q], corner, edge, m[q]);  // 32 reads before the first rank
#pragma unroll
    for (int q = 0; q < 4; q++) idx[q] = c3_sym_rank(h[q], m[q]);
    uint32_t v[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
#ifdef __HIP_DEVICE_COMPILE__
        v[q] = ((const __attribute__((address_space(1))) uint8_t*)(uintptr_t)h[q].table)[idx[q]];
#else
        v[q] = h[q].table[idx[q]];
#endif
    }
    const uint32_t a = v[0] > v[1] ? v[0] : v[1], b = v[2] > v[3] ? v[2] : v[3];
    return a > b ? a : b;
}

// what pdb_eval_kernel / pdb_eval_launch take for the symmetric value: c3_row_locs once per row, then the list
template <int ROWS>
struct C3EvalSym {
    static constexpr int N = 54;
    using Set = C3SymSet;
    static constexpr const char* kernel_name = "c3_eval_sym_kernel";

    __host__ __device__ static inline uint32_t row_value(const uint32_t (&w)[14], const C3SymSet& set) {
        const uint64_t corner = (set.kinds_used & 1) ? c3_row_locs<DCA_CUBE3_CORNERS, ROWS>(w) : 0ull;
        const uint64_t edge = (set.kinds_used & 2) ? c3_row_locs<DCA_CUBE3_EDGES, ROWS>(w) : 0ull;
        uint32_t best = 0;
        for (int p0 = 0; p0 < set.n; p0 += 4) {
            const uint32_t v = c3_sym_gather4(set.list, p0, corner, edge);
            best = best > v ? best : v;
        }
        return best;
    }
};

// ------------------------------------------------------------------------------------------------------------- duality
// The dual look-ups (include/dca.h "Dual look-ups"): the look-up list read a second time at the location words of the INVERSE
// state, which are made from the state's own words in registers — no row, no table, no memory access.
//
// Where cubie j sits in slot s, the inverse has cubie s in slot j.  Its orientation there: r counts the place, among a slot's
// ascending positions, of the cubie's smallest colour, and the ascending positions of a corner slot run clockwise round four
// of the corners and anticlockwise round the other four.  Between two corners of one class the cubie's positions are rotated
// by r and the inverse rotates back, r' = (3 - r) mod 3; between the classes they are reflected about r, and a reflection is
// its own inverse, r' = r.  An edge has r' = r = (2 - r) mod 2 either way.  The classes are read off the move table: a quarter
// turn carries a slot's positions x -> x + c onto a slot of its own class and x -> c - x onto one of the other.
constexpr uint32_t make_c3_corner_classes() {  // bit s = slot s is not of slot 0's class; 0xFFFFFFFF: the move table has no such classes
    uint32_t cls = 0, known = 1;
    for (int round = 0; round < 8; round++)
        for (int a = 0; a < 12; a++)
            for (int s = 0; s < 8; s++) {
                const int t0 = kC3.move[0][a][s * 3], t1 = kC3.move[0][a][s * 3 + 1], t = t0 / 3;
                if (t1 / 3 != t) return 0xFFFFFFFFu;
                const uint32_t flips = (t1 - t0 + 3) % 3 == 1 ? 0u : 1u;
                if (!((known >> s) & 1u)) continue;
                const uint32_t bit = ((cls >> s) & 1u) ^ flips;
                if (((known >> t) & 1u) && ((cls >> t) & 1u) != bit) return 0xFFFFFFFFu;
                known |= 1u << t;
                cls |= bit << t;
            }
    return known == 0xFFu ? cls : 0xFFFFFFFFu;
}
inline constexpr uint32_t kC3CornerClasses = make_c3_corner_classes();
static_assert(kC3CornerClasses < 0x100u && __builtin_popcount(kC3CornerClasses) == 4, "cube3: two classes of four corner slots");

// The inverse state's location words from the state's (5 bits a cubie, every location < 24 as c3_row_locs and the moves leave
// them): for cubie j = 0 .. n-1 in ascending order at (s_j, r_j), field s_j becomes (j, r'_j).
//   REPLACE  the field is masked, then set: the last writer wins and a slot no cubie names keeps location 0, so the result's
//            locations are < 24 for ANY words — the any-bytes rule of the eval kernels.
//   !REPLACE the field is or-ed onto zero: the same words wherever the n slots are distinct, which a search's state is (its
//            root is checked, the moves permute the slots); on other words fields would mix.
template <int KIND, bool REPLACE>
DCA_C3_INLINE uint64_t c3_inverse_locs(uint64_t locs) {
    constexpr int n = C3Kind<KIND>::n, o = C3Kind<KIND>::o;
    uint64_t inv = 0;
#pragma unroll
    for (int j = 0; j < n; j++) {
        const uint32_t l = (uint32_t)(locs >> (5 * j)) & 31u;
        const uint32_t s = l / (uint32_t)o, r = l - s * (uint32_t)o;
        uint32_t back = r;
        if (KIND == DCA_CUBE3_CORNERS) {
            const bool same = (((kC3CornerClasses >> s) ^ (kC3CornerClasses >> j)) & 1u) == 0u;
            back = same && r != 0u ? 3u - r : r;
        }
        const uint32_t sh = 5u * s;  // s <= 10 even for a field of 31: inside the word
        if (REPLACE) inv &= ~(31ull << sh);
        inv |= (uint64_t)((uint32_t)(j * o) + back) << sh;
    }
    return inv;
}

// Does the look-up's pattern name every cubie of its kind?  Then its byte at the inverted words is its byte at the state on
// every cube state, and the second pass counts it 0.  (An edge pattern has k <= 8 < 12.)
DCA_C3_INLINE bool c3_lookup_whole(const C3LookupHead& h) {
    return (h.meta & 0xFFFFu) == ((uint32_t)DCA_CUBE3_CORNERS | (uint32_t)C3Kind<DCA_CUBE3_CORNERS>::n << 8);
}

// c3_sym_gather4 for the second pass, over the inverted words: p0 is any look-up below n, so p0 + q may pass the list's end —
// such a look-up is entry 0 again — and a whole look-up counts 0.  (Written out a second time: as one template with
// c3_sym_gather4 it moved the symmetric kernels' scalar loads, profiles/cube3_dual_isa.txt.)
DCA_C3_INLINE uint32_t c3_dual_gather4(const C3SymList* list, int p0, uint64_t corner, uint64_t edge) {
    uint64_t idx[4];
    C3LookupHead h[4];
    uint32_t m[4][kPdbMaxK];
    const C3Lookup* lk[4];
#pragma unroll
    for (int q = 0; q < 4; q++) lk[q] = &list->lk[p0 + q < kC3SymMaxLookups ? p0 + q : 0];
#pragma unroll
    for (int q = 0; q < 4; q++) h[q] = c3_lookup_head(lk[q]);
#pragma unroll
    for (int q = 0; q < 4; q++) c3_sym_maps(lk[q], h[q], corner, edge, m[q]);
#pragma unroll
    for (int q = 0; q < 4; q++) idx[q] = c3_sym_rank(h[q], m[q]);
    uint32_t v[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
#ifdef __HIP_DEVICE_COMPILE__
        v[q] = ((const __attribute__((address_space(1))) uint8_t*)(uintptr_t)h[q].table)[idx[q]];
#else
        v[q] = h[q].table[idx[q]];
#endif
        v[q] = c3_lookup_whole(h[q]) ? 0u : v[q];
    }
    const uint32_t a = v[0] > v[1] ? v[0] : v[1], b = v[2] > v[3] ? v[2] : v[3];
    return a > b ? a : b;
}

// What the second pass needs of a list: `lead`, the look-ups in front that name every cubie of their kind (the pass starts
// behind them; one elsewhere in the list counts 0, c3_dual_gather4), n where there is no other; `kinds`, bit kind = some look-up of
// that kind is read in the pass, so its word is inverted.
struct C3DualPass {
    int lead;
    int kinds;
};

static C3DualPass c3_dual_pass(const C3SymList& list) {
    C3DualPass d{list.n, 0};
    for (int p = 0; p < list.n; p++) {
        if (c3_lookup_whole(c3_lookup_head(&list.lk[p]))) continue;
        d.lead = d.lead < p ? d.lead : p;
        d.kinds |= 1 << (list.lk[p].meta & 0xFFu);
    }
    return d;
}

struct C3DualSet : C3SymSet {  // the kernel argument
    C3DualPass dual;
};

// a list's kernel argument, the list where it stands (a device launch then names its device copy, c3_sym_device_list)
static void c3_list_arg(const C3SymList& list, C3DualSet& arg) {
    arg.list = &list;
    arg.n = list.n;
    arg.kinds_used = list.kinds_used;
    arg.dual = c3_dual_pass(list);
}

// the second pass: the largest byte over the look-ups from `lead` on at the inverted words, left at the first value above slack
DCA_C3_INLINE uint32_t c3_dual_value(const C3SymList* list, int n, int lead, uint64_t corner, uint64_t edge, uint32_t best, uint32_t slack) {
    for (int p0 = lead; p0 < n; p0 += 4) {
        const uint32_t v = c3_dual_gather4(list, p0, corner, edge);
        best = best > v ? best : v;
        if (best > slack) break;
    }
    return best;
}

// what pdb_eval_kernel / pdb_eval_launch take for the dual value: the symmetric value, then the same list at the inverted words.
// (C3EvalSym's list loop is written out a second time: as one inline function the two share it flipped the dual eval kernels'
// branch senses, profiles/cube3_lookups_isa.txt.)
template <int ROWS>
struct C3EvalDual {
    static constexpr int N = 54;
    using Set = C3DualSet;
    static constexpr const char* kernel_name = "c3_eval_dual_kernel";

    __host__ __device__ static inline uint32_t row_value(const uint32_t (&w)[14], const C3DualSet& set) {
        const uint64_t corner = (set.kinds_used & 1) ? c3_row_locs<DCA_CUBE3_CORNERS, ROWS>(w) : 0ull;
        const uint64_t edge = (set.kinds_used & 2) ? c3_row_locs<DCA_CUBE3_EDGES, ROWS>(w) : 0ull;
        uint32_t best = 0;
        for (int p0 = 0; p0 < set.n; p0 += 4) {
            const uint32_t v = c3_sym_gather4(set.list, p0, corner, edge);
            best = best > v ? best : v;
        }
        const uint64_t icorner = (set.dual.kinds & 1) ? c3_inverse_locs<DCA_CUBE3_CORNERS, true>(corner) : 0ull;
        const uint64_t iedge = (set.dual.kinds & 2) ? c3_inverse_locs<DCA_CUBE3_EDGES, true>(edge) : 0ull;
        return c3_dual_value(set.list, set.n, set.dual.lead, icorner, iedge, best, 0xFFFFFFFFu);
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

// A cube3 entry point's pattern set from its arrays (num_patterns in range, no array NULL: the caller's own refusals): every
// pattern's size, cubies and table checked, then the kinds.
static int c3_fill_set(const char* who, int num_patterns, const int* kinds, const uint8_t* cubies, const int* ks,
                       const uint8_t* const* tables, C3Set& set) {
    if (int rc = pdb_fill_set(
            who, set, num_patterns, cubies, ks, tables, [&](int p) { return c3_bytes_checked(who, kinds[p], ks[p]); },
            [&](int p, const uint8_t* c) { return c3_check_cubies(who, kinds[p], c, ks[p]); }))
        return rc;
    for (int p = 0; p < num_patterns; p++) {
        set.kind[p] = (uint8_t)kinds[p];
        set.kinds_used |= 1 << kinds[p];
    }
    return 0;
}

// A symmetric entry point's pattern set and look-up list from its arrays: the refusals of dca_cube3_pdb_eval, then those of
// the list.
static int c3_fill_sym_entry(const char* who, int num_patterns, const int* kinds, const uint8_t* cubies, const int* ks,
                             const uint8_t* const* tables, int max_images, C3Set& set, C3SymList& list) {
    if (num_patterns < 1 || num_patterns > kPdbMaxPatterns) {
        set_error("bad argument: %s: num_patterns = %d is not in 1..%d", who, num_patterns, kPdbMaxPatterns);
        return DCA_E_BADARG;
    }
    if (kinds == nullptr || cubies == nullptr || ks == nullptr || tables == nullptr) {
        set_error("bad argument: %s: kinds, cubies, ks and tables must not be NULL", who);
        return DCA_E_BADARG;
    }
    if (int rc = c3_fill_set(who, num_patterns, kinds, cubies, ks, tables, set)) return rc;
    return c3_fill_sym_list(who, set, max_images, list);
}

}  // namespace dca
