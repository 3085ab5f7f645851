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
//   eval_sym  the same frame on the symmetric look-ups (dca_pdb_cube3.h "symmetries", include/dca.h): the locations once per
//           row, then trips of four look-ups — their heads by scalar loads, their 32 map reads issued together, four ranks,
//           four gathers issued together.  The list is global memory.  Cost per row: profiles/idastar_sym_probe.txt.
//
//   eval_dual  the symmetric row value, then the location words of the inverse state made from the row's own (c3_inverse_locs, the
//           replacing form: in bounds for any bytes) and the list's trips again over them, but for the look-ups of a pattern that
//           names every cubie of its kind (dca_pdb_cube3.h "duality", include/dca.h).  Cost per row: profiles/idastar_dual_probe.txt.
//
// What bounds either kernel has not been measured (profiles/cube3_pdb_probe.txt holds only wall-clock times).
#include "dca_pdb_cube3.h"

namespace dca {

constexpr int kC3MaxSweeps = 64;  // far above any pattern's depth, far below the 0xFE byte

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

template <int ROWS>
static int64_t c3_host_index(int kind, const PdbPattern& pat, int k, const uint8_t* row) {
    uint32_t w[14];
    pdb_load_row<54, 1>(row, w);
    return kind == DCA_CUBE3_CORNERS ? (int64_t)c3_index<DCA_CUBE3_CORNERS>(c3_row_locs<DCA_CUBE3_CORNERS, ROWS>(w), pat, k)
                                     : (int64_t)c3_index<DCA_CUBE3_EDGES>(c3_row_locs<DCA_CUBE3_EDGES, ROWS>(w), pat, k);
}

// ---------------------------------------------------------------------------------------------------------------- eval
enum C3Mode { kC3Plain, kC3Sym, kC3Dual };  // which look-ups an eval reads (include/dca.h)

// a family's kernels or the host loop, for rows of sticker ids or of colours
template <template <int> class F>
static int c3_eval_run(const uint8_t* states, int64_t n, int64_t ld, int row_kind, const typename F<DCA_ROWS_STATE>::Set& set, float* out,
                       bool host, hipStream_t st) {
    if (host) {
        if (row_kind == DCA_ROWS_STATE)
            pdb_eval_rows_host<F<DCA_ROWS_STATE>>(states, n, ld, set, out);
        else
            pdb_eval_rows_host<F<DCA_ROWS_NNET>>(states, n, ld, set, out);
        return 0;
    }
    return row_kind == DCA_ROWS_STATE ? pdb_eval_launch<F<DCA_ROWS_STATE>>(states, n, ld, set, out, st)
                                      : pdb_eval_launch<F<DCA_ROWS_NNET>>(states, n, ld, set, out, st);
}

#define DCA_C3_ARG(cond)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            set_error("bad argument: %s: %s", who, #cond); \
            return DCA_E_BADARG;                           \
        }                                                  \
    } while (0)

// what the five eval entry points share: every refusal, before any HIP call, then the mode's kernels or the host loop.
// (max_images is not read in the plain mode; the host loop writes `out` float by float, so only a kernel needs it aligned.)
static int c3_eval_entry(const char* who, const uint8_t* states, int64_t n, int64_t ld, int row_kind, int num_patterns, const int* kinds,
                         const uint8_t* cubies, const int* ks, const uint8_t* const* tables, int max_images, float* out, C3Mode mode,
                         bool host, hipStream_t st) {
    DCA_C3_ARG(n >= 0 && n < ((int64_t)1 << 31));
    DCA_C3_ARG(ld >= 54);
    DCA_C3_ARG(row_kind == DCA_ROWS_STATE || row_kind == DCA_ROWS_NNET);
    C3Set set{};
    C3SymList list;
    if (mode == kC3Plain) {
        DCA_C3_ARG(num_patterns >= 1 && num_patterns <= 24);
        DCA_C3_ARG(kinds != nullptr && cubies != nullptr && ks != nullptr && tables != nullptr);
        if (int rc = c3_fill_set(who, num_patterns, kinds, cubies, ks, tables, set)) return rc;
    } else if (int rc = c3_fill_sym_entry(who, num_patterns, kinds, cubies, ks, tables, max_images, set, list)) {
        return rc;
    }
    if (n == 0) return 0;
    DCA_C3_ARG(states != nullptr && out != nullptr);
    if (!host) DCA_C3_ARG(((uintptr_t)out & 3) == 0);
    if (mode == kC3Plain) return c3_eval_run<C3Eval>(states, n, ld, row_kind, set, out, host, st);
    C3DualSet arg;
    c3_list_arg(list, arg);
    if (!host)
        if (int rc = c3_sym_device_list(list, arg.list)) return rc;
    return mode == kC3Dual ? c3_eval_run<C3EvalDual>(states, n, ld, row_kind, arg, out, host, st)
                           : c3_eval_run<C3EvalSym>(states, n, ld, row_kind, arg, out, host, st);
}
#undef DCA_C3_ARG

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
    return c3_eval_entry(__func__, states, n, ld, row_kind, num_patterns, kinds, cubies, ks, tables, 0, out, kC3Plain, false, (hipStream_t)stream);
}

int dca_cube3_pdb_eval_sym(const uint8_t* states, int64_t n, int64_t ld, int row_kind, int num_patterns, const int* kinds,
                           const uint8_t* cubies, const int* ks, const uint8_t* const* tables, int max_images, float* out,
                           void* stream) {
    return c3_eval_entry(__func__, states, n, ld, row_kind, num_patterns, kinds, cubies, ks, tables, max_images, out, kC3Sym, false, (hipStream_t)stream);
}

int dca_cube3_pdb_eval_sym_host(const uint8_t* states, int64_t n, int64_t ld, int row_kind, int num_patterns, const int* kinds,
                                const uint8_t* cubies, const int* ks, const uint8_t* const* tables, int max_images, float* out) {
    return c3_eval_entry(__func__, states, n, ld, row_kind, num_patterns, kinds, cubies, ks, tables, max_images, out, kC3Sym, true, nullptr);
}

int dca_cube3_pdb_eval_dual(const uint8_t* states, int64_t n, int64_t ld, int row_kind, int num_patterns, const int* kinds,
                            const uint8_t* cubies, const int* ks, const uint8_t* const* tables, int max_images, float* out,
                            void* stream) {
    return c3_eval_entry(__func__, states, n, ld, row_kind, num_patterns, kinds, cubies, ks, tables, max_images, out, kC3Dual, false, (hipStream_t)stream);
}

int dca_cube3_pdb_eval_dual_host(const uint8_t* states, int64_t n, int64_t ld, int row_kind, int num_patterns, const int* kinds,
                                 const uint8_t* cubies, const int* ks, const uint8_t* const* tables, int max_images, float* out) {
    return c3_eval_entry(__func__, states, n, ld, row_kind, num_patterns, kinds, cubies, ks, tables, max_images, out, kC3Dual, true, nullptr);
}

int dca_cube3_inverse_locs(const uint8_t* row, int row_kind, uint64_t* words) {
    DCA_ARG(row != nullptr && words != nullptr);
    DCA_ARG(row_kind == DCA_ROWS_STATE || row_kind == DCA_ROWS_NNET);
    uint32_t w[14];
    pdb_load_row<54, 1>(row, w);
    const bool ids = row_kind == DCA_ROWS_STATE;
    words[0] = c3_inverse_locs<DCA_CUBE3_CORNERS, true>(ids ? c3_row_locs<DCA_CUBE3_CORNERS, DCA_ROWS_STATE>(w)
                                                            : c3_row_locs<DCA_CUBE3_CORNERS, DCA_ROWS_NNET>(w));
    words[1] = c3_inverse_locs<DCA_CUBE3_EDGES, true>(ids ? c3_row_locs<DCA_CUBE3_EDGES, DCA_ROWS_STATE>(w)
                                                          : c3_row_locs<DCA_CUBE3_EDGES, DCA_ROWS_NNET>(w));
    return 0;
}

int dca_cube3_sym_tables(uint8_t* sticker_perms, uint8_t* move_maps) {
    DCA_ARG(sticker_perms != nullptr && move_maps != nullptr);
    const Cube3Syms& t = c3_syms();
    if (t.broken != nullptr) {
        set_error("%s: the cube's symmetries could not be derived from the move table: %s", __func__, t.broken);
        return DCA_E_STATE;
    }
    for (int s = 0; s < kC3Syms; s++) {
        for (int p = 0; p < 54; p++) sticker_perms[s * 54 + p] = t.sticker[s][p];
        for (int a = 0; a < 12; a++) move_maps[s * 12 + a] = t.move[s][a];
    }
    return 0;
}

int dca_cube3_sym_images(int kind, const uint8_t* cubies, int k, int max_images, int* num_images, uint8_t* syms, uint8_t* sources,
                         uint8_t* maps) {
    const int64_t total = c3_bytes_checked(__func__, kind, k);
    if (total < 0) return (int)total;
    DCA_ARG(cubies != nullptr);
    DCA_ARG(num_images != nullptr);
    if (int rc = c3_check_cubies(__func__, kind, cubies, k)) return rc;
    C3Set set{};
    set.np = 1;
    set.kind[0] = (uint8_t)kind;
    set.k[0] = (uint8_t)k;
    set.pat[0] = pdb_pattern(cubies, k);
    set.kinds_used = 1 << kind;
    C3SymList list;
    if (int rc = c3_fill_sym_list(__func__, set, max_images, list)) return rc;
    *num_images = list.n;
    const int o = kind == DCA_CUBE3_CORNERS ? 3 : 2;
    for (int i = 0; i < list.n; i++) {
        if (syms) syms[i] = (uint8_t)(list.lk[i].meta >> 16);
        for (int j = 0; j < k; j++) {
            if (sources) sources[i * kPdbMaxK + j] = (uint8_t)(list.lk[i].shift[j] / 5);
            for (int l = 0; l < kC3Locs; l++) {  // the location, from the list's slot | r << 4
                const int to = list.lk[i].map[j][l];
                if (maps) maps[(i * kPdbMaxK + j) * kC3Locs + l] = (uint8_t)((to & 15) * o + (to >> 4));
            }
        }
    }
    return 0;
}

}  // extern "C"
