// dca_pdb_shared.h — what the pattern-database files share (dca_pdb.hip: sliding puzzles, additive; dca_pdb_cube3.hip: cube3,
// max): the limits, the set a kernel is handed, the host loop of a build, and the frame of an eval — row load, grid-stride
// kernel, launcher, its loop on the CPU and the entry points' set filling.  A family supplies the row value (eval) and
// the sweep (build); nothing here is dispatched at run time on the device.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <hip/hip_runtime.h>

#include "dca_common.h"

namespace dca {

constexpr int kPdbThreads = 256;
constexpr int kPdbMaxPatterns = 24;
constexpr int kPdbMaxK = 8;  // ids per pattern: N^(k+1) <= 2^34 allows k = 8 on puzzle8 (all tiles), P(12, 8) * 2^8 on cube3
constexpr int kPdbMaxBuildBlocks = 1 << 16;
constexpr int kPdbMaxEvalBlocks = 1 << 14;
constexpr uint8_t kPdbInf = 0xFE;  // a state the goal cannot be reached from (or: not reached yet, during the build)
constexpr int64_t kPdbMaxBytes = (int64_t)1 << 34;

struct PdbPattern {
    uint8_t id[kPdbMaxK];  // tiles (puzzles) or cubies (cube3)
};

// What every family's set starts with.  `int np` follows in the family's own struct: with np in here cube3's `kind` would move
// behind it, and that changed layout renumbered the scalar registers of its eval kernels (profiles/pdb_shared_isa.txt).
struct PdbTables {
    const uint8_t* table[kPdbMaxPatterns];
    PdbPattern pat[kPdbMaxPatterns];
    uint8_t k[kPdbMaxPatterns];
};

struct PdbSet : PdbTables {
    int np;
};

static PdbPattern pdb_pattern(const uint8_t* ids, int k) {
    PdbPattern pat{};
    for (int j = 0; j < k; j++) pat.id[j] = ids[j];
    return pat;
}

static unsigned pdb_blocks(uint64_t n, int cap) {
    const uint64_t b = (n + kPdbThreads - 1) / kPdbThreads;
    return (unsigned)(b < (uint64_t)cap ? b : (uint64_t)cap);
}

// ---------------------------------------------------------------------------------------------------------------- build
// The host loop of a build: sweeps 1, 2, ... until one leaves the device flag word 0.  `sweep(d, flag)` enqueues sweep d on
// `st` (the word is cleared in front of it) and returns a code; reading the word back synchronises the stream.  -> the code,
// and in `done` the sweeps run.  DCA_E_STATE when sweep `cap` still set the word: the caller words that message.
template <typename Sweep>
static int pdb_sweep_until_quiet(hipStream_t st, int cap, const char* who, Sweep sweep, int& done) {
    uint32_t* word = nullptr;
    DCA_HIP(hipMalloc((void**)&word, sizeof(uint32_t)));
    char what[96];
    int rc = 0;
    bool quiet = false;
    done = 0;
    while (rc == 0 && !quiet && done < cap) {
        uint32_t flag = 0;
        hipError_t e = hipMemsetAsync(word, 0, sizeof(uint32_t), st);
        if (e != hipSuccess) {
            snprintf(what, sizeof(what), "%s: hipMemsetAsync(sweep flag)", who);
            rc = hip_fail(e, what);
            break;
        }
        if ((rc = sweep(done + 1, word)) != 0) break;
        e = hipMemcpyAsync(&flag, word, sizeof(uint32_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            snprintf(what, sizeof(what), "%s: sweep flag read-back", who);
            rc = hip_fail(e, what);
            break;
        }
        done++;
        quiet = flag == 0;
    }
    (void)hipFree(word);
    return rc == 0 && !quiet ? DCA_E_STATE : rc;
}

// ---------------------------------------------------------------------------------------------------------------- eval
// the row as little-endian 32-bit words, zero padded: W-byte loads (W = what the base pointer and the row stride are both
// multiples of) for the whole units inside the row, single bytes where a unit would cross the row's end
template <int N, int W>
__host__ __device__ inline void pdb_load_row(const uint8_t* __restrict__ p, uint32_t (&w)[(N + 3) / 4]) {
    constexpr int NW = (N + 3) / 4;
#pragma unroll
    for (int q = 0; q < NW; q++) w[q] = 0;
    if constexpr (W == 4) {
#pragma unroll
        for (int q = 0; q < N / 4; q++) w[q] = *(const uint32_t*)(p + 4 * q);
#pragma unroll
        for (int i = N / 4 * 4; i < N; i++) w[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
    } else {
#pragma unroll
        for (int i = 0; i < N; i++) w[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
    }
}

// F, the family's eval: N bytes a row, the Set it reads, row_value(w, set) and the kernel's name in messages.  (The loop that
// keeps four table gathers in flight stays written out in each row_value: as a shared template it moved the puzzle eval
// kernels' registers and instructions, profiles/pdb_shared_isa.txt.)
template <typename F, int W>
__global__ __launch_bounds__(kPdbThreads) void pdb_eval_kernel(const uint8_t* __restrict__ states, int64_t n, int64_t ld,
                                                               typename F::Set set, float* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * kPdbThreads;
    for (int64_t i = (int64_t)blockIdx.x * kPdbThreads + threadIdx.x; i < n; i += stride) {
        uint32_t w[(F::N + 3) / 4];
        pdb_load_row<F::N, W>(states + i * ld, w);
        out[i] = (float)F::row_value(w, set);  // <= 24 * 255: exact
    }
}

template <typename F>
static int pdb_eval_launch(const uint8_t* states, int64_t n, int64_t ld, const typename F::Set& set, float* out, hipStream_t st) {
    const unsigned blocks = pdb_blocks((uint64_t)n, kPdbMaxEvalBlocks);
    if ((((uintptr_t)states | (uintptr_t)ld) & 3) == 0)
        hipLaunchKernelGGL((pdb_eval_kernel<F, 4>), dim3(blocks), dim3(kPdbThreads), 0, st, states, n, ld, set, out);
    else
        hipLaunchKernelGGL((pdb_eval_kernel<F, 1>), dim3(blocks), dim3(kPdbThreads), 0, st, states, n, ld, set, out);
    return launch_check(F::kernel_name);
}

// the eval frame's loop on the CPU: the kernels' own row load and row_value, one row after another (the *_host entry points)
template <typename F>
static void pdb_eval_rows_host(const uint8_t* states, int64_t n, int64_t ld, const typename F::Set& set, float* out) {
    for (int64_t i = 0; i < n; i++) {
        uint32_t w[(F::N + 3) / 4];
        pdb_load_row<F::N, 1>(states + i * ld, w);
        out[i] = (float)F::row_value(w, set);
    }
}

// An eval entry point's set from its arrays, every refusal before any HIP call: per pattern the family's `bytes(p)` (< 0: a
// code, the message set) and `ids_ok(p, ids)` (a code) over the pattern's ks[p] ids, then the NULL-table refusal and the copy.
template <typename Set, typename Bytes, typename IdsOk>
static int pdb_fill_set(const char* who, Set& set, int num_patterns, const uint8_t* ids, const int* ks, const uint8_t* const* tables,
                        Bytes bytes, IdsOk ids_ok) {
    set.np = num_patterns;
    for (int p = 0; p < num_patterns; p++) {
        const int64_t b = bytes(p);
        if (b < 0) return (int)b;
        if (int rc = ids_ok(p, ids)) return rc;
        if (tables[p] == nullptr) {
            set_error("bad argument: %s: tables: table %d is NULL", who, p);
            return DCA_E_BADARG;
        }
        set.table[p] = tables[p];
        set.k[p] = (uint8_t)ks[p];
        set.pat[p] = pdb_pattern(ids, ks[p]);
        ids += ks[p];
    }
    return 0;
}

}  // namespace dca
