// dca_lightsout_exact.hip — the exact distance of a LightsOut state by a GF(2) solve (include/dca.h "exact LightsOut heuristic";
// `--env lightsout7 --model_dir exact:gf2`).  Presses commute and a cell pressed twice is not pressed, so a state is s = A x over
// GF(2): x the cells pressed an odd number of times, A[i][a] = lightsout_flip(DIM, a, i).  On the 7 x 7 board A is invertible:
// x = A^-1 s is the ONE press set that makes s, pressing its cells in any order is the shortest solution, h*(s) = popcount(x).
// A^-1 is derived at compile time from lightsout_flip (as cube3's cubies are from the move table) and reaches the kernel as
// instruction constants: no table, no memory traffic but the row itself.  One kernel, two outputs:
//
//   eval / solve   one thread per state row: the row's bytes in registers (pdb_load_row: word loads where the base pointer and
//                  the row stride allow them, byte loads otherwise), bit 0 of every byte folded into a 49-bit mask, then for
//                  every cell a the parity of popcount(Ainv[a] & mask).  eval writes popcount(x) as fp32, solve writes x.
//                  Nothing a row holds forms an address, so ANY bytes are in bounds.
//
// A few hundred integer operations per 49-byte row.  Rates are in profiles/lightsout_exact_probe.txt (device events only: what
// bounds the kernel, the row loads or the integer work, has not been measured with counters).
#include <utility>

#include "dca_pdb_shared.h"

namespace dca {

// ---------------------------------------------------------------------------------------------------------------- the inverse
template <int DIM>
struct LoInverse {
    uint64_t row[DIM * DIM];  // row a of A^-1: bit i = cell i of the state
    int rank;                 // of A; the rows are the inverse only when it is DIM * DIM
};

// Gauss-Jordan on [A | I] over GF(2), a row a 64-bit word
template <int DIM>
constexpr LoInverse<DIM> lightsout_inverse() {
    constexpr int N = DIM * DIM;
    static_assert(N <= 64, "a row of the board's matrix is one 64-bit word");
    uint64_t m[N] = {}, inv[N] = {};
    for (int i = 0; i < N; i++) {
        for (int a = 0; a < N; a++) m[i] |= (uint64_t)lightsout_flip(DIM, a, i) << a;
        inv[i] = 1ull << i;
    }
    LoInverse<DIM> out{};
    for (int col = 0; col < N; col++) {
        int piv = -1;
        for (int r = out.rank; r < N && piv < 0; r++)
            if ((m[r] >> col) & 1) piv = r;
        if (piv < 0) continue;  // a free column: the board has a null space
        const uint64_t tm = m[piv], ti = inv[piv];
        m[piv] = m[out.rank];
        inv[piv] = inv[out.rank];
        m[out.rank] = tm;
        inv[out.rank] = ti;
        for (int r = 0; r < N; r++)
            if (r != out.rank && ((m[r] >> col) & 1)) {
                m[r] ^= tm;
                inv[r] ^= ti;
            }
        out.rank++;
    }
    for (int a = 0; a < N; a++) out.row[a] = inv[a];  // full rank: m is the identity, pivot `col` sits in row `col`
    return out;
}

template <int DIM>
struct LoExact {
    static constexpr int N = DIM * DIM;
    static constexpr LoInverse<DIM> inverse = lightsout_inverse<DIM>();
    // A size with a null space (4 x 4, 5 x 5) has several press sets per state and would need a minimum over the cosets.
    static_assert(inverse.rank == DIM * DIM, "LightsOut: the board's press matrix is singular, A^-1 s is not its distance");
};

// bit i of the result = bit 0 of byte i of the row (words as pdb_load_row leaves them: little-endian, zero padded).  The
// multiply gathers a word's four low bits: bit 8 j of t lands on bit 24 + j, and no two of the sixteen partial products meet.
template <int N>
__host__ __device__ inline uint64_t lo_fold(const uint32_t (&w)[(N + 3) / 4]) {
    uint64_t mask = 0;
#pragma unroll
    for (int q = 0; q < (N + 3) / 4; q++) mask |= (uint64_t)((((w[q] & 0x01010101u) * 0x01020408u) >> 24) & 0xFu) << (4 * q);
    return mask;
}

// x = A^-1 s: bit a = the parity of the cells of s that row a of the inverse names (each row a compile-time constant)
template <int DIM, size_t... A>
__host__ __device__ inline uint64_t lo_press_set(uint64_t s, std::index_sequence<A...>) {
    return (((uint64_t)((uint32_t)__builtin_popcountll(s & LoExact<DIM>::inverse.row[A]) & 1u) << A) | ...);
}

template <int DIM>
__host__ __device__ inline uint64_t lo_solve_row(const uint32_t (&w)[(DIM * DIM + 3) / 4]) {
    return lo_press_set<DIM>(lo_fold<DIM * DIM>(w), std::make_index_sequence<DIM * DIM>{});
}

// Out = float: the distance popcount(x) (<= 49: exact); Out = uint64_t: the press set x itself
template <int DIM, int W, typename Out>
__global__ __launch_bounds__(kPdbThreads) void lightsout_exact_kernel(const uint8_t* __restrict__ states, int64_t n, int64_t ld,
                                                                      Out* __restrict__ out) {
    constexpr int N = DIM * DIM;
    const int64_t stride = (int64_t)gridDim.x * kPdbThreads;
    for (int64_t i = (int64_t)blockIdx.x * kPdbThreads + threadIdx.x; i < n; i += stride) {
        uint32_t w[(N + 3) / 4];
        pdb_load_row<N, W>(states + i * ld, w);
        const uint64_t x = lo_solve_row<DIM>(w);
        if constexpr (sizeof(Out) == sizeof(uint64_t))
            out[i] = x;
        else
            out[i] = (Out)__builtin_popcountll(x);
    }
}

template <int DIM, typename Out>
static int lightsout_exact_launch(const uint8_t* states, int64_t n, int64_t ld, Out* out, hipStream_t st) {
    const unsigned blocks = pdb_blocks((uint64_t)n, kPdbMaxEvalBlocks);
    if ((((uintptr_t)states | (uintptr_t)ld) & 3) == 0)
        hipLaunchKernelGGL((lightsout_exact_kernel<DIM, 4, Out>), dim3(blocks), dim3(kPdbThreads), 0, st, states, n, ld, out);
    else
        hipLaunchKernelGGL((lightsout_exact_kernel<DIM, 1, Out>), dim3(blocks), dim3(kPdbThreads), 0, st, states, n, ld, out);
    return launch_check("lightsout_exact_kernel");
}

static int lightsout_exact_dim_checked(const char* who, int dim) {
    if (dim != 7) {
        set_error("bad argument: %s: dim: the exact LightsOut heuristic is built for dim 7 only, not %d", who, dim);
        return DCA_E_BADARG;
    }
    return 0;
}

// what eval and solve share: every refusal before any HIP call, n == 0 launches nothing
template <typename Out>
static int lightsout_exact_run(const char* who, int dim, const uint8_t* states, int64_t n, int64_t ld, Out* out, const char* out_name,
                               void* stream) {
    if (int rc = lightsout_exact_dim_checked(who, dim)) return rc;
    if (n < 0 || n >= ((int64_t)1 << 31)) {
        set_error("bad argument: %s: n = %lld is not in 0..2^31-1", who, (long long)n);
        return DCA_E_BADARG;
    }
    if (ld < 49) {
        set_error("bad argument: %s: ld = %lld is below the row's 49 bytes", who, (long long)ld);
        return DCA_E_BADARG;
    }
    if (n == 0) return 0;
    if (states == nullptr) {
        set_error("bad argument: %s: states is NULL", who);
        return DCA_E_BADARG;
    }
    if (out == nullptr || ((uintptr_t)out & (sizeof(Out) - 1)) != 0) {
        set_error("bad argument: %s: %s is NULL or not %d-byte aligned", who, out_name, (int)sizeof(Out));
        return DCA_E_BADARG;
    }
    return lightsout_exact_launch<7, Out>(states, n, ld, out, (hipStream_t)stream);
}

}  // namespace dca

using namespace dca;

extern "C" {

int dca_lightsout_exact_matrix(int dim, uint64_t* rows) {
    if (int rc = lightsout_exact_dim_checked(__func__, dim)) return rc;
    DCA_ARG(rows != nullptr);
    for (int a = 0; a < LoExact<7>::N; a++) rows[a] = LoExact<7>::inverse.row[a];
    return 0;
}

int dca_lightsout_exact_eval(int dim, const uint8_t* states, int64_t n, int64_t ld, float* out, void* stream) {
    return lightsout_exact_run(__func__, dim, states, n, ld, out, "out", stream);
}

int dca_lightsout_exact_solve(int dim, const uint8_t* states, int64_t n, int64_t ld, uint64_t* presses, void* stream) {
    return lightsout_exact_run(__func__, dim, states, n, ld, presses, "presses", stream);
}

}  // extern "C"
