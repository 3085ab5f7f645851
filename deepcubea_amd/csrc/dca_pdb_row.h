// dca_pdb_row.h — the row load the pattern-database eval kernels share (dca_pdb.hip, dca_pdb_cube3.hip).
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace dca {

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

}  // namespace dca
