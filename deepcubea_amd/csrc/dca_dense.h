// dca_dense.h — what the dense-layer MFMA kernel files (dca_gemm.hip, dca_gemm16.hip, dca_gemm8.hip, dca_wgrad.hip; the number
// formats also dca_mlp.hip) have in common, written once: tile map, LDS swizzles, the LDS-DMA call, the counted waits, the
// half-tile slots, number formats, and the launchers' grid / attribute / overlap rules ("One header").  Schedules,
// MMA macros and layer tails stay with their kernels.  Everything here is __forceinline__, inline or constexpr: no device symbol
// is shared between translation units.
#pragma once
#include <atomic>
#include <initializer_list>

#include "dca_common.h"

namespace dca {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

// ---- LDS images.  An LDS-DMA instruction writes 64 lanes x 16 B linearly, so an image stays linear in LDS and the XOR swizzle
// that makes the ds_read_b128 fragment reads conflict-free is applied to each lane's GLOBAL source address.
// 128-byte rows: chunk ^ ((row >> 1) & 7) — every lane group of a ds_read_b128 touches each LDS bank exactly once.
__device__ __forceinline__ uint32_t swz128(uint32_t row, uint32_t chunk) { return row * 128u + ((chunk ^ ((row >> 1) & 7u)) << 4); }
// 64-byte rows read as 16-row fragments of v_mfma_f32_16x16x32 (lane (g = lane >> 4, j = lane & 15) holds row j, chunk g): chunk ^
// f((row >> 2) & 3) with f = (0, 2, 3, 1) — the four lane groups of a ds_read_b128, {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and
// their upper twins, then meet 16 different (row & 3, slot) pairs, i.e. every bank group once.
__device__ __forceinline__ uint32_t swz64_key(uint32_t row) { return (0x78u >> (((row >> 2) & 3u) * 2u)) & 3u; }
__device__ __forceinline__ uint32_t swz64(uint32_t row, uint32_t chunk) { return row * 64u + ((chunk ^ swz64_key(row)) << 4); }

// 16 bytes per lane from global memory straight into LDS (global_load_lds_dwordx4: no staging registers, no ds_write pass)
__device__ __forceinline__ void lds_dma16(const void* src, uint8_t* dst) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
}

// raw barrier and counted waits of the K loops (__syncthreads() would drain the DMA queue; the count must be a literal)
#define DCA_BAR() asm volatile("s_barrier" ::: "memory")
#define DCA_RD_DONE_BAR() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
#define DCA_VMCNT(N) asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory")

// ---- Tile map: one workgroup per BM x BN tile, ids remapped so that the N tiles of one M tile sit on one XCD (workgroup b runs
// on XCD b % 8) — its L2 then reads the A tile from HBM once.  The grid is tile_grid()'s; `has` is false for the surplus ids.
struct TileOfBlock {
    int64_t m0;
    int n0;
    bool has;
};
template <int BM, int BN>
__device__ __forceinline__ TileOfBlock tile_of_block(int64_t m, int n) {
    const int nNt = (n + BN - 1) / BN;
    const int64_t nMt = (m + BM - 1) / BM;
    const int64_t bid = blockIdx.x;
    const int64_t slot = bid >> 3;
    const int64_t mt = (slot / nNt) * 8 + (bid & 7);
    const int nt = (int)(slot % nNt);
    return {mt * BM, nt * BN, mt < nMt};
}

// ---- Half-tile slots of the ping-pong schedules (dca_gemm16.hip variant 2 has the derivation): a K-step of a 256 x 256 tile is
// staged as A01 / A23 = each wave row's first / last two 32-row blocks, B0 / B1 = each wave column's first / last 32 columns.
constexpr int PS_A01 = 0, PS_A23 = 1, PS_B0 = 2, PS_B1 = 3;
// Local row r (0..127, uint32_t) of A slot u stands for this matrix row of the tile whose first row is M0 (int64_t); the three terms
// join the 64-bit row one by one.  A macro, not a function: a function is optimised on its own before it is inlined, and every
// spelling tried (profiles/dense_header_isa.txt) then changed the kernels' address arithmetic and with it their K loops.
#define DCA_SLOT_ROW_A(M0, u, r) ((M0) + ((r) >> 6) * 128 + ((u) == PS_A23 ? 64 : 0) + ((r) & 63))
// ... and of B slot u for this column of the tile (int)
#define DCA_SLOT_COL_B(u, r) ((int)(((r) >> 5) * 64 + ((u) == PS_B1 ? 32 : 0) + ((r) & 31)))

// ---- Number formats.  bf16: round to nearest even (what torch does), NaN stays NaN — gfx950's v_cvt_pk_bf16_f32, one instruction
// per two values where the integer sequence (NaN test, bias add, shift) took six per value.
__device__ __forceinline__ uint32_t f32_to_bf16x2(float lo, float hi) {
    const f32x2 v = {lo, hi};
    const bf16x2 b = __builtin_convertvector(v, bf16x2);
    uint32_t u;
    __builtin_memcpy(&u, &b, 4);
    return u;
}
__device__ __forceinline__ uint16_t f32_to_bf16(float f) { return (uint16_t)(f32_to_bf16x2(f, 0.f) & 0xFFFFu); }
__device__ __forceinline__ float bf16_to_f32(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }
__device__ __forceinline__ uint16_t f32_to_f16(float f) {
    const _Float16 h = (_Float16)f;
    uint16_t r;
    __builtin_memcpy(&r, &h, 2);
    return r;
}
__device__ __forceinline__ float f16_to_f32(uint16_t b) {
    _Float16 h;
    __builtin_memcpy(&h, &b, 2);
    return (float)h;
}
// four floats -> four e4m3 bytes (round to nearest even, saturating at +-448: e4m3fn has no infinity)
__device__ __forceinline__ uint32_t pack_e4m3(float a, float b, float c, float d) {
    a = fminf(fmaxf(a, -448.f), 448.f);
    b = fminf(fmaxf(b, -448.f), 448.f);
    c = fminf(fmaxf(c, -448.f), 448.f);
    d = fminf(fmaxf(d, -448.f), 448.f);
    uint32_t r = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    r = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(c, d, (int)r, true);
    return r;
}
// The power of two that brings a tensor whose max |x| has these float bits into [2^14, 2^15) before it is split into fp16 planes
// (the training step's operands, dca_gemm.hip): the low plane of everything within 2^-10 of the largest element is then normal.
__device__ __forceinline__ float pow2_scale_of(uint32_t amax_bits) {
    const int ex = (int)((amax_bits >> 23) & 0xFFu) - 127;        // floor(log2 amax) for a normal amax
    if (ex < -100 || ex > 100) return 1.0f;                       // zero / denormal / inf / nan: leave as is
    return __uint_as_float((uint32_t)(127 + 14 - ex) << 23);
}

// ---- Launchers.
// Grid of tile_of_block(): ceil(nMt / 8) * 8 * nNt workgroups; refused, in the entry point's name, if that is no grid dimension.
inline int tile_grid(const char* entry, int64_t m, int n, int bm, int bn, unsigned* blocks) {
    const int64_t nMt = (m + bm - 1) / bm, nNt = (n + bn - 1) / bn;
    const int64_t b = ((nMt + 7) / 8) * 8 * nNt;
    if (b > 0x7FFFFFFFll) {
        set_error("%s: too many tiles", entry);
        return DCA_E_BADARG;
    }
    *blocks = (unsigned)b;
    return 0;
}
// The dynamic-LDS limit is a per-device function attribute: set it once per process for every device the process uses.  `devs`
// is the launcher's own static bit set of the devices already served (thread-safe: at worst two threads set the same value).
inline int dynamic_lds_once(std::atomic<uint64_t>& devs, std::initializer_list<const void*> kernels, int bytes) {
    int dev = 0;
    DCA_HIP(hipGetDevice(&dev));
    const uint64_t bit = 1ull << (dev & 63);
    if (!(devs.load(std::memory_order_acquire) & bit)) {
        for (const void* kernel : kernels) DCA_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        devs.fetch_or(bit, std::memory_order_release);
    }
    return 0;
}
// Bytes [lo, hi) of an [m, cols] matrix of esz-byte elements with row stride ld (m == 0: empty) and whether two of them meet: the
// operand tiles are re-read through LDS-DMA while the epilogues of other tiles write, so no output may overlap the operand.
struct ByteRange {
    uintptr_t lo, hi;
};
inline ByteRange rows_range(const void* p, int64_t m, int64_t cols, int64_t ld, size_t esz) {
    const uintptr_t lo = (uintptr_t)p;
    return {lo, lo + (m > 0 ? ((size_t)(m - 1) * (size_t)ld + (size_t)cols) * esz : 0)};
}
inline bool ranges_overlap(ByteRange a, ByteRange b) { return a.lo < b.hi && b.lo < a.hi; }

}  // namespace dca
