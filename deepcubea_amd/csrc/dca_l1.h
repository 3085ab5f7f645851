// dca_l1.h — what the layer-1 kernel files (dca_mlp.hip, dca_mlp8.hip, dca_embed.hip, dca_embed_train.hip) have in common,
// written once: the table of (state_dim, depth) geometries with its one dispatch, and the device pieces that more than one of
// the kernels spells the same way ("... and one for layer 1", also lists what stays written out and why).  K loops,
// MMA sequences and the tails' arithmetic stay with their kernels.  Everything here is __forceinline__, inline or constexpr
// (or a macro): no device symbol is shared between translation units.
#pragma once
#include "dca_dense.h"

namespace dca {

// ---- The geometries the project knows, once.  A kernel family says which of them it instantiates with a trait Family<D, DEPTH>
// that has `static constexpr bool built` (and whatever tile parameters its launcher wants next to it); its `supported` function
// and its dispatch are both l1_dispatch<Family>, so the list and the ladder cannot disagree.  A new geometry is one pair here
// plus `built` (and tile parameters) in the families that are to have it.
template <int D_, int DEPTH_>
struct L1Pair { static constexpr int D = D_, DEPTH = DEPTH_; };
template <class... P>
struct L1List {
    template <class F>
    static bool any(F&& one) { return (one(P{}) || ...); }
};
using L1Geometries = L1List<L1Pair<54, 6> /*cube3*/, L1Pair<9, 9> /*puzzle8*/, L1Pair<16, 16> /*puzzle15*/, L1Pair<25, 25> /*puzzle24*/,
                            L1Pair<36, 36> /*puzzle35*/, L1Pair<49, 49> /*puzzle48*/, L1Pair<49, 6> /*lightsout7*/>;
struct L1NotBuilt { static constexpr bool built = false; };  // base of a family's primary template; its built pairs are specialisations

// f(L1Pair<D, DEPTH>{})'s value — D and DEPTH compile-time constants — for the pair of the table that equals (state_dim, depth)
// and that Family has built; `not_built`, and f not called, for every other pair
template <template <int, int> class Family, class R, class F>
inline R l1_dispatch(int state_dim, int depth, R not_built, F&& f) {
    R r = not_built;
    L1Geometries::any([&](auto p) {
        if constexpr (Family<p.D, p.DEPTH>::built) {
            if (state_dim == p.D && depth == p.DEPTH) return r = f(p), true;
        }
        return false;
    });
    return r;
}
template <template <int, int> class Family>
inline bool l1_built(int state_dim, int depth) { return l1_dispatch<Family>(state_dim, depth, false, [](auto) { return true; }); }

// ---- The lean operand roles of the MFMA kernels (dca_mlp.hip has the story): weights = A operand, one-hot rows = B operand, and
// MFMA row i takes the weight column with bits 2 and 3 of i swapped, so that a lane's 8 consecutive accumulator registers are 8
// consecutive output columns of one state row.
// A macro, like the row maps of dca_dense.h: as a function it changed k_l1_onehot_gemm8's instructions (profiles/l1_shared_isa.txt).
#define DCA_L1_LEAN_WCOL(l31) (((l31) & 0x13) | (((l31) & 4) << 1) | (((l31) & 8) >> 1))

// The lean tails' exchange through a wave-private 4 KB LDS slice: 32 rows of 8 pieces of PB bytes, piece c of row `row` at slot
// c ^ (row & 7) — the writes (lane (l31, h) its own row l31) and the reads (lane (4 g + x, h) piece x * 2 + h of rows 4 g .. 4 g + 3,
// so that 8 lanes leave with one row segment) both meet every bank once.
template <int PB>
__device__ __forceinline__ uint8_t* l1_lean_piece(uint8_t* slice, int row, int c) { return slice + row * (8 * PB) + ((c ^ (row & 7)) * PB); }

// ---- fp32 -> the two fp16 planes the f16x3 layers read (x = hi + lo to 22 bits); beyond kF16Safe (or NaN) the value cannot be
// split (fp16 max 65504) and the caller redoes the batch in fp32.
constexpr float kF16Safe = 60000.0f;
__device__ __forceinline__ bool f16_unsafe(float v) { return !(fabsf(v) <= kF16Safe); }
__device__ __forceinline__ _Float16 f16_low_plane(float v, _Float16 hi) { return (_Float16)(v - (float)hi); }

// ---- 16 bytes of a byte matrix at offset `off`, of which only those in front of `end` exist: nothing is read past `end`, the
// missing bytes are zero (the last piece of a state matrix, or a matrix off the 16-byte grid).
__device__ __forceinline__ uint4 l1_load16_clipped(const uint8_t* __restrict__ base, int64_t off, int64_t end) {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < 16; e++)
        if (off + e < end) w[e >> 2] |= (uint32_t)base[off + e] << (8 * (e & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace dca
