// dca_gemm.hip — the dense layers of the cost-to-go network as ONE hand-written MFMA kernel per layer:
// an fp32-accurate GEMM on the f16 matrix pipes of gfx950 ("f16x3") with the whole layer tail in its epilogue.
//
// Reference arithmetic (utils/pytorch_models.py:57-86, BatchNorm folded): v = relu?(x . W^T + b (+ skip)), fp32.
// gfx950 has no TF32-like mode and its f32-input MFMA runs at 1/16 of the f16 rate, so the fp32 parity mode runs here
// on the f16 pipes instead: an fp32 value splits exactly into two fp16 numbers to 22 bits (x = xh + xl, xh = f16(x),
// xl = f16(x - xh)); with the weights split the same way (rows pre-scaled by a power of two so the low halves stay
// normal)          x.w = xh.wh + xl.wh + xh.wl + O(2^-22 |x.w|)          accumulated in the MFMA's fp32 accumulator.
//
// Round 1 expressed this as one LIBRARY f16 GEMM over a materialised 3x-wide operand plus a glue kernel per layer.
// This kernel keeps the operands as two fp16 PLANES (high / low halves; 4 bytes per activation, exactly what an fp32
// tensor costs — the 3x operand never exists), issues the three products per K-step from the same LDS fragments, and
// applies scale, bias, residual add, ReLU and the split of the RESULT into the next layer's planes in the epilogue: one
// launch per dense layer, activations cross HBM once in each direction.
//
// Tiling: workgroup = 128 x 128 outputs, 4 waves as 2 (M) x 2 (N), each wave 2 x 2 tiles of v_mfma_f32_32x32x16_f16
// (64 accumulator VGPRs).  K-step 64: the four operand images (A high/low, W high/low; 128 rows x 128 bytes each = 64 KB)
// are staged through registers — 16-byte coalesced global loads issued a whole K-step ahead of their LDS write, so they
// fly under the 48 MFMAs per wave of the current step — into row-major LDS rows whose 16-byte chunks are XOR-swizzled
// with (row >> 1) & 7: every ds_read_b128 lane group then touches each LDS bank exactly once.  Two workgroups per CU
// (2 x 64 KB LDS, <= 256 VGPRs) overlap one group's staging with the other's MFMAs.  Tile map, swizzles, the LDS-DMA call, the
// half-tile slots and the launchers' helpers are the shared ones of dca_dense.h.
#include <type_traits>

#include "dca_dense.h"

namespace dca {

constexpr int GBK = 64;  // K granularity of the planes (operands are padded to it)

struct GemmArgs {
    const _Float16 *ah, *al;  // activation planes [m, lda]
    const _Float16 *wh, *wl;  // weight planes [n, ldw] (row = output unit, pre-scaled by 1 / col_scale)
    const float* col_scale;   // [n] or null
    const float* bias;        // [n] or null
    const float* skip;        // [m, ldo] fp32 or null
    float alpha;
    int relu;
    int64_t m;
    int n, k;
    int64_t lda, ldw, ldo;
    _Float16 *oh, *ol;        // result planes [m, ldo] or null
    float* x_out;             // result fp32 [m, ldo] or null
    int* overflow;
};

// ---------------------------------------------------------------------------------------------------------------------
// v2 (default): 256 x 256 outputs per workgroup, 8 waves as 2 (M) x 4 (N), each wave 4 x 2 tiles of 32x32x16 (128
// accumulator VGPRs, 48 MFMAs per K-step of 32).  The four operand images of a K-step (256 rows x 64 B each = 64 KB) are
// filled by global_load_lds_dwordx4 — the LDS-DMA path: no staging registers, no ds_write pass — into one of TWO LDS
// stages, so the loads of step t+1 fly under the MFMAs of step t with a single raw s_barrier per K-step (a counted
// s_waitcnt in inline asm; __syncthreads() would drain the DMA queue).  An LDS-DMA instruction writes 64 lanes x 16 B
// linearly, so the image stays linear in LDS and the XOR swizzle that makes the ds_read_b128 fragment reads
// conflict-free (chunk ^ ((row >> 2) & 3) for 64-byte rows) is applied to each lane's GLOBAL source address instead:
// the four lanes of a row still read one contiguous 64-byte segment, in permuted order.
// (Round 1's first cut — 128 x 128 tiles, register staging, two barriers per K-step — measured 620 TF on the MFMA pipe and
// was deleted in round 5.)
// ---------------------------------------------------------------------------------------------------------------------
constexpr int HBM_T = 256, HBN_T = 256, HBK = 32, HTHREADS = 512;
constexpr int HIMG = 256 * HBK * 2;   // bytes of one operand image (16 KB)
constexpr int HSTAGE = 4 * HIMG;      // A high, A low, W high, W low
constexpr int HLDS = 2 * HSTAGE;      // two stages: 128 KB

// Round 6: the matrix instruction is v_mfma_f32_16x16x32_f16 (it was 32x32x16).  Same peak rate, less power per flop on random
// operands — MFMAs alone sustain 2030 instead of 1780 TFLOP/s at the chip's power limit (tools/mfma_power_probe.hip; csrc/
// dca_gemm16.hip has the story) — and these kernels run AT that limit.  A fragment of a 16-row block for one 32-deep K-step:
// lane (g = lane >> 4, j = lane & 15) holds row j, 16-byte chunk g of the 64-byte row; D = A . B: lane (g, j) holds D[4 g + r][j].
// The chunk swizzle of a 64-byte row is swz64 (dca_dense.h; it was the identity for the 32-row fragments).
__device__ __forceinline__ f32x4 mma16h(const f16x8& a, const f16x8& b, const f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// Layer tail of the 256 x 256 kernels (shared by the two-stage and the ping-pong schedule).
// MODE < 0: any shape, any form, every option tested at run time.  MODE >= 0 (bit 0 skip, bit 1 fp32 output, bit 2 planes): the
// same tail compiled for ONE of the network's layer forms on a tile that lies inside the matrix, with scale, bias and ReLU —
// no per-row / per-element tests left (round 5: the general tail is ~7400 instructions per wave, most of them branches around
// cases the network's own shapes never take; csrc/dca_gemm16.hip has the measurements that led here).
template <int MODE>
__device__ __forceinline__ void f16x3_epilogue_as(const GemmArgs& p, uint8_t* lds, const f32x4 (&acc)[8][4], int64_t m0, int n0, int w,
                                                  int wm, int wn, int lane, int l31, int h) {
    // accumulator layout: acc[ib][jb][r] = row ib * 16 + 4 g + r, column jb * 16 + j of the wave's 128 x 64 (g = lane >> 4, j = lane & 15)
    const int g4 = lane >> 4, j16 = lane & 15;
    // The accumulator layout (col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)) would make
    // every store a 4-byte (fp32) or 2-byte (planes) column access — measured 1.8 ms per layer, more than the K loop.  So
    // each wave transposes its tile through its own 16 KB of the (now idle) LDS, 32 rows at a time, and leaves with
    // 16-byte accesses: a lane owns 4 consecutive columns of a row — one float4 skip load, one float4 store, two 8-byte
    // plane stores; 16 lanes cover a row's 256 contiguous bytes.
    constexpr bool G = MODE < 0;  // general
    const bool has_skip = G ? p.skip != nullptr : (MODE & 1) != 0;
    const bool has_x = G ? p.x_out != nullptr : (MODE & 2) != 0;
    const bool has_planes = G ? p.oh != nullptr : (MODE & 4) != 0;
    const bool relu = G ? p.relu != 0 : true;
    float* sl = reinterpret_cast<float*>(lds + w * 16384);
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    float cs[4], bv[4];
#pragma unroll
    for (int jn = 0; jn < 4; jn++) {
        const int col = n0 + wn * 64 + jn * 16 + j16;
        const bool cv = G ? col < p.n : true;
        cs[jn] = cv ? ((G ? p.col_scale != nullptr : true) ? p.alpha * p.col_scale[col] : p.alpha) : 0.f;
        bv[jn] = (cv && (G ? p.bias != nullptr : true)) ? p.bias[col] : 0.f;
    }
    const int c4 = (lane & 15) * 4;              // this lane's 4 columns inside the wave's 64
    const int colg = n0 + wn * 64 + c4;
    const bool full4 = G ? colg + 3 < p.n : true;
    bool ovf = false;
#pragma unroll
    for (int i = 0; i < 4; i++) {
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int jb = 0; jb < 4; jb++)
#pragma unroll
                for (int r = 0; r < 4; r++) sl[(16 * b + 4 * g4 + r) * 64 + jb * 16 + j16] = acc[2 * i + b][jb][r] * cs[jb] + bv[jb];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // wave-private slice: no barrier, just the wave's own writes
        const int64_t rbase = m0 + wm * 128 + i * 32;
        float4 sk[8];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int64_t r = rbase + q * 4 + (lane >> 4);
            sk[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (has_skip && (G ? (r < p.m && full4) : true)) sk[q] = *reinterpret_cast<const float4*>(p.skip + r * p.ldo + colg);
        }
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int rl = q * 4 + (lane >> 4);
            const int64_t r = rbase + rl;
            const float4 v = *reinterpret_cast<const float4*>(sl + rl * 64 + c4);
            if (G && r >= p.m) continue;
            float u[4] = {v.x + sk[q].x, v.y + sk[q].y, v.z + sk[q].z, v.w + sk[q].w};
            const int64_t o = r * p.ldo + colg;
            if (full4) {
                h4 hi, lo;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    if (relu) u[e] = fmaxf(u[e], 0.f);
                    ovf |= !(fabsf(u[e]) <= 60000.0f);
                    hi[e] = (_Float16)u[e];
                    lo[e] = (_Float16)(u[e] - (float)hi[e]);
                }
                if (has_x) *reinterpret_cast<float4*>(p.x_out + o) = make_float4(u[0], u[1], u[2], u[3]);
                if (has_planes) {
                    *reinterpret_cast<h4*>(p.oh + o) = hi;
                    *reinterpret_cast<h4*>(p.ol + o) = lo;
                }
            } else {  // ragged right edge (n not a multiple of 4 columns here): element-wise
                for (int e = 0; e < 4 && colg + e < p.n; e++) {
                    float ue = u[e] + (has_skip ? p.skip[o + e] : 0.f);
                    if (relu) ue = fmaxf(ue, 0.f);
                    ovf |= !(fabsf(ue) <= 60000.0f);
                    if (has_x) p.x_out[o + e] = ue;
                    if (has_planes) {
                        const _Float16 hh = (_Float16)ue;
                        p.oh[o + e] = hh;
                        p.ol[o + e] = (_Float16)(ue - (float)hh);
                    }
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the slice is rewritten by the next 32 rows
    }
    if (ovf && has_planes && p.overflow) *p.overflow = 1;
}

__device__ __forceinline__ void f16x3_epilogue(const GemmArgs& p, uint8_t* lds, f32x4 (&acc)[8][4], int64_t m0, int n0, int w, int wm,
                                               int wn, int lane, int l31, int h) {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // every wave is done with the operand stages
    // the network's own layer forms on a tile inside the matrix (uniform over the workgroup) take a tail compiled for them
    const bool inside = m0 + HBM_T <= p.m && n0 + HBN_T <= p.n && p.relu && p.col_scale && p.bias;
    const int mode = inside ? ((p.skip ? 1 : 0) | (p.x_out ? 2 : 0) | (p.oh ? 4 : 0)) : -1;
    switch (mode) {
        case 4: f16x3_epilogue_as<4>(p, lds, acc, m0, n0, w, wm, wn, lane, l31, h); break;  // planes only (first layer of a block)
        case 6: f16x3_epilogue_as<6>(p, lds, acc, m0, n0, w, wm, wn, lane, l31, h); break;  // planes + fp32 (the 5120 -> 1024 layer)
        case 7: f16x3_epilogue_as<7>(p, lds, acc, m0, n0, w, wm, wn, lane, l31, h); break;  // residual: skip in, planes + fp32 out
        case 3: f16x3_epilogue_as<3>(p, lds, acc, m0, n0, w, wm, wn, lane, l31, h); break;  // last block: skip in, fp32 out
        default: f16x3_epilogue_as<-1>(p, lds, acc, m0, n0, w, wm, wn, lane, l31, h); break;
    }
}

__global__ __launch_bounds__(HTHREADS, 2) void k_f16x3_gemm_v2(const GemmArgs p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, l31 = lane & 31, h = lane >> 5;
    const int wm = w >> 2, wn = w & 3;
    const TileOfBlock tb = tile_of_block<HBM_T, HBN_T>(p.m, p.n);
    if (!tb.has) return;
    const int64_t m0 = tb.m0;
    const int n0 = tb.n0;

    // LDS-DMA map: instruction q of wave w fills rows [rb*16, rb*16+16) of image q >> 1, rb = (q & 1) * 8 + w; lane i
    // lands on row i >> 2, physical chunk i & 3, and therefore fetches logical chunk (i & 3) ^ ((row >> 2) & 3).
    // Rows past the matrix edge are clamped to the last row: their products are never stored.
    const _Float16* src[8];
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const int img = q >> 1;
        const uint32_t r = (uint32_t)(((q & 1) * 8 + w) * 16 + (lane >> 2));
        const uint32_t c = (uint32_t)(lane & 3) ^ swz64_key(r);
        if (img < 2) {
            int64_t gr = m0 + r;
            gr = gr < p.m ? gr : p.m - 1;
            src[q] = (img == 0 ? p.ah : p.al) + gr * p.lda + c * 8;
        } else {
            int gn = n0 + (int)r;
            gn = gn < p.n ? gn : p.n - 1;
            src[q] = (img == 2 ? p.wh : p.wl) + (int64_t)gn * p.ldw + c * 8;
        }
    }
    auto issue = [&](int stage, int k0) {
#pragma unroll
        for (int q = 0; q < 8; q++) {
            uint8_t* dst = lds + stage * HSTAGE + (q >> 1) * HIMG + ((q & 1) * 8 + w) * 1024;
            lds_dma16(src[q] + k0, dst);
        }
    };

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int jn = 0; jn < 4; jn++)
#pragma unroll
            for (int e = 0; e < 4; e++) acc[i][jn][e] = 0.f;
    const int g4 = lane >> 4, j16 = lane & 15;

    const int nk = p.k / HBK;
    issue(0, 0);
    for (int kt = 0; kt < nk; kt++) {
        // this wave's DMA of step kt has landed; the barrier makes that true of every wave's — and every wave has
        // finished reading the other stage, which the next issue overwrites
        // (lgkmcnt too: the fragment reads of step kt-1 must have RETURNED before any wave's next issue overwrites their
        // stage — their consumers are MFMAs, register-only, which the compiler may schedule below this point)
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (kt + 1 < nk) issue((kt + 1) & 1, (kt + 1) * HBK);
        const uint8_t* base = lds + (kt & 1) * HSTAGE;
        {  // one 32-deep step = one instruction deep
            const uint32_t c = (uint32_t)g4;
            f16x8 ah[8], al[8], wh[4], wl[4];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const uint32_t off = swz64((uint32_t)(wm * 128 + i * 16 + j16), c);
                ah[i] = *reinterpret_cast<const f16x8*>(base + off);
                al[i] = *reinterpret_cast<const f16x8*>(base + HIMG + off);
            }
#pragma unroll
            for (int jn = 0; jn < 4; jn++) {
                const uint32_t off = swz64((uint32_t)(wn * 64 + jn * 16 + j16), c);
                wh[jn] = *reinterpret_cast<const f16x8*>(base + 2 * HIMG + off);
                wl[jn] = *reinterpret_cast<const f16x8*>(base + 3 * HIMG + off);
            }
#pragma unroll
            for (int i = 0; i < 8; i++)
#pragma unroll
                for (int jn = 0; jn < 4; jn++) {
                    acc[i][jn] = mma16h(al[i], wh[jn], acc[i][jn]);
                    acc[i][jn] = mma16h(ah[i], wl[jn], acc[i][jn]);
                    acc[i][jn] = mma16h(ah[i], wh[jn], acc[i][jn]);
                }
        }
    }

    f16x3_epilogue(p, lds, acc, m0, n0, w, wm, wn, lane, l31, h);
}

// ---------------------------------------------------------------------------------------------------------------------
// v3 (default): the same tile and the same per-accumulator order of products as v2 (bit-identical results) on the
// ping-pong schedule of csrc/dca_gemm16.hip (variant 2; the derivation and the RAW / WAR argument are written out there):
// the two wave rows run one barrier apart — one issues the 12 MFMAs of its phase while the other reads the fragments of
// the next and issues DMA — a K-step (64 KB) is staged as four 16 KB half-tiles (A01 / A23 = each wave row's first / last
// two 32-row blocks, B0 / B1 = each wave column's first / last 32 columns; both fp16 planes of those rows, 64 B per row
// per plane), one restaged per phase, every half-tile given five phases to land, counted s_waitcnt vmcnt(10) — the DMA
// queue is never drained.  Phases: (A01,B0) (A01,B1) (A23,B1) (A23,B0); B0's fragments stay in registers for the fourth.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int PSLOT3 = 2 * 128 * 64;  // one half-tile: two planes of 128 rows x 64 B
constexpr int PBUF3 = 4 * PSLOT3;     // one K-step: A01 | A23 | B0 | B1

__global__ __launch_bounds__(HTHREADS, 2) void k_f16x3_gemm_v3(const GemmArgs p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, l31 = lane & 31, h = lane >> 5;
    const int wm = w >> 2, wn = w & 3;
    const TileOfBlock tb = tile_of_block<HBM_T, HBN_T>(p.m, p.n);
    if (!tb.has) return;
    const int64_t m0 = tb.m0;
    const int n0 = tb.n0;

    // DMA map: instruction q (0 = high plane, 1 = low plane) of wave w fills local rows [w*16, +16) of that plane of a
    // half-tile slot; lane i lands on local row r = w*16 + (i >> 2), physical chunk i & 3, and fetches logical chunk
    // (i & 3) ^ ((r >> 2) & 3) of the matrix row the slot's local row r stands for.
    const _Float16* src[4][2];
    {
        const uint32_t r = (uint32_t)(w * 16 + (lane >> 2));
        const uint32_t c = (uint32_t)(lane & 3) ^ swz64_key(r);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (u < 2) {
                int64_t gr = DCA_SLOT_ROW_A(m0, u, r);
                gr = gr < p.m ? gr : p.m - 1;
                src[u][0] = p.ah + gr * p.lda + c * 8;
                src[u][1] = p.al + gr * p.lda + c * 8;
            } else {
                int gn = n0 + DCA_SLOT_COL_B(u, r);
                gn = gn < p.n ? gn : p.n - 1;
                src[u][0] = p.wh + (int64_t)gn * p.ldw + c * 8;
                src[u][1] = p.wl + (int64_t)gn * p.ldw + c * 8;
            }
        }
    }
    auto issue = [&](int u, int buf, int k0) {
#pragma unroll
        for (int q = 0; q < 2; q++) {
            uint8_t* dst = lds + buf * PBUF3 + u * PSLOT3 + q * 8192 + w * 1024;
            lds_dma16(src[u][q] + k0, dst);
        }
    };

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int jn = 0; jn < 4; jn++)
#pragma unroll
            for (int e = 0; e < 4; e++) acc[i][jn][e] = 0.f;

    // fragment address inside a plane of a slot: local row = (wave's 16-row block) * 16 + j, logical chunk g
    const int g4 = lane >> 4, j16 = lane & 15;
    const uint32_t foff = swz64((uint32_t)j16, (uint32_t)g4);
    const uint32_t a_row0 = (uint32_t)wm * 64u * 64u;  // A slots: this wave row's 64 local rows (four 16-row blocks)
    const uint32_t b_row0 = (uint32_t)wn * 32u * 64u;  // B slots: this wave column's 32 local rows (two 16-row blocks)

    f16x8 avh[4], avl[4], wh0[2], wl0[2], wh1[2], wl1[2];
    auto read_a = [&](const uint8_t* base, int u) {
#pragma unroll
        for (int ii = 0; ii < 4; ii++) {
            avh[ii] = *reinterpret_cast<const f16x8*>(base + u * PSLOT3 + a_row0 + ii * 1024 + foff);
            avl[ii] = *reinterpret_cast<const f16x8*>(base + u * PSLOT3 + 8192 + a_row0 + ii * 1024 + foff);
        }
    };
    auto read_b = [&](const uint8_t* base, int u, f16x8 (&wh)[2], f16x8 (&wl)[2]) {
#pragma unroll
        for (int jj = 0; jj < 2; jj++) {
            wh[jj] = *reinterpret_cast<const f16x8*>(base + u * PSLOT3 + b_row0 + jj * 1024 + foff);
            wl[jj] = *reinterpret_cast<const f16x8*>(base + u * PSLOT3 + 8192 + b_row0 + jj * 1024 + foff);
        }
    };
    // 24 MFMAs: per accumulator the order of v2 (low x high, high x low, high x high), the eight accumulators of the phase
    // interleaved so that no MFMA waits on the one before it
#define DCA_MMA12(I0, JN, WH, WL)                                                                                       \
    do {                                                                                                                \
        __builtin_amdgcn_sched_barrier(0);                                                                              \
        __builtin_amdgcn_s_setprio(1);                                                                                  \
        _Pragma("unroll") for (int ii = 0; ii < 4; ii++) _Pragma("unroll") for (int jj = 0; jj < 2; jj++)               \
            acc[2 * (I0) + ii][2 * (JN) + jj] = mma16h(avl[ii], WH[jj], acc[2 * (I0) + ii][2 * (JN) + jj]);             \
        _Pragma("unroll") for (int ii = 0; ii < 4; ii++) _Pragma("unroll") for (int jj = 0; jj < 2; jj++)               \
            acc[2 * (I0) + ii][2 * (JN) + jj] = mma16h(avh[ii], WL[jj], acc[2 * (I0) + ii][2 * (JN) + jj]);             \
        _Pragma("unroll") for (int ii = 0; ii < 4; ii++) _Pragma("unroll") for (int jj = 0; jj < 2; jj++)               \
            acc[2 * (I0) + ii][2 * (JN) + jj] = mma16h(avh[ii], WH[jj], acc[2 * (I0) + ii][2 * (JN) + jj]);             \
        __builtin_amdgcn_s_setprio(0);                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                                              \
    } while (0)

    const int nk_all = p.k / HBK;
    const int nk = nk_all;
    // one K-step; N1 / N2: steps kt+1 / kt+2 exist (compile-time: the steady-state body is branch-free).  On entry:
    // issued = all of step kt and A01, B0, B1 of kt+1; landed and visible = A01, B0 of kt.  The vmcnt numbers count the
    // DMA instructions (2 per half-tile) issued AFTER the half-tile being waited for.
    auto step = [&](int kt, auto n1c, auto n2c) {
        constexpr bool N1 = decltype(n1c)::value, N2 = decltype(n2c)::value;
        const int b = kt & 1;
        const uint8_t* base = lds + b * PBUF3;
        // phase 1: (A01, B0); restage A23 of kt+1; retire B1 of kt
        read_b(base, PS_B0, wh0, wl0);
        read_a(base, PS_A01);
        if constexpr (N1) {
            issue(PS_A23, b ^ 1, (kt + 1) * HBK);
            DCA_VMCNT(10);  // behind B1(kt): A23(kt), A01 B0 B1 A23 (kt+1)
        } else {
            DCA_VMCNT(2);   // behind B1(kt): A23(kt)
        }
        DCA_RD_DONE_BAR();
        DCA_MMA12(0, 0, wh0, wl0);
        DCA_BAR();
        // phase 2: (A01, B1); restage A01 of kt+2; retire A23 of kt
        read_b(base, PS_B1, wh1, wl1);
        if constexpr (N2) {
            issue(PS_A01, b, (kt + 2) * HBK);
            DCA_VMCNT(10);  // behind A23(kt): A01 B0 B1 A23 (kt+1), A01(kt+2)
        } else if constexpr (N1) {
            DCA_VMCNT(8);
        } else {
            DCA_VMCNT(0);
        }
        DCA_RD_DONE_BAR();
        DCA_MMA12(0, 1, wh1, wl1);
        DCA_BAR();
        // phase 3: (A23, B1); restage B0 of kt+2
        read_a(base, PS_A23);
        if constexpr (N2) issue(PS_B0, b, (kt + 2) * HBK);
        DCA_RD_DONE_BAR();
        DCA_MMA12(2, 1, wh1, wl1);
        DCA_BAR();
        // phase 4: (A23, B0) from registers; restage B1 of kt+2; retire A01, B0 of kt+1
        if constexpr (N2) {
            issue(PS_B1, b, (kt + 2) * HBK);
            DCA_VMCNT(10);  // behind B0(kt+1): B1 A23 (kt+1), A01 B0 B1 (kt+2)
        } else if constexpr (N1) {
            DCA_VMCNT(4);   // behind B0(kt+1): B1 A23 (kt+1)
        }
        DCA_RD_DONE_BAR();
        DCA_MMA12(2, 0, wh0, wl0);
        DCA_BAR();
    };

    issue(PS_A01, 0, 0);
    issue(PS_B0, 0, 0);
    issue(PS_B1, 0, 0);
    issue(PS_A23, 0, 0);
    if (nk > 1) {
        issue(PS_A01, 1, HBK);
        issue(PS_B0, 1, HBK);
        issue(PS_B1, 1, HBK);
        DCA_VMCNT(10);  // A01, B0 of step 0 have landed
    } else {
        DCA_VMCNT(4);
    }
    DCA_BAR();
    if (wm == 1) DCA_BAR();  // the second wave row runs one barrier behind the first from here on
    {
        int kt = 0;
        for (; kt + 2 < nk; kt++) step(kt, std::true_type{}, std::true_type{});
        if (kt + 1 < nk) {
            step(kt, std::true_type{}, std::false_type{});
            kt++;
        }
        step(kt, std::false_type{}, std::false_type{});
    }
    if (wm == 0) DCA_BAR();  // ... and the first waits for it here
#undef DCA_MMA12

    f16x3_epilogue(p, lds, acc, m0, n0, w, wm, wn, lane, l31, h);
}

// ---------------------------------------------------------------------------------------------------------------------
// One-product kernel of the training step's NON-parity mode (`--train_gemm f16`): the high planes alone, 11-bit operands,
// fp32 accumulation — v2's tile, tile map, DMA map, swizzle, schedule (two whole-K-step stages, one wait + barrier per
// step) and epilogue, without the low images and without two of the three MFMAs per accumulator.  With a third of the
// MFMAs between two barriers a 32-deep step would be mostly barrier, so a K-step is 64 deep here (the entry point wants
// k % 64 == 0 anyway): a stage keeps v2's 64 KB and its four 16 KB images, which are now A[k0, k0+32) | A[k0+32, k0+64)
// | W[k0, k0+32) | W[k0+32, k0+64) — 64 MFMAs per wave and barrier instead of 32, the same eight DMA instructions per
// wave and step, and every image still a 256 x 64 B block that swz64 reads without bank conflicts.  Two stages = the
// 128 KB the epilogue's transposes need anyway.  Sums run over q ascending within an accumulator: no split-K, no atomics.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HTHREADS, 2) void k_f16_gemm(const GemmArgs p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, l31 = lane & 31, h = lane >> 5;
    const int wm = w >> 2, wn = w & 3;
    // tile_of_block(), written out: through the call one scalar register of the DMA setup gets another number, and this kernel's
    // instructions are pinned from the first LDS-DMA on (profiles/dense_header_isa.txt)
    const int nNt = (p.n + HBN_T - 1) / HBN_T;
    const int64_t nMt = (p.m + HBM_T - 1) / HBM_T;
    const int64_t bid = blockIdx.x;
    const int64_t slot = bid >> 3;
    const int64_t mt = (slot / nNt) * 8 + (bid & 7);
    const int nt = (int)(slot % nNt);
    if (mt >= nMt) return;
    const int64_t m0 = mt * HBM_T;
    const int n0 = nt * HBN_T;

    // LDS-DMA map (v2's): instruction q of wave w fills rows [rb*16, rb*16+16) of image q >> 1, rb = (q & 1) * 8 + w; lane i
    // lands on row i >> 2, physical chunk i & 3, and fetches logical chunk (i & 3) ^ swz64_key(row) of the image's 32 columns
    // (images 1 and 3 start 32 columns into the K-step).  Rows past the matrix edge are clamped: their products are never stored.
    const _Float16* src[8];
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const int img = q >> 1;
        const uint32_t r = (uint32_t)(((q & 1) * 8 + w) * 16 + (lane >> 2));
        const uint32_t c = (uint32_t)(lane & 3) ^ swz64_key(r);
        if (img < 2) {
            int64_t gr = m0 + r;
            gr = gr < p.m ? gr : p.m - 1;
            src[q] = p.ah + gr * p.lda + (img & 1) * HBK + c * 8;
        } else {
            int gn = n0 + (int)r;
            gn = gn < p.n ? gn : p.n - 1;
            src[q] = p.wh + (int64_t)gn * p.ldw + (img & 1) * HBK + c * 8;
        }
    }
    auto issue = [&](int stage, int k0) {
#pragma unroll
        for (int q = 0; q < 8; q++) {
            uint8_t* dst = lds + stage * HSTAGE + (q >> 1) * HIMG + ((q & 1) * 8 + w) * 1024;
            lds_dma16(src[q] + k0, dst);
        }
    };

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int jn = 0; jn < 4; jn++)
#pragma unroll
            for (int e = 0; e < 4; e++) acc[i][jn][e] = 0.f;
    const int g4 = lane >> 4, j16 = lane & 15;

    const int nk = p.k / GBK;
    issue(0, 0);
    for (int kt = 0; kt < nk; kt++) {
        // as in v2: this wave's DMA of step kt has landed and its fragment reads of step kt-1 have returned; behind the barrier
        // that is true of every wave, so the other stage may be overwritten
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (kt + 1 < nk) issue((kt + 1) & 1, (kt + 1) * GBK);
        const uint8_t* base = lds + (kt & 1) * HSTAGE;
#pragma unroll
        for (int s = 0; s < 2; s++) {  // the two 32-deep halves of the step, each one instruction deep
            const uint32_t c = (uint32_t)g4;
            f16x8 ah[8], wh[4];
#pragma unroll
            for (int i = 0; i < 8; i++)
                ah[i] = *reinterpret_cast<const f16x8*>(base + s * HIMG + swz64((uint32_t)(wm * 128 + i * 16 + j16), c));
#pragma unroll
            for (int jn = 0; jn < 4; jn++)
                wh[jn] = *reinterpret_cast<const f16x8*>(base + (2 + s) * HIMG + swz64((uint32_t)(wn * 64 + jn * 16 + j16), c));
#pragma unroll
            for (int i = 0; i < 8; i++)
#pragma unroll
                for (int jn = 0; jn < 4; jn++) acc[i][jn] = mma16h(ah[i], wh[jn], acc[i][jn]);
        }
    }

    f16x3_epilogue(p, lds, acc, m0, n0, w, wm, wn, lane, l31, h);
}

typedef _Float16 h4 __attribute__((ext_vector_type(4)));

// four floats -> their high fp16 plane at oh + at and, for PLANES == 2, what the rounding left as the low plane at ol + at
template <int PLANES>
__device__ __forceinline__ void store_planes(const float (&u)[4], _Float16* __restrict__ oh, _Float16* __restrict__ ol, int64_t at) {
    h4 hi, lo;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        hi[q] = (_Float16)u[q];
        lo[q] = (_Float16)(u[q] - (float)hi[q]);
    }
    *reinterpret_cast<h4*>(oh + at) = hi;
    if constexpr (PLANES == 2) *reinterpret_cast<h4*>(ol + at) = lo;
}

// fp32 [m, n] (row stride ld) -> its two fp16 planes (and the overflow flag): the entry into an f16x3 layer for
// activations that did not come out of an f16x3 epilogue
__global__ __launch_bounds__(256) void k_split_planes(const float* __restrict__ x, int64_t m, int64_t n, int64_t ld,
                                                      _Float16* __restrict__ oh, _Float16* __restrict__ ol,
                                                      int64_t ldo, int* __restrict__ overflow) {
    const int64_t n4 = n / 4;
    const int64_t total = m * n4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / n4, c = (i - r * n4) * 4;
        const float4 v = *reinterpret_cast<const float4*>(x + r * ld + c);
        const float u[4] = {v.x, v.y, v.z, v.w};
        h4 hi, lo;
#pragma unroll
        for (int k = 0; k < 4; k++) {  // (store_planes<2> with the overflow test in its loop)
            if (!(fabsf(u[k]) <= 60000.0f) && overflow) *overflow = 1;
            hi[k] = (_Float16)u[k];
            lo[k] = (_Float16)(u[k] - (float)hi[k]);
        }
        *reinterpret_cast<h4*>(oh + r * ldo + c) = hi;
        *reinterpret_cast<h4*>(ol + r * ldo + c) = lo;
    }
}

// ---- operands of the TRAINING step's dense layers (utils/nnet_utils.py train_nnet; reference nnet_utils.py:53-118 runs
// nn.Linear forward / backward as the library's fp32 GEMMs).  Forward y = x . W^T and backward dx = dy . W go through
// dca_f16x3_gemm too; what differs from inference is that nothing is prepared ahead: the weights change every step and the
// gradients span many binades.  So every operand is scaled by a POWER OF TWO chosen from its own magnitude before it is
// split (exact: only the exponent moves), bringing its largest element into [2^14, 2^15): the low plane of everything
// within 2^-10 of that is a normal fp16 number, what lies below is held to 2^-39 of the largest element.  The inverse scales
// come back through the GEMM's per-column factor.  (pow2_scale_of: dca_dense.h — the weight-gradient kernel undoes the same scales.)
// PLANES == 1 is the HIGH plane alone (the one-product GEMM and products = 1 of dca_wgrad_f16 read nothing else): the same
// scale, the same rounding (bit for bit plane 0 of PLANES == 2), the same zero pad, half the bytes written; ol is not looked at.

// max |x| as float bits (non-negative floats order like their bit patterns): four elements folded into a thread's maximum,
// and the maxima of a workgroup's 256 threads into one word that every thread gets back (wave shuffle, then 4 words of LDS)
__device__ __forceinline__ uint32_t absmax_fold(uint32_t mx, const float4 v) {
    return max(max(mx, __float_as_uint(fabsf(v.x))), max(__float_as_uint(fabsf(v.y)), max(__float_as_uint(fabsf(v.z)), __float_as_uint(fabsf(v.w)))));
}
__device__ __forceinline__ uint32_t absmax_block(uint32_t mx) {
    __shared__ uint32_t sh[4];
    uint32_t* mine = &sh[threadIdx.x >> 6];  // (taken in front of the shuffles: behind them the compiler places one shift elsewhere)
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
    if ((threadIdx.x & 63) == 0) *mine = mx;
    __syncthreads();
    return max(max(sh[0], sh[1]), max(sh[2], sh[3]));
}

// max |x| over the matrix; out zeroed by the host
__global__ __launch_bounds__(256) void k_absmax_bits(const float* __restrict__ x, int64_t m, int64_t n, int64_t ld,
                                                     uint32_t* __restrict__ out) {
    const int64_t n4 = n / 4, total = m * n4;
    uint32_t mx = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / n4, c = (i - r * n4) * 4;
        mx = absmax_fold(mx, *reinterpret_cast<const float4*>(x + r * ld + c));
    }
    mx = absmax_block(mx);
    if (threadIdx.x == 0) atomicMax(out, mx);
}

// x * 2^e -> planes, columns n..n_pad zero.  amax_bits == nullptr: no scaling.
template <int PLANES>
__global__ __launch_bounds__(256) void k_planes_scaled(const float* __restrict__ x, int64_t m, int64_t n, int64_t ld,
                                                       const uint32_t* __restrict__ amax_bits, _Float16* __restrict__ oh,
                                                       _Float16* __restrict__ ol, int64_t ldo, int64_t n_pad) {
    const float s = amax_bits ? pow2_scale_of(*amax_bits) : 1.0f;
    const int64_t n4 = n_pad / 4, total = m * n4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / n4, c = (i - r * n4) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < n) v = *reinterpret_cast<const float4*>(x + r * ld + c);
        const float u[4] = {v.x * s, v.y * s, v.z * s, v.w * s};
        store_planes<PLANES>(u, oh, ol, r * ldo + c);
    }
}

// one workgroup per row of w [n, k]: the row's own power-of-two scale, its planes (columns k..k_pad zero), and
// col_scale[row] = 1 / (row scale * scale of the OTHER operand, if its |max| is given)
template <int PLANES>
__global__ __launch_bounds__(256) void k_rows_scaled(const float* __restrict__ w, int64_t k, int64_t ld,
                                                     _Float16* __restrict__ oh, _Float16* __restrict__ ol, int64_t ldo,
                                                     int64_t k_pad, float* __restrict__ col_scale,
                                                     const uint32_t* __restrict__ other_amax_bits) {
    const int64_t r = blockIdx.x;
    const float* row = w + r * ld;
    const int64_t k4 = k / 4;
    uint32_t mx = 0;
    for (int64_t i = threadIdx.x; i < k4; i += 256) mx = absmax_fold(mx, *reinterpret_cast<const float4*>(row + i * 4));
    const float s = pow2_scale_of(absmax_block(mx));
    if (threadIdx.x == 0) {
        const float so = other_amax_bits ? pow2_scale_of(*other_amax_bits) : 1.0f;
        col_scale[r] = (1.0f / s) * (1.0f / so);  // powers of two: exact (2^-15-100 .. 2^+100: far inside fp32)
    }
    for (int64_t i = threadIdx.x; i < k_pad / 4; i += 256) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < k4) v = *reinterpret_cast<const float4*>(row + i * 4);  // (second read of the row: L2)
        const float u[4] = {v.x * s, v.y * s, v.z * s, v.w * s};
        store_planes<PLANES>(u, oh, ol, r * ldo + i * 4);
    }
}

__global__ void k_fill_inv_pow2(float* __restrict__ out, int64_t n, const uint32_t* __restrict__ amax_bits) {
    const float v = 1.0f / pow2_scale_of(*amax_bits);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = v;
}

}  // namespace dca

using namespace dca;

static int g_gemm_variant = 3;

// tile count, dynamic-LDS limit (once per device), launch: what dca_f16x3_gemm and dca_f16_gemm do once their arguments are accepted
static int launch_gemm(const char* entry, void (*kernel)(GemmArgs), const char* kernel_name, const GemmArgs& p, void* stream) {
    unsigned blocks;
    if (int rc = tile_grid(entry, p.m, p.n, HBM_T, HBN_T, &blocks)) return rc;
    static std::atomic<uint64_t> attr_devs{0};
    if (int rc = dynamic_lds_once(attr_devs, {reinterpret_cast<const void*>(k_f16x3_gemm_v2), reinterpret_cast<const void*>(k_f16x3_gemm_v3),
                                              reinterpret_cast<const void*>(k_f16_gemm)}, HLDS)) return rc;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(HTHREADS), HLDS, (hipStream_t)stream, p);
    return launch_check(kernel_name);
}

// DCA_ARG in the name of the entry point that handed its arguments on
#define DCA_ARG_OF(entry, cond)                                        \
    do {                                                               \
        if (!(cond)) {                                                 \
            ::dca::set_error("bad argument: %s: %s", entry, #cond);    \
            return DCA_E_BADARG;                                       \
        }                                                              \
    } while (0)

// what dca_split_planes_scaled (PLANES == 2) and dca_cast_planes_scaled (1: no out_l) do: argument clauses, grid, launch
template <int PLANES>
static int launch_planes_scaled(const char* entry, const float* x, int64_t m, int64_t n, int64_t ld, const uint32_t* amax_bits,
                                void* out_h, void* out_l, int64_t ldo, int64_t n_pad, void* stream) {
    DCA_ARG_OF(entry, x && out_h && (out_l || PLANES == 1) && m >= 0 && n >= 4 && n % 4 == 0 && ld >= n && ld % 4 == 0 && n_pad >= n &&
                          n_pad % 4 == 0 && ldo >= n_pad && ldo % 4 == 0);
    DCA_ARG_OF(entry, (uintptr_t)x % 16 == 0 && ((uintptr_t)out_h | (uintptr_t)out_l) % 8 == 0);  // float4 loads, 8-byte plane stores
    if (m == 0) return 0;
    int64_t blocks = (m * (n_pad / 4) + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_planes_scaled<PLANES>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, m, n, ld, amax_bits,
                       reinterpret_cast<_Float16*>(out_h), reinterpret_cast<_Float16*>(out_l), ldo, n_pad);
    return launch_check(PLANES == 2 ? "k_planes_scaled<2>" : "k_planes_scaled<1>");
}

// the same for dca_split_rows_scaled and dca_cast_rows_scaled: one workgroup per row
template <int PLANES>
static int launch_rows_scaled(const char* entry, const float* w, int64_t n, int64_t k, int64_t ld, void* out_h, void* out_l, int64_t ldo,
                              int64_t k_pad, float* col_scale, const uint32_t* other_amax_bits, void* stream) {
    DCA_ARG_OF(entry, w && out_h && (out_l || PLANES == 1) && col_scale && n >= 0 && n < (1ll << 31) && k >= 4 && k % 4 == 0 && ld >= k &&
                          ld % 4 == 0 && k_pad >= k && k_pad % 4 == 0 && ldo >= k_pad && ldo % 4 == 0);
    DCA_ARG_OF(entry, (uintptr_t)w % 16 == 0 && ((uintptr_t)out_h | (uintptr_t)out_l) % 8 == 0);
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_rows_scaled<PLANES>, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, w, k, ld,
                       reinterpret_cast<_Float16*>(out_h), reinterpret_cast<_Float16*>(out_l), ldo, k_pad, col_scale, other_amax_bits);
    return launch_check(PLANES == 2 ? "k_rows_scaled<2>" : "k_rows_scaled<1>");
}

extern "C" {

/* test hook: 2 = the LDS-DMA 256 x 256 kernel with two whole-K-step stages (the reference the race screens compare against),
 * 3 (default) = the same tile on the ping-pong / half-tile schedule (bit-identical to 2; measured at 204 800 x 1024, candidates
 * taking turns: k = 1024 1.42 vs 1.47 ms, k = 5120 5.67 vs 6.07 ms) */
int dca_f16x3_gemm_variant(int v) {
    DCA_ARG(v == 2 || v == 3);
    g_gemm_variant = v;
    return 0;
}

int dca_f16x3_gemm(const void* a_h, const void* a_l, int64_t m, int k, int64_t lda, const void* w_h, const void* w_l, int n,
                   int64_t ldw, const float* col_scale, double alpha, const float* bias, const float* skip, int relu,
                   void* out_h, void* out_l, float* x_out, int64_t ldo, int* overflow, void* stream) {
    DCA_ARG(a_h && a_l && w_h && w_l && m >= 0 && n >= 1 && k >= GBK && k % GBK == 0);  // (v2 alone would take k % 32)
    DCA_ARG(lda >= k && ldw >= k && lda % 8 == 0 && ldw % 8 == 0 && ldo >= n);
    DCA_ARG((out_h != nullptr) == (out_l != nullptr) && (out_h != nullptr || x_out != nullptr));
    DCA_ARG(((uintptr_t)a_h | (uintptr_t)a_l | (uintptr_t)w_h | (uintptr_t)w_l) % 16 == 0);
    // the kernels leave with 16-byte row segments: 4-column-aligned outputs (every layer of the network has them)
    DCA_ARG(ldo % 4 == 0 && ((uintptr_t)out_h | (uintptr_t)out_l) % 8 == 0 && ((uintptr_t)x_out | (uintptr_t)skip) % 16 == 0);
    if (m == 0) return 0;
    GemmArgs p{};
    p.ah = reinterpret_cast<const _Float16*>(a_h);
    p.al = reinterpret_cast<const _Float16*>(a_l);
    p.wh = reinterpret_cast<const _Float16*>(w_h);
    p.wl = reinterpret_cast<const _Float16*>(w_l);
    p.col_scale = col_scale;
    p.bias = bias;
    p.skip = skip;
    p.alpha = (float)alpha;
    p.relu = relu;
    p.m = m;
    p.n = n;
    p.k = k;
    p.lda = lda;
    p.ldw = ldw;
    p.ldo = ldo;
    p.oh = reinterpret_cast<_Float16*>(out_h);
    p.ol = reinterpret_cast<_Float16*>(out_l);
    p.x_out = x_out;
    p.overflow = overflow;
    return launch_gemm(__func__, g_gemm_variant == 2 ? k_f16x3_gemm_v2 : k_f16x3_gemm_v3, "k_f16x3_gemm", p, stream);
}

int dca_f16_gemm(const void* a_h, int64_t m, int k, int64_t lda, const void* w_h, int n, int64_t ldw, const float* col_scale,
                 double alpha, const float* bias, float* x_out, int64_t ldo, void* stream) {
    DCA_ARG(a_h && w_h && x_out && m >= 0 && n >= 1 && k >= GBK && k % GBK == 0);
    DCA_ARG(lda >= k && ldw >= k && lda % 8 == 0 && ldw % 8 == 0 && ldo >= n && ldo % 4 == 0);
    DCA_ARG(((uintptr_t)a_h | (uintptr_t)w_h | (uintptr_t)x_out) % 16 == 0);
    if (m == 0) return 0;
    GemmArgs p{};  // (no low planes, no skip, no ReLU, no result planes)
    p.ah = reinterpret_cast<const _Float16*>(a_h);
    p.wh = reinterpret_cast<const _Float16*>(w_h);
    p.col_scale = col_scale;
    p.bias = bias;
    p.alpha = (float)alpha;
    p.m = m;
    p.n = n;
    p.k = k;
    p.lda = lda;
    p.ldw = ldw;
    p.ldo = ldo;
    p.x_out = x_out;
    return launch_gemm(__func__, k_f16_gemm, "k_f16_gemm", p, stream);
}

int dca_split_planes(const float* x, int64_t m, int64_t n, int64_t ld, void* out_h, void* out_l, int64_t ldo, int* overflow,
                     void* stream) {
    DCA_ARG(x && out_h && out_l && m >= 0 && n >= 4 && n % 4 == 0 && ld >= n && ld % 4 == 0 && ldo >= n && ldo % 4 == 0);
    DCA_ARG((uintptr_t)x % 16 == 0 && ((uintptr_t)out_h | (uintptr_t)out_l) % 8 == 0);  // float4 loads, 8-byte plane stores
    if (m == 0) return 0;
    int64_t blocks = (m * (n / 4) + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_split_planes, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, m, n, ld,
                       reinterpret_cast<_Float16*>(out_h), reinterpret_cast<_Float16*>(out_l), ldo, overflow);
    return launch_check("k_split_planes");
}

int dca_absmax_bits(const float* x, int64_t m, int64_t n, int64_t ld, uint32_t* out_bits, void* stream) {
    DCA_ARG(x && out_bits && m >= 0 && n >= 4 && n % 4 == 0 && ld >= n && ld % 4 == 0 && (uintptr_t)x % 16 == 0);
    DCA_HIP(hipMemsetAsync(out_bits, 0, sizeof(uint32_t), (hipStream_t)stream));
    if (m == 0) return 0;
    int64_t blocks = (m * (n / 4) + 255) / 256;
    if (blocks > 768) blocks = 768;  // (one same-address atomic per workgroup: 4096 of them cost 50 us, whatever the matrix)
    hipLaunchKernelGGL(k_absmax_bits, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, m, n, ld, out_bits);
    return launch_check("k_absmax_bits");
}

int dca_split_planes_scaled(const float* x, int64_t m, int64_t n, int64_t ld, const uint32_t* amax_bits, void* out_h, void* out_l,
                            int64_t ldo, int64_t n_pad, void* stream) {
    return launch_planes_scaled<2>(__func__, x, m, n, ld, amax_bits, out_h, out_l, ldo, n_pad, stream);
}

int dca_cast_planes_scaled(const float* x, int64_t m, int64_t n, int64_t ld, const uint32_t* amax_bits, void* out_h, int64_t ldo,
                           int64_t n_pad, void* stream) {
    return launch_planes_scaled<1>(__func__, x, m, n, ld, amax_bits, out_h, nullptr, ldo, n_pad, stream);
}

int dca_split_rows_scaled(const float* w, int64_t n, int64_t k, int64_t ld, void* out_h, void* out_l, int64_t ldo, int64_t k_pad,
                          float* col_scale, const uint32_t* other_amax_bits, void* stream) {
    return launch_rows_scaled<2>(__func__, w, n, k, ld, out_h, out_l, ldo, k_pad, col_scale, other_amax_bits, stream);
}

int dca_cast_rows_scaled(const float* w, int64_t n, int64_t k, int64_t ld, void* out_h, int64_t ldo, int64_t k_pad, float* col_scale,
                         const uint32_t* other_amax_bits, void* stream) {
    return launch_rows_scaled<1>(__func__, w, n, k, ld, out_h, nullptr, ldo, k_pad, col_scale, other_amax_bits, stream);
}

int dca_fill_inv_pow2(float* out, int64_t n, const uint32_t* amax_bits, void* stream) {
    DCA_ARG(out && amax_bits && n >= 0);
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_fill_inv_pow2, dim3((unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024)), dim3(256), 0,
                       (hipStream_t)stream, out, n, amax_bits);
    return launch_check("k_fill_inv_pow2");
}

}  // extern "C"
