// dca_wgrad.hip — weight gradient of the training step's dense layers, dW = dy^T . x, from the fp16 planes the step already has.
//
// Reference arithmetic (utils/nnet_utils.py:53-118 calls loss.backward(); nn.Linear's weight gradient is the library's fp32 GEMM
// dy.t().mm(x)):      dW[j, c] = sum over the batch rows r of dy[r, j] * x[r, c].
// The contraction index is the ROW of both operands: dy [m, n] and x [m, k] are row-major with the batch index as the row, which
// is how linear_f16x3 leaves their planes (vh = f16(v * 2^e), vl = f16(v * 2^e - vh); dca_split_planes_scaled).  A GEMM kernel that
// reads its fragments along rows would want both transposed (round 4 paid 0.46 ms per step for exactly that); here the tiles go
// into LDS as they lie in memory and gfx950's transposing LDS read delivers them column-major:
//
//   * a workgroup (256 threads, 2 x 2 waves) owns a 128 x 128 tile of dW and one slice of the batch; a wave owns 64 x 64 of it,
//     4 x 4 accumulators of v_mfma_f32_16x16x32_f16;
//   * the slice goes by in K-tiles of KT = 32 batch rows: [32][128] fp16 of every plane (256-byte rows), loaded 16 bytes per lane
//     into registers one K-tile ahead and parked in LDS between two barriers.  Rows past the slice and columns past pad64(width)
//     are ZEROS in LDS — the transposing read needs EXEC all ones, nothing is masked;
//   * LDS image: plain 256-byte rows with the chunk XOR  off(row, ch) = 256 row + 16 (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))),
//     ch = 16-byte chunk of the row.  Stores and reads both go through lds_off().  A 32-lane half of ds_read_b64_tr_b16 takes two
//     4-row blocks 8 rows apart in the same 16 columns: 8 rows x 32 bytes whose XORed chunk pairs are all different, 64 distinct
//     banks, conflict-free (the XOR can swap the two 16-byte chunks of a block's 32 bytes: never address a block as base + 8 p);
//   * both MFMA operands come from the same read pattern: the 16-lane group g of a wave reads rows 8 g .. 8 g + 3 and 8 g + 4 ..
//     8 g + 7 of the K-tile at 16 columns, lane i of the group receives column i — A[i][kk] = dy[r0 + kk][n0 + i] and
//     B[kk][i] = x[r0 + kk][k0 + i] with kk = 8 g + e for element e.  Whatever order the hardware gives the 8 rows inside a lane,
//     it is the same for both operands;
//   * products = 3: dyh.xh + dyh.xl + dyl.xh into one fp32 accumulator (the lo.lo term is below fp32: dca_f16x3_gemm's
//     arithmetic); products = 1: dyh.xh alone, 11-bit operands, a third of the matrix work;
//   * the batch is cut into S = dca_wgrad_splits(m, n, k) slices (the layers' 64-320 tiles do not fill 256 CUs); with S > 1 a
//     workgroup leaves its partial tile in the fp32 workspace [S][n][k] and k_wgrad_fold adds the slices in ascending order and
//     applies 2^-(e_dy + e_x); with S == 1 the tile is scaled and written straight to dW.  No atomics: the bits depend on the
//     inputs and the sizes alone.
// Measured (profiles/wgrad_probe.txt, batch 10 000, library fp32 GEMM / products 3 / products 1, ms): 5000 x 324 0.33 / 0.17 / 0.10,
// 1000 x 5000 0.91 / 0.40 / 0.23, 1000 x 1000 0.17 / 0.11 / 0.08; the fold is 6-8 us.  Built, measured, removed: two LDS buffers and
// one barrier per K-tile — 0.44 against 0.40 ms at 1000 x 5000: the barriers are not what bounds it.
#include "dca_dense.h"

namespace dca {

// every pointer a kernel dereferences is a global-memory pointer (global_* accesses on vmcnt alone, never flat_*: DCA_GLOBAL)
template <class T>
using gp = T DCA_GLOBAL*;

constexpr int WG_TN = 128, WG_TK = 128;   // tile of dW: rows (dy's columns) x columns (x's columns)
constexpr int WG_KT = 32;                 // batch rows per K-tile = one k-step of the 16x16x32 MFMA
constexpr int WG_THREADS = 256;
constexpr int WG_PLANE_BYTES = WG_KT * 256;
constexpr int64_t WG_MIN_SLICE = 256;     // no slice shorter than this many rows (8 K-tiles)
constexpr int WG_FILL = 256;              // workgroups that fill the machine (one per CU)

typedef short s4v __attribute__((ext_vector_type(4)));
typedef short s8v __attribute__((ext_vector_type(8)));

// undoes the scale dca_split_planes_scaled derives from max|v| (pow2_scale_of, dca_dense.h)
__device__ __forceinline__ float wg_inv_scale(gp<const uint32_t> amax_bits) { return amax_bits ? 1.0f / pow2_scale_of(*amax_bits) : 1.0f; }

// byte offset of 16-byte chunk ch (0..15) of row `row` inside a plane's K-tile
__device__ __forceinline__ uint32_t lds_off(uint32_t row, uint32_t ch) {
    return 256u * row + 16u * (ch ^ (((row & 3u) << 2) | ((row >> 2) & 3u)));
}

// ds_read_b64_tr_b16 at LDS byte address `a` (8-byte aligned, EXEC all ones)
__device__ __forceinline__ s4v tr_read(uint32_t a) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((DCA_LDS s4v*)(uintptr_t)a);
#else
    return s4v{};
#endif
}
__device__ __forceinline__ f16x8 frag_of(s4v a, s4v b) {
    return __builtin_bit_cast(f16x8, (s8v)__builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
}

struct WgradArgs {
    const _Float16 *dyh, *dyl, *xh, *xl;  // (dyl / xl unused when products == 1)
    int64_t ld_dy, ld_x, m, slice_rows;
    int n, k, tiles_k, tiles;
    float* out;                           // dW (S == 1) or the workspace
    int64_t ld_out, slice_stride;         // workspace: ld_out = k, slice_stride = n * k
    const uint32_t *amax_dy, *amax_x;     // applied here only when S == 1 (NULL otherwise, and NULL = scale 1)
};

template <int PRODUCTS>
__global__ __launch_bounds__(WG_THREADS, 2) void k_wgrad(const WgradArgs p) {
    constexpr int NPL = PRODUCTS == 3 ? 2 : 1;  // planes per operand
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * NPL * WG_PLANE_BYTES];  // dy planes, then x planes
    const uint32_t lbase = (uint32_t)(uintptr_t)((DCA_LDS uint8_t*)lds);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wn = wave >> 1, wk = wave & 1;
    const uint32_t slice = blockIdx.x / (uint32_t)p.tiles, tile = blockIdx.x - slice * (uint32_t)p.tiles;
    const int tn = (int)(tile / (uint32_t)p.tiles_k), tk = (int)(tile - (uint32_t)tn * (uint32_t)p.tiles_k);
    const int n0 = tn * WG_TN, k0 = tk * WG_TK;
    const int64_t r_begin = (int64_t)slice * p.slice_rows;
    const int64_t r_end = r_begin + p.slice_rows < p.m ? r_begin + p.slice_rows : p.m;
    const int padn = (p.n + 63) / 64 * 64, padk = (p.k + 63) / 64 * 64;  // the planes hold zeros up to here

    // staging: thread t carries chunk (t & 15) of rows (t >> 4) and (t >> 4) + 16 of every plane's K-tile
    const int s_ch = t & 15, s_row = t >> 4;
    const bool dy_in = n0 + 8 * s_ch < padn, x_in = k0 + 8 * s_ch < padk;
    gp<const _Float16> src[2 * NPL];
    src[0] = (gp<const _Float16>)p.dyh + n0 + 8 * s_ch;
    src[NPL] = (gp<const _Float16>)p.xh + k0 + 8 * s_ch;
    if constexpr (NPL == 2) {
        src[1] = (gp<const _Float16>)p.dyl + n0 + 8 * s_ch;
        src[NPL + 1] = (gp<const _Float16>)p.xl + k0 + 8 * s_ch;
    }
    u32x4 pre[2 * NPL][2];
    auto prefetch = [&](int64_t r0) {
#pragma unroll
        for (int q = 0; q < 2 * NPL; q++) {
            const bool in = q < NPL ? dy_in : x_in;
            const int64_t ld = q < NPL ? p.ld_dy : p.ld_x;
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int64_t r = r0 + s_row + 16 * u;
                pre[q][u] = u32x4{0u, 0u, 0u, 0u};
                if (in && r < r_end) pre[q][u] = *(gp<const u32x4>)(src[q] + r * ld);
            }
        }
    };
    uint32_t st_off[2];
#pragma unroll
    for (int u = 0; u < 2; u++) st_off[u] = lds_off((uint32_t)(s_row + 16 * u), (uint32_t)s_ch);

    // fragment reads: group g = lane >> 4 of the wave, lane 4 q + pp of the group supplies row 8 g + 4 h + q, columns 4 pp .. 4 pp + 3
    // of the block's 16 — chunk (pp >> 1) of the block's two, byte 8 (pp & 1) inside it
    const uint32_t g = (uint32_t)lane >> 4, q4 = ((uint32_t)lane >> 2) & 3u, pp = (uint32_t)lane & 3u;
    uint32_t a_addr[4][2], b_addr[4][2];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t row = 8u * g + 4u * (uint32_t)h + q4;
            a_addr[i][h] = lbase + lds_off(row, (uint32_t)(8 * wn + 2 * i) + (pp >> 1)) + 8u * (pp & 1u);
            b_addr[i][h] = lbase + (uint32_t)(NPL * WG_PLANE_BYTES) + lds_off(row, (uint32_t)(8 * wk + 2 * i) + (pp >> 1)) + 8u * (pp & 1u);
        }

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    prefetch(r_begin);
    for (int64_t r0 = r_begin; r0 < r_end; r0 += WG_KT) {
#pragma unroll
        for (int q = 0; q < 2 * NPL; q++)
#pragma unroll
            for (int u = 0; u < 2; u++) *reinterpret_cast<u32x4*>(lds + q * WG_PLANE_BYTES + st_off[u]) = pre[q][u];
        __syncthreads();
        if (r0 + WG_KT < r_end) prefetch(r0 + WG_KT);
        f16x8 bh[4], bl[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            bh[j] = frag_of(tr_read(b_addr[j][0]), tr_read(b_addr[j][1]));
            if (NPL == 2) bl[j] = frag_of(tr_read(b_addr[j][0] + WG_PLANE_BYTES), tr_read(b_addr[j][1] + WG_PLANE_BYTES));
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const f16x8 ah = frag_of(tr_read(a_addr[i][0]), tr_read(a_addr[i][1]));
            f16x8 al;
            if (NPL == 2) al = frag_of(tr_read(a_addr[i][0] + WG_PLANE_BYTES), tr_read(a_addr[i][1] + WG_PLANE_BYTES));
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (NPL == 2) {  // the two cross terms first, the leading term last
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh[j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl[j], acc[i][j], 0, 0, 0);
                }
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh[j], acc[i][j], 0, 0, 0);
            }
        }
        __syncthreads();  // every wave has read the K-tile: it may be overwritten
    }

    // accumulator (i, j): rows n0 + 64 wn + 16 i + 4 (lane >> 4) + e of dW, column k0 + 64 wk + 16 j + (lane & 15)
    const float inv_dy = wg_inv_scale((gp<const uint32_t>)p.amax_dy), inv_x = wg_inv_scale((gp<const uint32_t>)p.amax_x);
    gp<float> out = (gp<float>)p.out + (int64_t)slice * p.slice_stride;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int col = k0 + 64 * wk + 16 * j + (lane & 15);
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int row = n0 + 64 * wn + 16 * i + 4 * (lane >> 4) + e;
                if (row < p.n && col < p.k) out[(int64_t)row * p.ld_out + col] = acc[i][j][e] * inv_dy * inv_x;
            }
        }
}

// dW[j, c] = 2^-(e_dy + e_x) * (slab 0 + slab 1 + ...), ascending slice order, fp32
__global__ __launch_bounds__(256) void k_wgrad_fold(const float* ws_, int nslices, int64_t n, int64_t k, const uint32_t* amax_dy,
                                                    const uint32_t* amax_x, float* dw_, int64_t ld_dw) {
    gp<const float> ws = (gp<const float>)ws_;
    gp<float> dw = (gp<float>)dw_;
    const float inv_dy = wg_inv_scale((gp<const uint32_t>)amax_dy), inv_x = wg_inv_scale((gp<const uint32_t>)amax_x);
    const int64_t nk = n * k;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nk; i += (int64_t)gridDim.x * 256) {
        float acc = ws[i];
        for (int s = 1; s < nslices; s++) acc += ws[(int64_t)s * nk + i];
        const int64_t j = i / k;
        dw[j * ld_dw + (i - j * k)] = acc * inv_dy * inv_x;
    }
}

// rows per slice: enough slices that tiles x slices reaches one workgroup per CU, no slice under WG_MIN_SLICE rows, the length a
// multiple of the K-tile.  A function of (m, n, k) alone: the summation order is part of the ABI.
static int64_t wgrad_slice_rows(int64_t m, int n, int k) {
    const int64_t tiles = (int64_t)((n + WG_TN - 1) / WG_TN) * ((k + WG_TK - 1) / WG_TK);
    int64_t want = (WG_FILL + tiles - 1) / tiles;
    const int64_t cap = (m + WG_MIN_SLICE - 1) / WG_MIN_SLICE;
    if (want > cap) want = cap;
    if (want < 1) want = 1;
    const int64_t rows = (m + want - 1) / want;
    return (rows + WG_KT - 1) / WG_KT * WG_KT;
}

static bool wgrad_sizes_ok(int64_t m, int n, int k) { return m >= 1 && n >= 4 && k >= 4 && n % 4 == 0 && k % 4 == 0; }

}  // namespace dca

using namespace dca;

extern "C" {

int dca_wgrad_splits(int64_t m, int n, int k) {
    if (!wgrad_sizes_ok(m, n, k)) {
        set_error("dca_wgrad_splits: bad sizes (m %lld, n %d, k %d)", (long long)m, n, k);
        return DCA_E_BADARG;
    }
    const int64_t rows = wgrad_slice_rows(m, n, k);
    return (int)((m + rows - 1) / rows);
}

int64_t dca_wgrad_workspace_bytes(int64_t m, int n, int k) {
    const int S = dca_wgrad_splits(m, n, k);
    if (S < 0) return S;
    return S == 1 ? 0 : (int64_t)S * n * k * 4;
}

int dca_wgrad_f16(const void* dy_h, const void* dy_l, int64_t ld_dy, const void* x_h, const void* x_l, int64_t ld_x, int64_t m, int n,
                  int k, const uint32_t* amax_dy_bits, const uint32_t* amax_x_bits, int products, float* dw, int64_t ld_dw,
                  void* workspace, int64_t workspace_bytes, void* stream) {
    DCA_ARG(products == 1 || products == 3);
    DCA_ARG(m >= 1 && n >= 4 && k >= 4 && n % 4 == 0 && k % 4 == 0);
    DCA_ARG(ld_dy >= (n + 63) / 64 * 64 && ld_x >= (k + 63) / 64 * 64 && ld_dy % 8 == 0 && ld_x % 8 == 0 && ld_dw >= k);
    DCA_ARG(dy_h && x_h && dw && (products == 1 || (dy_l && x_l)));
    DCA_ARG(((uintptr_t)dy_h | (uintptr_t)x_h) % 16 == 0 && (products == 1 || ((uintptr_t)dy_l | (uintptr_t)x_l) % 16 == 0));
    DCA_ARG((uintptr_t)dw % 4 == 0 && ((uintptr_t)amax_dy_bits | (uintptr_t)amax_x_bits) % 4 == 0);
    const int64_t rows = wgrad_slice_rows(m, n, k), S = (m + rows - 1) / rows;
    const int64_t need = S == 1 ? 0 : S * n * k * 4;
    if (need > 0 && (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 3))) {
        set_error("dca_wgrad_f16: workspace of %lld bytes at %p, %lld needed (4-byte aligned)", (long long)workspace_bytes, workspace,
                  (long long)need);
        return DCA_E_BADARG;
    }
    WgradArgs p;
    p.dyh = reinterpret_cast<const _Float16*>(dy_h);
    p.dyl = reinterpret_cast<const _Float16*>(dy_l);
    p.xh = reinterpret_cast<const _Float16*>(x_h);
    p.xl = reinterpret_cast<const _Float16*>(x_l);
    p.ld_dy = ld_dy;
    p.ld_x = ld_x;
    p.m = m;
    p.slice_rows = rows;
    p.n = n;
    p.k = k;
    p.tiles_k = (k + WG_TK - 1) / WG_TK;
    p.tiles = ((n + WG_TN - 1) / WG_TN) * p.tiles_k;
    if ((int64_t)p.tiles * S > 0x7fffffffll) {
        set_error("dca_wgrad_f16: %d tiles x %lld slices exceed the grid", p.tiles, (long long)S);
        return DCA_E_BADARG;
    }
    const bool direct = S == 1;
    p.out = direct ? dw : reinterpret_cast<float*>(workspace);
    p.ld_out = direct ? ld_dw : k;
    p.slice_stride = direct ? 0 : (int64_t)n * k;
    p.amax_dy = direct ? amax_dy_bits : nullptr;
    p.amax_x = direct ? amax_x_bits : nullptr;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(p.tiles * S));
    if (products == 3)
        hipLaunchKernelGGL(k_wgrad<3>, grid, dim3(WG_THREADS), 0, s, p);
    else
        hipLaunchKernelGGL(k_wgrad<1>, grid, dim3(WG_THREADS), 0, s, p);
    if (int rc = launch_check("k_wgrad")) return rc;
    if (direct) return 0;
    const int64_t fold_blocks = ((int64_t)n * k + 255) / 256;
    hipLaunchKernelGGL(k_wgrad_fold, dim3((unsigned)(fold_blocks < 8192 ? fold_blocks : 8192)), dim3(256), 0, s,
                       reinterpret_cast<const float*>(workspace), (int)S, (int64_t)n, (int64_t)k, amax_dy_bits, amax_x_bits, dw, ld_dw);
    return launch_check("k_wgrad_fold");
}

}  // extern "C"
