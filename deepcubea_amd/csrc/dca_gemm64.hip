// dca_gemm64.hip — the float64 heuristic mode (`--nnet_dtype fp64`): the cost-to-go network evaluated in float64 from its fp32
// weights (BatchNorm folded in float64), rounded once to fp32 by the output layer (dca_head_gemv, DCA_DT_F64 rows).
//
//   * dca_gemm64: every dense layer after the first, out = relu?(a . w^T + bias (+ skip)), on v_mfma_f64_16x16x4_f64.
//     Workgroup = 4 waves, output tile 128 rows x 128 units, K-tiles of 16 staged in LDS (double buffered: the next tile's global
//     loads are in flight while the current one is multiplied, one barrier per K-tile); each wave owns 64 x 64 = 4 x 4 fragments,
//     i.e. per k-step of 4: 4 A and 4 B fragment reads (ds_read_b64) feed 16 MFMAs.  No split-K: every output element is summed
//     over K in ascending order, 4 products per instruction, by the one lane that owns it — a row's value has the same bits
//     in any batch, at any position, under any padding.
//     Lane maps (cdna_hip_programming, "Fragment layout"): A and B as in the f32 16x16x4 form — lane l holds A[row l & 15][k l >> 4]
//     and B[k l >> 4][col l & 15], one double each — but C/D is NOT the f32 map: register i of lane l is
//     row (l >> 4) + 4 * i, col l & 15 (the f32 row formula runs clean and puts 3 of 4 results in the wrong row).
//     LDS images are k-major ([k][row]) so a fragment read is 16 consecutive doubles per k; rows are padded by 4 doubles.
//   * dca_l1_embed64: layer 1 as an embedding sum in float64 (a one-hot row has one 1 per position):
//     out[r, j] = relu?(bias[j] + sum_pos w_t[pos * depth + s[r, pos]][j]), bias first, positions ascending.  One generic kernel for
//     every geometry: a workgroup keeps NT columns of the transposed table in LDS (the widest NT of 64 / 32 / 16 / 8 that fits),
//     stages blocks of state rows into LDS and sums with NT lanes per state, two states per lane.
#include "dca_dense.h"

namespace dca {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int G64_BM = 128, G64_BN = 128, G64_BK = 16, G64_PAD = 4, G64_THREADS = 256;
constexpr int G64_LDA = G64_BM + G64_PAD, G64_LDW = G64_BN + G64_PAD;  // LDS row strides (doubles) of the k-major images

__global__ __launch_bounds__(G64_THREADS, 2) void k_gemm64(const double* __restrict__ a, int64_t m, int k, int64_t lda,
                                                           const double* __restrict__ w, int n, int64_t ldw,
                                                           const double* __restrict__ bias, const double* skip, int relu,
                                                           double* out, int64_t ldo) {
    __shared__ __attribute__((aligned(16))) double la[2][G64_BK][G64_LDA];
    __shared__ __attribute__((aligned(16))) double lw[2][G64_BK][G64_LDW];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    // one-dimensional grid, column tiles fastest: the workgroups of a row block run side by side and share its A rows in L2
    const int ntn = (n + G64_BN - 1) / G64_BN;
    const int64_t m0 = (int64_t)(blockIdx.x / ntn) * G64_BM;
    const int n0 = (int)(blockIdx.x % ntn) * G64_BN;
    // global -> register staging: thread t loads pairs (k 2 * (t & 7), +1) of rows (t >> 3) + 32 * i, i < 4, of both operands;
    // rows past m / n and k past k load zeros (a zero product adds +0: the sums of real elements are unchanged)
    const int kc = 2 * (t & 7), r0 = t >> 3;
    double2 ra[4], rw[4];
    auto load = [&](int kt) {
        const int kk = kt * G64_BK + kc;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int64_t ar = m0 + r0 + 32 * i;
            const int wr = n0 + r0 + 32 * i;
            ra[i] = (ar < m && kk < k) ? *reinterpret_cast<const double2*>(a + ar * lda + kk) : make_double2(0.0, 0.0);
            rw[i] = (wr < n && kk < k) ? *reinterpret_cast<const double2*>(w + (int64_t)wr * ldw + kk) : make_double2(0.0, 0.0);
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            la[buf][kc][r0 + 32 * i] = ra[i].x;
            la[buf][kc + 1][r0 + 32 * i] = ra[i].y;
            lw[buf][kc][r0 + 32 * i] = rw[i].x;
            lw[buf][kc + 1][r0 + 32 * i] = rw[i].y;
        }
    };
    f64x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int nkt = (k + G64_BK - 1) / G64_BK;
    load(0);
    store(0);
    __syncthreads();
    const int fr = lane & 15, fk = lane >> 4;
    for (int kt = 0; kt < nkt; kt++) {
        const int buf = kt & 1;
        if (kt + 1 < nkt) load(kt + 1);
#pragma unroll
        for (int ks = 0; ks < G64_BK / 4; ks++) {
            double fa[4], fb[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                fa[i] = la[buf][4 * ks + fk][wm * 64 + 16 * i + fr];
                fb[i] = lw[buf][4 * ks + fk][wn * 64 + 16 * i + fr];
            }
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        if (kt + 1 < nkt) store(buf ^ 1);
        __syncthreads();
    }
    // epilogue: (acc + bias) (+ skip), ReLU.  skip may be `out` itself: each element is read, then written, by the same lane
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int col = n0 + wn * 64 + 16 * j + fr;
        if (col >= n) continue;
        const double b = bias ? bias[col] : 0.0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int64_t row = m0 + wm * 64 + 16 * i + fk + 4 * e;
                if (row < m) {
                    double v = acc[i][j][e] + b;
                    if (skip) v += skip[row * ldo + col];
                    if (relu) v = v > 0.0 ? v : 0.0;
                    out[row * ldo + col] = v;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// layer 1: workgroup = 16 waves owning NT columns (their table slice stays in LDS for the workgroup's life); per step it stages
// `rows` state rows into LDS at a stride padded to 8 bytes, then every lane sums its column for two states at a time (two
// independent chains), reading 8 state bytes per LDS access and gathering 8 table entries before the 8 ordered adds
constexpr int E64_THREADS = 1024;
constexpr int E64_LDS_MAX = 160 * 1024;

template <int NT>
__global__ __launch_bounds__(E64_THREADS) void k_l1_embed64(const uint8_t* __restrict__ nn, int64_t m, int d, int depth,
                                                            const double* __restrict__ wt /*[d * depth][n_pad]*/, int64_t n_pad,
                                                            const double* __restrict__ bias, int relu, double* __restrict__ out,
                                                            int rows) {
    extern __shared__ __attribute__((aligned(16))) uint8_t le64[];
    const int kdim = d * depth, dp = (d + 7) & ~7;
    double* lw = reinterpret_cast<double*>(le64);
    double* lb = lw + (int64_t)kdim * NT;
    uint8_t* ls = reinterpret_cast<uint8_t*>(lb + NT);  // [rows][dp] (16-byte aligned: the table and bias are whole 64-byte rows)
    const int t = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * NT;
    for (int q = t; q < kdim * NT; q += E64_THREADS) {
        const int kr = q / NT, c = q - kr * NT;
        lw[q] = wt[(int64_t)kr * n_pad + c0 + c];
    }
    if (t < NT) lb[t] = bias[c0 + t];
    const int c = t % NT, sub = t / NT;  // this lane's column; its state slot within a pass of E64_THREADS / NT states
    constexpr int SPP = E64_THREADS / NT;
    for (int64_t r0 = (int64_t)blockIdx.y * rows; r0 < m; r0 += (int64_t)gridDim.y * rows) {
        const int nr = (int)((m - r0 < rows) ? (m - r0) : rows);
        __syncthreads();  // (the previous block's bytes are consumed; the table is staged before the first pass)
        const uint8_t* src = nn + r0 * d;
        for (int q = t; q < nr * d; q += E64_THREADS) {
            const int sr = q / d;
            ls[sr * dp + (q - sr * d)] = src[q];
        }
        __syncthreads();
        const int half = (nr + 1) / 2;  // lane states s and s + half
        for (int s = sub; s < half; s += SPP) {
            const bool two = s + half < nr;
            const uint8_t* ra = ls + s * dp;
            const uint8_t* rb = ls + (two ? s + half : s) * dp;  // (an odd block's last state is summed twice, stored once)
            double acc0 = lb[c], acc1 = acc0;
            for (int p = 0; p < d; p += 8) {
                const uint2 va = *reinterpret_cast<const uint2*>(ra + p), vb = *reinterpret_cast<const uint2*>(rb + p);
                double ga[8], gb[8];
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const uint32_t ba = ((u < 4 ? va.x : va.y) >> (8 * (u & 3))) & 0xFFu;
                    const uint32_t bb = ((u < 4 ? vb.x : vb.y) >> (8 * (u & 3))) & 0xFFu;
                    const int row0 = (p + u) * depth;
                    ga[u] = p + u < d ? lw[(row0 + (int)ba) * NT + c] : 0.0;
                    gb[u] = p + u < d ? lw[(row0 + (int)bb) * NT + c] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 8; u++) {  // positions in ascending order (a past-the-end position adds nothing)
                    if (p + u < d) {
                        acc0 += ga[u];
                        acc1 += gb[u];
                    }
                }
            }
            if (relu) {
                acc0 = acc0 > 0.0 ? acc0 : 0.0;
                acc1 = acc1 > 0.0 ? acc1 : 0.0;
            }
            out[(r0 + s) * n_pad + c0 + c] = acc0;
            if (two) out[(r0 + s + half) * n_pad + c0 + c] = acc1;
        }
    }
}

// LDS of one workgroup: the table slice, the bias slice and `rows` padded state rows
template <int NT>
size_t embed64_lds(int kdim, int d, int rows) { return (size_t)kdim * NT * 8 + NT * 8 + (size_t)rows * ((d + 7) & ~7); }

// the most state rows per step (at most 1024) that fit next to the table; 0 if fewer than min_rows
template <int NT>
int embed64_rows(int kdim, int d, int min_rows) {
    const int64_t avail = (int64_t)E64_LDS_MAX - (int64_t)embed64_lds<NT>(kdim, d, 0);
    const int64_t r = avail > 0 ? avail / ((d + 7) & ~7) : 0;
    return r >= min_rows ? (int)(r < 1024 ? r : 1024) : 0;
}

template <int NT>
int launch_embed64(const uint8_t* nn, int64_t m, int d, int depth, const double* wt, int64_t n_pad, const double* bias, int relu,
                   double* out, hipStream_t s) {
    const int rows = embed64_rows<NT>(d * depth, d, 1);
    const size_t lds = embed64_lds<NT>(d * depth, d, rows);
    const int64_t tiles = n_pad / NT, steps = (m + rows - 1) / rows;
    // one workgroup fits a CU: >= 2048 workgroups (>= 8 rounds over 256 CUs) keep the last round's idle share small; the table
    // slice is staged once per workgroup
    int64_t gy = (2048 + tiles - 1) / tiles;
    if (gy > steps) gy = steps;
    if (gy < 1) gy = 1;
    static std::atomic<uint64_t> attr_devs{0};  // (lds follows the geometry at run time: raised once to the ceiling embed64_rows() fills up to)
    if (int rc = dynamic_lds_once(attr_devs, {reinterpret_cast<const void*>(k_l1_embed64<NT>)}, E64_LDS_MAX)) return rc;
    hipLaunchKernelGGL(k_l1_embed64<NT>, dim3((unsigned)tiles, (unsigned)gy), dim3(E64_THREADS), lds, s, nn, m, d, depth, wt, n_pad,
                       bias, relu, out, rows);
    return launch_check("k_l1_embed64");
}

}  // namespace dca

using namespace dca;

extern "C" {

int dca_gemm64(const double* a, int64_t m, int k, int64_t lda, const double* w, int n, int64_t ldw, const double* bias,
               const double* skip, int relu, double* out, int64_t ldo, void* stream) {
    DCA_ARG(a && w && out && m >= 0 && k >= 2 && k % 2 == 0 && n >= 1 && lda >= k && ldw >= k && ldo >= n);
    DCA_ARG(lda % 2 == 0 && ldw % 2 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(w)) & 15) == 0);
    DCA_ARG(out != a && (skip == nullptr || skip == out || skip != a));
    if (m == 0) return 0;
    const int64_t blocks = (m + G64_BM - 1) / G64_BM * ((n + G64_BN - 1) / G64_BN);
    DCA_ARG(blocks < (1ll << 31));
    hipLaunchKernelGGL(k_gemm64, dim3((unsigned)blocks), dim3(G64_THREADS), 0, (hipStream_t)stream, a, m, k, lda, w, n, ldw, bias, skip, relu, out, ldo);
    return launch_check("k_gemm64");
}

int dca_l1_embed64(const uint8_t* nnet_in, int64_t m, int state_dim, int depth, const double* w_t, int64_t n_pad, const double* bias,
                   int relu, double* out, void* stream) {
    DCA_ARG(nnet_in && w_t && bias && out && m >= 0 && state_dim >= 1 && depth >= 1 && depth <= 256 && n_pad >= 8 && n_pad % 8 == 0);
    const int kdim = state_dim * depth;
    hipStream_t s = (hipStream_t)stream;
    if (m == 0) return 0;
    // the widest column tile that leaves room for >= 256 staged states (narrower tiles stage the table more often), else 8 columns
    if (n_pad % 64 == 0 && embed64_rows<64>(kdim, state_dim, 256) > 0)
        return launch_embed64<64>(nnet_in, m, state_dim, depth, w_t, n_pad, bias, relu, out, s);
    if (n_pad % 32 == 0 && embed64_rows<32>(kdim, state_dim, 256) > 0)
        return launch_embed64<32>(nnet_in, m, state_dim, depth, w_t, n_pad, bias, relu, out, s);
    if (n_pad % 16 == 0 && embed64_rows<16>(kdim, state_dim, 256) > 0)
        return launch_embed64<16>(nnet_in, m, state_dim, depth, w_t, n_pad, bias, relu, out, s);
    if (embed64_rows<8>(kdim, state_dim, 1) > 0) return launch_embed64<8>(nnet_in, m, state_dim, depth, w_t, n_pad, bias, relu, out, s);
    set_error("dca_l1_embed64: the weight table of geometry (%d, %d) does not fit LDS in 8 columns", state_dim, depth);
    return DCA_E_BADARG;
}

}  // extern "C"
