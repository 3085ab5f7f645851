// dca_embed_train.hip — weight gradient of layer 1 as the SCATTER that belongs to the embedding sum of csrc/dca_embed.hip.
//
// Reference arithmetic (utils/nnet_utils.py:53-118 calls loss.backward() on utils/pytorch_models.py:49-60): with x = onehot(s),
// fc1's weight gradient is dW = dy^T . x — a [n, K] GEMM over the batch, K = state_dim * depth, in which x has one 1 per position:
//            dW[j, pos * DEPTH + v] = sum over the rows r with s[r, pos] == v of dy[r, j],        db[j] = sum over all rows of dy[r, j].
// As a GEMM puzzle48's costs 2 * 10000 * 2401 * 5000 flops of which 48 / 49 multiply by zero; as a scatter it is state_dim adds
// per (row, column), the same count as the forward's gathers.
//
//   * a workgroup owns NT output columns (64; 32 for puzzle24, 16 for puzzle35 / 48) and one slice of S consecutive rows; the whole
//     fp32 accumulator table [K][NT] sits in LDS (puzzle48: 154 KB), zeroed at the start;
//   * the slice goes by in chunks of R rows: state bytes (16-byte pieces) and the tile's dy row segments (float4 pieces) are
//     loaded into registers one chunk ahead and parked in the small rest of the LDS between two barriers;
//   * every table address (pos * DEPTH + v, column) belongs to ONE thread: thread (pos, column group of CW columns) owns the
//     DEPTH rows of its position.  No two threads ever touch one address, no atomics: a plain LDS read - add - write per row, rows
//     in ascending order, so every element is a sequential fp32 sum whose bits a host loop reproduces;
//   * a state byte >= DEPTH selects no row: the position contributes nothing (one compare per position; the forward would
//     gather from a foreign row — here it would be a WRITE outside the position's rows, or outside the table);
//   * the table leaves transposed: lane <-> k, so a wave's stores run along K in dW[j, :] (row stride ldw) — or, when the batch
//     has more than one slice, in the slice's slab of the workspace, which k_l1_wgrad_fold then adds up in ascending slice order.
// The summation order is part of the ABI (include/dca.h): S depends on the geometry alone.
// What bounds it: the LDS instruction stream, not its latency.  Per row a wave issues four LDS instructions (state byte, dy, table
// read, table write; ~11 LDS cycles), 13 waves per CU for puzzle48.  Built, measured, removed: the table reads of four rows issued
// together with a repeated address taking the earlier row's sum (one latency per four rows instead of four) — puzzle48 1.44 -> 1.56 ms
// per 10 000 x 5000, slower on every geometry (profiles/l1_train_probe.txt has the shipped form).
#include "dca_l1.h"

namespace dca {

template <int D_, int DEPTH_, int NT_, int CW_, int R_, int S_>
struct WgradGeo {
    static constexpr int D = D_, DEPTH = DEPTH_, NT = NT_, CW = CW_, R = R_, S = S_;
    static constexpr int K = D * DEPTH;
    static constexpr int NCG = NT / CW;                          // column groups = owner threads per position
    static constexpr int OWN = D * NCG;                          // owner threads
    static constexpr int THREADS = (OWN + 63) / 64 * 64;
    static constexpr int TAB_BYTES = K * NT * 4;
    static constexpr int DY_PIECES = R * NT / 4, ST_PIECES = R * D / 16;
    static constexpr int LDS = TAB_BYTES + DY_PIECES * 16 + ST_PIECES * 16;
    static_assert(CW == 1 || CW == 4, "a thread's columns are one float or one float4");
    static_assert(NT % 4 == 0 && NT % CW == 0 && THREADS <= 1024, "tile geometry");
    static_assert((R * D) % 16 == 0 && S % R == 0, "chunks start on a 16-byte boundary of the state matrix");
    static_assert(DY_PIECES <= THREADS && ST_PIECES <= THREADS, "one piece of each kind per thread");
    static_assert(LDS <= 160 * 1024, "accumulator table does not fit LDS");
};

template <class G>
__global__ __launch_bounds__(G::THREADS) void k_l1_embed_wgrad(const uint8_t* __restrict__ nn, int64_t m, int nn_aligned,
                                                              const float* __restrict__ dy, int64_t ld_dy, int64_t n, uint32_t tiles,
                                                              float* __restrict__ w_out, int64_t ldw, int64_t w_slice_stride,
                                                              float* __restrict__ b_out /*or NULL*/, int64_t b_slice_stride) {
    constexpr int D = G::D, DEPTH = G::DEPTH, NT = G::NT, CW = G::CW, R = G::R, K = G::K, NCG = G::NCG, THREADS = G::THREADS;
    extern __shared__ __attribute__((aligned(16))) uint8_t lt[];
    float* tab = reinterpret_cast<float*>(lt);                                  // [K][NT]
    float* ldy = tab + K * NT;                                                  // [R][NT]
    uint8_t* lst = reinterpret_cast<uint8_t*>(ldy + R * NT);                    // [R][D]
    const int t = threadIdx.x;
    const uint32_t slice = blockIdx.x / tiles, tile = blockIdx.x - slice * tiles;  // neighbours share state rows and dy lines
    const int64_t n0 = (int64_t)tile * NT;
    const int64_t r_begin = (int64_t)slice * G::S, r_end = r_begin + G::S < m ? r_begin + G::S : m;
    const int64_t st_end = r_end * D;                                           // first state byte past the slice

    for (int q = t; q < K * NT / 4; q += THREADS) reinterpret_cast<float4*>(tab)[q] = make_float4(0.f, 0.f, 0.f, 0.f);

    // this thread's piece of the chunk that starts at row r0: 16 state bytes and one float4 of dy
    uint4 pre_s = make_uint4(0u, 0u, 0u, 0u);
    float4 pre_d = make_float4(0.f, 0.f, 0.f, 0.f);
    auto prefetch = [&](int64_t r0) {
        if (t < G::ST_PIECES) {
            const int64_t b = r0 * D + 16 * t;
            if (nn_aligned && b + 16 <= st_end) {
                pre_s = *reinterpret_cast<const uint4*>(nn + b);
            } else {  // the slice's last piece, or a state matrix off the 16-byte grid: byte by byte, nothing read past the slice
                pre_s = l1_load16_clipped(nn, b, st_end);
            }
        }
        if (t < G::DY_PIECES) {
            const int row = t / (NT / 4), c4 = t - row * (NT / 4);
            const int64_t r = r0 + row, col = n0 + 4 * c4;
            pre_d = (r < r_end && col < n) ? *reinterpret_cast<const float4*>(dy + r * ld_dy + col) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };

    const bool owner = t < G::OWN;
    const int pos = t / NCG, c0 = (t - pos * NCG) * CW;
    float* const trow = tab + pos * DEPTH * NT + c0;    // the DEPTH rows of this thread's position, at its columns
    float bacc[CW];
#pragma unroll
    for (int i = 0; i < CW; i++) bacc[i] = 0.f;

    typedef float accv __attribute__((ext_vector_type(CW)));  // the thread's CW columns of one table row
    // one row: v = the position's state byte, g = the row's dy at the thread's columns
    auto fetch = [&](int rr, uint32_t& v, accv& g) {
        v = lst[rr * D + pos];
        g = *reinterpret_cast<const accv*>(ldy + rr * NT + c0);
    };
    auto bias_add = [&](const accv& g) {
        if (pos == 0) {
#pragma unroll
            for (int i = 0; i < CW; i++) bacc[i] += g[i];
        }
    };
    auto apply = [&](uint32_t v, const accv& g) {
        bias_add(g);
        if (v < (uint32_t)DEPTH) *reinterpret_cast<accv*>(trow + v * NT) += g;  // (a byte >= DEPTH selects nothing)
    };

    prefetch(r_begin);
    for (int64_t r0 = r_begin; r0 < r_end; r0 += R) {
        if (t < G::ST_PIECES) reinterpret_cast<uint4*>(lst)[t] = pre_s;
        if (t < G::DY_PIECES) reinterpret_cast<float4*>(ldy)[t] = pre_d;
        __syncthreads();  // (the first one also covers the zeroed table)
        if (r0 + R < r_end) prefetch(r0 + R);
        const int nr = r_end - r0 < R ? (int)(r_end - r0) : R;
        if (owner) {
            constexpr int U = 4;  // the state bytes and dy values of U rows are read ahead of their U dependent table updates
            int rr = 0;
            for (; rr + U <= nr; rr += U) {
                uint32_t v[U];
                accv g[U];
#pragma unroll
                for (int u = 0; u < U; u++) fetch(rr + u, v[u], g[u]);
#pragma unroll
                for (int u = 0; u < U; u++) apply(v[u], g[u]);
            }
            for (; rr < nr; rr++) {
                uint32_t v;
                accv g;
                fetch(rr, v, g);
                apply(v, g);
            }
        }
        __syncthreads();  // every owner has read the chunk: it may be overwritten
    }

    // the table, transposed: lane <-> k, a wave's 64 stores are 256 contiguous bytes of one output row
    float* wo = w_out + (int64_t)slice * w_slice_stride;
    for (int q = t; q < K * (NT / 4); q += THREADS) {
        const int g = q / K, k = q - g * K;
        const float4 x = *reinterpret_cast<const float4*>(tab + k * NT + 4 * g);
        const float u[4] = {x.x, x.y, x.z, x.w};
        const int64_t col = n0 + 4 * g;
        if (col < n) {  // (n % 4 == 0: a group of four columns is inside or outside as a whole)
#pragma unroll
            for (int i = 0; i < 4; i++) wo[(col + i) * ldw + k] = u[i];
        }
    }
    if (b_out && t < NCG) {
        float* bo = b_out + (int64_t)slice * b_slice_stride;
#pragma unroll
        for (int i = 0; i < CW; i++)
            if (n0 + c0 + i < n) bo[n0 + c0 + i] = bacc[i];
    }
}

// dW[j, k] = slab 0 + slab 1 + ... in ascending slice order (fp32, from +0.0), db likewise; nslices == 0 writes zeros
__global__ __launch_bounds__(256) void k_l1_wgrad_fold(const float* __restrict__ ws_w, const float* __restrict__ ws_b, int nslices,
                                                       int64_t n, int64_t K, float* __restrict__ dW, int64_t ldw,
                                                       float* __restrict__ db /*or NULL*/) {
    const int64_t nk = n * K, total = nk + (db ? n : 0);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        float acc = 0.f;
        if (i < nk) {
            for (int s = 0; s < nslices; s++) acc += ws_w[s * nk + i];
            const int64_t j = i / K;
            dW[j * ldw + (i - j * K)] = acc;
        } else {
            for (int s = 0; s < nslices; s++) acc += ws_b[s * n + (i - nk)];
            db[i - nk] = acc;
        }
    }
}

template <class G>
int launch_wgrad(const uint8_t* nn, int64_t m, const float* dy, int64_t ld_dy, int64_t n, float* dW, int64_t ldw, float* db,
                 void* workspace, hipStream_t s) {
    auto kern = k_l1_embed_wgrad<G>;
    static std::atomic<uint64_t> attr_devs{0};
    if (int rc = dynamic_lds_once(attr_devs, {reinterpret_cast<const void*>(kern)}, G::LDS)) return rc;
    const int64_t tiles = (n + G::NT - 1) / G::NT, nslices = (m + G::S - 1) / G::S, K = G::K;
    if (tiles * nslices > 0x7fffffffll) {
        set_error("dca_l1_embed_wgrad: %lld column tiles x %lld row slices exceed the grid", (long long)tiles, (long long)nslices);
        return DCA_E_BADARG;
    }
    const int aligned = (reinterpret_cast<uintptr_t>(nn) & 15) == 0;
    const int64_t fold_blocks = (n * K + n + 255) / 256;
    const unsigned fold_grid = (unsigned)(fold_blocks < 8192 ? fold_blocks : 8192);
    if (nslices <= 1) {
        if (nslices == 0) {
            hipLaunchKernelGGL(k_l1_wgrad_fold, dim3(fold_grid), dim3(256), 0, s, nullptr, nullptr, 0, n, K, dW, ldw, db);
            return launch_check("k_l1_wgrad_fold");
        }
        hipLaunchKernelGGL(kern, dim3((unsigned)tiles), dim3(G::THREADS), G::LDS, s, nn, m, aligned, dy, ld_dy, n, (uint32_t)tiles, dW,
                           ldw, (int64_t)0, db, (int64_t)0);
        return launch_check("k_l1_embed_wgrad");
    }
    float* ws_w = reinterpret_cast<float*>(workspace);
    float* ws_b = ws_w + nslices * n * K;
    hipLaunchKernelGGL(kern, dim3((unsigned)(tiles * nslices)), dim3(G::THREADS), G::LDS, s, nn, m, aligned, dy, ld_dy, n,
                       (uint32_t)tiles, ws_w, K, n * K, ws_b, n);
    if (int rc = launch_check("k_l1_embed_wgrad")) return rc;
    hipLaunchKernelGGL(k_l1_wgrad_fold, dim3(fold_grid), dim3(256), 0, s, ws_w, ws_b, (int)nslices, n, K, dW, ldw, db);
    return launch_check("k_l1_wgrad_fold");
}

// the tile of each geometry: column tile NT, columns per owner thread CW, rows per chunk R, rows per slice S
template <int D, int DEPTH> struct WgTile : L1NotBuilt {};
template <int D, int DEPTH, int NT, int CW, int R, int S>
struct WgTileOf { static constexpr bool built = true; using G = WgradGeo<D, DEPTH, NT, CW, R, S>; };
//                                                       D  DEPTH NT CW  R    S
template <> struct WgTile<54, 6> : WgTileOf<54, 6, 64, 4, 32, 1024> {};    // cube3
template <> struct WgTile<9, 9> : WgTileOf<9, 9, 64, 1, 32, 1024> {};      // puzzle8
template <> struct WgTile<16, 16> : WgTileOf<16, 16, 64, 1, 32, 1024> {};  // puzzle15
template <> struct WgTile<25, 25> : WgTileOf<25, 25, 32, 1, 64, 2048> {};  // puzzle24
template <> struct WgTile<36, 36> : WgTileOf<36, 36, 16, 1, 64, 2048> {};  // puzzle35
template <> struct WgTile<49, 49> : WgTileOf<49, 49, 16, 1, 64, 2048> {};  // puzzle48
template <> struct WgTile<49, 6> : WgTileOf<49, 6, 64, 4, 32, 1024> {};    // lightsout7

static int64_t wgrad_slice_rows(int state_dim, int depth) {
    return l1_dispatch<WgTile>(state_dim, depth, (int64_t)-1, [](auto g) { return (int64_t)WgTile<g.D, g.DEPTH>::G::S; });
}

}  // namespace dca

using namespace dca;

extern "C" {

int64_t dca_l1_embed_wgrad_slice_rows(int state_dim, int depth) {
    const int64_t S = wgrad_slice_rows(state_dim, depth);
    if (S < 0) {
        set_error("dca_l1_embed_wgrad: geometry (%d, %d) not instantiated", state_dim, depth);
        return DCA_E_BADARG;
    }
    return S;
}

int64_t dca_l1_embed_wgrad_workspace_bytes(int64_t m, int state_dim, int depth, int64_t n) {
    const int64_t S = wgrad_slice_rows(state_dim, depth);
    if (S < 0 || m < 0 || n < 0) {
        set_error("dca_l1_embed_wgrad_workspace_bytes: bad argument (m %lld, geometry (%d, %d), n %lld)", (long long)m, state_dim, depth,
                  (long long)n);
        return DCA_E_BADARG;
    }
    const int64_t nslices = (m + S - 1) / S;
    return nslices <= 1 ? 0 : nslices * (n * state_dim * depth + n) * 4;
}

int dca_l1_embed_wgrad(const uint8_t* nnet_in, int64_t m, int state_dim, int depth, const float* dy, int64_t ld_dy, int64_t n, float* dW,
                       int64_t ldw, float* db, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!l1_built<WgTile>(state_dim, depth)) {
        set_error("dca_l1_embed_wgrad: geometry (%d, %d) not instantiated", state_dim, depth);
        return DCA_E_BADARG;
    }
    DCA_ARG(m >= 0 && n >= 0 && n % 4 == 0);
    DCA_ARG(nnet_in && dy && dW);
    DCA_ARG((reinterpret_cast<uintptr_t>(dy) & 15) == 0 && ld_dy % 4 == 0);
    DCA_ARG(ld_dy >= n && ldw >= (int64_t)state_dim * depth);
    const int64_t need = dca_l1_embed_wgrad_workspace_bytes(m, state_dim, depth, n);
    if (need > 0 && (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 3))) {
        set_error("dca_l1_embed_wgrad: workspace of %lld bytes at %p, %lld needed (4-byte aligned)", (long long)workspace_bytes, workspace,
                  (long long)need);
        return DCA_E_BADARG;
    }
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    return l1_dispatch<WgTile>(state_dim, depth, DCA_E_BADARG, [&](auto g) {
        return launch_wgrad<typename WgTile<g.D, g.DEPTH>::G>(nnet_in, m, dy, ld_dy, n, dW, ldw, db, workspace, s);
    });
}

}  // extern "C"
