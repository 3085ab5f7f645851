// What do gfx950's float64 instructions cost?  The fp64 heuristic mode (csrc/dca_gemm64.hip) is built on v_mfma_f64_16x16x4_f64;
// its rate is in no guide (the spec sheet's 78.6 TF for FP64 matrix implies 64 cycles per instruction at ~2.4 GHz, a derived
// figure).  This probe measures, from registers only:
//   * the MFMA's issue interval (8 and 16 independent accumulators — dca_gemm64 keeps 16 per wave) and its dependent latency (one
//     accumulator chain), in shader cycles (s_memtime) for one wave alone, and the chip-wide TFLOP/s with 1, 2 and 4 waves per SIMD;
//   * the same for v_fma_f64 on the vector ALU (8 independent chains per lane / one chain).
// Build: hipcc --offload-arch=gfx950 -O3 tools/fp64_rate_probe.hip -o tools/bin/fp64_rate_probe
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
typedef double f64x4 __attribute__((ext_vector_type(4)));

#define CHECK(x)                                                                     \
    do {                                                                             \
        hipError_t e_ = (x);                                                         \
        if (e_ != hipSuccess) {                                                      \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                  \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)

template <int NACC>  // NACC independent accumulators; NACC = 1 is a dependent chain
__global__ __launch_bounds__(256) void k_mfma64(const double* __restrict__ in, double* __restrict__ out, long long* __restrict__ cyc,
                                                int iters) {
    const int t = threadIdx.x + blockIdx.x * blockDim.x;
    const double a = in[t & 1023], b = in[(t + 7) & 1023];
    f64x4 acc[NACC];
#pragma unroll
    for (int j = 0; j < NACC; j++) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};
    const long long t0 = clock64();
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int j = 0; j < NACC; j++) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[j], 0, 0, 0);
    }
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < NACC; j++) s += acc[j][0] + acc[j][1] + acc[j][2] + acc[j][3];
    const long long t1 = clock64();
    out[t] = s;
    if ((threadIdx.x & 63) == 0) cyc[t >> 6] = t1 - t0;
}

template <int NCH>  // NCH independent FMA chains per lane; NCH = 1 is a dependent chain
__global__ __launch_bounds__(256) void k_fma64(const double* __restrict__ in, double* __restrict__ out, long long* __restrict__ cyc,
                                               int iters) {
    const int t = threadIdx.x + blockIdx.x * blockDim.x;
    const double a = in[t & 1023], b = in[(t + 7) & 1023];
    double acc[NCH];
#pragma unroll
    for (int j = 0; j < NCH; j++) acc[j] = in[(t + j) & 1023];
    const long long t0 = clock64();
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int j = 0; j < NCH; j++) acc[j] = fma(acc[j], a, b);
    }
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < NCH; j++) s += acc[j];
    const long long t1 = clock64();
    out[t] = s;
    if ((threadIdx.x & 63) == 0) cyc[t >> 6] = t1 - t0;
}

template <typename K>
static void run(const char* name, K kern, int n_acc, double flop_per_instr, int iters, int blocks, int threads, const double* din,
                double* dout, long long* dcyc) {
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), 0, 0, din, dout, dcyc, iters);  // warm-up
    CHECK(hipDeviceSynchronize());
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    CHECK(hipEventRecord(e0));
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), 0, 0, din, dout, dcyc, iters);
    CHECK(hipEventRecord(e1));
    CHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    const int waves = blocks * threads / 64;
    long long* h = (long long*)malloc(sizeof(long long) * waves);
    CHECK(hipMemcpy(h, dcyc, sizeof(long long) * waves, hipMemcpyDeviceToHost));
    double cmean = 0.0;
    for (int i = 0; i < waves; i++) cmean += (double)h[i];
    cmean /= waves;
    free(h);
    const double instr = (double)iters * n_acc;
    printf("%-44s waves %6d  cycles/instr per wave %7.2f  wall %8.3f ms  %8.2f TFLOP/s\n", name, waves, cmean / instr, ms,
           flop_per_instr * instr * waves / (ms * 1e-3) / 1e12);
}

int main(int argc, char** argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 20000;
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    printf("%s, %d CUs, iters %d\n", prop.gcnArchName, cus, iters);
    double h[1024];
    for (int i = 0; i < 1024; i++) h[i] = 1.0 + 1e-3 * (double)((i * 7919) % 1000);  // finite, non-trivial operands
    double *din, *dout;
    long long* dcyc;
    const int max_threads = cus * 4 * 4 * 64;
    CHECK(hipMalloc(&din, sizeof(h)));
    CHECK(hipMalloc(&dout, sizeof(double) * max_threads));
    CHECK(hipMalloc(&dcyc, sizeof(long long) * (max_threads / 64)));
    CHECK(hipMemcpy(din, h, sizeof(h), hipMemcpyHostToDevice));
    const double mf = 16.0 * 16 * 4 * 2, vf = 64.0 * 2;
    // one wave alone: issue interval (8 independent accumulators) and dependent latency (1)
    run("mfma_f64_16x16x4 1 wave, 8 indep", k_mfma64<8>, 8, mf, iters, 1, 64, din, dout, dcyc);
    run("mfma_f64_16x16x4 1 wave, 16 indep", k_mfma64<16>, 16, mf, iters / 2, 1, 64, din, dout, dcyc);
    run("mfma_f64_16x16x4 1 wave, dependent", k_mfma64<1>, 1, mf, iters, 1, 64, din, dout, dcyc);
    run("v_fma_f64 1 wave, 8 indep chains", k_fma64<8>, 8, vf, iters, 1, 64, din, dout, dcyc);
    run("v_fma_f64 1 wave, dependent", k_fma64<1>, 1, vf, iters, 1, 64, din, dout, dcyc);
    // every CU: blocks of 4 waves (one per SIMD), 1 / 2 / 4 blocks per CU
    for (int w = 1; w <= 4; w *= 2) {
        char nm[96];
        snprintf(nm, sizeof nm, "mfma_f64_16x16x4 chip, %d wave/SIMD, 8 indep", w);
        run(nm, k_mfma64<8>, 8, mf, iters, cus * w, 256, din, dout, dcyc);
        snprintf(nm, sizeof nm, "mfma_f64_16x16x4 chip, %d wave/SIMD, 16 indep", w);
        run(nm, k_mfma64<16>, 16, mf, iters / 2, cus * w, 256, din, dout, dcyc);
        snprintf(nm, sizeof nm, "v_fma_f64 chip, %d wave/SIMD, 8 indep", w);
        run(nm, k_fma64<8>, 8, vf, iters, cus * w, 256, din, dout, dcyc);
    }
    CHECK(hipFree(din));
    CHECK(hipFree(dout));
    CHECK(hipFree(dcyc));
    return 0;
}
