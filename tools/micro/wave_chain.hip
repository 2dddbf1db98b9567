// micro-benchmark of the building blocks of the wave-owned policy forward (csrc/cm_policy_w_dev.h), ONE wave per SIMD:
// cycles (s_memtime) of  (a) back-to-back v_mfma_f32_16x16x32_f16,  (b) the stage-wise epilogue (join, tanh, split) of 8 values,
// (c) whole layers 128 -> 64 and 64 -> 128 as the kernel runs them (fragments from LDS, one layer ahead), chained.
// (b) and (c) once per form of the split's residual (SPLIT_SUB / SPLIT_MIX / SPLIT_MIXLO, cm_policy_w_dev.h), after (d): every form's
// (hi, lo) bit patterns on random and edge inputs against split_u on the host - a form that differs anywhere fails the run.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -mllvm -amdgpu-mfma-vgpr-form -fno-slp-vectorize -I../../com-marl_amd/csrc wave_chain.hip -o wave_chain
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <vector>
#include <string.h>
#include <algorithm>
#include "cm_policy_w_dev.h"
using namespace cm;
using namespace cm::mw;

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_mfma(unsigned long long *clk, float *sink, int iters) {
    const int lane = threadIdx.x & 63;
    v8h a, b;
    for (int e = 0; e < 8; ++e) { a[e] = (h16)(0.01f * (lane + e)); b[e] = (h16)(0.02f * (lane - e)); }
    v4f acc[8];
    for (int i = 0; i < 8; ++i) acc[i] = (v4f){ 0.f, 0.f, 0.f, 0.f };
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; ++it)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc[i], 0, 0, 0);
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    float s = 0; for (int i = 0; i < 8; ++i) s += acc[i][0] + acc[i][3];
    sink[blockIdx.x * 256 + threadIdx.x] = s;
    if (blockIdx.x == 0 && threadIdx.x == 0) clk[0] = t1 - t0;
}

template <int SPLIT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_epi(unsigned long long *clk, float *sink, int iters, int mode) {
    const int lane = threadIdx.x & 63;
    float v[8];
    for (int e = 0; e < 8; ++e) v[e] = 0.01f * (lane + e);
    float accum = 0.0f;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; ++it) {
        float w[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) w[e] = fmaf(v[e], 0.000244140625f, accum);
        if (mode & 1) tanh_stage<8>(w);
        h16 h[8], l[8];
        if (mode & 2) {
            split_stage<8, SPLIT>(w, h, l);
#pragma unroll
            for (int e = 0; e < 8; ++e) accum += (float)h[e] + (float)l[e];          // dependency to the next iteration
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) accum += w[e];
        }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    sink[blockIdx.x * 256 + threadIdx.x] = accum;
    if (blockIdx.x == 0 && threadIdx.x == 0) clk[0] = t1 - t0;
}

// two chained layers 128 -> 64 -> 128 (tanh), fragments from LDS (random f16), repeated
template <int SPLIT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_layers(unsigned long long *clk, float *sink, int iters) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    uint4 *WL = reinterpret_cast<uint4 *>(lds);
    const int tid = threadIdx.x, lane = tid & 63;
    constexpr int NA = frag_u4(128, 64), NB = frag_u4(64, 128);
    for (int i = tid; i < NA + NB; i += 256) { const unsigned x = 0x1c001c00u + (i * 2654435761u & 0x03ff03ffu); WL[i] = make_uint4(x, x ^ 0x80000000u, x + 7u, x ^ 0x00008000u); }
    float *BL = reinterpret_cast<float *>(WL + NA + NB);
    for (int i = tid; i < 256; i += 256) BL[i] = 0.01f * i;
    __syncthreads();
    Act<4> x;
    for (int q = 0; q < 4; ++q) for (int e = 0; e < 8; ++e) { x.hi[q][e] = (h16)(0.01f * (lane % 7 + e)); x.lo[q][e] = (h16)0.5f; }
    Frags<4, 4> fa; Frags<2, 8> fb;
    fa.fetch(WL, lane);
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; ++it) {
        fb.fetch(WL + NA, lane);
        Act<2> y;
        dense_act<4, 4, true, true, SPLIT>(fa, BL, x, y, nullptr, lane);
        fa.fetch(WL, lane);
        dense_act<2, 8, true, true, SPLIT>(fb, BL + 64, y, x, nullptr, lane);
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    float s = 0; for (int q = 0; q < 4; ++q) s += (float)x.hi[q][0] + (float)x.lo[q][3];
    sink[blockIdx.x * 256 + threadIdx.x] = s;
    if (blockIdx.x == 0 && threadIdx.x == 0) clk[0] = t1 - t0;
}

// (d) the split of n values (n a multiple of 8 x 256): bit patterns of hi and lo, one thread per 8 values as the epilogue has them
template <int SPLIT>
__global__ __launch_bounds__(256) void k_split(const float *in, unsigned short *hi, unsigned short *lo, int n) {
    const int i0 = (blockIdx.x * 256 + threadIdx.x) * 8;
    if (i0 + 8 > n) return;
    float y[8];
    h16 h[8], l[8];
    for (int e = 0; e < 8; ++e) y[e] = in[i0 + e];
    split_stage<8, SPLIT>(y, h, l);
    for (int e = 0; e < 8; ++e) { hi[i0 + e] = __builtin_bit_cast(unsigned short, h[e]); lo[i0 + e] = __builtin_bit_cast(unsigned short, l[e]); }
}

static float from_bits(unsigned u) { float f; memcpy(&f, &u, 4); return f; }

// inputs of the split check: the edges first, then seeded random values over the magnitudes the network sees and beyond
static std::vector<float> split_inputs(int n) {
    std::vector<float> v;
    const float edge[] = { 0.0f, 1.0f, 0.5f, 65504.0f, 65519.0f, 65520.0f, 1.0e6f, 3.0e38f,   // largest f16, the last value below / first at the overflow to inf
                           5.9604645e-8f, 2.9802322e-8f, 8.9406967e-8f, 6.0975552e-5f, 6.1035156e-5f,   // 2^-24, 2^-25 (tie to zero), 1.5 x 2^-24, largest subnormal, smallest normal
                           1.0e-8f, 1.0e-40f, 1.17549435e-38f,                                 // below half the smallest subnormal, f32 subnormal, smallest f32 normal
                           0.125f + 9.5367432e-7f, 1.0f + 6.1035156e-5f, 0.25f + 5.9604645e-8f, 2.0f + 0.00048828125f,   // residuals that are f16 subnormals / the smallest normal / a tie
                           1.0009765625f, 1.00048828125f, 1.000732421875f, 0.333333343f, 3.14159274f, 2047.5f, 2048.5f };
    for (float e : edge) { v.push_back(e); v.push_back(-e); }
    unsigned long long st = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (unsigned)(st >> 16); };
    while ((int)v.size() < n) {
        const unsigned r = next();
        const unsigned mant = r & 0x007fffffu, sign = (r >> 23 & 1u) << 31;
        // exponents 2^-30 .. 2^17 (f16 subnormal range, the whole normal range, past the overflow), every mantissa
        const unsigned ex = 127u - 30u + (next() % 48u);
        v.push_back(from_bits(sign | ex << 23 | mant));
    }
    return v;
}

template <int SPLIT>
static int check_split(const char *name, const std::vector<float> &in, float *d_in, unsigned short *d_hi, unsigned short *d_lo) {
    const int n = (int)in.size();
    hipMemset(d_hi, 0xff, n * 2); hipMemset(d_lo, 0xff, n * 2);
    hipLaunchKernelGGL(k_split<SPLIT>, dim3(n / (8 * 256)), dim3(256), 0, 0, d_in, d_hi, d_lo, n);
    std::vector<unsigned short> hi(n), lo(n);
    hipMemcpy(hi.data(), d_hi, n * 2, hipMemcpyDeviceToHost); hipMemcpy(lo.data(), d_lo, n * 2, hipMemcpyDeviceToHost);
    int bad = 0;
    for (int i = 0; i < n; ++i) {
        h16 h, l;
        split_u(in[i], h, l);
        const unsigned short eh = __builtin_bit_cast(unsigned short, h), el = __builtin_bit_cast(unsigned short, l);
        if (eh != hi[i] || el != lo[i]) {
            if (bad < 8) printf("  %s: y = %.9g  hi %04x lo %04x, split_u gives hi %04x lo %04x\n", name, in[i], hi[i], lo[i], eh, el);
            ++bad;
        }
    }
    printf("split check %-11s: %d values, %d differ from split_u\n", name, n, bad);
    return bad;
}

template <int SPLIT>
static void time_split(const char *name, int blocks, unsigned long long *d, float *sink, int iters) {
    unsigned long long h;
    for (int mode = 2; mode < 4; ++mode) {
        for (int rep = 0; rep < 2; ++rep) hipLaunchKernelGGL(k_epi<SPLIT>, dim3(blocks), dim3(256), 0, 0, d, sink, iters, mode);
        hipMemcpy(&h, d, 8, hipMemcpyDeviceToHost);
        printf("blocks %3d  %-11s epilogue of 8 values (join%s + split)     : %.1f clk per value\n", blocks, name, (mode & 1) ? " + tanh" : "", (double)h / (iters * 8));
    }
    // the layer pair, REPS launches after a warm-up one: the spread of the repeats is the yardstick between the forms
    constexpr int REPS = 9;
    double c[REPS];
    for (int rep = -1; rep < REPS; ++rep) {
        hipLaunchKernelGGL(k_layers<SPLIT>, dim3(blocks), dim3(256), (frag_u4(128, 64) + frag_u4(64, 128)) * 16 + 1024, 0, d, sink, iters);
        hipMemcpy(&h, d, 8, hipMemcpyDeviceToHost);
        if (rep >= 0) c[rep] = (double)h / iters;
    }
    std::sort(c, c + REPS);
    printf("blocks %3d  %-11s layers 128->64 + 64->128 (96 MFMA, 48 values/lane)  : %.0f clk per pair, %.0f .. %.0f over %d launches  (MFMA floor %d)\n",
           blocks, name, c[REPS / 2], c[0], c[REPS - 1], REPS, 96 * 16);
}

int main() {
    unsigned long long *d; float *sink;
    hipMalloc(&d, 8); hipMalloc(&sink, 256 * 256 * 4);
    unsigned long long h;
    const int iters = 200;
    int bad = 0;
    {
        const int n = 64 * 8 * 256;
        const std::vector<float> in = split_inputs(n);
        float *d_in; unsigned short *d_hi, *d_lo;
        hipMalloc(&d_in, n * 4); hipMalloc(&d_hi, n * 2); hipMalloc(&d_lo, n * 2);
        hipMemcpy(d_in, in.data(), n * 4, hipMemcpyHostToDevice);
        bad += check_split<SPLIT_SUB>("SPLIT_SUB", in, d_in, d_hi, d_lo);
        bad += check_split<SPLIT_MIX>("SPLIT_MIX", in, d_in, d_hi, d_lo);
        bad += check_split<SPLIT_MIXLO>("SPLIT_MIXLO", in, d_in, d_hi, d_lo);
        hipFree(d_in); hipFree(d_hi); hipFree(d_lo);
    }
    hipFuncSetAttribute((const void *)k_layers<SPLIT_SUB>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipFuncSetAttribute((const void *)k_layers<SPLIT_MIX>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipFuncSetAttribute((const void *)k_layers<SPLIT_MIXLO>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    for (int blocks : { 1, 256 }) {
        for (int rep = 0; rep < 2; ++rep) hipLaunchKernelGGL(k_mfma, dim3(blocks), dim3(256), 0, 0, d, sink, iters);
        hipMemcpy(&h, d, 8, hipMemcpyDeviceToHost);
        printf("blocks %3d  mfma 16x16x32 f16, 8 accumulators round robin : %.1f clk per MFMA\n", blocks, (double)h / (iters * 8));
        for (int mode = 0; mode < 2; ++mode) {
            for (int rep = 0; rep < 2; ++rep) hipLaunchKernelGGL(k_epi<SPLIT_SUB>, dim3(blocks), dim3(256), 0, 0, d, sink, iters, mode);
            hipMemcpy(&h, d, 8, hipMemcpyDeviceToHost);
            printf("blocks %3d  epilogue of 8 values (join%s)            : %.1f clk per value\n", blocks, (mode & 1) ? " + tanh" : "", (double)h / (iters * 8));
        }
        time_split<SPLIT_SUB>("SPLIT_SUB", blocks, d, sink, iters);
        time_split<SPLIT_MIX>("SPLIT_MIX", blocks, d, sink, iters);
        time_split<SPLIT_MIXLO>("SPLIT_MIXLO", blocks, d, sink, iters);
    }
    hipError_t e = hipDeviceSynchronize();
    printf("%s\n", hipGetErrorString(e));
    return (bad || e != hipSuccess) ? 1 : 0;
}
