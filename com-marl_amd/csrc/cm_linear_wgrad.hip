// cm_linear_wgrad.hip - the skinny-GEMM weight gradient of a per-agent dense layer (gfx950):
//   * cm_linear_wgrad, cm_linear_wgrad_det, cm_linear_wgrad_det_ws_bytes :
//         C[p][q] += sum_r A[r][p] * B[r][q]  over R = P*T*N rows, and colsum(A)
//     which is autograd's dW / db of nn.Linear (A = dY, B = X) and dW of the GCN's H.W (A = H, B = dZ,
//     graph_conv_module.py:63-70).  The other dense-layer backward kernels (one layer streamed, the encoder's two layers
//     chained) are in cm_linear_bwd.hip.
#include <algorithm>

#include "cm_internal.h"

namespace cm {

constexpr int TPB = 256;

// ---------------------------------------------------------------------------------------------
// Weight gradient of a per-agent dense layer over R = P*T*N rows (R ~ 1e6, P,Q <= 128):
//   C[p][q] += sum_r A[r][p] * B[r][q]         ( nn.Linear: A = dY, B = X -> dW [out][in], db = colsum(dY);
//                                                GCN H.W   : A = H,  B = dZ -> dW [in][out] )
// rocBLAS/hipBLASLt run these "skinny" GEMMs (tiny output, million-deep reduction) at ~10 TFLOP/s; they
// were 42 % of the PPO update.  Here a workgroup streams 64-row chunks of A and B through LDS and keeps
// its share of the P x Q output in f32 MFMA accumulators; partial results are merged with float atomics.
// ---------------------------------------------------------------------------------------------
typedef float v4f __attribute__((ext_vector_type(4)));
constexpr int WG_ROWS = 64;

// coalesced [WG_ROWS x W] global -> LDS copy (float4 when the row is a power-of-two number of float4s and src is 16-byte
// aligned; the ABI asks for 4 bytes)
__device__ __forceinline__ void stage_rows(float *dst, int stride, const float *__restrict__ src, int W, long r0, int rows, int tid) {
    const int w4 = W >> 2;
    if (!((uintptr_t)src & 15) && (W & 3) == 0 && (w4 & (w4 - 1)) == 0 && w4 <= TPB) {
        const int x = tid & (w4 - 1), rstep = TPB / w4;
        for (int r = tid / w4; r < WG_ROWS; r += rstep) {
            const float4 v = r < rows ? reinterpret_cast<const float4 *>(src + (r0 + r) * W)[x] : make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4 *>(dst + (size_t)r * stride + 4 * x) = v;
        }
    } else {
        for (int k = tid; k < WG_ROWS * W; k += TPB) { const int r = k / W, x = k - r * W; dst[(size_t)r * stride + x] = r < rows ? src[(r0 + r) * W + x] : 0.0f; }
    }
}

template <int MAXT, bool DET = false>   // accumulator tiles per wave; DET: slab mode (C, colsum_a address row 0, P Q + P floats per workgroup)
__global__ __launch_bounds__(TPB) void wgrad_kernel(long R, int P, int Q, const float *__restrict__ A, const float *__restrict__ B,
                                                   float *__restrict__ C, float *__restrict__ colsum_a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int PT = (P + 15) >> 4, QT = (Q + 15) >> 4, NT = PT * QT;
    const int SP = PT * 16 + 16, SQ = QT * 16 + 16;          // row strides == 16 (mod 32): conflict-free operand reads
    if constexpr (DET) {
        const size_t off = (size_t)blockIdx.x * ((size_t)P * Q + P);
        C += off;
        if (colsum_a) colsum_a += off;
    }
    float *As = lds, *Bs = As + (size_t)WG_ROWS * SP;
    v4f acc[MAXT];
    int aoff[MAXT], boff[MAXT];       // per-tile operand offsets, hoisted out of the k loop (no division per MFMA)
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
        acc[t] = (v4f){ 0.f, 0.f, 0.f, 0.f };
        const int tile = wave + 4 * t;
        const int tl = tile < NT ? tile : 0;              // idle slots recompute tile 0 and are never stored
        const int pt = tl / QT, qt = tl - pt * QT;
        aoff[t] = g * SP + c + pt * 16;
        boff[t] = g * SQ + c + qt * 16;
    }
    float csum = 0.0f;
    // zero the padding columns once (they feed MFMAs whose results are never stored)
    for (int k = tid; k < WG_ROWS * SP; k += TPB) As[k] = 0.0f;
    for (int k = tid; k < WG_ROWS * SQ; k += TPB) Bs[k] = 0.0f;
    __syncthreads();
    const long n_chunks = (R + WG_ROWS - 1) / WG_ROWS;
    for (long ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        const long r0 = ch * WG_ROWS;
        const int rows = (int)min((long)WG_ROWS, R - r0);
        stage_rows(As, SP, A, P, r0, rows, tid);
        stage_rows(Bs, SQ, B, Q, r0, rows, tid);
        __syncthreads();
        if (colsum_a && tid < P) { float sacc = 0.0f; for (int r = 0; r < WG_ROWS; ++r) sacc += As[(size_t)r * SP + tid]; csum += sacc; }
#pragma unroll 2
        for (int kk = 0; kk < WG_ROWS / 4; ++kk) {
            const float *ar = As + (size_t)(4 * kk) * SP, *br = Bs + (size_t)(4 * kk) * SQ;
            float av[MAXT], bw[MAXT];
#pragma unroll
            for (int t = 0; t < MAXT; ++t) { av[t] = ar[aoff[t]]; bw[t] = br[boff[t]]; }
#pragma unroll
            for (int t = 0; t < MAXT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t], bw[t], acc[t], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
        const int tile = wave + 4 * t;
        if (tile < NT) {
            const int pt = tile / QT, qt = tile - pt * QT, q = qt * 16 + c;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int pp = pt * 16 + 4 * g + r;
                if (pp < P && q < Q) merge_add<DET>(C + (size_t)pp * Q + q, acc[t][r]);
            }
        }
    }
    if (colsum_a && tid < P) merge_add<DET>(colsum_a + tid, csum);
}

}  // namespace cm

using namespace cm;

extern "C" size_t cm_linear_wgrad_det_ws_bytes(int64_t R, int32_t P, int32_t Q) {
    if (R <= 0 || P < 1 || Q < 1) return 0;
    return (size_t)std::min<int64_t>((R + WG_ROWS - 1) / WG_ROWS, 512) * ((size_t)P * Q + P) * sizeof(float);
}

// cm_linear_wgrad and its slab twin (DET: C and colsum_a from one P Q + P float row per workgroup, summed in index order)
template <bool DET>
static int linear_wgrad(const char *fn, int64_t R, int32_t P, int32_t Q, const float *a, const float *b, float *c, float *colsum_a, void *ws,
                        size_t ws_bytes, void *stream) {
    if (!a || !b || !c) return set_error(CM_ERR_ARG, std::string(fn) + ": null argument");
    if (P < 1 || Q < 1 || P > 128 || Q > 128) return set_error(CM_ERR_ARG, std::string(fn) + ": 1 <= P, Q <= 128 required");
    if (DET)
        if (const int rc = slab_check(ws, ws_bytes, cm_linear_wgrad_det_ws_bytes(R, P, Q), fn)) return rc;
    if (R <= 0) return CM_OK;
    const int PT = (P + 15) / 16, QT = (Q + 15) / 16, NT = PT * QT;
    const size_t lds = ((size_t)WG_ROWS * (PT * 16 + 16) + (size_t)WG_ROWS * (QT * 16 + 16)) * sizeof(float);
    const long chunks = (R + WG_ROWS - 1) / WG_ROWS;
    const int blocks = (int)std::min<long>(chunks, 512);
    const hipStream_t st = (hipStream_t)stream;
    const int per_wave = (NT + 3) / 4;
    static unsigned long long once = 0;
    if (cm::dev_first(once)) {
        CM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&wgrad_kernel<16, DET>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        CM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&wgrad_kernel<8, DET>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        CM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&wgrad_kernel<4, DET>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        CM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&wgrad_kernel<2, DET>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        CM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&wgrad_kernel<1, DET>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    }
    float *const slab = static_cast<float *>(ws);
    float *const gc = DET ? slab : c, *const gs = DET ? (colsum_a ? slab + (size_t)P * Q : nullptr) : colsum_a;
#define CM_WG(M) hipLaunchKernelGGL((wgrad_kernel<M, DET>), dim3(blocks), dim3(TPB), lds, st, (long)R, P, Q, a, b, gc, gs)
    if (per_wave <= 1) CM_WG(1); else if (per_wave <= 2) CM_WG(2); else if (per_wave <= 4) CM_WG(4);
    else if (per_wave <= 8) CM_WG(8); else CM_WG(16);
#undef CM_WG
    CM_HIP(hipGetLastError());
    if (!DET) return CM_OK;
    SlabSegs segs{};
    segs.s[0] = { c, 0, P * Q };
    segs.s[1] = { colsum_a, P * Q, P };
    segs.n_seg = colsum_a ? 2 : 1;
    return slab_reduce(slab, blocks, P * Q + P, segs, st);
}

extern "C" int cm_linear_wgrad(int64_t R, int32_t P, int32_t Q, const float *a, const float *b, float *c, float *colsum_a,
                               void *stream) {
    return linear_wgrad<false>(__func__, R, P, Q, a, b, c, colsum_a, nullptr, 0, stream);
}

extern "C" int cm_linear_wgrad_det(int64_t R, int32_t P, int32_t Q, const float *a, const float *b, float *c, float *colsum_a, void *ws,
                                   size_t ws_bytes, void *stream) {
    return linear_wgrad<true>(__func__, R, P, Q, a, b, c, colsum_a, ws, ws_bytes, stream);
}
