// cm_graph_ops.hip - the E = 64 graph ops of the training path (gfx950), forward and backward, each kernel family above
// the launchers that size it:
//   * cm_masked_agg_forward, cm_masked_agg_backward, cm_masked_agg_backward_r, cm_masked_agg_backward_det,
//     cm_masked_agg_backward_det_ws_bytes : the adjacency-masked GCN aggregation as one fused op for the autograd path
//     (com_marl/torch/modules/comm_base_net.py:99-105 + graph_conv_module.py:63-70):
//         A = M*R*C ; A /= rowsum + 1e-12 ; out = tanh(A.(HW) + b)
//   * cm_attention_forward, cm_attention_backward : attention scores + softmax (attention_module.py:39-49):
//         M[s,i,:] = softmax_j( Q[s,i,:] . E[s,j,:] )
// Samples are [P*T] env states; a 256-thread workgroup owns EPB whole samples so that the N x N mask tile and the N x 64
// feature tile are read from HBM exactly once.  Teams of 4 (the headline config) take the register kernels
// agg_bwd4_kernel / attn_bwd4_kernel in the backward, teams of 8 .. 128 the matrix-core kernels of cm_graph_ops_mfma.hip;
// the kernels for any embedding width are in cm_graph_any.hip.
#include <algorithm>

#include "cm_internal.h"

namespace cm {

constexpr int TPB = 256;
constexpr int RC = 4;

__host__ __device__ inline int agg_epb(int N) { return (N % RC == 0) ? (48 / N > 0 ? 48 / N : 1) : 1; }

// ---------------------------------------------------------------------------------------------------------------
// Teams of 4 (the headline config): the two generic backward kernels (agg_bwd_kernel, attn_bwd_kernel) as register
// kernels (agg_bwd4_kernel, attn_bwd4_kernel).  16 lanes own one env, lane c
// the four features 4c .. 4c+3 of each of the env's four agent rows: every global access is a 16-byte load / store in
// 256-byte row segments, ~256 bytes in flight per lane (the generic kernels stage through LDS with 4-byte accesses and
// run at ~2 TB/s once they read more than three streams).  The 4 x 4 coefficient matrices (normalised A, softmax
// gradient) are computed one element per lane and shared through LDS.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 f4_fma(float s, const float4 &v, const float4 &a) {
    return make_float4(fmaf(s, v.x, a.x), fmaf(s, v.y, a.y), fmaf(s, v.z, a.z), fmaf(s, v.w, a.w));
}
__device__ __forceinline__ float quad_sum(float v) {      // sum over the 4 lanes of a quad (lanes 4k .. 4k+3)
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    return v;
}

// ---------------------------------------------------------------------------------------------
// masked aggregation
// ---------------------------------------------------------------------------------------------
// LDS: A [rows][NP], HW [rows][SE], (bwd: dP [rows][SE], dA [rows][NP], mask [rows][NP], den [rows])
template <int E>
__global__ __launch_bounds__(TPB) void agg_fwd_kernel(int S, int N, int EPB, const float *__restrict__ attn,
                                                     const float *__restrict__ adj, const float *__restrict__ chan,
                                                     long ch_stride, const float *__restrict__ hw,
                                                     const float *__restrict__ bias, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int SE = E + 4;
    const int tid = threadIdx.x, NN = N * N, NP = N | 1, rows_max = EPB * N;
    float *A = lds, *HW = A + (size_t)rows_max * NP;
    for (int s0 = blockIdx.x * EPB; s0 < S; s0 += gridDim.x * EPB) {
        const int envs = min(EPB, S - s0), rows = envs * N;
        for (int k = tid; k < envs * NN; k += TPB) {
            const int e = k / NN, ij = k - e * NN, r = k / N, j = k - r * N;
            float v = attn[(size_t)s0 * NN + k];
            if (adj) v *= adj[(size_t)s0 * NN + k];
            if (chan) v *= chan[(size_t)(s0 + e) * ch_stride + ij];
            A[(size_t)r * NP + j] = v;
        }
        for (int k = tid; k < rows * E; k += TPB) { const int r = k / E, o = k - r * E; HW[(size_t)r * SE + o] = hw[(size_t)s0 * N * E + k]; }
        __syncthreads();
        for (int r = tid; r < rows; r += TPB) {
            float *ar = A + (size_t)r * NP;
            float sum = 0.0f;
            for (int j = 0; j < N; ++j) sum += ar[j];
            const float den = sum + 1e-12f;
            for (int j = 0; j < N; ++j) ar[j] = ar[j] / den;
        }
        __syncthreads();
        const int o = tid % E, rg = tid / E;
        const float bv = bias ? bias[o] : 0.0f;
        for (int r0 = rg * RC; r0 < rows; r0 += (TPB / E) * RC) {
            const int e = r0 / N;
            const float *h = HW + (size_t)e * N * SE + o;
            float acc[RC] = { 0.0f, 0.0f, 0.0f, 0.0f };
            const float *ar[RC];
#pragma unroll
            for (int i = 0; i < RC; ++i) ar[i] = A + (size_t)min(r0 + i, rows - 1) * NP;
            for (int j = 0; j < N; ++j) {
                const float hv = h[(size_t)j * SE];
#pragma unroll
                for (int i = 0; i < RC; ++i) acc[i] = fmaf(ar[i][j], hv, acc[i]);
            }
#pragma unroll
            for (int i = 0; i < RC; ++i)
                if (r0 + i < rows && (r0 + i) / N == e) out[((size_t)s0 * N + r0 + i) * E + o] = tanhf(acc[i] + bv);
        }
        __syncthreads();
    }
}

template <int E, bool DET = false>
__global__ __launch_bounds__(TPB) void agg_bwd_kernel(int S, int N, int EPB, const float *__restrict__ attn,
                                                     const float *__restrict__ adj, const float *__restrict__ chan,
                                                     long ch_stride, const float *__restrict__ hw,
                                                     const float *__restrict__ outv, const float *__restrict__ out_minus,
                                                     const float *__restrict__ d_out,
                                                     float *__restrict__ d_attn, float *__restrict__ d_hw,
                                                     float *__restrict__ d_bias) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int SE = E + 4;
    const int tid = threadIdx.x, NN = N * N, NP = N | 1, rows_max = EPB * N;
    float *A = lds;                                   // normalised A
    float *MK = A + (size_t)rows_max * NP;            // mask product R*C
    float *DA = MK + (size_t)rows_max * NP;           // dL/dA
    float *HW = DA + (size_t)rows_max * NP;           // [rows][SE]
    float *DP = HW + (size_t)rows_max * SE;           // dL/d(pre-activation) [rows][SE]
    float *den = DP + (size_t)rows_max * SE;          // [rows]
    float *dbs = den + rows_max;                      // [TPB/E][E] partial bias grads
    const int o = tid % E, rg = tid / E;
    float dbias_acc = 0.0f;
    for (int s0 = blockIdx.x * EPB; s0 < S; s0 += gridDim.x * EPB) {
        const int envs = min(EPB, S - s0), rows = envs * N;
        for (int k = tid; k < envs * NN; k += TPB) {
            const int e = k / NN, ij = k - e * NN, r = k / N, j = k - r * N;
            float m = 1.0f;
            if (adj) m *= adj[(size_t)s0 * NN + k];
            if (chan) m *= chan[(size_t)(s0 + e) * ch_stride + ij];
            MK[(size_t)r * NP + j] = m;
            A[(size_t)r * NP + j] = attn[(size_t)s0 * NN + k] * m;
        }
        for (int k = tid; k < rows * E; k += TPB) {
            const int r = k / E, c = k - r * E;
            const size_t g = (size_t)s0 * N * E + k;
            HW[(size_t)r * SE + c] = hw[g];
            const float y = out_minus ? outv[g] - out_minus[g] : outv[g];
            const float dp = d_out[g] * (fmaf(-y, y, 1.0f));          // tanh'
            DP[(size_t)r * SE + c] = dp;
        }
        __syncthreads();
        for (int r = tid; r < rows; r += TPB) {
            float *ar = A + (size_t)r * NP;
            float sum = 0.0f;
            for (int j = 0; j < N; ++j) sum += ar[j];
            const float dn = sum + 1e-12f;
            den[r] = dn;
            for (int j = 0; j < N; ++j) ar[j] = ar[j] / dn;
        }
        // bias grad partial: column o over this thread's row group
        for (int r = rg; r < rows; r += TPB / E) dbias_acc += DP[(size_t)r * SE + o];
        __syncthreads();
        // d_hw[j][o] = sum_i A[i][j] * dP[i][o]   (rows i of the same sample)
        for (int r0 = rg * RC; r0 < rows; r0 += (TPB / E) * RC) {
            const int e = r0 / N;
            float acc[RC] = { 0.0f, 0.0f, 0.0f, 0.0f };
            for (int i = 0; i < N; ++i) {
                const float dpv = DP[(size_t)(e * N + i) * SE + o];
                const float *ai = A + (size_t)(e * N + i) * NP;
#pragma unroll
                for (int q = 0; q < RC; ++q) {
                    const int j = min(r0 + q, rows - 1) - e * N;
                    if (j < N) acc[q] = fmaf(ai[j], dpv, acc[q]);
                }
            }
#pragma unroll
            for (int q = 0; q < RC; ++q)
                if (r0 + q < rows && (r0 + q) / N == e) d_hw[((size_t)s0 * N + r0 + q) * E + o] = acc[q];
        }
        // dA[i][j] = sum_o dP[i][o] * HW[j][o]
        for (int k = tid; k < envs * NN; k += TPB) {
            const int e = k / NN, ij = k - e * NN, i = ij / N, j = ij - i * N;
            const float4 *x = reinterpret_cast<const float4 *>(DP + (size_t)(e * N + i) * SE);
            const float4 *y = reinterpret_cast<const float4 *>(HW + (size_t)(e * N + j) * SE);
            float acc = 0.0f;
#pragma unroll
            for (int c = 0; c < E / 4; ++c) {
                const float4 u = x[c], v = y[c];
                acc = fmaf(u.x, v.x, acc); acc = fmaf(u.y, v.y, acc); acc = fmaf(u.z, v.z, acc); acc = fmaf(u.w, v.w, acc);
            }
            DA[(size_t)(e * N + i) * NP + j] = acc;
        }
        __syncthreads();
        // through the renormalisation: dM_ij = mask_ij * (dA_ij - sum_k dA_ik A_ik) / den_i
        for (int r = tid; r < rows; r += TPB) {
            const float *ar = A + (size_t)r * NP, *da = DA + (size_t)r * NP, *mk = MK + (size_t)r * NP;
            float t = 0.0f;
            for (int j = 0; j < N; ++j) t = fmaf(da[j], ar[j], t);
            const float inv = 1.0f / den[r];
            float *dst = d_attn + ((size_t)s0 * N + r) * N;
            for (int j = 0; j < N; ++j) dst[j] = mk[j] * (da[j] - t) * inv;
        }
        __syncthreads();
    }
    if (d_bias) {
        dbs[rg * E + o] = dbias_acc;
        __syncthreads();
        if (rg == 0) {
            float v = 0.0f;
            for (int q = 0; q < TPB / E; ++q) v += dbs[q * E + o];
            if constexpr (DET) d_bias[(size_t)blockIdx.x * E + o] = v;     // slab mode: row blockIdx.x
            else atomicAdd(d_bias + o, v);
        }
    }
}

template <bool DET = false>
__global__ __launch_bounds__(256) void agg_bwd4_kernel(int S, const float *__restrict__ attn, const float *__restrict__ adj,
                                                       const float *__restrict__ chan, long ch_stride, const float *__restrict__ hw,
                                                       const float *__restrict__ outv, const float *__restrict__ out_minus,
                                                       const float *__restrict__ d_out, float *__restrict__ d_attn,
                                                       float *__restrict__ d_hw, float *__restrict__ d_bias, int bias_reps) {
    __shared__ __attribute__((aligned(16))) float As[16][16];
    __shared__ float4 dbs[256];
    const int tid = threadIdx.x, grp = tid >> 4, c = tid & 15;
    float4 db = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int base = blockIdx.x * 16; base < S; base += gridDim.x * 16) {
        const int s = base + grp;
        const bool live = s < S;
        const size_t row0 = (size_t)s * 4 * 64;
        float4 h[4], dp[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            h[i] = dp[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live) {
                h[i] = *reinterpret_cast<const float4 *>(hw + row0 + i * 64 + 4 * c);
                float4 y = *reinterpret_cast<const float4 *>(outv + row0 + i * 64 + 4 * c);
                if (out_minus) {
                    const float4 u = *reinterpret_cast<const float4 *>(out_minus + row0 + i * 64 + 4 * c);
                    y.x -= u.x; y.y -= u.y; y.z -= u.z; y.w -= u.w;
                }
                const float4 d = *reinterpret_cast<const float4 *>(d_out + row0 + i * 64 + 4 * c);
                dp[i] = make_float4(d.x * (fmaf(-y.x, y.x, 1.0f)), d.y * (fmaf(-y.y, y.y, 1.0f)), d.z * (fmaf(-y.z, y.z, 1.0f)), d.w * (fmaf(-y.w, y.w, 1.0f)));   // tanh'
            }
        }
        // normalised A, element (i = c / 4, j = c % 4)
        float mk = 1.0f, av = 0.0f;
        if (live) {
            if (adj) mk *= adj[(size_t)s * 16 + c];
            if (chan) mk *= chan[(size_t)s * ch_stride + c];
            av = attn[(size_t)s * 16 + c] * mk;
        }
        const float den = quad_sum(av) + 1e-12f;
        const float an = av / den;
        __syncthreads();
        As[grp][c] = an;
        __syncthreads();
        float A[16];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 v = *reinterpret_cast<const float4 *>(&As[grp][4 * k]);
            A[4 * k] = v.x; A[4 * k + 1] = v.y; A[4 * k + 2] = v.z; A[4 * k + 3] = v.w;
        }
        // d_hw[j] = sum_i A[i][j] dP[i]
        if (live) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc = f4_fma(A[4 * i + j], dp[i], acc);
                *reinterpret_cast<float4 *>(d_hw + row0 + j * 64 + 4 * c) = acc;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) { db.x += dp[i].x; db.y += dp[i].y; db.z += dp[i].z; db.w += dp[i].w; }
        // dA[i][j] = sum_o dP[i][o] HW[j][o]: this lane's four features, then a reduce-scatter over the env's 16 lanes
        float v[16];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                v[4 * i + j] = fmaf(dp[i].x, h[j].x, fmaf(dp[i].y, h[j].y, fmaf(dp[i].z, h[j].z, dp[i].w * h[j].w)));
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const bool hi = c & 8;
            const float mine = hi ? v[k + 8] : v[k], other = hi ? v[k] : v[k + 8];
            v[k] = mine + __shfl_xor(other, 8);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool hi = c & 4;
            const float mine = hi ? v[k + 4] : v[k], other = hi ? v[k] : v[k + 4];
            v[k] = mine + __shfl_xor(other, 4);
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const bool hi = c & 2;
            const float mine = hi ? v[k + 2] : v[k], other = hi ? v[k] : v[k + 2];
            v[k] = mine + __shfl_xor(other, 2);
        }
        {
            const bool hi = c & 1;
            const float mine = hi ? v[1] : v[0], other = hi ? v[0] : v[1];
            v[0] = mine + __shfl_xor(other, 1);
        }
        // through the renormalisation: dM_ij = mask_ij * (dA_ij - sum_k dA_ik A_ik) / den_i
        const float da = v[0];
        const float tt = quad_sum(da * an);
        if (live) d_attn[(size_t)s * 16 + c] = mk * (da - tt) * (1.0f / den);
    }
    if (d_bias) {
        // 64 atomics per workgroup on the same two cache lines: with 2048 workgroups they serialise in the L2 (0.8 ns each: 105 of the
        // kernel's 312 us at 275 k envs) - the caller may hand `bias_reps` copies of the row, workgroup b adds into copy b % reps
        // (slab mode: bias_reps is the grid size, every workgroup stores into its own row)
        float *dbp = d_bias + (size_t)(blockIdx.x % (unsigned)bias_reps) * 64;
        dbs[tid] = db;
        __syncthreads();
        if (tid < 16) {
            float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int g2 = 0; g2 < 16; ++g2) { const float4 u = dbs[g2 * 16 + tid]; sum.x += u.x; sum.y += u.y; sum.z += u.z; sum.w += u.w; }
            merge_add<DET>(dbp + 4 * tid + 0, sum.x); merge_add<DET>(dbp + 4 * tid + 1, sum.y);
            merge_add<DET>(dbp + 4 * tid + 2, sum.z); merge_add<DET>(dbp + 4 * tid + 3, sum.w);
        }
    }
}

}  // namespace cm

using namespace cm;

static size_t agg_lds_fwd(int N, int E) { const int epb = agg_epb(N), rows = epb * N; return ((size_t)rows * (N | 1) + (size_t)rows * (E + 4)) * 4; }
static size_t agg_lds_bwd(int N, int E) {
    const int epb = agg_epb(N), rows = epb * N;
    return ((size_t)rows * (N | 1) * 3 + (size_t)rows * (E + 4) * 2 + rows + TPB) * 4;
}

extern "C" int cm_masked_agg_forward(int32_t S, int32_t N, int32_t E, const float *attn, const float *dist_adj,
                                     const float *chan, int64_t ch_stride, const float *hw, const float *bias,
                                     float *out, void *stream) {
    if (!attn || !hw || !out) return set_error(CM_ERR_ARG, "cm_masked_agg_forward: null argument");
    if (E != 64) return set_error(CM_ERR_ARG, "cm_masked_agg_forward: embedding dim 64 only");
    if (S <= 0) return CM_OK;
    const size_t lds = agg_lds_fwd(N, E);
    if (lds > 160 * 1024) return set_error(CM_ERR_ARG, "cm_masked_agg_forward: n_agents too large");
    const int epb = agg_epb(N);
    const int blocks = (int)std::min<long>((S + epb - 1) / epb, 256 * 8);
    return launch_lds<&agg_fwd_kernel<64>>(dim3(blocks), dim3(TPB), lds, stream, S, N, epb, attn, dist_adj, chan, (long)ch_stride, hw, bias, out);
}

extern "C" size_t cm_masked_agg_backward_det_ws_bytes(int32_t S, int32_t N, int32_t E) {
    if (S <= 0 || N < 1 || E < 1) return 0;
    return (size_t)std::min<int32_t>(S, 2048) * E * sizeof(float);        // every backward kernel's grid is <= min(S, 2048)
}

// cm_masked_agg_backward(_r) and the slab twin (DET: one 64-float row of d_bias per workgroup, summed in index order)
template <bool DET>
static int masked_agg_backward(const char *fn, int32_t S, int32_t N, int32_t E, const float *attn, const float *dist_adj,
                               const float *chan, int64_t ch_stride, const float *hw, const float *out, const float *out_minus,
                               const float *d_out, float *d_attn, float *d_hw, float *d_bias, int32_t bias_replicas, void *ws,
                               size_t ws_bytes, void *stream) {
    if (!attn || !hw || !out || !d_out || !d_attn || !d_hw) return set_error(CM_ERR_ARG, std::string(fn) + ": null argument");
    if (bias_replicas < 1) return set_error(CM_ERR_ARG, std::string(fn) + ": bias_replicas >= 1 required");
    if (E != 64) return set_error(CM_ERR_ARG, std::string(fn) + ": embedding dim 64 only");
    if (DET)
        if (const int rc = slab_check(ws, ws_bytes, cm_masked_agg_backward_det_ws_bytes(S, N, E), fn)) return rc;
    if (S <= 0) return CM_OK;
    if (DET && !d_bias)   // the twin without a bias gradient has no cross-workgroup sum left: the default kernels
        return cm_masked_agg_backward_r(S, N, E, attn, dist_adj, chan, ch_stride, hw, out, out_minus, d_out, d_attn, d_hw, nullptr, 1, stream);
    const hipStream_t st = (hipStream_t)stream;
    float *const slab = static_cast<float *>(ws), *const gb = DET ? slab : d_bias;
    int grid = 0;
    if (N == 4 && !(((uintptr_t)hw | (uintptr_t)out | (uintptr_t)out_minus | (uintptr_t)d_out | (uintptr_t)d_hw) & 15)) {
        // small batches: fewer workgroups looping (the bias atomics again: 2 500 envs take 11.6 us on 64 workgroups, 19 on 157)
        const long chunks = ((long)S + 15) / 16;
        grid = (int)(chunks <= 512 ? std::min<long>(chunks, 64) : std::min<long>(chunks, 2048));
        // (slab mode: bias_reps = the grid size, every workgroup stores its own row)
        hipLaunchKernelGGL(agg_bwd4_kernel<DET>, dim3(grid), dim3(256), 0, st, S, attn, dist_adj, chan, (long)ch_stride, hw, out,
                           out_minus, d_out, d_attn, d_hw, gb, DET ? grid : (int)bias_replicas);
        CM_HIP(hipGetLastError());
    } else if (const int rc = agg_bwd_mfma(DET, S, N, attn, dist_adj, chan, (long)ch_stride, hw, out, out_minus, d_out, d_attn, d_hw, gb,
                                           stream, &grid); rc != 1) {
        if (rc) return rc;
    } else {
        const size_t lds = agg_lds_bwd(N, E);
        if (lds > 160 * 1024) return set_error(CM_ERR_ARG, std::string(fn) + ": n_agents too large");
        const int epb = agg_epb(N);
        grid = (int)std::min<long>((S + epb - 1) / epb, 256 * 4);
        if (int rc = launch_lds<&agg_bwd_kernel<64, DET>>(dim3(grid), dim3(TPB), lds, st, S, N, epb, attn, dist_adj, chan, (long)ch_stride, hw, out,
                                                         out_minus, d_out, d_attn, d_hw, gb)) return rc;
    }
    if (!DET) return CM_OK;
    SlabSegs segs{};
    segs.s[0] = { d_bias, 0, 64 };
    segs.n_seg = 1;
    return slab_reduce(slab, grid, 64, segs, st);
}

extern "C" int cm_masked_agg_backward(int32_t S, int32_t N, int32_t E, const float *attn, const float *dist_adj,
                                      const float *chan, int64_t ch_stride, const float *hw, const float *out, const float *out_minus,
                                      const float *d_out, float *d_attn, float *d_hw, float *d_bias, void *stream) {
    return cm_masked_agg_backward_r(S, N, E, attn, dist_adj, chan, ch_stride, hw, out, out_minus, d_out, d_attn, d_hw, d_bias, 1, stream);
}

// (both default entry points land here: their messages name the family)
extern "C" int cm_masked_agg_backward_r(int32_t S, int32_t N, int32_t E, const float *attn, const float *dist_adj,
                                        const float *chan, int64_t ch_stride, const float *hw, const float *out, const float *out_minus,
                                        const float *d_out, float *d_attn, float *d_hw, float *d_bias, int32_t bias_replicas, void *stream) {
    return masked_agg_backward<false>("cm_masked_agg_backward", S, N, E, attn, dist_adj, chan, ch_stride, hw, out, out_minus, d_out, d_attn,
                                      d_hw, d_bias, bias_replicas, nullptr, 0, stream);
}

extern "C" int cm_masked_agg_backward_det(int32_t S, int32_t N, int32_t E, const float *attn, const float *dist_adj,
                                          const float *chan, int64_t ch_stride, const float *hw, const float *out, const float *out_minus,
                                          const float *d_out, float *d_attn, float *d_hw, float *d_bias, void *ws, size_t ws_bytes,
                                          void *stream) {
    return masked_agg_backward<true>(__func__, S, N, E, attn, dist_adj, chan, ch_stride, hw, out, out_minus, d_out, d_attn, d_hw, d_bias, 1,
                                     ws, ws_bytes, stream);
}

namespace cm {

// ---------------------------------------------------------------------------------------------
// attention scores + softmax for the autograd path (attention_module.py:39-49):
//   M[s,i,:] = softmax_j( Q[s,i,:] . E[s,j,:] )          Q = linear_in(E) comes from a torch GEMM
// torch.matmul lowers this to a batched GEMM with N x N outputs (4 x 4 at config 2): three such GEMMs
// (forward, dQ, dE) were 31 % of the PPO update.  Here a workgroup owns EPB whole samples, the Q / E
// tiles are read from HBM once and everything else happens in LDS.
// ---------------------------------------------------------------------------------------------
template <int E>
__global__ __launch_bounds__(TPB) void attn_fwd_kernel(int S, int N, int EPB, const float *__restrict__ q,
                                                      const float *__restrict__ e, float *__restrict__ m) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int SE = E + 4;
    const int tid = threadIdx.x, NN = N * N, NP = N | 1, rows_max = EPB * N;
    float *Q = lds, *K = Q + (size_t)rows_max * SE, *M = K + (size_t)rows_max * SE;
    for (int s0 = blockIdx.x * EPB; s0 < S; s0 += gridDim.x * EPB) {
        const int envs = min(EPB, S - s0), rows = envs * N;
        for (int k = tid; k < rows * (E / 4); k += TPB) {
            const int r = k / (E / 4), c = k - r * (E / 4);
            reinterpret_cast<float4 *>(Q + (size_t)r * SE)[c] = reinterpret_cast<const float4 *>(q + ((size_t)s0 * N + r) * E)[c];
            reinterpret_cast<float4 *>(K + (size_t)r * SE)[c] = reinterpret_cast<const float4 *>(e + ((size_t)s0 * N + r) * E)[c];
        }
        __syncthreads();
        for (int k = tid; k < envs * NN; k += TPB) {
            const int en = k / NN, ij = k - en * NN, i = ij / N, j = ij - i * N;
            const float4 *x = reinterpret_cast<const float4 *>(Q + (size_t)(en * N + i) * SE);
            const float4 *y = reinterpret_cast<const float4 *>(K + (size_t)(en * N + j) * SE);
            float acc = 0.0f;
#pragma unroll
            for (int c = 0; c < E / 4; ++c) {
                const float4 u = x[c], v = y[c];
                acc = fmaf(u.x, v.x, acc); acc = fmaf(u.y, v.y, acc); acc = fmaf(u.z, v.z, acc); acc = fmaf(u.w, v.w, acc);
            }
            M[(size_t)(en * N + i) * NP + j] = acc;
        }
        __syncthreads();
        for (int r = tid; r < rows; r += TPB) {
            float *mr = M + (size_t)r * NP;
            float mx = -INFINITY, sum = 0.0f;
            for (int j = 0; j < N; ++j) mx = fmaxf(mx, mr[j]);
            for (int j = 0; j < N; ++j) { const float ex = expf(mr[j] - mx); mr[j] = ex; sum += ex; }
            float *dst = m + ((size_t)s0 * N + r) * N;
            for (int j = 0; j < N; ++j) dst[j] = mr[j] / sum;
        }
        __syncthreads();
    }
}

// dS = M * (dM - sum_j dM*M) ; dQ = dS . E ; dE = dS^T . Q
template <int E>
__global__ __launch_bounds__(TPB) void attn_bwd_kernel(int S, int N, int EPB, const float *__restrict__ q,
                                                      const float *__restrict__ e, const float *__restrict__ m,
                                                      const float *__restrict__ d_m, const float *__restrict__ add0,
                                                      const float *__restrict__ add1, float *__restrict__ d_q,
                                                      float *__restrict__ d_e) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int SE = E + 4;
    const int tid = threadIdx.x, NP = N | 1, rows_max = EPB * N;
    float *Q = lds, *K = Q + (size_t)rows_max * SE, *DS = K + (size_t)rows_max * SE;
    for (int s0 = blockIdx.x * EPB; s0 < S; s0 += gridDim.x * EPB) {
        const int envs = min(EPB, S - s0), rows = envs * N;
        for (int k = tid; k < rows * (E / 4); k += TPB) {
            const int r = k / (E / 4), c = k - r * (E / 4);
            reinterpret_cast<float4 *>(Q + (size_t)r * SE)[c] = reinterpret_cast<const float4 *>(q + ((size_t)s0 * N + r) * E)[c];
            reinterpret_cast<float4 *>(K + (size_t)r * SE)[c] = reinterpret_cast<const float4 *>(e + ((size_t)s0 * N + r) * E)[c];
        }
        for (int r = tid; r < rows; r += TPB) {
            const float *mr = m + ((size_t)s0 * N + r) * N, *dr = d_m + ((size_t)s0 * N + r) * N;
            float t = 0.0f;
            for (int j = 0; j < N; ++j) t = fmaf(dr[j], mr[j], t);
            for (int j = 0; j < N; ++j) DS[(size_t)r * NP + j] = mr[j] * (dr[j] - t);
        }
        __syncthreads();
        const int o = tid % E, rg = tid / E;
        for (int r0 = rg * RC; r0 < rows; r0 += (TPB / E) * RC) {
            const int en = r0 / N;
            float aq[RC] = { 0.f, 0.f, 0.f, 0.f }, ae[RC] = { 0.f, 0.f, 0.f, 0.f };
            for (int j = 0; j < N; ++j) {
                const float ev = K[(size_t)(en * N + j) * SE + o], qv = Q[(size_t)(en * N + j) * SE + o];
#pragma unroll
                for (int i = 0; i < RC; ++i) {
                    const int r = min(r0 + i, rows - 1), li = r - en * N;
                    if (li < N) {
                        aq[i] = fmaf(DS[(size_t)r * NP + j], ev, aq[i]);                  // dQ[i] += dS[i][j] E[j]
                        ae[i] = fmaf(DS[(size_t)(en * N + j) * NP + li], qv, ae[i]);      // dE[i] += dS[j][i] Q[j]
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < RC; ++i)
                if (r0 + i < rows && (r0 + i) / N == en) {
                    const size_t at = ((size_t)s0 * N + r0 + i) * E + o;
                    d_q[at] = aq[i];
                    float v = ae[i];
                    if (add0) v += add0[at];
                    if (add1) v += add1[at];
                    d_e[at] = v;
                }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void attn_bwd4_kernel(int S, const float *__restrict__ q, const float *__restrict__ e,
                                                        const float *__restrict__ m, const float *__restrict__ d_m,
                                                        const float *__restrict__ add0, const float *__restrict__ add1,
                                                        float *__restrict__ d_q, float *__restrict__ d_e) {
    __shared__ __attribute__((aligned(16))) float DSs[16][16];
    const int tid = threadIdx.x, grp = tid >> 4, c = tid & 15;
    for (int base = blockIdx.x * 16; base < S; base += gridDim.x * 16) {
        const int s = base + grp;
        const bool live = s < S;
        const size_t row0 = (size_t)s * 4 * 64;
        float4 qv[4], ev[4], a0[4], a1[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            qv[i] = ev[i] = a0[i] = a1[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live) {
                qv[i] = *reinterpret_cast<const float4 *>(q + row0 + i * 64 + 4 * c);
                ev[i] = *reinterpret_cast<const float4 *>(e + row0 + i * 64 + 4 * c);
                if (add0) a0[i] = *reinterpret_cast<const float4 *>(add0 + row0 + i * 64 + 4 * c);
                if (add1) a1[i] = *reinterpret_cast<const float4 *>(add1 + row0 + i * 64 + 4 * c);
            }
        }
        // softmax backward, element (i = c / 4, j = c % 4): dS = m * (dm - sum_j dm m)
        const float mv = live ? m[(size_t)s * 16 + c] : 0.0f, dv = live ? d_m[(size_t)s * 16 + c] : 0.0f;
        const float t = quad_sum(dv * mv);
        __syncthreads();                                   // previous iteration's readers are done
        DSs[grp][c] = mv * (dv - t);
        __syncthreads();
        float ds[16];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 v = *reinterpret_cast<const float4 *>(&DSs[grp][4 * k]);
            ds[4 * k] = v.x; ds[4 * k + 1] = v.y; ds[4 * k + 2] = v.z; ds[4 * k + 3] = v.w;
        }
        if (live) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float4 aq = make_float4(0.f, 0.f, 0.f, 0.f), ae = aq;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    aq = f4_fma(ds[4 * i + j], ev[j], aq);                 // dQ[i] += dS[i][j] E[j]
                    ae = f4_fma(ds[4 * j + i], qv[j], ae);                 // dE[i] += dS[j][i] Q[j]
                }
                if (add0) { ae.x += a0[i].x; ae.y += a0[i].y; ae.z += a0[i].z; ae.w += a0[i].w; }
                if (add1) { ae.x += a1[i].x; ae.y += a1[i].y; ae.z += a1[i].z; ae.w += a1[i].w; }
                *reinterpret_cast<float4 *>(d_q + row0 + i * 64 + 4 * c) = aq;
                *reinterpret_cast<float4 *>(d_e + row0 + i * 64 + 4 * c) = ae;
            }
        }
    }
}

}  // namespace cm

static size_t attn_lds(int N, int E) { const int epb = agg_epb(N), rows = epb * N; return ((size_t)rows * (E + 4) * 2 + (size_t)rows * (N | 1)) * 4; }

extern "C" int cm_attention_forward(int32_t S, int32_t N, int32_t E, const float *q, const float *e, float *m, void *stream) {
    if (!q || !e || !m) return set_error(CM_ERR_ARG, "cm_attention_forward: null argument");
    if (E != 64) return set_error(CM_ERR_ARG, "cm_attention_forward: embedding dim 64 only");
    if (S <= 0) return CM_OK;
    const size_t lds = attn_lds(N, E);
    if (lds > 160 * 1024) return set_error(CM_ERR_ARG, "cm_attention_forward: n_agents too large");
    const int epb = agg_epb(N);
    const int blocks = (int)std::min<long>((S + epb - 1) / epb, 256 * 8);
    return launch_lds<&attn_fwd_kernel<64>>(dim3(blocks), dim3(TPB), lds, stream, S, N, epb, q, e, m);
}

extern "C" int cm_attention_backward(int32_t S, int32_t N, int32_t E, const float *q, const float *e, const float *m,
                                     const float *d_m, const float *d_e_add0, const float *d_e_add1, float *d_q, float *d_e,
                                     void *stream) {
    if (!q || !e || !m || !d_m || !d_q || !d_e) return set_error(CM_ERR_ARG, "cm_attention_backward: null argument");
    if (d_e == d_e_add0 || d_e == d_e_add1) return set_error(CM_ERR_ARG, "cm_attention_backward: d_e must not alias its addends");
    if (E != 64) return set_error(CM_ERR_ARG, "cm_attention_backward: embedding dim 64 only");
    if (S <= 0) return CM_OK;
    if (N == 4 && !(((uintptr_t)q | (uintptr_t)e | (uintptr_t)d_e_add0 | (uintptr_t)d_e_add1 | (uintptr_t)d_q | (uintptr_t)d_e) & 15)) {
        const int blocks = (int)std::min<long>((S + 15) / 16, 4096);
        hipLaunchKernelGGL(attn_bwd4_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, S, q, e, m, d_m, d_e_add0, d_e_add1, d_q, d_e);
        CM_HIP(hipGetLastError());
        return CM_OK;
    }
    if (const int rc = attn_bwd_mfma(S, N, q, e, m, d_m, d_e_add0, d_e_add1, d_q, d_e, stream); rc != 1) return rc;
    const size_t lds = attn_lds(N, E);
    if (lds > 160 * 1024) return set_error(CM_ERR_ARG, "cm_attention_backward: n_agents too large");
    const int epb = agg_epb(N);
    const int blocks = (int)std::min<long>((S + epb - 1) / epb, 256 * 8);
    return launch_lds<&attn_bwd_kernel<64>>(dim3(blocks), dim3(TPB), lds, stream, S, N, epb, q, e, m, d_m, d_e_add0, d_e_add1, d_q, d_e);
}
