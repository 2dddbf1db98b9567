// cm_graph_any.hip - the graph ops of the PPO update for ANY embedding width E in 1..128 (gfx950):
//   cm_attention_forward_any / _backward_any     M = softmax_j(q_i . e_j) and its gradients
//   cm_masked_agg_forward_any / _backward_any    out = tanh(A.(HW) + b), A = M*R*C row-renormalised, and its gradients
// cm_attention_* / cm_masked_agg_* (cm_graph_ops.hip, cm_graph_ops_mfma.hip) are built for E = 64: their lane map o = tid % E needs
// E | 256.  Here E is a run-time argument: the N x E products are dealt to the threads as (group of RC rows, column) work
// items, so any width runs; the arithmetic per element is that of the E = 64 first-generation kernels of cm_graph_ops.hip (tanh'
// as one fma, the +1e-12 row sum, softmax with the max subtracted, the same order of every sum).
// A 256-thread workgroup owns EPB whole envs per round of a grid-stride loop.  LDS planes (floats, integer offsets into one
// array, every base a multiple of 4): N x N planes with row stride NP = N | 1, N x E planes with row stride SE = pad4(E) + 4.
// A ragged E (no multiple of 4) is zero-filled up to pad4(E) in LDS - the 16-byte dot products read the padding, HBM is
// never read past a row - and rows whose byte length is no multiple of 16 (or whose base is not 16-byte aligned) are
// staged with 4-byte accesses.
#include <algorithm>

#include "cm_internal.h"

namespace cm {
namespace ga {

constexpr int TPB = 256, RC = 4, MAX_E = 128, MAX_N = 128;
constexpr size_t LDS_LIMIT = 160 * 1024;
constexpr int GRID_CAP = 2048, GRID_CAP_AGG_BWD = 1024;     // (<= min(S, 2048): the slab of the _det twin has that many rows)

// The one place the LDS need is computed.  ALL six entry points answer "fits" from the largest of the four kernels' needs
// (the aggregation backward's), so a shape whose forward runs never meets a backward that does not.
struct Plan { int EPB, NP, SE, matN, matE, rv; size_t agg_fwd, agg_bwd, attn_fwd, attn_bwd; };

__host__ inline int r4(int x) { return (x + 3) & ~3; }
__host__ inline Plan plan(int N, int E) {
    Plan p;
    p.EPB = (N % RC == 0) ? (48 / N > 0 ? 48 / N : 1) : 1;  // agg_epb of cm_graph_ops.hip: a group of RC rows never straddles envs
    const int rows = p.EPB * N;
    p.NP = N | 1;
    p.SE = r4(E) + 4;
    p.matN = r4(rows * p.NP);
    p.matE = rows * p.SE;
    p.rv = r4(rows);
    p.agg_fwd = (size_t)(p.matN + p.matE) * 4;
    p.agg_bwd = (size_t)(2 * p.matN + 2 * p.matE + 2 * p.rv + TPB) * 4;   // (+ the bias partials [TPB / E][E])
    p.attn_fwd = (size_t)(2 * p.matE + p.matN + p.rv) * 4;
    p.attn_bwd = (size_t)(2 * p.matE + 2 * p.matN) * 4;
    return p;
}
__host__ inline bool fits(const Plan &p) {
    return std::max(std::max(p.agg_fwd, p.agg_bwd), std::max(p.attn_fwd, p.attn_bwd)) <= LDS_LIMIT;
}

__device__ __forceinline__ void zero_lds(float *lds, int total, int tid) {
    for (int k = tid * 4; k < total; k += TPB * 4) *reinterpret_cast<float4 *>(&lds[k]) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// rows x E contiguous floats at src -> the plane at `off` (row stride SE).  vec: E % 4 == 0 and src 16-byte aligned.
__device__ __forceinline__ void stage_rows(float *lds, int off, int SE, const float *__restrict__ src, int rows, int E, int vec, int tid) {
    if (vec) {
        const int e4 = E >> 2;
        for (int k = tid; k < rows * e4; k += TPB) {
            const int r = k / e4, c = k - r * e4;
            *reinterpret_cast<float4 *>(&lds[off + r * SE + 4 * c]) = reinterpret_cast<const float4 *>(src)[k];
        }
    } else {
        for (int k = tid; k < rows * E; k += TPB) { const int r = k / E, c = k - r * E; lds[off + r * SE + c] = src[k]; }
    }
}

// sum_c x[c] * y[c] over the pad4(E) floats of two LDS rows, in the order of the E = 64 kernels' float4 loop
__device__ __forceinline__ float dot_rows(const float *lds, int x, int y, int e4) {
    float acc = 0.0f;
    for (int c = 0; c < e4; ++c) {
        const float4 u = *reinterpret_cast<const float4 *>(&lds[x + 4 * c]), v = *reinterpret_cast<const float4 *>(&lds[y + 4 * c]);
        acc = fmaf(u.x, v.x, acc); acc = fmaf(u.y, v.y, acc); acc = fmaf(u.z, v.z, acc); acc = fmaf(u.w, v.w, acc);
    }
    return acc;
}

// LDS: A [rows][NP], HW [rows][SE]
__global__ __launch_bounds__(TPB) void agg_fwd_any_kernel(int S, int N, int E, int EPB, int vec, const float *__restrict__ attn,
                                                         const float *__restrict__ adj, const float *__restrict__ chan, long ch_stride,
                                                         const float *__restrict__ hw, const float *__restrict__ bias,
                                                         float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, NN = N * N, NP = N | 1, SE = ((E + 3) & ~3) + 4, rows_max = EPB * N;
    const int oA = 0, oHW = (rows_max * NP + 3) & ~3;
    for (int s0 = blockIdx.x * EPB; s0 < S; s0 += gridDim.x * EPB) {
        const int envs = min(EPB, S - s0), rows = envs * N;
        for (int k = tid; k < envs * NN; k += TPB) {
            const int e = k / NN, ij = k - e * NN, r = k / N, j = k - r * N;
            float v = attn[(size_t)s0 * NN + k];
            if (adj) v *= adj[(size_t)s0 * NN + k];
            if (chan) v *= chan[(size_t)(s0 + e) * ch_stride + ij];
            lds[oA + r * NP + j] = v;
        }
        stage_rows(lds, oHW, SE, hw + (size_t)s0 * N * E, rows, E, vec, tid);
        __syncthreads();
        for (int r = tid; r < rows; r += TPB) {
            const int ar = oA + r * NP;
            float sum = 0.0f;
            for (int j = 0; j < N; ++j) sum += lds[ar + j];
            const float den = sum + 1e-12f;
            for (int j = 0; j < N; ++j) lds[ar + j] = lds[ar + j] / den;
        }
        __syncthreads();
        const int nrg = (rows + RC - 1) / RC;
        for (int it = tid; it < nrg * E; it += TPB) {
            const int rg = it / E, o = it - rg * E, r0 = rg * RC, e = r0 / N;
            const float bv = bias ? bias[o] : 0.0f;
            const int h = oHW + e * N * SE + o;
            const int a0 = oA + min(r0, rows - 1) * NP, a1 = oA + min(r0 + 1, rows - 1) * NP;
            const int a2 = oA + min(r0 + 2, rows - 1) * NP, a3 = oA + min(r0 + 3, rows - 1) * NP;
            float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f;
            for (int j = 0; j < N; ++j) {
                const float hv = lds[h + j * SE];
                c0 = fmaf(lds[a0 + j], hv, c0); c1 = fmaf(lds[a1 + j], hv, c1);
                c2 = fmaf(lds[a2 + j], hv, c2); c3 = fmaf(lds[a3 + j], hv, c3);
            }
            float *dst = out + ((size_t)s0 * N + r0) * E + o;
            if (r0 < rows) dst[0] = tanhf(c0 + bv);
            if (r0 + 1 < rows && (r0 + 1) / N == e) dst[E] = tanhf(c1 + bv);
            if (r0 + 2 < rows && (r0 + 2) / N == e) dst[2 * E] = tanhf(c2 + bv);
            if (r0 + 3 < rows && (r0 + 3) / N == e) dst[3 * E] = tanhf(c3 + bv);
        }
        __syncthreads();
    }
}

// LDS: A [rows][NP] normalised, DA [rows][NP] dL/dA, HW [rows][SE], DP [rows][SE] dL/d(pre-activation), den [rows], tr [rows],
// dbs [TPB / E][E] bias partials
template <bool DET>
__global__ __launch_bounds__(TPB) void agg_bwd_any_kernel(int S, int N, int E, int EPB, int vec, const float *__restrict__ attn,
                                                         const float *__restrict__ adj, const float *__restrict__ chan, long ch_stride,
                                                         const float *__restrict__ hw, const float *__restrict__ outv,
                                                         const float *__restrict__ out_minus, const float *__restrict__ d_out,
                                                         float *__restrict__ d_attn, float *__restrict__ d_hw, float *__restrict__ d_bias) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, NN = N * N, NP = N | 1, EP4 = (E + 3) & ~3, SE = EP4 + 4, e4 = EP4 >> 2, rows_max = EPB * N;
    const int matN = (rows_max * NP + 3) & ~3, matE = rows_max * SE, rv = (rows_max + 3) & ~3;
    const int oA = 0, oDA = matN, oHW = 2 * matN, oDP = oHW + matE, oDen = oDP + matE, oTr = oDen + rv, oDb = oTr + rv;
    zero_lds(lds, oDb + TPB, tid);                    // (the padding columns of HW / DP stay zero from here on)
    __syncthreads();
    // bias gradient: thread (q, o) = (tid / E, tid % E), q < TPB / E, sums column o over rows q, q + nq, ... of every round
    const int nq = TPB / E, bq = tid / E, bo = tid - bq * E;
    float dbias_acc = 0.0f;
    for (int s0 = blockIdx.x * EPB; s0 < S; s0 += gridDim.x * EPB) {
        const int envs = min(EPB, S - s0), rows = envs * N;
        for (int k = tid; k < envs * NN; k += TPB) {
            const int e = k / NN, ij = k - e * NN, r = k / N, j = k - r * N;
            float m = 1.0f;
            if (adj) m *= adj[(size_t)s0 * NN + k];
            if (chan) m *= chan[(size_t)(s0 + e) * ch_stride + ij];
            lds[oA + r * NP + j] = attn[(size_t)s0 * NN + k] * m;
        }
        {
            const size_t g0 = (size_t)s0 * N * E;
            stage_rows(lds, oHW, SE, hw + g0, rows, E, vec, tid);
            if (vec) {
                const int q4 = E >> 2;
                const float4 *po = reinterpret_cast<const float4 *>(outv + g0), *pd = reinterpret_cast<const float4 *>(d_out + g0);
                const float4 *pm = out_minus ? reinterpret_cast<const float4 *>(out_minus + g0) : nullptr;
                for (int k = tid; k < rows * q4; k += TPB) {
                    const int r = k / q4, c = k - r * q4;
                    float4 y = po[k];
                    const float4 dv = pd[k];
                    if (pm) { const float4 mv = pm[k]; y.x -= mv.x; y.y -= mv.y; y.z -= mv.z; y.w -= mv.w; }
                    *reinterpret_cast<float4 *>(&lds[oDP + r * SE + 4 * c]) =
                        make_float4(dv.x * fmaf(-y.x, y.x, 1.0f), dv.y * fmaf(-y.y, y.y, 1.0f), dv.z * fmaf(-y.z, y.z, 1.0f),
                                    dv.w * fmaf(-y.w, y.w, 1.0f));
                }
            } else {
                for (int k = tid; k < rows * E; k += TPB) {
                    const int r = k / E, c = k - r * E;
                    const float y = out_minus ? outv[g0 + k] - out_minus[g0 + k] : outv[g0 + k];
                    lds[oDP + r * SE + c] = d_out[g0 + k] * fmaf(-y, y, 1.0f);          // tanh'
                }
            }
        }
        __syncthreads();
        for (int r = tid; r < rows; r += TPB) {
            const int ar = oA + r * NP;
            float sum = 0.0f;
            for (int j = 0; j < N; ++j) sum += lds[ar + j];
            const float dn = sum + 1e-12f;
            lds[oDen + r] = dn;
            for (int j = 0; j < N; ++j) lds[ar + j] = lds[ar + j] / dn;
        }
        if (bq < nq)
            for (int r = bq; r < rows; r += nq) dbias_acc += lds[oDP + r * SE + bo];
        __syncthreads();
        // d_hw[j][o] = sum_i A[i][j] * dP[i][o]   (rows i of the same env)
        const int nrg = (rows + RC - 1) / RC;
        for (int it = tid; it < nrg * E; it += TPB) {
            const int rg = it / E, o = it - rg * E, r0 = rg * RC, e = r0 / N;
            const int j0 = min(r0, rows - 1) - e * N, j1 = min(r0 + 1, rows - 1) - e * N;
            const int j2 = min(r0 + 2, rows - 1) - e * N, j3 = min(r0 + 3, rows - 1) - e * N;
            float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f;
            for (int i = 0; i < N; ++i) {
                const float dpv = lds[oDP + (e * N + i) * SE + o];
                const int ai = oA + (e * N + i) * NP;
                if (j0 < N) c0 = fmaf(lds[ai + j0], dpv, c0);
                if (j1 < N) c1 = fmaf(lds[ai + j1], dpv, c1);
                if (j2 < N) c2 = fmaf(lds[ai + j2], dpv, c2);
                if (j3 < N) c3 = fmaf(lds[ai + j3], dpv, c3);
            }
            float *dst = d_hw + ((size_t)s0 * N + r0) * E + o;
            if (r0 < rows) dst[0] = c0;
            if (r0 + 1 < rows && (r0 + 1) / N == e) dst[E] = c1;
            if (r0 + 2 < rows && (r0 + 2) / N == e) dst[2 * E] = c2;
            if (r0 + 3 < rows && (r0 + 3) / N == e) dst[3 * E] = c3;
        }
        // dA[i][j] = sum_o dP[i][o] * HW[j][o]
        for (int k = tid; k < envs * NN; k += TPB) {
            const int e = k / NN, ij = k - e * NN, i = ij / N, j = ij - i * N;
            lds[oDA + (e * N + i) * NP + j] = dot_rows(lds, oDP + (e * N + i) * SE, oHW + (e * N + j) * SE, e4);
        }
        __syncthreads();
        // through the renormalisation: dM_ij = mask_ij * (dA_ij - sum_k dA_ik A_ik) / den_i
        for (int r = tid; r < rows; r += TPB) {
            const int ar = oA + r * NP, da = oDA + r * NP;
            float t = 0.0f;
            for (int j = 0; j < N; ++j) t = fmaf(lds[da + j], lds[ar + j], t);
            lds[oTr + r] = t;
        }
        __syncthreads();
        for (int k = tid; k < envs * NN; k += TPB) {
            const int e = k / NN, ij = k - e * NN, r = k / N, j = k - r * N;
            float m = 1.0f;
            if (adj) m *= adj[(size_t)s0 * NN + k];
            if (chan) m *= chan[(size_t)(s0 + e) * ch_stride + ij];
            const float inv = 1.0f / lds[oDen + r];
            d_attn[(size_t)s0 * NN + k] = m * (lds[oDA + r * NP + j] - lds[oTr + r]) * inv;
        }
        __syncthreads();
    }
    if (d_bias) {
        if (bq < nq) lds[oDb + bq * E + bo] = dbias_acc;
        __syncthreads();
        if (tid < E) {
            float v = 0.0f;
            for (int q = 0; q < nq; ++q) v += lds[oDb + q * E + tid];
            if constexpr (DET) d_bias[(size_t)blockIdx.x * E + tid] = v;     // slab mode: row blockIdx.x
            else atomicAdd(d_bias + tid, v);
        }
    }
}

// LDS: Q [rows][SE], K [rows][SE], M [rows][NP], sum [rows]
__global__ __launch_bounds__(TPB) void attn_fwd_any_kernel(int S, int N, int E, int EPB, int vec, const float *__restrict__ q,
                                                          const float *__restrict__ e, float *__restrict__ m) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, NN = N * N, NP = N | 1, EP4 = (E + 3) & ~3, SE = EP4 + 4, e4 = EP4 >> 2, rows_max = EPB * N;
    const int matN = (rows_max * NP + 3) & ~3, matE = rows_max * SE, rv = (rows_max + 3) & ~3;
    const int oQ = 0, oK = matE, oM = 2 * matE, oSum = oM + matN;
    zero_lds(lds, oSum + rv, tid);
    __syncthreads();
    for (int s0 = blockIdx.x * EPB; s0 < S; s0 += gridDim.x * EPB) {
        const int envs = min(EPB, S - s0), rows = envs * N;
        stage_rows(lds, oQ, SE, q + (size_t)s0 * N * E, rows, E, vec, tid);
        stage_rows(lds, oK, SE, e + (size_t)s0 * N * E, rows, E, vec, tid);
        __syncthreads();
        for (int k = tid; k < envs * NN; k += TPB) {
            const int en = k / NN, ij = k - en * NN, i = ij / N, j = ij - i * N;
            lds[oM + (en * N + i) * NP + j] = dot_rows(lds, oQ + (en * N + i) * SE, oK + (en * N + j) * SE, e4);
        }
        __syncthreads();
        for (int r = tid; r < rows; r += TPB) {
            const int mr = oM + r * NP;
            float mx = -INFINITY, sum = 0.0f;
            for (int j = 0; j < N; ++j) mx = fmaxf(mx, lds[mr + j]);
            for (int j = 0; j < N; ++j) { const float ex = expf(lds[mr + j] - mx); lds[mr + j] = ex; sum += ex; }
            lds[oSum + r] = sum;
        }
        __syncthreads();
        for (int k = tid; k < envs * NN; k += TPB) {
            const int r = k / N, j = k - r * N;
            m[(size_t)s0 * NN + k] = lds[oM + r * NP + j] / lds[oSum + r];
        }
        __syncthreads();
    }
}

// dS = M * (dM - sum_j dM*M) ; dQ = dS . E ; dE = dS^T . Q.   LDS: Q [rows][SE], K [rows][SE], DS [rows][NP], DM [rows][NP]
__global__ __launch_bounds__(TPB) void attn_bwd_any_kernel(int S, int N, int E, int EPB, int vec, const float *__restrict__ q,
                                                          const float *__restrict__ e, const float *__restrict__ m,
                                                          const float *__restrict__ d_m, const float *__restrict__ add0,
                                                          const float *__restrict__ add1, float *__restrict__ d_q,
                                                          float *__restrict__ d_e) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, NN = N * N, NP = N | 1, SE = ((E + 3) & ~3) + 4, rows_max = EPB * N;
    const int matN = (rows_max * NP + 3) & ~3, matE = rows_max * SE;
    const int oQ = 0, oK = matE, oDS = 2 * matE, oDM = oDS + matN;
    for (int s0 = blockIdx.x * EPB; s0 < S; s0 += gridDim.x * EPB) {
        const int envs = min(EPB, S - s0), rows = envs * N;
        stage_rows(lds, oQ, SE, q + (size_t)s0 * N * E, rows, E, vec, tid);
        stage_rows(lds, oK, SE, e + (size_t)s0 * N * E, rows, E, vec, tid);
        for (int k = tid; k < envs * NN; k += TPB) {
            const int r = k / N, j = k - r * N;
            lds[oDS + r * NP + j] = m[(size_t)s0 * NN + k];
            lds[oDM + r * NP + j] = d_m[(size_t)s0 * NN + k];
        }
        __syncthreads();
        for (int r = tid; r < rows; r += TPB) {
            const int mr = oDS + r * NP, dr = oDM + r * NP;
            float t = 0.0f;
            for (int j = 0; j < N; ++j) t = fmaf(lds[dr + j], lds[mr + j], t);
            for (int j = 0; j < N; ++j) lds[mr + j] = lds[mr + j] * (lds[dr + j] - t);
        }
        __syncthreads();
        const int nrg = (rows + RC - 1) / RC;
        for (int it = tid; it < nrg * E; it += TPB) {
            const int rg = it / E, o = it - rg * E, r0 = rg * RC, en = r0 / N;
            const int ra = min(r0, rows - 1), rb = min(r0 + 1, rows - 1), rc = min(r0 + 2, rows - 1), rd = min(r0 + 3, rows - 1);
            const int la = ra - en * N, lb = rb - en * N, lc = rc - en * N, ld = rd - en * N;
            float q0 = 0.f, q1 = 0.f, q2 = 0.f, q3 = 0.f, k0 = 0.f, k1 = 0.f, k2 = 0.f, k3 = 0.f;
            for (int j = 0; j < N; ++j) {
                const float ev = lds[oK + (en * N + j) * SE + o], qv = lds[oQ + (en * N + j) * SE + o];
                const int dj = oDS + (en * N + j) * NP;
                if (la < N) { q0 = fmaf(lds[oDS + ra * NP + j], ev, q0); k0 = fmaf(lds[dj + la], qv, k0); }   // dQ[i] += dS[i][j] E[j]
                if (lb < N) { q1 = fmaf(lds[oDS + rb * NP + j], ev, q1); k1 = fmaf(lds[dj + lb], qv, k1); }   // dE[i] += dS[j][i] Q[j]
                if (lc < N) { q2 = fmaf(lds[oDS + rc * NP + j], ev, q2); k2 = fmaf(lds[dj + lc], qv, k2); }
                if (ld < N) { q3 = fmaf(lds[oDS + rd * NP + j], ev, q3); k3 = fmaf(lds[dj + ld], qv, k3); }
            }
            const size_t at = ((size_t)s0 * N + r0) * E + o;
#define CM_GA_STORE(i, qa, ka)                                                  \
            if (r0 + i < rows && (r0 + i) / N == en) {                          \
                const size_t p = at + (size_t)i * E;                            \
                d_q[p] = qa;                                                    \
                float v = ka;                                                   \
                if (add0) v += add0[p];                                         \
                if (add1) v += add1[p];                                         \
                d_e[p] = v;                                                     \
            }
            CM_GA_STORE(0, q0, k0) CM_GA_STORE(1, q1, k1) CM_GA_STORE(2, q2, k2) CM_GA_STORE(3, q3, k3)
#undef CM_GA_STORE
        }
        __syncthreads();
    }
}

// < 0: bad arguments; 1: the planes of this (N, E) do not fit (nothing launched); 0: p is the plan
static int shape_rc(const std::string &fn, int N, int E, Plan &p) {
    if (N < 1 || E < 1 || E > MAX_E) return set_error(CM_ERR_ARG, fn + ": n_agents >= 1 and 1 <= embedding dim <= 128 required");
    if (N > MAX_N) return 1;
    p = plan(N, E);
    return fits(p) ? 0 : 1;
}
static int aligned16(std::initializer_list<const void *> ps) {
    uintptr_t u = 0;
    for (const void *q : ps) u |= (uintptr_t)q;
    return !(u & 15);
}
static int grid_of(int S, int EPB, int cap) { return (int)std::min<long>(((long)S + EPB - 1) / EPB, cap); }

template <bool DET>
static int masked_agg_backward_any(const char *fn, int32_t S, int32_t N, int32_t E, const float *attn, const float *dist_adj,
                                   const float *chan, int64_t ch_stride, const float *hw, const float *out, const float *out_minus,
                                   const float *d_out, float *d_attn, float *d_hw, float *d_bias, void *ws, size_t ws_bytes, void *stream) {
    if (!attn || !hw || !out || !d_out || !d_attn || !d_hw) return set_error(CM_ERR_ARG, std::string(fn) + ": null argument");
    Plan p;
    if (const int rc = shape_rc(fn, N, E, p)) return rc;
    if (DET)
        if (const int rc = slab_check(ws, ws_bytes, cm_masked_agg_backward_any_det_ws_bytes(S, N, E), fn)) return rc;
    if (S <= 0) return CM_OK;
    if (DET && !d_bias)   // the twin without a bias gradient has no cross-workgroup sum left: the default kernel
        return masked_agg_backward_any<false>(fn, S, N, E, attn, dist_adj, chan, ch_stride, hw, out, out_minus, d_out, d_attn, d_hw, nullptr,
                                              nullptr, 0, stream);
    const hipStream_t st = (hipStream_t)stream;
    float *const slab = static_cast<float *>(ws);
    const int vec = E % 4 == 0 && aligned16({ hw, out, out_minus, d_out });
    const int grid = grid_of(S, p.EPB, GRID_CAP_AGG_BWD);
    if (int rc = launch_lds<&agg_bwd_any_kernel<DET>>(dim3(grid), dim3(TPB), p.agg_bwd, st, S, N, E, p.EPB, vec, attn, dist_adj, chan,
                                                     (long)ch_stride, hw, out, out_minus, d_out, d_attn, d_hw, DET ? slab : d_bias)) return rc;
    if (!DET) return CM_OK;
    SlabSegs segs{};
    segs.s[0] = { d_bias, 0, E };
    segs.n_seg = 1;
    return slab_reduce(slab, grid, E, segs, st);
}

}  // namespace ga
}  // namespace cm

using namespace cm;

extern "C" int cm_masked_agg_forward_any(int32_t S, int32_t N, int32_t E, const float *attn, const float *dist_adj,
                                         const float *chan, int64_t ch_stride, const float *hw, const float *bias, float *out,
                                         void *stream) {
    if (!attn || !hw || !out) return set_error(CM_ERR_ARG, "cm_masked_agg_forward_any: null argument");
    ga::Plan p;
    if (const int rc = ga::shape_rc(__func__, N, E, p)) return rc;
    if (S <= 0) return CM_OK;
    const int vec = E % 4 == 0 && ga::aligned16({ hw });
    return launch_lds<&ga::agg_fwd_any_kernel>(dim3(ga::grid_of(S, p.EPB, ga::GRID_CAP)), dim3(ga::TPB), p.agg_fwd, stream, S, N, E, p.EPB, vec, attn,
                                               dist_adj, chan, (long)ch_stride, hw, bias, out);
}

extern "C" int cm_masked_agg_backward_any(int32_t S, int32_t N, int32_t E, const float *attn, const float *dist_adj,
                                          const float *chan, int64_t ch_stride, const float *hw, const float *out, const float *out_minus,
                                          const float *d_out, float *d_attn, float *d_hw, float *d_bias, void *stream) {
    return ga::masked_agg_backward_any<false>(__func__, S, N, E, attn, dist_adj, chan, ch_stride, hw, out, out_minus, d_out, d_attn, d_hw,
                                              d_bias, nullptr, 0, stream);
}

extern "C" size_t cm_masked_agg_backward_any_det_ws_bytes(int32_t S, int32_t N, int32_t E) {
    if (S <= 0 || N < 1 || E < 1) return 0;
    return (size_t)std::min<int32_t>(S, 2048) * E * sizeof(float);        // one E-float row per workgroup, grid <= min(S, 2048)
}

extern "C" int cm_masked_agg_backward_any_det(int32_t S, int32_t N, int32_t E, const float *attn, const float *dist_adj,
                                              const float *chan, int64_t ch_stride, const float *hw, const float *out,
                                              const float *out_minus, const float *d_out, float *d_attn, float *d_hw, float *d_bias,
                                              void *ws, size_t ws_bytes, void *stream) {
    return ga::masked_agg_backward_any<true>(__func__, S, N, E, attn, dist_adj, chan, ch_stride, hw, out, out_minus, d_out, d_attn, d_hw,
                                             d_bias, ws, ws_bytes, stream);
}

extern "C" int cm_attention_forward_any(int32_t S, int32_t N, int32_t E, const float *q, const float *e, float *m, void *stream) {
    if (!q || !e || !m) return set_error(CM_ERR_ARG, "cm_attention_forward_any: null argument");
    ga::Plan p;
    if (const int rc = ga::shape_rc(__func__, N, E, p)) return rc;
    if (S <= 0) return CM_OK;
    const int vec = E % 4 == 0 && ga::aligned16({ q, e });
    return launch_lds<&ga::attn_fwd_any_kernel>(dim3(ga::grid_of(S, p.EPB, ga::GRID_CAP)), dim3(ga::TPB), p.attn_fwd, stream, S, N, E, p.EPB, vec, q, e, m);
}

extern "C" int cm_attention_backward_any(int32_t S, int32_t N, int32_t E, const float *q, const float *e, const float *m,
                                         const float *d_m, const float *d_e_add0, const float *d_e_add1, float *d_q, float *d_e,
                                         void *stream) {
    if (!q || !e || !m || !d_m || !d_q || !d_e) return set_error(CM_ERR_ARG, "cm_attention_backward_any: null argument");
    if (d_e == d_e_add0 || d_e == d_e_add1) return set_error(CM_ERR_ARG, "cm_attention_backward_any: d_e must not alias its addends");
    ga::Plan p;
    if (const int rc = ga::shape_rc(__func__, N, E, p)) return rc;
    if (S <= 0) return CM_OK;
    const int vec = E % 4 == 0 && ga::aligned16({ q, e });
    return launch_lds<&ga::attn_bwd_any_kernel>(dim3(ga::grid_of(S, p.EPB, ga::GRID_CAP)), dim3(ga::TPB), p.attn_bwd, stream, S, N, E, p.EPB, vec, q, e, m,
                                                d_m, d_e_add0, d_e_add1, d_q, d_e);
}
