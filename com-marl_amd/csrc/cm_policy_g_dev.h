// cm_policy_g_dev.h - device side of the run-time-sized Comm-DP forwards: the policy (cm_policy_g.hip) and the critic
// (cm_critic_g.hip) are the two instantiations of one kernel, which share trunk() and head() below; the policy-set kernel
// (cm_policy_gm.hip: every workgroup runs the net its table record names) calls the same two and includes the same sampler
// tail (cm_policy_g_tail.h).
//
// One 256-thread workgroup owns EPB whole envs (rows = EPB * N agent rows, padded to R16 = a multiple of 16) and carries
// them from the observation load to the sampled action.  LDS map (floats; every plane base and stride a multiple of 4):
//   E  [R16][SE]   encoder output                      H  [R16][SE]   hop output, then the head's input x
//   P0 [R16][SW]   ping   } as wide as the widest      P1 [R16][SW]   pong  (the staged observation starts here)
//   M  [rows][NP]  attention softmax                   A  [rows][NP]  masked, row-renormalised attention of the hop
// Every dense layer is v_mfma_f32_16x16x4_f32 (exact f32) with the lane maps of cm_mlp_body.h: lane group g = lane >> 4
// supplies k = 16*kq + 4*g + j at MFMA (kq, j), so a lane's four A words are one 16-byte LDS read; B comes straight from
// the [in,out] weights with the ragged edge zeroed by predicate.  The whole LDS tile is zeroed first, so what a padded
// k-slot or row reads is finite and meets a zero weight.  LDS is addressed by integer offsets into one array; there is
// no dynamically indexed local array (layer loops are unrolled over the argument block's fixed slots).
#pragma once
#include "cm_internal.h"
#include "cm_rng.h"

namespace cm {
namespace pg {

constexpr int TPB = 256, MAX_ENC = 3, MAX_HEAD = 4, MAX_W = 128, MAX_ACT = 8;
constexpr size_t LDS_LIMIT = 160 * 1024;
typedef float v4f __attribute__((ext_vector_type(4)));

struct Args {
    int S, N, d, L, A, emb, no_residual;
    int n_enc, enc_h[MAX_ENC];
    int n_head, head_h[MAX_HEAD];
    int EPB, R16, SE, SW, NP;                     // the launch plan (plan())
    const float *enc_w[MAX_ENC], *enc_b[MAX_ENC], *enc_wo, *enc_bo;
    const float *attn_wt, *gcn_w, *gcn_b;
    const float *head_w[MAX_HEAD], *head_b[MAX_HEAD], *head_wo, *head_bo;
    const float *obs, *avail, *adj, *chan;
    uint32_t key0, key1, policy_step;
    const uint32_t *step_base;
    int env_id_offset, greedy;
    int32_t *actions;
    float *probs, *attn;
    float *values;                                // the critic instantiation: [S]
};

// The one place the LDS need is computed: the "fits" test and the launch both read it.
struct Plan { int EPB, R16, SE, SW, NP; size_t lds_bytes; };

__host__ inline int pad16(int x) { return (x + 15) & ~15; }

__host__ inline Plan plan(int N, int d, int emb, int widest) {
    Plan p;
    // max(1, 48 / N) whole envs for EVERY team size: 25-48 rows for teams up to 24, one env per workgroup above that.  (cm_policy.hip's
    // pick_epb gives 1 when N is no multiple of its 4-row register tile; MFMA tiles may straddle envs here, so no such rule.)
    p.EPB = 48 / N > 0 ? 48 / N : 1;
    p.R16 = pad16(p.EPB * N);
    p.SE = pad16(emb) + 4;                        // +4 keeps float4 alignment and staggers the banks
    p.SW = pad16(widest > d ? widest : d) + 4;
    p.NP = N | 1;
    const size_t mat = ((size_t)p.EPB * N * p.NP + 3) & ~(size_t)3;
    p.lds_bytes = ((size_t)p.R16 * (2 * p.SE + 2 * p.SW) + 2 * mat) * sizeof(float);
    return p;
}

// cm_net_weights -> Args + Plan, for both entry points.  0: ready to launch; 1: outside the bounds the kernel is written for
// or more than 160 KB of LDS ("not for this shape", nothing launched); < 0: a null weight pointer (cm_last_error names `fn`).
__host__ inline bool width_ok(int w) { return w >= 1 && w <= MAX_W; }
__host__ inline int fill(const char *fn, const cm_net_weights *w, int n_samples, Args &a, Plan &p) {
    if (w->n_enc < 1 || w->n_enc > MAX_ENC || w->n_head < 1 || w->n_head > MAX_HEAD) return 1;
    if (!width_ok(w->emb) || !width_ok(w->d) || w->n_act < 1 || w->n_act > MAX_ACT || w->n_agents < 1 || w->n_hops < 0) return 1;
    int widest = w->emb;
    for (int i = 0; i < w->n_enc; ++i) { if (!width_ok(w->enc_hidden[i])) return 1; widest = widest > w->enc_hidden[i] ? widest : w->enc_hidden[i]; }
    for (int i = 0; i < w->n_head; ++i) { if (!width_ok(w->head_hidden[i])) return 1; widest = widest > w->head_hidden[i] ? widest : w->head_hidden[i]; }
    p = plan(w->n_agents, w->d, w->emb, widest);
    if (p.lds_bytes > LDS_LIMIT) return 1;
    for (int i = 0; i <= w->n_enc; ++i)
        if (!w->enc_wt[i]) return set_error(CM_ERR_ARG, std::string(fn) + ": null encoder weight");
    for (int i = 0; i <= w->n_head; ++i)
        if (!w->head_wt[i]) return set_error(CM_ERR_ARG, std::string(fn) + ": null head weight");
    if (w->n_hops > 0 && !w->gcn_w) return set_error(CM_ERR_ARG, std::string(fn) + ": null gcn_w");
    a.S = n_samples; a.N = w->n_agents; a.d = w->d; a.L = w->n_hops; a.A = w->n_act; a.emb = w->emb;
    a.no_residual = w->no_residual;
    a.n_enc = w->n_enc; a.n_head = w->n_head;
    for (int i = 0; i < w->n_enc; ++i) { a.enc_h[i] = w->enc_hidden[i]; a.enc_w[i] = w->enc_wt[i]; a.enc_b[i] = w->enc_b[i]; }
    a.enc_wo = w->enc_wt[w->n_enc]; a.enc_bo = w->enc_b[w->n_enc];
    for (int i = 0; i < w->n_head; ++i) { a.head_h[i] = w->head_hidden[i]; a.head_w[i] = w->head_wt[i]; a.head_b[i] = w->head_b[i]; }
    a.head_wo = w->head_wt[w->n_head]; a.head_bo = w->head_b[w->n_head];
    a.attn_wt = w->attn_wt; a.gcn_w = w->gcn_w; a.gcn_b = w->gcn_b;
    a.EPB = p.EPB; a.R16 = p.R16; a.SE = p.SE; a.SW = p.SW; a.NP = p.NP;
    return 0;
}

__device__ __forceinline__ float fast_tanh(float x) {      // same form as cm_mlp.hip (abs err <= 2e-7)
    const float t = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(t + 1.0f);
}

// out[r][o] = act(sum_k in[r][k] Wt[k][o] + b[o]) for every row of the R16-row tile and every column of the 16-padded
// width (padding columns come out as act(0) = 0).  Work items = (column tile, pair of row tiles), dealt to the 4 waves.
template <bool TANH>
__device__ __forceinline__ void dense(float *lds, int in, int in_s, int K, const float *__restrict__ Wt,
                                      const float *__restrict__ bias, int OUT, int out, int out_s, int R16, int tid) {
    const int wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int nct = (OUT + 15) >> 4, k16 = (K + 15) >> 4, rtn = R16 >> 4, rp = (rtn + 1) >> 1;
    for (int it = wave; it < nct * rp; it += 4) {
        const int ct = it % nct, rt0 = (it / nct) * 2;
        const bool two = rt0 + 1 < rtn;                      // wave-uniform
        const int col = ct * 16 + c;
        const int a0o = in + (rt0 * 16 + c) * in_s + 4 * g;
        const int a1o = two ? a0o + 16 * in_s : a0o;
        v4f acc0 = (v4f){ 0.f, 0.f, 0.f, 0.f }, acc1 = (v4f){ 0.f, 0.f, 0.f, 0.f };
        for (int kq = 0; kq < k16; ++kq) {
            const float4 x0 = *reinterpret_cast<const float4 *>(&lds[a0o + 16 * kq]);
            const float4 x1 = *reinterpret_cast<const float4 *>(&lds[a1o + 16 * kq]);
            const float xa[4] = { x0.x, x0.y, x0.z, x0.w }, xb[4] = { x1.x, x1.y, x1.z, x1.w };
            float bw[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = 16 * kq + 4 * g + j;
                bw[j] = (k < K && col < OUT) ? Wt[(size_t)k * OUT + col] : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[j], bw[j], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xb[j], bw[j], acc1, 0, 0, 0);
            }
        }
        const float bv = (bias && col < OUT) ? bias[col] : 0.0f;
        const int o0 = out + (rt0 * 16 + 4 * g) * out_s + col;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float v = acc0[r] + bv;
            lds[o0 + r * out_s] = TANH ? fast_tanh(v) : v;
        }
        if (two) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = acc1[r] + bv;
                lds[o0 + (16 + r) * out_s] = TANH ? fast_tanh(v) : v;
            }
        }
    }
}

// What a workgroup owns and where its planes start (float offsets into the one LDS array).
struct Tile { int s0, envs, rows, oE, oH, oP0, oP1; };

// The trunk both kernels share: zeroing, observation staging, encoder, attention + softmax, L hops, residual.  Leaves x in H.
// `blk`: the workgroup's block index in the batch `a` describes (blockIdx.x, or the block inside a set member's group).
__device__ __forceinline__ Tile trunk(const Args &a, float *lds, int tid, unsigned blk) {
    const int N = a.N, d = a.d, L = a.L, NN = N * N, NP = a.NP, EM = a.emb;
    const int SE = a.SE, SW = a.SW, R16 = a.R16;
    const int s0 = blk * a.EPB;
    const int envs = min(a.EPB, a.S - s0);
    const int rows = envs * N, rows_max = a.EPB * N;
    const int mat = (rows_max * NP + 3) & ~3;
    const int oE = 0, oH = oE + R16 * SE, oP0 = oH + R16 * SE, oP1 = oP0 + R16 * SW, oM = oP1 + R16 * SW, oA = oM + mat;
    const int total = oA + mat;
    // ---- zero the tile (16-byte stores), then stage the observations: coalesced HBM read of rows*d floats ----
    for (int k = tid * 4; k < total; k += TPB * 4) *reinterpret_cast<float4 *>(&lds[k]) = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    {
        const float *src = a.obs + (size_t)s0 * N * d;
        const int n = rows * d;
        for (int k = tid; k < n; k += TPB) { const int r = k / d, f = k - r * d; lds[oP1 + r * SW + f] = src[k]; }
    }
    __syncthreads();

    // ---- encoder: n_enc tanh hidden layers, tanh output layer into E ----
    int cur = oP1, nxt = oP0, K = d;
#pragma unroll
    for (int i = 0; i < MAX_ENC; ++i) {
        if (i < a.n_enc) {
            dense<true>(lds, cur, SW, K, a.enc_w[i], a.enc_b[i], a.enc_h[i], nxt, SW, R16, tid);
            __syncthreads();
            const int t = cur; cur = nxt; nxt = t;
            K = a.enc_h[i];
        }
    }
    dense<true>(lds, cur, SW, K, a.enc_wo, a.enc_bo, EM, oE, SE, R16, tid);
    __syncthreads();

    // ---- attention: Q = E.Wa ('general') or E ('dot'); scores = Q.E^T; softmax over j ----
    int oQ = oE, sQ = SE;
    if (a.attn_wt) {
        dense<false>(lds, oE, SE, EM, a.attn_wt, nullptr, EM, oP0, SW, R16, tid);
        __syncthreads();
        oQ = oP0; sQ = SW;
    }
    for (int k = tid; k < envs * NN; k += TPB) {
        const int e = k / NN, ij = k - e * NN, i = ij / N, j = ij - i * N;
        const int q = oQ + (e * N + i) * sQ, kk = oE + (e * N + j) * SE;
        float acc = 0.0f;
        for (int x = 0; x < EM; ++x) acc = fmaf(lds[q + x], lds[kk + x], acc);
        lds[oM + (e * N + i) * NP + j] = acc;
    }
    __syncthreads();
    for (int r = tid; r < rows; r += TPB) {
        const int m = oM + r * NP;
        float mx = -INFINITY, sum = 0.0f;
        for (int j = 0; j < N; ++j) mx = fmaxf(mx, lds[m + j]);
        for (int j = 0; j < N; ++j) { const float ex = expf(lds[m + j] - mx); lds[m + j] = ex; sum += ex; }
        for (int j = 0; j < N; ++j) lds[m + j] = lds[m + j] / sum;
    }
    __syncthreads();
    if (a.attn) {                                       // attention_weights output [S,N,N]
        float *dst = a.attn + (size_t)s0 * NN;
        for (int k = tid; k < envs * NN; k += TPB) { const int r = k / N, j = k - r * N; dst[k] = lds[oM + r * NP + j]; }
    }

    // ---- L hops: A = M * adj * ch_l, row-renormalised; H' = tanh(A.(H.Wg_l) + b_l) ----
    const int EP = (EM + 15) & ~15;
    for (int l = 0; l < L; ++l) {
        dense<false>(lds, l == 0 ? oE : oH, SE, EM, a.gcn_w + (size_t)l * EM * EM, nullptr, EM, oP0, SW, R16, tid);
        for (int k = tid; k < envs * NN; k += TPB) {
            const int e = k / NN, ij = k - e * NN, r = k / N, j = k - r * N;
            float v = lds[oM + r * NP + j];
            if (a.adj) v *= a.adj[(size_t)(s0 + e) * NN + ij];
            if (a.chan) v *= a.chan[((size_t)(s0 + e) * L + l) * NN + ij];
            lds[oA + r * NP + j] = v;
        }
        __syncthreads();
        for (int r = tid; r < rows; r += TPB) {
            const int ar = oA + r * NP;
            float sum = 0.0f;
            for (int j = 0; j < N; ++j) sum += lds[ar + j];
            const float den = sum + 1e-12f;
            for (int j = 0; j < N; ++j) lds[ar + j] = lds[ar + j] / den;
        }
        __syncthreads();
        for (int k = tid; k < rows * EP; k += TPB) {
            const int r = k / EP, o = k - r * EP, e = r / N;
            const int ar = oA + r * NP, hw = oP0 + e * N * SW + o;
            float acc = 0.0f;
            for (int j = 0; j < N; ++j) acc = fmaf(lds[ar + j], lds[hw + j * SW], acc);
            const float bv = (a.gcn_b && o < EM) ? a.gcn_b[(size_t)l * EM + o] : 0.0f;
            lds[oH + r * SE + o] = o < EM ? fast_tanh(acc + bv) : 0.0f;
        }
        __syncthreads();
    }
    // ---- x = H_L (E when there are no hops) + E unless no_residual (comm_categorical_mlp_policy.py:74-77) ----
    for (int k = tid; k < rows * EM; k += TPB) {
        const int r = k / EM, o = k - r * EM;
        const float ev = lds[oE + r * SE + o];
        lds[oH + r * SE + o] = (L > 0 ? lds[oH + r * SE + o] : ev) + (a.no_residual ? 0.0f : ev);
    }
    __syncthreads();

    return Tile{ s0, envs, rows, oE, oH, oP0, oP1 };
}

// The head both kernels share: n_head tanh hidden layers over x (in H), then the linear output layer of a.A columns.
// Returns the plane (stride SW) that holds the outputs.
__device__ __forceinline__ int head(const Args &a, float *lds, const Tile &t, int tid) {
    const int SE = a.SE, SW = a.SW, R16 = a.R16, oP0 = t.oP0, oP1 = t.oP1;
    int cur = t.oH, nxt = oP0, K = a.emb;
    int cs = SE;
#pragma unroll
    for (int i = 0; i < MAX_HEAD; ++i) {
        if (i < a.n_head) {
            dense<true>(lds, cur, cs, K, a.head_w[i], a.head_b[i], a.head_h[i], nxt, SW, R16, tid);
            __syncthreads();
            cur = nxt; nxt = (nxt == oP0) ? oP1 : oP0; cs = SW;
            K = a.head_h[i];
        }
    }
    dense<false>(lds, cur, cs, K, a.head_wo, a.head_bo, a.A, nxt, SW, R16, tid);
    __syncthreads();
    return nxt;
}

// CRITIC false: the policy - per-agent softmax x avail, renormalise, sample.  CRITIC true (cm_critic_g.hip): the head is the
// critic's decoder with ONE output column, and one thread per env sums its agents' values in agent order.
template <bool CRITIC>
__global__ __launch_bounds__(TPB) void fwd_any_kernel(Args a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, N = a.N, SW = a.SW;
    const Tile t = trunk(a, lds, tid, blockIdx.x);
    const int s0 = t.s0, rows = t.rows;
    const int nxt = head(a, lds, t, tid);
    if constexpr (CRITIC) {
        for (int e = tid; e < t.envs; e += TPB) {
            float v = 0.0f;
            for (int i = 0; i < N; ++i) v += lds[nxt + (e * N + i) * SW];
            a.values[s0 + e] = v;
        }
        return;
    }
#include "cm_policy_g_tail.h"
}

}  // namespace pg
}  // namespace cm
