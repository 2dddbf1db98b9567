// cm_ppo.hip - the loss side of the PPO update (gfx950), each kernel family above the launchers that size it:
//   * cm_discount_returns : garage/misc/tensor_utils.py:7-23 (f64 recurrence)
//   * cm_gae              : garage/torch/algos/_utils.py:56-113 + the per-path normalisation of
//                           centralized_ma_ppo.py:422-426
//   * cm_ppo_surrogate, cm_ppo_surrogate_det, cm_ppo_surrogate_det_ws_bytes : the clipped surrogate + entropy bonus and
//                           its gradient wrt the logits (centralized_ma_ppo.py:390-438, :540-589)
//   * cm_entropy_gae      : entropy_method "max" - entropy -> r + c H -> GAE (:415-418, :499-538)
//   * cm_gauss_nll_forward, cm_gauss_nll_forward_det, cm_gauss_nll_forward_det_ws_bytes, cm_gauss_nll_backward : the
//                           critic's Gaussian negative log-likelihood (comm_base_critic.py:59-89)
// The graph ops of the training path are in cm_graph_ops.hip, the dense layers' weight gradient in cm_linear_wgrad.hip,
// the optimiser in cm_optim.hip, the update's per-step statistics in cm_ppo_stats.hip.
#include <algorithm>

#include "cm_internal.h"

namespace cm {

constexpr int PPO_MAX_A = 8;

__global__ void returns_kernel(int P, int T, const double *__restrict__ rewards, const int32_t *__restrict__ lens,
                               double gamma, float *__restrict__ returns) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int n = lens ? lens[p] : T;
    double y = 0.0;
    for (int t = T - 1; t >= 0; --t) {
        if (t < n) { y = rewards[(size_t)p * T + t] + gamma * y; returns[(size_t)p * T + t] = (float)y; }
        else returns[(size_t)p * T + t] = 0.0f;
    }
}

// delta_t = r_t + g V_{t+1} - V_t over the PADDED length (V past the end = 0), A_t = delta_t + g*lam*A_{t+1};
// optional per-path normalisation over the first lens[p] steps, biased variance, applied to the whole row.
__global__ void gae_kernel(int P, int T, const float *__restrict__ rewards, const float *__restrict__ baselines,
                           const int32_t *__restrict__ lens, float gamma, float lam, int normalize, float eps,
                           float *__restrict__ adv) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const float *r = rewards + (size_t)p * T, *v = baselines + (size_t)p * T;
    float *a = adv + (size_t)p * T;
    const double gl = (double)(gamma * lam);
    double acc = 0.0, vnext = 0.0;
    for (int t = T - 1; t >= 0; --t) {
        const float delta = (r[t] + gamma * (float)vnext) - v[t];       // f32 like the reference's tensor expression
        acc = (double)delta + gl * acc;
        a[t] = (float)acc;
        vnext = v[t];
    }
    if (!normalize) return;
    const int n = lens ? lens[p] : T;
    if (n <= 0) return;
    double s = 0.0;
    for (int t = 0; t < n; ++t) s += a[t];
    const double mean = s / n;
    double q = 0.0;
    for (int t = 0; t < n; ++t) { const double dlt = a[t] - mean; q += dlt * dlt; }
    const float m32 = (float)mean, inv = 1.0f / sqrtf((float)(q / n) + eps);
    for (int t = 0; t < T; ++t) a[t] = (a[t] - m32) * inv;
}

}  // namespace cm

using namespace cm;

extern "C" int cm_discount_returns(int32_t P, int32_t T, const double *rewards, const int32_t *lens, double gamma,
                                   float *returns, void *stream) {
    if (!rewards || !returns) return set_error(CM_ERR_ARG, "cm_discount_returns: null argument");
    if (P <= 0 || T <= 0) return CM_OK;
    hipLaunchKernelGGL(returns_kernel, dim3((P + 63) / 64), dim3(64), 0, (hipStream_t)stream, P, T, rewards, lens, gamma, returns);
    CM_HIP(hipGetLastError());
    return CM_OK;
}

extern "C" int cm_gae(int32_t P, int32_t T, const float *rewards, const float *baselines, const int32_t *lens,
                      float gamma, float lam, int32_t normalize, float eps, float *adv, void *stream) {
    if (!rewards || !baselines || !adv) return set_error(CM_ERR_ARG, "cm_gae: null argument");
    if (P <= 0 || T <= 0) return CM_OK;
    hipLaunchKernelGGL(gae_kernel, dim3((P + 63) / 64), dim3(64), 0, (hipStream_t)stream, P, T, rewards, baselines, lens, gamma, lam, normalize, eps, adv);
    CM_HIP(hipGetLastError());
    return CM_OK;
}

// sum of n f64 partials in a fixed order: thread t adds slab[t], slab[t + 256], ... in turn, then a fixed tree over the threads.
// One 256-thread workgroup.  (What ends the slab twins' launches below: slab_total_kernel, gauss_nll_finish_kernel.)
__device__ double fixed_order_sum(const double *__restrict__ slab, int n) {
    __shared__ double red[256];
    double s = 0.0;
    for (int b = threadIdx.x; b < n; b += 256) s += slab[b];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) { if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k]; __syncthreads(); }
    return red[0];
}

__global__ __launch_bounds__(256) void slab_total_kernel(const double *__restrict__ slab, int n, double *__restrict__ total) {
    const double t = fixed_order_sum(slab, n);
    if (threadIdx.x == 0) *total = t;
}

namespace cm {

// ---------------------------------------------------------------------------------------------------------------
// PPO clipped-surrogate loss + entropy bonus and its gradient wrt the logits, one launch (reference:
// centralized_ma_ppo.py:390-438 _compute_loss, :540-589 _compute_objective; the Categorical(probs=...) arithmetic of
// comm_categorical_mlp_policy.py:121-137: probs = softmax renormalised twice, logits = log(clamp(probs, eps, 1 - eps))).
// One thread per env step: N agents x A <= 8 logits in registers; the chain rule is walked link by link (clamp ->
// normalise -> normalise -> softmax) so that the result is the autograd one, term for term.
//   total = - sum_{valid s} [ min(r adv, clamp(r, 1 - c, 1 + c) adv) + ent_coeff * mean_i H_i ],  r = exp(new_ll - old_ll)
// ---------------------------------------------------------------------------------------------------------------
template <bool DET = false>   // slab mode: `total` is a slab of one f64 per workgroup
__global__ __launch_bounds__(256) void ppo_surrogate_kernel(int P, int T, int N, int A, const float *__restrict__ logits,
                                                            const int32_t *__restrict__ actions, const float *__restrict__ old_ll,
                                                            const float *__restrict__ adv, const int32_t *__restrict__ lens,
                                                            float clip, float ent_coeff, int add_entropy,
                                                            double *__restrict__ total, long long *__restrict__ count,
                                                            float *__restrict__ dlogits) {
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    const long S = (long)P * T;
    double part = 0.0;
    int valid_here = 0;
    if (s < S) {
        const int pth = (int)(s / T), t = (int)(s - (long)pth * T);
        const bool valid = t < lens[pth];
        valid_here = valid ? 1 : 0;
        const float EPS = 1.1920928955078125e-07f;            // torch.finfo(float32).eps: probs_to_logits clamps to [eps, 1 - eps]
        const float *z0 = logits + s * N * A;
        const int32_t *a0 = actions + s * N;
        const float ol = old_ll[s], ad = adv[s];
        // pass 1: new log-likelihood and entropy
        float new_ll = 0.0f, ent = 0.0f;
        for (int i = 0; i < N; ++i) {
            float z[PPO_MAX_A], p[PPO_MAX_A];
            float mx = -INFINITY;
#pragma unroll
            for (int b = 0; b < PPO_MAX_A; ++b) if (b < A) { z[b] = z0[i * A + b]; mx = fmaxf(mx, z[b]); }
            float s0 = 0.0f;
#pragma unroll
            for (int b = 0; b < PPO_MAX_A; ++b) if (b < A) { p[b] = expf(z[b] - mx); s0 += p[b]; }
            float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
            for (int b = 0; b < PPO_MAX_A; ++b) if (b < A) { p[b] = p[b] / s0; s1 += p[b]; }
#pragma unroll
            for (int b = 0; b < PPO_MAX_A; ++b) if (b < A) { p[b] = p[b] / s1; s2 += p[b]; }
            const int ai = a0[i];
            float h = 0.0f;
#pragma unroll
            for (int b = 0; b < PPO_MAX_A; ++b) if (b < A) {
                const float p3 = p[b] / s2;
                const float lg = logf(fminf(fmaxf(p3, EPS), 1.0f - EPS));
                h -= lg * p3;
                if (b == ai) new_ll += lg;
            }
            ent += h;
        }
        ent /= (float)N;
        const float r = expf(new_ll - ol);
        const float rc = fminf(fmaxf(r, 1.0f - clip), 1.0f + clip);
        const float sur = r * ad, clp = rc * ad;
        float obj = fminf(sur, clp);
        // CM_ENT_* bits (include/commarl.h): softplus after the mean over agents (centralized_ma_ppo.py:535-536), torch's
        // threshold 20; its derivative z / (z + 1) as torch's softplus_backward writes it
        const bool ent_on = add_entropy & 1, ent_sp = add_entropy & 2, ent_grad = !(add_entropy & 4);
        float ent_term = ent, ent_slope = 1.0f;
        if (ent_sp && ent <= 20.0f) { const float z = expf(ent); ent_term = log1pf(z); ent_slope = z / (z + 1.0f); }
        if (ent_on) obj += ent_coeff * ent_term;
        if (valid) part = -(double)obj;
        if (dlogits) {
            // d total / d new_ll: torch.min splits ties evenly; clamp passes the gradient inside [1 - c, 1 + c] (ends included)
            const float wa = sur < clp ? 1.0f : (sur == clp ? 0.5f : 0.0f), wb = sur > clp ? 1.0f : (sur == clp ? 0.5f : 0.0f);
            const float cg = (r >= 1.0f - clip && r <= 1.0f + clip) ? 1.0f : 0.0f;
            const float g_ll = valid ? -(ad * wa + ad * cg * wb) * r : 0.0f;
            const float g_h = (valid && ent_on && ent_grad) ? -ent_coeff * ent_slope / (float)N : 0.0f;     // d total / d H_i
            float *d0 = dlogits + s * N * A;
            for (int i = 0; i < N; ++i) {
                float z[PPO_MAX_A], p[PPO_MAX_A], p1[PPO_MAX_A], p2[PPO_MAX_A], p3[PPO_MAX_A], d[PPO_MAX_A];
                float mx = -INFINITY;
#pragma unroll
                for (int b = 0; b < PPO_MAX_A; ++b) if (b < A) { z[b] = z0[i * A + b]; mx = fmaxf(mx, z[b]); }
                float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
                for (int b = 0; b < PPO_MAX_A; ++b) if (b < A) { p[b] = expf(z[b] - mx); s0 += p[b]; }
#pragma unroll
                for (int b = 0; b < PPO_MAX_A; ++b) if (b < A) { p1[b] = p[b] / s0; s1 += p1[b]; }       // softmax
#pragma unroll
                for (int b = 0; b < PPO_MAX_A; ++b) if (b < A) { p2[b] = p1[b] / s1; s2 += p2[b]; }      // _probs: probs / probs.sum
#pragma unroll
                for (int b = 0; b < PPO_MAX_A; ++b) if (b < A) p3[b] = p2[b] / s2;                        // Categorical: again
                const int ai = a0[i];
                // d wrt p3: through logits = log(clamp(p3)) (log_prob gather + entropy's logits factor) and entropy's probs factor
                float dot = 0.0f;
#pragma unroll
                for (int b = 0; b < PPO_MAX_A; ++b) if (b < A) {
                    const float pc = fminf(fmaxf(p3[b], EPS), 1.0f - EPS);
                    const float lg = logf(pc);
                    const bool in = p3[b] >= EPS && p3[b] <= 1.0f - EPS;
                    const float g_lg = (b == ai ? g_ll : 0.0f) - g_h * p3[b];       // H = - sum lg * p3
                    d[b] = (in ? g_lg / pc : 0.0f) - g_h * lg;
                    dot += d[b] * p3[b];
                }
#pragma unroll
                for (int b = 0; b < PPO_MAX_A; ++b) if (b < A) d[b] = (d[b] - dot) / s2;                   // p3 = p2 / s2
                dot = 0.0f;
#pragma unroll
                for (int b = 0; b < PPO_MAX_A; ++b) if (b < A) dot += d[b] * p2[b];
#pragma unroll
                for (int b = 0; b < PPO_MAX_A; ++b) if (b < A) d[b] = (d[b] - dot) / s1;                   // p2 = p1 / s1
                dot = 0.0f;
#pragma unroll
                for (int b = 0; b < PPO_MAX_A; ++b) if (b < A) dot += d[b] * p1[b];
#pragma unroll
                for (int b = 0; b < PPO_MAX_A; ++b) if (b < A) d0[i * A + b] = p1[b] * (d[b] - dot);       // softmax
            }
        }
    }
    // block sums: f64 total, valid count
    __shared__ double sh_t[4];
    __shared__ int sh_c[4];
    for (int o = 32; o > 0; o >>= 1) { part += __shfl_down(part, o); valid_here += __shfl_down(valid_here, o); }
    if ((threadIdx.x & 63) == 0) { sh_t[threadIdx.x >> 6] = part; sh_c[threadIdx.x >> 6] = valid_here; }
    __syncthreads();
    if (threadIdx.x == 0) {
        if constexpr (DET) total[blockIdx.x] = sh_t[0] + sh_t[1] + sh_t[2] + sh_t[3];
        else atomicAdd(total, sh_t[0] + sh_t[1] + sh_t[2] + sh_t[3]);
        atomicAdd((unsigned long long *)count, (unsigned long long)(sh_c[0] + sh_c[1] + sh_c[2] + sh_c[3]));
    }
}

}  // namespace cm

extern "C" size_t cm_ppo_surrogate_det_ws_bytes(int32_t P, int32_t T) {
    if (P <= 0 || T <= 0) return 0;
    return (size_t)(((long)P * T + 255) / 256) * sizeof(double);
}

// cm_ppo_surrogate and its slab twin (DET: one f64 block sum per workgroup, summed by slab_total_kernel in a fixed order)
template <bool DET>
static int ppo_surrogate(const char *fn, int32_t P, int32_t T, int32_t N, int32_t A, const float *logits, const int32_t *actions,
                         const float *old_ll, const float *adv, const int32_t *lens, float clip, float ent_coeff, int32_t add_entropy,
                         double *total, int64_t *count, float *dlogits, void *ws, size_t ws_bytes, void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    const bool empty = P <= 0 || T <= 0, no_input = !logits || !actions || !old_ll || !adv || !lens;
    if (!total || !count) return set_error(CM_ERR_ARG, std::string(fn) + ": null argument");
    if (A < 1 || A > PPO_MAX_A || N < 1) return set_error(CM_ERR_ARG, std::string(fn) + ": 1 <= n_actions <= 8 and n_agents >= 1 required");
    if (DET) {   // the twin checks its pointers and the slab before clearing total / count, the default clears them first
        if (!empty && no_input) return set_error(CM_ERR_ARG, std::string(fn) + ": null argument");
        if (const int rc = slab_check(ws, ws_bytes, cm_ppo_surrogate_det_ws_bytes(P, T), fn)) return rc;
    }
    CM_HIP(hipMemsetAsync(total, 0, sizeof(double), st));      // an empty minibatch still reports (0, 0)
    CM_HIP(hipMemsetAsync(count, 0, sizeof(int64_t), st));     // (an integer sum: the default atomics are exact)
    if (empty) return CM_OK;
    if (no_input) return set_error(CM_ERR_ARG, std::string(fn) + ": null argument");
    const long S = (long)P * T;
    const int blocks = (int)((S + 255) / 256);
    double *const slab = static_cast<double *>(ws);
    hipLaunchKernelGGL(ppo_surrogate_kernel<DET>, dim3((unsigned)blocks), dim3(256), 0, st, P, T, N, A, logits, actions, old_ll, adv, lens,
                       clip, ent_coeff, add_entropy, DET ? slab : total, (long long *)count, dlogits);
    CM_HIP(hipGetLastError());
    if (!DET) return CM_OK;
    hipLaunchKernelGGL(slab_total_kernel, dim3(1), dim3(256), 0, st, slab, blocks, total);
    CM_HIP(hipGetLastError());
    return CM_OK;
}

extern "C" int cm_ppo_surrogate(int32_t P, int32_t T, int32_t N, int32_t A, const float *logits, const int32_t *actions,
                                const float *old_ll, const float *adv, const int32_t *lens, float clip, float ent_coeff,
                                int32_t add_entropy, double *total, int64_t *count, float *dlogits, void *stream) {
    return ppo_surrogate<false>(__func__, P, T, N, A, logits, actions, old_ll, adv, lens, clip, ent_coeff, add_entropy, total, count, dlogits,
                                nullptr, 0, stream);
}

extern "C" int cm_ppo_surrogate_det(int32_t P, int32_t T, int32_t N, int32_t A, const float *logits, const int32_t *actions,
                                    const float *old_ll, const float *adv, const int32_t *lens, float clip, float ent_coeff,
                                    int32_t add_entropy, double *total, int64_t *count, float *dlogits, void *ws, size_t ws_bytes,
                                    void *stream) {
    return ppo_surrogate<true>(__func__, P, T, N, A, logits, actions, old_ll, adv, lens, clip, ent_coeff, add_entropy, total, count, dlogits,
                               ws, ws_bytes, stream);
}

namespace cm {

// ---------------------------------------------------------------------------------------------------------------
// entropy_method == "max" (centralized_ma_ppo.py:415-418, entropy :499-538): the advantages depend on the current policy's
// entropy, so every loss evaluation runs  H -> r + c H -> GAE  on its own batch.  One 256-thread workgroup per path: the
// threads over t compute the per-step entropy (N x A exp / log each - the parallel part) into LDS next to the path's
// baselines, then one thread runs gae_kernel's recurrence over the padded length out of LDS (T f64 FMAs).
// H[t] = mean_i H_i with ppo_surrogate_kernel's Categorical arithmetic (softmax normalised twice, log(clamp(p, eps, 1-eps))),
// softplus after the mean when asked (:535-536).
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void entropy_gae_kernel(int T, int N, int A, const float *__restrict__ logits,
                                                          const float *rewards, const float *__restrict__ baselines, float gamma,
                                                          float lam, float ent_coeff, int softplus, float *rewards_out,
                                                          float *__restrict__ entropy_out, float *__restrict__ adv) {
    extern __shared__ float ent_lds[];                       // r' [T], V [T]
    float *rs = ent_lds, *vs = ent_lds + T;
    const int p = blockIdx.x;
    const size_t row = (size_t)p * T;
    const float EPS = 1.1920928955078125e-07f;
    for (int t = threadIdx.x; t < T; t += blockDim.x) {
        const float *z0 = logits + (row + t) * N * A;
        float ent = 0.0f;
        for (int i = 0; i < N; ++i) {
            float z[PPO_MAX_A], q[PPO_MAX_A];
            float mx = -INFINITY;
#pragma unroll
            for (int b = 0; b < PPO_MAX_A; ++b) if (b < A) { z[b] = z0[i * A + b]; mx = fmaxf(mx, z[b]); }
            float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
            for (int b = 0; b < PPO_MAX_A; ++b) if (b < A) { q[b] = expf(z[b] - mx); s0 += q[b]; }
#pragma unroll
            for (int b = 0; b < PPO_MAX_A; ++b) if (b < A) { q[b] = q[b] / s0; s1 += q[b]; }
#pragma unroll
            for (int b = 0; b < PPO_MAX_A; ++b) if (b < A) { q[b] = q[b] / s1; s2 += q[b]; }
            float h = 0.0f;
#pragma unroll
            for (int b = 0; b < PPO_MAX_A; ++b) if (b < A) {
                const float p3 = q[b] / s2;
                h -= logf(fminf(fmaxf(p3, EPS), 1.0f - EPS)) * p3;
            }
            ent += h;
        }
        ent /= (float)N;
        if (softplus && ent <= 20.0f) ent = log1pf(expf(ent));          // F.softplus (threshold 20)
        const float r = rewards[row + t] + ent_coeff * ent;              // rewards += c * H (f32, :415-416)
        rs[t] = r;
        vs[t] = baselines[row + t];
        if (entropy_out) entropy_out[row + t] = ent;
        if (rewards_out) rewards_out[row + t] = r;                       // (same thread read rewards[row + t]: aliasing is fine)
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float *a = adv + row;                                                // gae_kernel's recurrence, bit for bit
    const double gl = (double)(gamma * lam);
    double acc = 0.0, vnext = 0.0;
#pragma unroll 8
    for (int t = T - 1; t >= 0; --t) {
        const float delta = (rs[t] + gamma * (float)vnext) - vs[t];
        acc = (double)delta + gl * acc;
        a[t] = (float)acc;
        vnext = vs[t];
    }
}

}  // namespace cm

extern "C" int cm_entropy_gae(int32_t P, int32_t T, int32_t N, int32_t A, const float *logits, const float *rewards,
                              const float *baselines, float gamma, float lam, float ent_coeff, int32_t softplus, float *rewards_out,
                              float *entropy_out, float *adv, void *stream) {
    if (A < 1 || A > PPO_MAX_A || N < 1) return set_error(CM_ERR_ARG, "cm_entropy_gae: 1 <= n_actions <= 8 and n_agents >= 1 required");
    if (T > CM_ENT_GAE_MAX_T) return set_error(CM_ERR_ARG, "cm_entropy_gae: T above CM_ENT_GAE_MAX_T");
    if (P <= 0 || T <= 0) return CM_OK;
    if (!logits || !rewards || !baselines || !adv) return set_error(CM_ERR_ARG, "cm_entropy_gae: null argument");
    hipLaunchKernelGGL(entropy_gae_kernel, dim3((unsigned)P), dim3(256), 2 * (size_t)T * sizeof(float), (hipStream_t)stream, T, N, A,
                       logits, rewards, baselines, gamma, lam, ent_coeff, softplus, rewards_out, entropy_out, adv);
    CM_HIP(hipGetLastError());
    return CM_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Gaussian negative log-likelihood of the critic (comm_base_critic.py:59-89: -Normal(values, std.mean()).log_prob(returns).mean()
// with values = the per-agent outputs summed over the team (:110-112) and std = exp(clamp(log_std, min)) of
// gaussian_mlp_module.py:62-188) in ONE launch, and its gradient in one more - the framework spells the same arithmetic as
// ~25 elementwise / reduction launches forward and as many backward, which at the reference's batch size is half of an
// optimiser step's launches.  Normal.log_prob's own expression is kept: var = sigma^2, log_scale = log(sigma),
//   loss = mean_s[(r_s - v_s)^2] / (2 var) + log_scale + log(sqrt(2 pi))
// The sum of squares is accumulated in f64 (block sums + one f64 atomic per block); the last block to finish writes the two
// results and clears the workspace for the next launch.
// ---------------------------------------------------------------------------------------------------------------
struct GaussWs { double sum; unsigned int done; unsigned int pad; };

__device__ __forceinline__ float gauss_sigma(const float *log_std, float min_log_std, int has_min) {
    float ls = log_std[0];
    if (has_min) ls = fmaxf(ls, min_log_std);
    return expf(ls);
}

template <bool DET = false>   // slab mode: `ws` is a slab of one f64 per workgroup, gauss_nll_finish_kernel ends the launch
__global__ __launch_bounds__(256) void gauss_nll_fwd_kernel(long S, int N, const float *__restrict__ per_agent, const float *__restrict__ returns,
                                                            const float *__restrict__ log_std, float min_log_std, int has_min,
                                                            float *__restrict__ out, GaussWs *__restrict__ ws) {
    double part = 0.0;
    for (long s = (long)blockIdx.x * 256 + threadIdx.x; s < S; s += (long)gridDim.x * 256) {
        float v = 0.0f;
        for (int i = 0; i < N; ++i) v += per_agent[s * N + i];
        const float d = returns[s] - v;
        part += (double)(d * d);
    }
    __shared__ double red[256];
    __shared__ bool last;
    red[threadIdx.x] = part;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) { if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k]; __syncthreads(); }
    if constexpr (DET) {
        if (threadIdx.x == 0) reinterpret_cast<double *>(ws)[blockIdx.x] = red[0];
        return;
    }
    if (threadIdx.x == 0) {
        atomicAdd(&ws->sum, red[0]);
        __threadfence();
        last = atomicAdd(&ws->done, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (last && threadIdx.x == 0) {
        __threadfence();
        const double total = atomicAdd(&ws->sum, 0.0);             // through L2, after every block's contribution
        const float msq = (float)(total / (double)S);
        const float sigma = gauss_sigma(log_std, min_log_std, has_min);
        const float var = sigma * sigma, log_scale = logf(sigma);
        out[0] = msq / (2.0f * var) + log_scale + 0.918938533204672742f;   // log(sqrt(2 pi))
        out[1] = msq;
        ws->sum = 0.0;
        ws->done = 0u;
    }
}

__global__ __launch_bounds__(256) void gauss_nll_finish_kernel(long S, const double *__restrict__ slab, int n, const float *__restrict__ log_std,
                                                               float min_log_std, int has_min, float *__restrict__ out) {
    const double total = fixed_order_sum(slab, n);
    if (threadIdx.x == 0) {                                        // gauss_nll_fwd_kernel's last-block arithmetic
        const float msq = (float)(total / (double)S);
        const float sigma = gauss_sigma(log_std, min_log_std, has_min);
        const float var = sigma * sigma, log_scale = logf(sigma);
        out[0] = msq / (2.0f * var) + log_scale + 0.918938533204672742f;
        out[1] = msq;
    }
}

// d loss / d per_agent[s][i] = -(r_s - v_s) / (var S);  d loss / d log_std = 1 - msq / var (zero below the clamp);  both times *g
__global__ __launch_bounds__(256) void gauss_nll_bwd_kernel(long S, int N, const float *__restrict__ per_agent, const float *__restrict__ returns,
                                                            const float *__restrict__ log_std, float min_log_std, int has_min,
                                                            const float *__restrict__ out, const float *__restrict__ g,
                                                            float *__restrict__ d_per_agent, float *__restrict__ d_log_std) {
    const float sigma = gauss_sigma(log_std, min_log_std, has_min), var = sigma * sigma;
    const float gs = g ? g[0] : 1.0f;
    const float k = -gs / (var * (float)S);
    for (long s = (long)blockIdx.x * 256 + threadIdx.x; s < S; s += (long)gridDim.x * 256) {
        float v = 0.0f;
        for (int i = 0; i < N; ++i) v += per_agent[s * N + i];
        const float dv = k * (returns[s] - v);
        for (int i = 0; i < N; ++i) d_per_agent[s * N + i] = dv;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && d_log_std)
        d_log_std[0] = (has_min && log_std[0] < min_log_std) ? 0.0f : gs * (1.0f - out[1] / var);
}

extern "C" size_t cm_gauss_nll_forward_det_ws_bytes(int64_t S) {
    if (S < 1) return 0;
    return (size_t)std::min<long>((S + 255) / 256, 256) * sizeof(double);
}

// cm_gauss_nll_forward and its slab twin (DET: one f64 block sum per workgroup, gauss_nll_finish_kernel ends the launch)
template <bool DET>
static int gauss_nll_forward(const char *fn, int64_t S, int32_t N, const float *per_agent, const float *returns, const float *log_std,
                             float min_log_std, int32_t has_min, float *out, void *ws, size_t ws_bytes, void *stream) {
    // the default requires its GaussWs; the twin's ws is the slab, checked by slab_check
    if (!per_agent || !returns || !log_std || !out || (!DET && !ws)) return set_error(CM_ERR_ARG, std::string(fn) + ": null argument");
    if (S < 1 || N < 1) return set_error(CM_ERR_ARG, std::string(fn) + ": S >= 1 and n_agents >= 1 required");
    if (DET)
        if (const int rc = slab_check(ws, ws_bytes, cm_gauss_nll_forward_det_ws_bytes(S), fn)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    const int blocks = (int)std::min<long>((S + 255) / 256, 256);
    hipLaunchKernelGGL(gauss_nll_fwd_kernel<DET>, dim3(blocks), dim3(256), 0, st, (long)S, N, per_agent, returns, log_std, min_log_std,
                       has_min, out, reinterpret_cast<GaussWs *>(ws));
    CM_HIP(hipGetLastError());
    if (!DET) return CM_OK;
    hipLaunchKernelGGL(gauss_nll_finish_kernel, dim3(1), dim3(256), 0, st, (long)S, static_cast<const double *>(ws), blocks, log_std,
                       min_log_std, has_min, out);
    CM_HIP(hipGetLastError());
    return CM_OK;
}

extern "C" int cm_gauss_nll_forward(int64_t S, int32_t N, const float *per_agent, const float *returns, const float *log_std, float min_log_std,
                                    int32_t has_min, float *out, void *ws, void *stream) {
    return gauss_nll_forward<false>(__func__, S, N, per_agent, returns, log_std, min_log_std, has_min, out, ws, 0, stream);
}

extern "C" int cm_gauss_nll_forward_det(int64_t S, int32_t N, const float *per_agent, const float *returns, const float *log_std,
                                        float min_log_std, int32_t has_min, float *out, void *ws, size_t ws_bytes, void *stream) {
    return gauss_nll_forward<true>(__func__, S, N, per_agent, returns, log_std, min_log_std, has_min, out, ws, ws_bytes, stream);
}

extern "C" int cm_gauss_nll_backward(int64_t S, int32_t N, const float *per_agent, const float *returns, const float *log_std, float min_log_std,
                                     int32_t has_min, const float *out, const float *g, float *d_per_agent, float *d_log_std, void *stream) {
    if (!per_agent || !returns || !log_std || !out || !d_per_agent) return set_error(CM_ERR_ARG, "cm_gauss_nll_backward: null argument");
    if (S < 1 || N < 1) return set_error(CM_ERR_ARG, "cm_gauss_nll_backward: S >= 1 and n_agents >= 1 required");
    const int blocks = (int)std::min<long>((S + 255) / 256, 1024);
    hipLaunchKernelGGL(gauss_nll_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (long)S, N, per_agent, returns, log_std, min_log_std,
                       has_min, out, g, d_per_agent, d_log_std);
    CM_HIP(hipGetLastError());
    return CM_OK;
}
