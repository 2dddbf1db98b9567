// cm_ppo_stats.hip - what one optimiser step of the PPO update did to the policy, and the KL early stop
//   * cm_ppo_update_stats : one row of CM_UPD_COLS doubles per call (approximate KL, clip fraction, ratio range, entropy) from the
//                           minibatch's logits and old log-likelihoods, and the decision whether the step about to be taken is applied
// The optimiser steps of a minibatch replay from hipGraphs with their step counter on the device (algos._UpdateGraphs), so a
// `target_kl` stop cannot be a host-side `if`: this unit takes the decision on the device (a sticky gate word) and
// cm_multi_adam_step_gated (cm_optim.hip) obeys it.
//
// Two launches, the shape of gauss_nll_fwd_kernel<DET> + gauss_nll_finish_kernel: a grid-stride kernel of at most UPD_MAX_BLOCKS
// workgroups writes per-workgroup f64 partials and the ratio's min / max into the workspace; a one-workgroup finish kernel adds
// them in a fixed order, writes the row, sets the gate and advances the row cursor.  No float atomics, no last-block ticket:
// the kernel boundary is the visibility, every workspace word read was written by this call, and the row is bit-reproducible
// in every mode (there is no deterministic twin).
#include <string>

#include "cm_internal.h"
#include "cm_ppo_cat_dev.h"

namespace cm {

constexpr int UPD_MAX_BLOCKS = 256;
// workspace: UPD_PARTS planes of `blocks` doubles - the five sums, then the ratio's min and max
enum { UPD_P_VALID = 0, UPD_P_K3, UPD_P_K1, UPD_P_CLIPPED, UPD_P_ENT, UPD_P_RMIN, UPD_P_RMAX, UPD_PARTS };

static int upd_blocks(int32_t P, int32_t T) {
    if (P <= 0 || T <= 0) return 1;
    const long b = ((long)P * T + 255) / 256;
    return (int)(b < UPD_MAX_BLOCKS ? b : UPD_MAX_BLOCKS);
}

// red[q][tid] -> red[q][0] by a fixed tree over the 256 threads; q < UPD_P_RMIN are sums, then a min and a max
__device__ __forceinline__ void upd_tree(double (*red)[256]) {
    const int tid = threadIdx.x;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (tid < k) {
#pragma unroll
            for (int q = 0; q < UPD_P_RMIN; ++q) red[q][tid] += red[q][tid + k];
            red[UPD_P_RMIN][tid] = fmin(red[UPD_P_RMIN][tid], red[UPD_P_RMIN][tid + k]);
            red[UPD_P_RMAX][tid] = fmax(red[UPD_P_RMAX][tid], red[UPD_P_RMAX][tid + k]);
        }
        __syncthreads();
    }
}

// One thread handles one env step at a time; new_ll and H with ppo_surrogate_kernel's Categorical arithmetic
// (categorical_ll_entropy), lr = new_ll - old_ll in f32 as the loss takes it, everything after it in f64: in f32
// (r - 1) - log r cancels to nothing near r = 1.
__global__ __launch_bounds__(256) void ppo_update_stats_kernel(int P, int T, int N, int A, const float *__restrict__ logits,
                                                               const int32_t *__restrict__ actions, const float *__restrict__ old_ll,
                                                               const int32_t *__restrict__ lens, float clip, double *__restrict__ ws) {
    const long S = (long)P * T;
    double n_valid = 0.0, k3 = 0.0, k1 = 0.0, clipped = 0.0, ent_sum = 0.0;
    double rmin = INFINITY, rmax = -INFINITY;
    for (long s = (long)blockIdx.x * 256 + threadIdx.x; s < S; s += (long)gridDim.x * 256) {
        const int pth = (int)(s / T), t = (int)(s - (long)pth * T);
        if (t >= lens[pth]) continue;
        float new_ll, ent;
        categorical_ll_entropy(logits + s * N * A, actions + s * N, N, A, new_ll, ent);
        const float lr = new_ll - old_ll[s];
        const float r = expf(lr);                              // the ratio the loss clamps
        const double d = (double)lr;
        n_valid += 1.0;
        k3 += expm1(d) - d;
        k1 -= d;
        if (fabsf(r - 1.0f) > clip) clipped += 1.0;
        ent_sum += (double)ent;
        rmin = fmin(rmin, (double)r);
        rmax = fmax(rmax, (double)r);
    }
    __shared__ double red[UPD_PARTS][256];
    const int tid = threadIdx.x;
    red[UPD_P_VALID][tid] = n_valid; red[UPD_P_K3][tid] = k3; red[UPD_P_K1][tid] = k1; red[UPD_P_CLIPPED][tid] = clipped;
    red[UPD_P_ENT][tid] = ent_sum; red[UPD_P_RMIN][tid] = rmin; red[UPD_P_RMAX][tid] = rmax;
    upd_tree(red);
    if (tid < UPD_PARTS) ws[(long)tid * gridDim.x + blockIdx.x] = red[tid][0];
}

// One workgroup: the `blocks` partials of each plane in a fixed order (thread t takes partial t - there are at most 256 - then
// the fixed tree: fixed_order_sum's scheme), the row, the decision.
__global__ __launch_bounds__(256) void ppo_update_stats_finish_kernel(const double *__restrict__ ws, int blocks, double kl_stop,
                                                                      double *__restrict__ rows, int max_rows,
                                                                      int32_t *__restrict__ row_cursor, int32_t *__restrict__ gate) {
    __shared__ double red[UPD_PARTS][256];
    const int tid = threadIdx.x;
    const bool has = tid < blocks;
#pragma unroll
    for (int q = 0; q < UPD_P_RMIN; ++q) red[q][tid] = has ? ws[(long)q * blocks + tid] : 0.0;
    red[UPD_P_RMIN][tid] = has ? ws[(long)UPD_P_RMIN * blocks + tid] : (double)INFINITY;
    red[UPD_P_RMAX][tid] = has ? ws[(long)UPD_P_RMAX * blocks + tid] : -(double)INFINITY;
    upd_tree(red);
    if (tid != 0) return;
    const int cur = *row_cursor;
    const int k = cur < 0 ? 0 : (cur > max_rows - 1 ? max_rows - 1 : cur);
    const int was = gate ? *gate : 0;
    const double n = red[UPD_P_VALID][0];
    double *row = rows + (long)k * CM_UPD_COLS;
    const bool any = n > 0.0;
    const double approx_kl = any ? red[UPD_P_K3][0] / n : 0.0;
    const bool stop = was != 0 || (kl_stop > 0.0 && any && approx_kl > kl_stop);   // (a NaN kl_stop compares false: never stops)
    row[CM_UPD_N_VALID] = n;
    row[CM_UPD_APPROX_KL] = approx_kl;
    row[CM_UPD_KL] = any ? red[UPD_P_K1][0] / n : 0.0;
    row[CM_UPD_CLIP_FRAC] = any ? red[UPD_P_CLIPPED][0] / n : 0.0;
    row[CM_UPD_RATIO_MIN] = any ? red[UPD_P_RMIN][0] : 0.0;
    row[CM_UPD_RATIO_MAX] = any ? red[UPD_P_RMAX][0] : 0.0;
    row[CM_UPD_ENTROPY] = any ? red[UPD_P_ENT][0] / n : 0.0;
    row[CM_UPD_STOPPED] = stop ? 1.0 : 0.0;
    if (gate) *gate = stop ? 1 : 0;
    *row_cursor = cur + 1;
}

}  // namespace cm

using namespace cm;

extern "C" size_t cm_ppo_update_stats_ws_bytes(int32_t P, int32_t T) {
    return (size_t)UPD_PARTS * upd_blocks(P, T) * sizeof(double);
}

extern "C" int cm_ppo_update_stats(int32_t P, int32_t T, int32_t N, int32_t A, const float *logits, const int32_t *actions,
                                   const float *old_ll, const int32_t *lens, float clip, double kl_stop, double *rows, int32_t max_rows,
                                   int32_t *row_cursor, int32_t *gate, void *ws, size_t ws_bytes, void *stream) {
    const char *fn = __func__;
    if (!rows || !row_cursor || max_rows < 1) return set_error(CM_ERR_ARG, std::string(fn) + ": null rows / row_cursor or max_rows < 1");
    if (A < 1 || A > PPO_MAX_A || N < 1) return set_error(CM_ERR_ARG, std::string(fn) + ": 1 <= n_actions <= 8 and n_agents >= 1 required");
    const bool empty = P <= 0 || T <= 0;
    if (!empty && (!logits || !actions || !old_ll || !lens)) return set_error(CM_ERR_ARG, std::string(fn) + ": null argument");
    const size_t need = cm_ppo_update_stats_ws_bytes(P, T);
    if (!ws) return set_error(CM_ERR_ARG, std::string(fn) + ": null workspace");
    if (ws_bytes < need)
        return set_error(CM_ERR_ARG, std::string(fn) + ": workspace of " + std::to_string(ws_bytes) + " bytes, " + std::to_string(need) +
                                         " required");
    const hipStream_t st = (hipStream_t)stream;
    const int blocks = upd_blocks(P, T);
    double *const part = static_cast<double *>(ws);
    hipLaunchKernelGGL(ppo_update_stats_kernel, dim3((unsigned)blocks), dim3(256), 0, st, empty ? 0 : P, empty ? 0 : T, N, A, logits, actions,
                       old_ll, lens, clip, part);
    CM_HIP(hipGetLastError());
    hipLaunchKernelGGL(ppo_update_stats_finish_kernel, dim3(1), dim3(256), 0, st, part, blocks, kl_stop, rows, (int)max_rows, row_cursor, gate);
    CM_HIP(hipGetLastError());
    return CM_OK;
}
