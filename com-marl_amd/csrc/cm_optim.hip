// cm_optim.hip - the optimiser side of the update (gfx950): the two kernels that walk a table of up to 40 tensors passed
// by value, so that a whole net takes one launch.
//   * cm_multi_adam_step, cm_multi_adam_step_dev, cm_multi_adam_step_gated, cm_adam_bias_corrections : multi-tensor Adam
//     with the gradient-norm clip (com_marl/torch/algos/my_optimizer/_functional.py:72-98, the vendored torch-1.9 Adam;
//     torch.nn.utils.clip_grad_norm_ as centralized_ma_ppo.py:253-255 calls it)
//   * cm_multi_copy_t : the flat weight copy of a net, what nets._flat_copy fills the C-ABI weight structs' storage
//     with after an optimiser step (the framework's per-tensor copy_)
#include "cm_internal.h"

namespace cm {

// ---------------------------------------------------------------------------------------------
// Multi-tensor Adam (+ gradient-norm clip) for the ~17 + ~15 small parameter tensors of the policy / critic: ONE launch
// for the norm, ONE for the update, instead of ~6 framework kernels per tensor and a host sync per tensor norm.
// The update is the vendored torch-1.9 Adam of the reference (com_marl/torch/algos/my_optimizer/_functional.py:72-98):
//   m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;  p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// and the clip is torch.nn.utils.clip_grad_norm_ (centralized_ma_ppo.py:253-255): g *= min(1, max_norm / (|g| + 1e-6)),
// written back so that p.grad holds the clipped gradient as it does in the reference.
// ---------------------------------------------------------------------------------------------
struct TensorTable { float *p[40]; float *g[40]; float *m[40]; float *v[40]; long n[40]; int count; };

// |g|^2 in two deterministic stages (replicas of a data-parallel job must take bit-identical steps from bit-identical
// all-reduced gradients; a float-atomic sum's order - and with it the clip factor's last bit - varies run to run):
// block b writes its partial sum to ws[1 + b]; the update kernel adds the NORM_BLOCKS partials in index order.
constexpr int NORM_BLOCKS = 64;

__global__ __launch_bounds__(256) void multi_norm_kernel(TensorTable t, float *ws) {
    float acc = 0.0f;
    const long stride = (long)gridDim.x * blockDim.x, i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    for (int k = 0; k < t.count; ++k)
        for (long i = i0; i < t.n[k]; i += stride) { const float g = t.g[k][i]; acc = fmaf(g, g, acc); }
    __shared__ float red[256];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s]; __syncthreads(); }
    if (threadIdx.x == 0) ws[1 + blockIdx.x] = red[0];
}

// bc_tab / cursor (cm_multi_adam_step_dev): the two bias-correction factors come from a device table indexed by a device step
// counter, so that a captured hipGraph of the optimiser step can be replayed for successive steps
// GATED (cm_multi_adam_step_gated) adds one trailing argument, the device gate word the launch before this one wrote: with
// *gate != 0 the step is not taken - norm_ws[0] still receives |g|^2, and the parameters, the moments and the gradients (not
// clipped) stay as they are.  The ungated instantiation has no such argument: its argument block and code are what they were.
template <bool GATED = false, class... Gate>
__global__ __launch_bounds__(256) void multi_adam_kernel(TensorTable t, float *norm_ws, float max_norm, float lr,
                                                        float b1, float b2, float eps, float bc1, float sqrt_bc2,
                                                        const float *__restrict__ bc_tab, const int32_t *__restrict__ cursor, int tab_steps,
                                                        Gate... gate) {
    if (bc_tab) {
        int c = *cursor;
        c = c < 0 ? 0 : (c >= tab_steps ? tab_steps - 1 : c);
        bc1 = bc_tab[2 * c]; sqrt_bc2 = bc_tab[2 * c + 1];
    }
    float coef = 1.0f;
    if (norm_ws) {
        float nsq = 0.0f;
        for (int b = 0; b < NORM_BLOCKS; ++b) nsq += norm_ws[1 + b];
        const float c = max_norm / (sqrtf(nsq) + 1e-6f);
        coef = c < 1.0f ? c : 1.0f;
        if (blockIdx.x == 0 && threadIdx.x == 0) norm_ws[0] = nsq;
    }
    if constexpr (GATED) {
        const int32_t *const g[] = { gate... };
        if (*g[0] != 0) return;
    }
    const bool norm_sq = norm_ws != nullptr;
    const float step_size = lr / bc1;
    const long stride = (long)gridDim.x * blockDim.x, i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    for (int k = 0; k < t.count; ++k)
        for (long i = i0; i < t.n[k]; i += stride) {
            float g = t.g[k][i];
            if (norm_sq) { g *= coef; t.g[k][i] = g; }
            const float m = t.m[k][i] * b1 + (1.0f - b1) * g;
            const float v = t.v[k][i] * b2 + (1.0f - b2) * g * g;
            t.m[k][i] = m; t.v[k][i] = v;
            const float denom = sqrtf(v) / sqrt_bc2 + eps;
            t.p[k][i] = t.p[k][i] - step_size * (m / denom);
        }
}

}  // namespace cm

using namespace cm;

static int multi_adam(int32_t n, float *const *params, float *const *grads, float *const *exp_avg, float *const *exp_avg_sq, const int64_t *sizes,
                      float *norm_ws, float max_norm, float lr, float beta1, float beta2, float eps, int32_t step, const float *bc_tab,
                      const int32_t *cursor, int32_t tab_steps, void *stream, const int32_t *gate = nullptr) {
    if (n < 0 || n > 40) return set_error(CM_ERR_ARG, "cm_multi_adam_step: at most 40 tensors per call");
    if (n == 0) return CM_OK;
    if (!params || !grads || !exp_avg || !exp_avg_sq || !sizes) return set_error(CM_ERR_ARG, "cm_multi_adam_step: bad argument");
    if (bc_tab ? (!cursor || tab_steps < 1) : step < 1) return set_error(CM_ERR_ARG, "cm_multi_adam_step: bad step / bias-correction table");
    TensorTable t{};
    t.count = n;
    for (int k = 0; k < n; ++k) { t.p[k] = params[k]; t.g[k] = grads[k]; t.m[k] = exp_avg[k]; t.v[k] = exp_avg_sq[k]; t.n[k] = (long)sizes[k]; }
    const hipStream_t st = (hipStream_t)stream;
    if (norm_ws) hipLaunchKernelGGL(multi_norm_kernel, dim3(NORM_BLOCKS), dim3(256), 0, st, t, norm_ws);
    const int hs = bc_tab ? 1 : step;
    const float bc1 = (float)(1.0 - pow((double)beta1, (double)hs)), sqrt_bc2 = (float)sqrt(1.0 - pow((double)beta2, (double)hs));
    if (gate)
        hipLaunchKernelGGL((multi_adam_kernel<true, const int32_t *>), dim3(64), dim3(256), 0, st, t, norm_ws, max_norm, lr, beta1, beta2, eps,
                           bc1, sqrt_bc2, bc_tab, cursor, (int)tab_steps, gate);
    else
        hipLaunchKernelGGL((multi_adam_kernel<false>), dim3(64), dim3(256), 0, st, t, norm_ws, max_norm, lr, beta1, beta2, eps, bc1, sqrt_bc2,
                           bc_tab, cursor, (int)tab_steps);
    CM_HIP(hipGetLastError());
    return CM_OK;
}

extern "C" int cm_multi_adam_step(int32_t n, float *const *params, float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                                  const int64_t *sizes, float *norm_ws, float max_norm, float lr, float beta1,
                                  float beta2, float eps, int32_t step, void *stream) {
    return multi_adam(n, params, grads, exp_avg, exp_avg_sq, sizes, norm_ws, max_norm, lr, beta1, beta2, eps, step, nullptr, nullptr, 0, stream);
}

extern "C" void cm_adam_bias_corrections(float beta1, float beta2, int32_t first_step, int32_t n_steps, float *table) {
    for (int i = 0; i < n_steps; ++i) {
        const double s = (double)first_step + i;
        table[2 * i] = (float)(1.0 - pow((double)beta1, s));
        table[2 * i + 1] = (float)sqrt(1.0 - pow((double)beta2, s));
    }
}

extern "C" int cm_multi_adam_step_dev(int32_t n, float *const *params, float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                                      const int64_t *sizes, float *norm_ws, float max_norm, float lr, float beta1, float beta2, float eps,
                                      const float *bc_table, const int32_t *cursor, int32_t table_steps, void *stream) {
    return multi_adam(n, params, grads, exp_avg, exp_avg_sq, sizes, norm_ws, max_norm, lr, beta1, beta2, eps, 0, bc_table, cursor, table_steps,
                      stream);
}

// cm_multi_adam_step_dev behind a device gate (the KL early stop of the PPO update, cm_ppo_stats.hip): *gate == 0 takes the step
// bit for bit, *gate != 0 leaves parameters, moments and gradients alone and still reports |g|^2
extern "C" int cm_multi_adam_step_gated(int32_t n, float *const *params, float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                                        const int64_t *sizes, float *norm_ws, float max_norm, float lr, float beta1, float beta2, float eps,
                                        const float *bc_table, const int32_t *cursor, int32_t table_steps, const int32_t *gate, void *stream) {
    if (!gate) return set_error(CM_ERR_ARG, "cm_multi_adam_step_gated: null gate");
    return multi_adam(n, params, grads, exp_avg, exp_avg_sq, sizes, norm_ws, max_norm, lr, beta1, beta2, eps, 0, bc_table, cursor, table_steps,
                      stream, gate);
}

// ---------------------------------------------------------------------------------------------------------------
// The flat weight copy of a net (transposed [in,out] matrices + biases, what the C-ABI weight structs point into) in ONE
// launch: tensor k is a [rows, cols] row-major source written to dst[k] as its TRANSPOSE ([cols, rows]) when transpose[k], else
// copied as it is.  (The framework's per-tensor copy_ cost 17 launches per net and optimiser step.)
// ---------------------------------------------------------------------------------------------------------------
struct CopyTable { const float *src[40]; float *dst[40]; int rows[40], cols[40], transpose[40]; int count; };

__global__ __launch_bounds__(256) void multi_copy_t_kernel(CopyTable t) {
    const long stride = (long)gridDim.x * blockDim.x, i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    for (int k = 0; k < t.count; ++k) {
        const int R = t.rows[k], C = t.cols[k];
        const long n = (long)R * C;
        if (t.transpose[k]) {
            for (long i = i0; i < n; i += stride) { const int c = (int)(i / R), r = (int)(i - (long)c * R); t.dst[k][i] = t.src[k][(long)r * C + c]; }   // dst [C][R]
        } else {
            for (long i = i0; i < n; i += stride) t.dst[k][i] = t.src[k][i];
        }
    }
}

extern "C" int cm_multi_copy_t(int32_t n, const float *const *src, float *const *dst, const int32_t *rows, const int32_t *cols,
                               const int32_t *transpose, void *stream) {
    if (n < 0 || n > 40) return set_error(CM_ERR_ARG, "cm_multi_copy_t: at most 40 tensors per call");
    if (n == 0) return CM_OK;
    if (!src || !dst || !rows || !cols || !transpose) return set_error(CM_ERR_ARG, "cm_multi_copy_t: null argument");
    CopyTable t{};
    t.count = n;
    for (int k = 0; k < n; ++k) {
        if (!src[k] || !dst[k] || rows[k] < 1 || cols[k] < 1) return set_error(CM_ERR_ARG, "cm_multi_copy_t: bad tensor");
        t.src[k] = src[k]; t.dst[k] = dst[k]; t.rows[k] = rows[k]; t.cols[k] = cols[k]; t.transpose[k] = transpose[k];
    }
    hipLaunchKernelGGL(multi_copy_t_kernel, dim3(64), dim3(256), 0, (hipStream_t)stream, t);
    CM_HIP(hipGetLastError());
    return CM_OK;
}
