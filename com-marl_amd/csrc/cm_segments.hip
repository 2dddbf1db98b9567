// cm_segments.hip - fixed-length rollout segments for the PPO update (gfx950): what a batch of n-step fragments of episodes needs
// where whole paths have cm_discount_returns / cm_gae / the host's per-path sums (DESIGN.md §7 "Rollout segments"):
//   * cm_segment_targets  : advantages and critic targets of a [P,T] batch of segments - episode ends inside a segment cut
//                           the scans, the cut at the segment's end is bootstrapped from the critic (v_last)
//   * cm_adv_normalize, cm_adv_normalize_ws_bytes : the batch-wide center_adv (f64 mean and biased variance over all values)
//   * cm_segment_episodes, cm_segment_episodes_ws_bytes : episode bookkeeping across segments - one carried record per env,
//                           the episodes that ended in this segment reduced into one row of CM_SEG_COLS doubles
// Small streaming kernels.  The engine's time-major buffers ([T,B]: rewards, dones, details, success) are read in place with one
// lane per env, so a wave's loads of one step are consecutive addresses.  No float atomics anywhere: every cross-thread sum is a
// butterfly inside the wave, the waves of a workgroup in index order, the workgroups in index order by a later launch - the grid
// depends on the shape alone, so the bits repeat from run to run (no deterministic twin).
#include <math.h>

#include "cm_internal.h"

namespace cm {
namespace seg {

constexpr int ROWS = 64;                                       // rows per workgroup of the targets scan (gae_kernel's)
constexpr int TPB = 256, WAVES = TPB / 64;
constexpr int NORM_MAX_GRID = 256, NORM_PER_WG = 4 * TPB;      // cm_adv_normalize: workgroups <= 256, >= 1024 values each
constexpr int WS_COLS = 16;                                    // a workgroup's row of the episode partials (CM_SEG_COLS used)

// One thread per row, backwards.  The arithmetic is gae_kernel's and returns_kernel's (cm_ppo.hip), bit for bit on a piece
// between two cuts: f32 delta, f64 accumulator, f64 return recurrence; g32 / lam32 are gamma / lam as cm_gae gets them.
__global__ __launch_bounds__(ROWS) void segment_targets_kernel(int P, int T, const double *__restrict__ rewards,
                                                               const uint8_t *__restrict__ dones, long long row_stride,
                                                               long long step_stride, const float *__restrict__ baselines,
                                                               const float *__restrict__ v_last, double gamma, float g32, float lam32,
                                                               float *__restrict__ adv, float *__restrict__ returns) {
    const int p = blockIdx.x * ROWS + threadIdx.x;
    if (p >= P) return;
    const float *v = baselines + (size_t)p * T;
    float *a = adv + (size_t)p * T, *ret = returns + (size_t)p * T;
    const double *r = rewards + (long long)p * row_stride;
    const uint8_t *d = dones + (long long)p * row_stride;
    const double gl = (double)(g32 * lam32);
    const float vl = v_last[p];
    double acc = 0.0, y = (double)vl;
    float vnext = vl;
    for (int t = T - 1; t >= 0; --t) {
        const long long i = (long long)t * step_stride;
        const double r64 = r[i];
        if (d[i]) { acc = 0.0; y = 0.0; vnext = 0.0f; }            // the episode ended with step t: nothing behind it counts
        const float delta = ((float)r64 + g32 * vnext) - v[t];
        acc = (double)delta + gl * acc;
        a[t] = (float)acc;
        vnext = v[t];
        y = r64 + gamma * y;
        ret[t] = (float)y;
    }
}

template <typename V>
__device__ __forceinline__ V wave_sum(V v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// sum over the workgroup in a fixed order (butterfly per wave, waves 0..3 in turn); every thread returns the same bits
__device__ __forceinline__ double block_sum(double v, double *lds) {
    v = wave_sum(v);
    __syncthreads();                                            // (lds may still be read from an earlier call)
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = lds[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s += lds[w];
    return s;
}

__device__ __forceinline__ double ordered_sum(const double *__restrict__ part, int n) {
    double s = 0.0;
    for (int j = 0; j < n; ++j) s += part[j];
    return s;
}

inline int norm_grid(long long count) {
    const long long g = (count + NORM_PER_WG - 1) / NORM_PER_WG;
    return (int)(g < 1 ? 1 : (g > NORM_MAX_GRID ? NORM_MAX_GRID : g));
}

// pass 1: the workgroups' sums -> ws[0 .. grid)
__global__ __launch_bounds__(TPB) void adv_sum_kernel(long long count, const float *__restrict__ a, double *__restrict__ ws) {
    __shared__ double lds[WAVES];
    double s = 0.0;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < count; i += (long long)gridDim.x * TPB) s += (double)a[i];
    s = block_sum(s, lds);
    if (threadIdx.x == 0) ws[blockIdx.x] = s;
}

// pass 2: around the mean of pass 1, the workgroups' sums of squares -> ws[NORM_MAX_GRID .. NORM_MAX_GRID + grid)
__global__ __launch_bounds__(TPB) void adv_sq_kernel(long long count, const float *__restrict__ a, double *__restrict__ ws) {
    __shared__ double lds[WAVES];
    const double mean = ordered_sum(ws, gridDim.x) / (double)count;
    double q = 0.0;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < count; i += (long long)gridDim.x * TPB) {
        const double dlt = (double)a[i] - mean;
        q += dlt * dlt;
    }
    q = block_sum(q, lds);
    if (threadIdx.x == 0) ws[NORM_MAX_GRID + blockIdx.x] = q;
}

// the expression gae_kernel applies per path, with the moments of the whole batch
__global__ __launch_bounds__(TPB) void adv_apply_kernel(long long count, float *__restrict__ a, const double *__restrict__ ws, float eps) {
    const double mean = ordered_sum(ws, gridDim.x) / (double)count;
    const double var = ordered_sum(ws + NORM_MAX_GRID, gridDim.x) / (double)count;
    const float m32 = (float)mean, inv = 1.0f / sqrtf((float)var + eps);
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < count; i += (long long)gridDim.x * TPB) a[i] = (a[i] - m32) * inv;
}

// One lane per env, forwards over the segment's n slots: the carried record goes on, an episode that ends is added to the lane's
// partial row; the rows meet per workgroup in ws[blockIdx][WS_COLS].  rec_f64 [3][B]: return so far, discounted return so far,
// gamma^length; rec_i64 [6][B]: length, the five details sums.
__global__ __launch_bounds__(TPB) void segment_episodes_kernel(int n, int B, const double *__restrict__ reward,
                                                               const uint8_t *__restrict__ done, const int32_t *__restrict__ details,
                                                               const int32_t *__restrict__ success, double gamma,
                                                               double *__restrict__ rec_f64, long long *__restrict__ rec_i64,
                                                               double *__restrict__ ws) {
    __shared__ double lds[WAVES][WS_COLS];
    const int b = blockIdx.x * TPB + threadIdx.x;
    const bool valid = b < B;
    const size_t sB = (size_t)B;
    double ret = 0.0, disc = 0.0, gp = 1.0;
    long long len = 0, d0 = 0, d1 = 0, d2 = 0, d3 = 0, d4 = 0;
    if (valid) {
        ret = rec_f64[b], disc = rec_f64[sB + b], gp = rec_f64[2 * sB + b];
        len = rec_i64[b], d0 = rec_i64[sB + b], d1 = rec_i64[2 * sB + b], d2 = rec_i64[3 * sB + b], d3 = rec_i64[4 * sB + b];
        d4 = rec_i64[5 * sB + b];
    }
    double cnt = 0.0, s = 0.0, q = 0.0, lo = INFINITY, hi = -INFINITY, ds = 0.0;
    long long ls = 0, ss = 0, e0 = 0, e1 = 0, e2 = 0, e3 = 0, e4 = 0;
    if (valid) {
        for (int t = 0; t < n; ++t) {
            const size_t i = (size_t)t * sB + b;
            const double r = reward[i];
            const int2 *__restrict__ dd = reinterpret_cast<const int2 *>(details + i * 6);    // rows of 24 bytes: 8-byte aligned
            const int2 x = dd[0], yv = dd[1], z = dd[2];
            ret += r;
            disc += gp * r;
            gp *= gamma;
            len += 1;
            d0 += x.x, d1 += x.y, d2 += yv.x, d3 += yv.y, d4 += z.x;
            if (done[i]) {
                cnt += 1.0, s += ret, q += ret * ret, lo = fmin(lo, ret), hi = fmax(hi, ret), ds += disc;
                ls += len, ss += success[i], e0 += d0, e1 += d1, e2 += d2, e3 += d3, e4 += d4;
                ret = 0.0, disc = 0.0, gp = 1.0;
                len = 0, d0 = 0, d1 = 0, d2 = 0, d3 = 0, d4 = 0;
            }
        }
        rec_f64[b] = ret, rec_f64[sB + b] = disc, rec_f64[2 * sB + b] = gp;
        rec_i64[b] = len, rec_i64[sB + b] = d0, rec_i64[2 * sB + b] = d1, rec_i64[3 * sB + b] = d2, rec_i64[4 * sB + b] = d3;
        rec_i64[5 * sB + b] = d4;
    }
    cnt = wave_sum(cnt), s = wave_sum(s), q = wave_sum(q), ds = wave_sum(ds);
    ls = wave_sum(ls), ss = wave_sum(ss), e0 = wave_sum(e0), e1 = wave_sum(e1), e2 = wave_sum(e2), e3 = wave_sum(e3), e4 = wave_sum(e4);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, d));
        hi = fmax(hi, __shfl_xor(hi, d));
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        double *row = lds[w];
        row[CM_SEG_COUNT] = cnt, row[CM_SEG_RET_SUM] = s, row[CM_SEG_RET_SUMSQ] = q, row[CM_SEG_RET_MIN] = lo, row[CM_SEG_RET_MAX] = hi;
        row[CM_SEG_DISC_SUM] = ds, row[CM_SEG_LEN_SUM] = (double)ls, row[CM_SEG_SUCCESS] = (double)ss;
        row[CM_SEG_DETAILS] = (double)e0, row[CM_SEG_DETAILS + 1] = (double)e1, row[CM_SEG_DETAILS + 2] = (double)e2;
        row[CM_SEG_DETAILS + 3] = (double)e3, row[CM_SEG_DETAILS + 4] = (double)e4;
    }
    __syncthreads();
    if (threadIdx.x < CM_SEG_COLS) {
        const int c = threadIdx.x;
        double v = lds[0][c];
#pragma unroll
        for (int k = 1; k < WAVES; ++k)
            v = c == CM_SEG_RET_MIN ? fmin(v, lds[k][c]) : (c == CM_SEG_RET_MAX ? fmax(v, lds[k][c]) : v + lds[k][c]);
        ws[(size_t)blockIdx.x * WS_COLS + c] = v;
    }
}

// the workgroups' rows in index order -> table [CM_SEG_COLS]
__global__ __launch_bounds__(64) void segment_episodes_finish_kernel(int grid, const double *__restrict__ ws, double *__restrict__ table) {
    const int c = threadIdx.x;
    if (c >= CM_SEG_COLS) return;
    double v = ws[c];
    for (int j = 1; j < grid; ++j) {
        const double x = ws[(size_t)j * WS_COLS + c];
        v = c == CM_SEG_RET_MIN ? fmin(v, x) : (c == CM_SEG_RET_MAX ? fmax(v, x) : v + x);
    }
    table[c] = v;
}

}  // namespace seg
}  // namespace cm

using namespace cm;

extern "C" int cm_segment_targets(int32_t P, int32_t T, const double *rewards64, const uint8_t *dones, int64_t row_stride,
                                  int64_t step_stride, const float *baselines, const float *v_last, double gamma, double lam,
                                  float *adv, float *returns, void *stream) {
    if (!rewards64 || !dones || !baselines || !v_last || !adv || !returns) return set_error(CM_ERR_ARG, "cm_segment_targets: null argument");
    if (T <= 0) return set_error(CM_ERR_ARG, "cm_segment_targets: T >= 1 required");
    if (P < 0 || row_stride < 0 || step_stride < 0) return set_error(CM_ERR_ARG, "cm_segment_targets: P and the strides must not be negative");
    if (P == 0) return CM_OK;
    hipLaunchKernelGGL(seg::segment_targets_kernel, dim3((P + seg::ROWS - 1) / seg::ROWS), dim3(seg::ROWS), 0, (hipStream_t)stream, P, T,
                       rewards64, dones, (long long)row_stride, (long long)step_stride, baselines, v_last, gamma, (float)gamma, (float)lam,
                       adv, returns);
    CM_HIP(hipGetLastError());
    return CM_OK;
}

extern "C" size_t cm_adv_normalize_ws_bytes(void) { return 2 * seg::NORM_MAX_GRID * sizeof(double); }

extern "C" int cm_adv_normalize(int64_t count, float *adv, float eps, void *ws, size_t ws_bytes, void *stream) {
    if (count < 0) return set_error(CM_ERR_ARG, "cm_adv_normalize: count >= 0 required");
    if (!adv) return set_error(CM_ERR_ARG, "cm_adv_normalize: null argument");
    if (!ws) return set_error(CM_ERR_ARG, "cm_adv_normalize: null workspace");
    if (ws_bytes < cm_adv_normalize_ws_bytes()) return set_error(CM_ERR_ARG, "cm_adv_normalize: workspace of cm_adv_normalize_ws_bytes() bytes required");
    if (count == 0) return CM_OK;
    const int grid = seg::norm_grid(count);
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(seg::adv_sum_kernel, dim3(grid), dim3(seg::TPB), 0, st, (long long)count, adv, (double *)ws);
    hipLaunchKernelGGL(seg::adv_sq_kernel, dim3(grid), dim3(seg::TPB), 0, st, (long long)count, adv, (double *)ws);
    hipLaunchKernelGGL(seg::adv_apply_kernel, dim3(grid), dim3(seg::TPB), 0, st, (long long)count, adv, (const double *)ws, eps);
    CM_HIP(hipGetLastError());
    return CM_OK;
}

extern "C" size_t cm_segment_episodes_ws_bytes(int32_t B) {
    const size_t grid = B > 0 ? ((size_t)B + seg::TPB - 1) / seg::TPB : 1;
    return grid * seg::WS_COLS * sizeof(double);
}

extern "C" int cm_segment_episodes(int32_t n_steps, int32_t B, const double *reward_f64, const uint8_t *done, const int32_t *details,
                                   const int32_t *success, double gamma, double *rec_f64, int64_t *rec_i64, double *table, void *ws,
                                   size_t ws_bytes, void *stream) {
    if (n_steps < 1 || B < 1) return set_error(CM_ERR_ARG, "cm_segment_episodes: n_steps >= 1 and B >= 1 required");
    if (!reward_f64 || !done || !details || !success || !rec_f64 || !rec_i64 || !table)
        return set_error(CM_ERR_ARG, "cm_segment_episodes: null argument");
    if (!ws) return set_error(CM_ERR_ARG, "cm_segment_episodes: null workspace");
    if (ws_bytes < cm_segment_episodes_ws_bytes(B))
        return set_error(CM_ERR_ARG, "cm_segment_episodes: workspace of cm_segment_episodes_ws_bytes(B) bytes required");
    const int grid = (B + seg::TPB - 1) / seg::TPB;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(seg::segment_episodes_kernel, dim3(grid), dim3(seg::TPB), 0, st, n_steps, B, reward_f64, done, details, success,
                       gamma, rec_f64, (long long *)rec_i64, (double *)ws);
    hipLaunchKernelGGL(seg::segment_episodes_finish_kernel, dim3(1), dim3(64), 0, st, grid, (const double *)ws, table);
    CM_HIP(hipGetLastError());
    return CM_OK;
}
