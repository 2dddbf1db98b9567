// cm_value_stats.hip - cm_value_stats, cm_episode_value, cm_value_means, cm_value_curves, cm_value_curve_means: how good the critic's
// values are (gfx950).  cm_value_stats compares, for the first episode of each of B envs over T recorded steps, the critic's value
// v[t] (f32) with the discounted return-to-go of the rewards (f64)
//   G[n-1] = r[n-1],  G[t] = r[t] + gamma G[t+1]           n = the episode's length (cm_episode_stats' rule); no bootstrap at a cut
// and with the values the same critic gives under a mute and a lossless channel.  Per (t, b) CM_VALUE_COLS doubles: value, ret,
// sq_err = (v - G)^2, ret_sq = G^2, msg_value = v - v_mute, loss_value = v_lossless - v (include/commarl.h); rows at t >= n are exact
// zeros.  All arithmetic is f64; the product and the sum of the recurrence are rounded separately (-ffp-contract=off).
// Decomposition: one lane per env, the lanes of a wave on consecutive b, and every lane walks the SAME t at the same time - first
// ascending for the length, then descending from T - 1 for the recurrence, a lane whose episode has ended (t >= n) keeping G = 0
// and storing the zero row - so every load and store of a step is coalesced over [T, B] whatever the lengths are.  Both walks are
// sequential in t per lane: the loads of SCAN / STEPS steps are issued together ahead of the dependent chain.  Loads that a lane has
// no use for are not branched around: such a lane reads element 0 of the array and drops the value.  No atomics, no LDS, no
// shuffles; the batches are unrolled with constant indices, so no private array is indexed dynamically: no private segment.  A
// row depends on its env's column of the inputs alone, its order of operations on (T, n) alone - not on B or the grid: the same
// inputs give the same bits.  The NULL counterfactuals are template arguments: their column is the constant +0.0, nothing is read.
// The four reductions are the shared ones of csrc/cm_stat_rows.hip on rows of six doubles, every column divided by n (n_episodes
// for the curves): rows::Div{ 1 }, no column also by N or L.
#include "cm_internal.h"

static_assert(CM_VALUE_COLS == 6 && CM_EPV_COLS == CM_VALUE_COLS,
              "cm_stat_rows.hip's <double, 6> rows; an episode row has its step rows' columns");

#include <cmath>

namespace cm {
namespace vs {

// TPB = one wave: the launch has only B lanes of work, one wave per workgroup spreads them over the most compute units
constexpr int TPB = 64, SCAN = 32, STEPS = 16, COLS = CM_VALUE_COLS;

template <bool MUTE, bool LOSSLESS>
__global__ __launch_bounds__(TPB) void value_stats_kernel(int T, int B, const double *__restrict__ rewards,
                                                          const int32_t *__restrict__ path_len, const float *__restrict__ values,
                                                          const float *__restrict__ mute, const float *__restrict__ lossless,
                                                          double gamma, double *__restrict__ stats) {
    const long long gid = (long long)blockIdx.x * TPB + threadIdx.x;
    if (gid >= B) return;                                           // (a ragged last wave; nothing below needs the whole wave)
    const size_t b = (size_t)gid;

    // ---- length: n = t + 1 for the first t with path_len[t][b] > 0, else T (as cm_episode_stats) ----
    int first = T;
    for (int t0 = 0; t0 < T && __ballot(first == T) != 0ull; t0 += SCAN) {
        int32_t e[SCAN];
#pragma unroll
        for (int u = 0; u < SCAN; ++u) e[u] = path_len[t0 + u < T ? (size_t)(t0 + u) * B + b : (size_t)0];
        int f = T;
#pragma unroll
        for (int u = SCAN - 1; u >= 0; --u) f = ((t0 + u < T) & (e[u] > 0)) ? t0 + u : f;
        first = min(first, f);                                      // (batches ascend: the earliest stays)
    }
    const int n = first < T ? first + 1 : T;

    // ---- the recurrence, t = T-1 .. 0: G = 0 past the episode's end ----
    double G = 0.0;
    for (int t1 = T; t1 > 0; t1 -= STEPS) {                         // the steps t1-1, t1-2, ..., t1-STEPS that exist
        double r[STEPS];
        float v[STEPS], m[STEPS], l[STEPS];
#pragma unroll
        for (int u = 0; u < STEPS; ++u) {
            const int t = t1 - 1 - u;
            const size_t at = (t >= 0 && t < n) ? (size_t)t * B + b : (size_t)0;
            r[u] = rewards[at];
            v[u] = values[at];
            if constexpr (MUTE) m[u] = mute[at];
            if constexpr (LOSSLESS) l[u] = lossless[at];
        }
#pragma unroll
        for (int u = 0; u < STEPS; ++u) {
            const int t = t1 - 1 - u;
            if (t < 0) continue;                                    // (wave-uniform: the first steps' batch may be short)
            const bool run = t < n;
            const double vv = (double)v[u];
            const double g = t == n - 1 ? r[u] : r[u] + gamma * G;
            G = run ? g : 0.0;
            const double err = vv - G;
            double *__restrict__ row = stats + ((size_t)t * B + b) * COLS;
            row[0] = run ? vv : 0.0;
            row[1] = G;
            row[2] = run ? err * err : 0.0;
            row[3] = G * G;
            if constexpr (MUTE)
                row[4] = run ? vv - (double)m[u] : 0.0;
            else
                row[4] = 0.0;
            if constexpr (LOSSLESS)
                row[5] = run ? (double)l[u] - vv : 0.0;
            else
                row[5] = 0.0;
        }
    }
}

}  // namespace vs
}  // namespace cm

using namespace cm;

extern "C" int cm_value_stats(int32_t T, int32_t B, const double *rewards, const int32_t *path_len, const float *values,
                              const float *mute, const float *lossless, double gamma, double *stats, void *stream) {
    if (T < 0 || B < 0) return set_error(CM_ERR_ARG, "cm_value_stats: T >= 0 and B >= 0 required");
    if (!(gamma >= 0.0 && gamma <= 1.0)) return set_error(CM_ERR_ARG, "cm_value_stats: 0 <= gamma <= 1 required");   // (a NaN too)
    if (T == 0 || B == 0) return CM_OK;
    if (!rewards || !path_len || !values || !stats) return set_error(CM_ERR_ARG, "cm_value_stats: null rewards, path_len, values or stats");
    const int grid = (int)(((long long)B + vs::TPB - 1) / vs::TPB);
    const hipStream_t st = (hipStream_t)stream;
#define CM_VALUE_LAUNCH(M, LS)                                                                                                       \
    hipLaunchKernelGGL((vs::value_stats_kernel<M, LS>), dim3(grid), dim3(vs::TPB), 0, st, T, B, rewards, path_len, values, mute, lossless, \
                       gamma, stats)
    if (mute && lossless)
        CM_VALUE_LAUNCH(true, true);
    else if (mute)
        CM_VALUE_LAUNCH(true, false);
    else if (lossless)
        CM_VALUE_LAUNCH(false, true);
    else
        CM_VALUE_LAUNCH(false, false);
#undef CM_VALUE_LAUNCH
    CM_HIP(hipGetLastError());
    return CM_OK;
}

// every column is a mean per step: divided by n alone (rows::Div{ 1 })
extern "C" int cm_episode_value(int32_t T, int32_t B, const int32_t *path_len, const double *stats, int32_t group_size, int32_t take,
                                int32_t episodes_per_group, int32_t row0, double *episodes, void *stream) {
    return rows::episode_rows<double, CM_VALUE_COLS>("cm_episode_value", T, B, { 1 }, path_len, stats,
                                   group_size, take, episodes_per_group, row0, episodes, stream);
}

extern "C" int cm_value_means(int32_t K, int32_t E, const double *episodes, double *summary, void *stream) {
    return rows::group_means<CM_VALUE_COLS>("cm_value_means", K, E, episodes, summary, stream);
}

extern "C" int cm_value_curves(int32_t T, int32_t B, const int32_t *path_len, const double *stats, int32_t group_size, int32_t take,
                               int32_t accumulate, double *sums, void *stream) {
    return rows::curve_sums<double, CM_VALUE_COLS>("cm_value_curves", T, B, { 1 }, path_len, stats,
                                   group_size, take, accumulate, sums, stream);
}

extern "C" int cm_value_curve_means(int32_t cells, int32_t T, int32_t n_episodes, const double *sums, double *curves, void *stream) {
    return rows::curve_means<CM_VALUE_COLS>("cm_value_curve_means", cells, T, n_episodes, { 1 }, sums, curves, stream);
}
