// cm_stat_rows.hip - the four reductions every statistics family of the evaluation shares (gfx950): a round's per-step rows
// stats [slots, B, COLS] - int32 x 4 from cm_comm_stats, double x 6 from cm_attn_stats / cm_listen_stats / cm_value_stats - reduced
// over each env's FIRST episode (slots 0 .. n-1: what the policy acted through).  Behind the 16 entry points cm_episode_<family>,
// cm_<family>_means, cm_<family>_curves and cm_<family>_curve_means (include/commarl.h), which stay in their family's unit as
// one-line calls:
//   episode_rows   one wave per env: the episode's length (ep::episode_len), lane l sums its steps t = l, l + 64, ... < n in ascending
//                  t, the lanes meet in the xor tree; every column is divided ONCE, by n N or n N L.  -> a row of [cells, E, COLS].
//   group_means    one wave per cell: the mean of its E episode rows, lane-strided ascending, then the xor tree.
//   curve_sums     one wave per cell and tile of steps, lane l env l of a chunk of 64 (the chunks ascending): per step the sum over
//                  the episodes still running (an ended episode adds zero) into [cells, T, COLS]; accumulate = 0 starts the table.
//   curve_means    every entry of that table divided once, by N E or N E L.
// Which columns are also divided by L is the family's `l_cols` mask (rows::Div): no rule hides in a column index.
// Integer rows are summed as integers per episode (long long per lane, then the tree) and as exactly representable doubles per
// step; rows of doubles keep ONE order for every launch: the same episodes give the same bits.  No LDS, no barrier, no atomic, one
// writer per table entry.  Output columns are chosen by lane through selects, no private array is indexed dynamically: no
// private segment, no flat or scratch addressing.
#include "cm_episode_dev.h"

#include <type_traits>

namespace cm {
namespace rows {

using namespace ep;
constexpr int TPB = 256, WAVES = TPB / 64, MAX_N = 255, MAX_L = 8;

// Four columns per lane -> every lane holds the wave's total of ONE column, column lane >> 4: a butterfly that halves the columns a
// lane carries at each of its first two stages - a lane keeps the half its lane bit names, sends the other half to its partner
// and adds what it receives - and carries one column through the rest.  7 exchanges instead of 24; the order of every sum is fixed.
__device__ __forceinline__ double wave_sum4(const double (&v)[4], int lane) {
    const bool h5 = (lane & 32) != 0, h4 = (lane & 16) != 0;
    double a[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) a[i] = (h5 ? v[2 + i] : v[i]) + __shfl_xor(h5 ? v[i] : v[2 + i], 32);
    double s = (h4 ? a[1] : a[0]) + __shfl_xor(h4 ? a[0] : a[1], 16);
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    return s;
}

template <typename V, int COLS>
__global__ __launch_bounds__(TPB) void episode_rows_kernel(int T, int B, int N, int L, unsigned l_cols, const int32_t *__restrict__ path_len,
                                                           const V *__restrict__ stats, int group_size, int take,
                                                           int episodes_per_group, int row0, int n_rows, double *__restrict__ episodes) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * WAVES + (threadIdx.x >> 6);          // the w-th env that is summarised
    if (w >= n_rows) return;                                        // (wave-uniform: a ragged last workgroup)
    const int k = w / take, j = w - k * take;
    const size_t b = (size_t)k * group_size + j;
    const int n = episode_len(path_len, T, B, b, lane);

    // ---- slots 0 .. n-1: the graphs the policy acted through ----
    std::conditional_t<std::is_integral<V>::value, long long, double> c[COLS];
#pragma unroll
    for (int q = 0; q < COLS; ++q) c[q] = 0;
    for (int t = lane; t < n; t += 64) {
        const V *__restrict__ r = stats + ((size_t)t * B + b) * COLS;
#pragma unroll
        for (int q = 0; q < COLS; ++q) c[q] += r[q];
    }
    const double nN = (double)n * (double)N, nNL = nN * (double)L;  // exact: below 2^53
    double out = 0.0;
#pragma unroll
    for (int q = 0; q < COLS; ++q) {
        const double v = (double)wave_sum(c[q]) / (((l_cols >> q) & 1u) ? nNL : nN);
        out = lane == q ? v : out;
    }
    if (lane < COLS) episodes[((size_t)k * episodes_per_group + row0 + j) * COLS + lane] = out;
}

template <int COLS>
__global__ __launch_bounds__(TPB) void group_means_kernel(int K, int E, const double *__restrict__ episodes, double *__restrict__ summary) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (k >= K) return;
    const double *__restrict__ rows = episodes + (size_t)k * E * COLS;
    double s[COLS];
#pragma unroll
    for (int c = 0; c < COLS; ++c) s[c] = 0.0;
    for (int i = lane; i < E; i += 64) {
#pragma unroll
        for (int c = 0; c < COLS; ++c) s[c] += rows[(size_t)i * COLS + c];
    }
    double out = 0.0;
#pragma unroll
    for (int c = 0; c < COLS; ++c) {
        s[c] = wave_sum(s[c]) / (double)E;
        out = lane == c ? s[c] : out;
    }
    if (lane < COLS) summary[(size_t)k * COLS + lane] = out;
}

template <typename V, int COLS>
__global__ __launch_bounds__(TPB) void curve_sums_kernel(int T, int B, const int32_t *__restrict__ path_len, const V *__restrict__ stats,
                                                         int group_size, int take, int tile, int tiles, long long n_waves,
                                                         int accumulate, double *__restrict__ sums) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (w >= n_waves) return;                                   // (wave-uniform: a ragged last workgroup)
    const int k = (int)(w / tiles);
    const int t0 = (int)(w - (long long)k * tiles) * tile, t1 = min(T, t0 + tile);

    for (int j0 = 0; j0 < take; j0 += 64) {                     // the group's envs, 64 at a time, in ascending order
        const int j = j0 + lane;
        const size_t b = (size_t)k * group_size + j;
        const bool fresh = j0 == 0 && accumulate == 0;          // this chunk starts the table's entries
        const bool first = running_at(path_len, B, b, t0, j < take);
        const int stop = last_running(path_len, B, b, t0, t1, first);
        for (int t = t0; t < t1; ++t) {
            const bool run = first && t - t0 <= stop;
            if (__ballot(run) == 0ull && !fresh) break;         // nothing more to add
            // slot t: the graph the policy acted through
            const V *__restrict__ row = stats + (run ? (size_t)t * B + b : (size_t)0) * COLS;
            double out = 0.0;
            int col = lane;                                     // the column this lane holds the total of (lane < COLS)
            bool writer = lane < COLS;
            if constexpr (COLS == 4) {                          // one butterfly for the four columns: column lane >> 4
                double v[4] = { (double)row[0], (double)row[1], (double)row[2], (double)row[3] };
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] = run ? v[c] : 0.0;
                out = wave_sum4(v, lane);
                col = lane >> 4;
                writer = (lane & 15) == 0;
            } else {
#pragma unroll
                for (int q = 0; q < COLS; ++q) {
                    const double v = wave_sum(run ? (double)row[q] : 0.0);
                    out = lane == q ? v : out;
                }
            }
            if (writer) {
                double *__restrict__ at = sums + ((size_t)k * T + t) * COLS + col;
                *at = (fresh ? 0.0 : *at) + out;
            }
        }
    }
}

template <int COLS>
__global__ __launch_bounds__(TPB) void curve_means_kernel(long long n, int n_episodes, int N, int L, unsigned l_cols,
                                                          const double *__restrict__ sums, double *__restrict__ curves) {
    const double nNE = (double)N * (double)n_episodes, nNLE = nNE * (double)L;   // exact: below 2^53
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long long)gridDim.x * TPB)
        curves[i] = sums[i] / (((l_cols >> (int)(i % COLS)) & 1u) ? nNLE : nNE);
}

// ---- the host side; `who` names the entry point in the refusals' texts ----------------------------------------------------------------
static int refuse(const char *who, const char *what) { return set_error(CM_ERR_ARG, std::string(who) + ": " + what); }

template <typename V, int COLS>
int episode_rows(const char *who, int T, int B, Div d, const int32_t *path_len, const V *stats, int group_size, int take,
                 int episodes_per_group, int row0, double *episodes, void *stream) {
    if (T < 1 || B < 0) return refuse(who, "T >= 1 and B >= 0 required");
    if (d.N < 1 || d.N > MAX_N) return refuse(who, "1 <= n_agents <= 255 required");
    if (d.L < 1 || d.L > MAX_L) return refuse(who, "1 <= n_hops <= 8 required");
    if (group_size < 1 || B % group_size != 0) return refuse(who, "group_size >= 1 must divide B");
    if (take < 0 || take > group_size) return refuse(who, "0 <= take <= group_size required");
    if (row0 < 0 || (int64_t)row0 + take > episodes_per_group)
        return refuse(who, "rows row0 .. row0 + take - 1 must lie in 0 .. episodes_per_group - 1");
    if (B == 0 || take == 0) return CM_OK;
    if (!path_len || !stats || !episodes) return refuse(who, "null argument");
    const int n_rows = (int)((int64_t)(B / group_size) * take);     // <= B
    const int grid = (n_rows + WAVES - 1) / WAVES;
    hipLaunchKernelGGL((episode_rows_kernel<V, COLS>), dim3(grid), dim3(TPB), 0, (hipStream_t)stream, T, B, d.N, d.L, d.l_cols, path_len,
                       stats, group_size, take, episodes_per_group, row0, n_rows, episodes);
    CM_HIP(hipGetLastError());
    return CM_OK;
}

template <int COLS>
int group_means(const char *who, int K, int E, const double *episodes, double *summary, void *stream) {
    if (K < 1 || E < 1) return refuse(who, "K >= 1 and E >= 1 required");
    if (!episodes || !summary) return refuse(who, "null argument");
    const int grid = (K + WAVES - 1) / WAVES;
    hipLaunchKernelGGL(group_means_kernel<COLS>, dim3(grid), dim3(TPB), 0, (hipStream_t)stream, K, E, episodes, summary);
    CM_HIP(hipGetLastError());
    return CM_OK;
}

template <typename V, int COLS>
int curve_sums(const char *who, int T, int B, Div d, const int32_t *path_len, const V *stats, int group_size, int take, int accumulate,
               double *sums, void *stream) {
    if (T < 1 || B < 0) return refuse(who, "T >= 1 and B >= 0 required");
    if (d.N < 1 || d.N > MAX_N) return refuse(who, "1 <= n_agents <= 255 required");
    if (d.L < 1 || d.L > MAX_L) return refuse(who, "1 <= n_hops <= 8 required");
    if (group_size < 1 || B % group_size != 0) return refuse(who, "group_size >= 1 must divide B");
    if (take < 0 || take > group_size) return refuse(who, "0 <= take <= group_size required");
    if (accumulate != 0 && accumulate != 1) return refuse(who, "accumulate must be 0 or 1");
    if (B == 0 || take == 0) return CM_OK;
    if (!path_len || !stats || !sums) return refuse(who, "null argument");
    const int groups = B / group_size, tile = tile_of(groups, T), tiles = (T + tile - 1) / tile;
    const long long n_waves = (long long)groups * tiles;
    const long long grid = (n_waves + WAVES - 1) / WAVES;
    if (grid > INT32_MAX) return refuse(who, "too many (group, step) pairs for one launch");
    hipLaunchKernelGGL((curve_sums_kernel<V, COLS>), dim3((unsigned)grid), dim3(TPB), 0, (hipStream_t)stream, T, B, path_len, stats,
                       group_size, take, tile, tiles, n_waves, accumulate, sums);
    CM_HIP(hipGetLastError());
    return CM_OK;
}

template <int COLS>
int curve_means(const char *who, int cells, int T, int n_episodes, Div d, const double *sums, double *curves, void *stream) {
    if (cells < 1 || T < 1 || n_episodes < 1) return refuse(who, "cells, T and n_episodes >= 1 required");
    if (d.N < 1 || d.N > MAX_N) return refuse(who, "1 <= n_agents <= 255 required");
    if (d.L < 1 || d.L > MAX_L) return refuse(who, "1 <= n_hops <= 8 required");
    if (!sums || !curves) return refuse(who, "null argument");
    const long long n = (long long)cells * T * COLS;
    const long long blocks = (n + TPB - 1) / TPB;
    hipLaunchKernelGGL(curve_means_kernel<COLS>, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(TPB), 0, (hipStream_t)stream, n,
                       n_episodes, d.N, d.L, d.l_cols, sums, curves);
    CM_HIP(hipGetLastError());
    return CM_OK;
}

// the two row kinds there are: cm_comm_stats' and the six doubles of cm_attn_stats / cm_listen_stats / cm_value_stats
#define CM_STAT_ROWS(V, COLS)                                                                                                           \
    template int episode_rows<V, COLS>(const char *, int, int, Div, const int32_t *, const V *, int, int, int, int, double *, void *); \
    template int curve_sums<V, COLS>(const char *, int, int, Div, const int32_t *, const V *, int, int, int, double *, void *);        \
    template int group_means<COLS>(const char *, int, int, const double *, double *, void *);                                           \
    template int curve_means<COLS>(const char *, int, int, int, Div, const double *, double *, void *);
// (each family's unit asserts that its CM_*_COLS are these counts)
CM_STAT_ROWS(int32_t, 4)
CM_STAT_ROWS(double, 6)

}  // namespace rows
}  // namespace cm
