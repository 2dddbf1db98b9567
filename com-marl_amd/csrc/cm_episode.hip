// cm_episode.hip - cm_episode_stats, cm_episode_means: what evaluate._rounds + evaluate._episode compute on the host from copied
// trajectory buffers, reduced on the device (gfx950).  Each env's FIRST episode of a round becomes one row of CM_EPI_COLS doubles
// (success, then evaluate.VECTORS); cm_episode_means turns a policy's rows into its score (CM_SUM_COLS doubles).
// One wave owns one env (stats) or one group of rows (means); a 256-thread workgroup holds four independent waves - no LDS, no
// barrier, no atomic.  A wave's work on env b:
//   length      lane l looks at path_len[t][b] for t = l, l + 64, ...; the wave minimum of the lanes' first ends gives n.  The
//               scan stops at the first round of 64 steps that holds an end.
//   columns     lane l sums reward_f64 (f64) and the detail columns (integers) over its steps t < n in ascending t; the lanes'
//               sums meet in an xor butterfly (32, 16, ..., 1): one order for every launch, every lane holds the same bits.
//   degree      the adjacency slots the terminal-step rule needs - 1 .. n-1, or slot 0 alone for n = 1 - are walked as ONE flat
//               range of (slot, element) positions, 64 consecutive positions per load instruction and four instructions in flight:
//               with N*N a multiple of 4 a position is 16 bytes (at N = 4 a load instruction covers 16 steps), else one float.
//               Slots past n are never read.  Entries are 0 / 1, so the sums are integers: slot n-1 is kept apart and counted
//               twice (deg[1], ..., deg[n-1], deg[n-1]).
// The [T,B] arrays are read with one lane per step (stride B elements): 40 bytes per (step, env), ~33 MB at 4096 envs x 200 steps,
// next to which the adjacency walk (coalesced) is the traffic that counts.
// Output columns are chosen by lane through selects, no private array is indexed dynamically: no private segment, no flat or
// scratch addressing.
#include "cm_episode_dev.h"

#include <math.h>

namespace cm {
namespace epi {

using namespace ep;
typedef unsigned long long u64;
constexpr int TPB = 256, WAVES = TPB / 64, MAX_N = 255, UNROLL = 4;

template <int VEC>
__device__ __forceinline__ float load_sum(const float *p) {
    if constexpr (VEC == 4) {
        const float4 v = *reinterpret_cast<const float4 *>(p);
        return (v.x + v.y) + (v.z + v.w);
    } else {
        return *p;
    }
}

// VEC: floats per position of the adjacency walk (4: N*N % 4 == 0 and a 16-byte aligned buffer; else 1)
template <int VEC>
__global__ __launch_bounds__(TPB) void episode_stats_kernel(int T, int B, int N, int scenario, const double *__restrict__ reward,
                                                            const int32_t *__restrict__ details, const int32_t *__restrict__ success,
                                                            const int32_t *__restrict__ path_len, const float *__restrict__ adj,
                                                            int group_size, int take, int episodes_per_group, int row0, int n_rows,
                                                            double *__restrict__ episodes) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * WAVES + (threadIdx.x >> 6);      // the w-th env that is summarised
    if (w >= n_rows) return;                                    // (wave-uniform: a ragged last workgroup)
    const int k = w / take, j = w - k * take;
    const size_t b = (size_t)k * group_size + j;

    const int n = episode_len(path_len, T, B, b, lane);         // t + 1 for the first t with path_len[t][b] > 0, else T

    // ---- columns ----
    double r = 0.0;
    long long d0 = 0, d1 = 0, d2 = 0, d3 = 0, d4 = 0;
    for (int t = lane; t < n; t += 64) {
        const size_t i = (size_t)t * B + b;
        r += reward[i];
        const int32_t *__restrict__ d = details + i * 6;
        d0 += d[0];
        d1 += d[1];
        d2 += d[2];
        d3 += d[3];
        d4 += d[4];
    }
    r = wave_sum(r);
    d0 = wave_sum(d0);
    d1 = wave_sum(d1);
    d2 = wave_sum(d2);
    d3 = wave_sum(d3);
    d4 = wave_sum(d4);
    const int succ = success[(size_t)(n - 1) * B + b];

    // ---- degree ----
    double deg = (double)N;
    if (adj != nullptr) {
        const int s_lo = n > 1 ? 1 : 0, cnt = n > 1 ? n - 1 : 1;    // slots s_lo .. s_lo + cnt - 1
        const int Q = N * N / VEC;                                  // positions per slot
        const size_t slot = (size_t)N * N, step = (size_t)B * slot;
        const float *__restrict__ base = adj + ((size_t)s_lo * B + b) * slot;
        const int ds = 64 / Q, de = 64 - ds * Q;                    // 64 positions on: ds slots and de positions
        int s = lane / Q, e = lane - s * Q;
        u64 all = 0, last = 0;
        while (__ballot(s < cnt) != 0ull) {
            float v[UNROLL];
            int at[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                at[u] = s;
                // a lane past the end reads its element of the last slot again (in bounds) and drops it
                v[u] = load_sum<VEC>(base + (size_t)min(s, cnt - 1) * step + (size_t)e * VEC);
                s += ds;
                e += de;
                if (e >= Q) {
                    e -= Q;
                    ++s;
                }
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const u64 c = (u64)(unsigned)(int)v[u];
                all += at[u] < cnt ? c : 0ull;
                last += at[u] == cnt - 1 ? c : 0ull;
            }
        }
        all = wave_sum(all);
        last = wave_sum(last);
        // mean of deg[1], ..., deg[n-1], deg[n-1] (n = 1: deg[0]), deg[t] = (sum of slot t) / N: one division by the exact N n
        deg = (double)(all + (n > 1 ? last : 0ull)) / ((double)N * (double)n);
    }

    const double nA = (double)N;
    const bool pp = scenario == CM_PP;
    const double capture = pp ? (double)d0 : (double)d0 / nA;
    const double penalty = pp ? (double)d2 : (double)d2 / nA;
    const double vars2 = pp ? 0.0 : (double)d3 / nA;
    double out = (double)succ;
    out = lane == 1 ? r : out;
    out = lane == 2 ? capture : out;
    out = lane == 3 ? (double)n : out;
    out = lane == 4 ? (double)d1 / nA : out;
    out = lane == 5 ? penalty : out;
    out = lane == 6 ? deg : out;
    out = lane == 7 ? (double)d4 / nA : out;
    out = lane == 8 ? vars2 : out;
    if (lane < CM_EPI_COLS) episodes[((size_t)k * episodes_per_group + row0 + j) * CM_EPI_COLS + lane] = out;
}

__global__ __launch_bounds__(TPB) void episode_means_kernel(int K, int E, const double *__restrict__ episodes, double *__restrict__ summary) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (k >= K) return;
    const double *__restrict__ rows = episodes + (size_t)k * E * CM_EPI_COLS;
    double s[CM_EPI_COLS];
#pragma unroll
    for (int c = 0; c < CM_EPI_COLS; ++c) s[c] = 0.0;
    double lo = INFINITY, hi = -INFINITY;
    for (int i = lane; i < E; i += 64) {
        const double *__restrict__ row = rows + (size_t)i * CM_EPI_COLS;
#pragma unroll
        for (int c = 0; c < CM_EPI_COLS; ++c) s[c] += row[c];
        lo = fmin(lo, row[1]);
        hi = fmax(hi, row[1]);
    }
#pragma unroll
    for (int c = 0; c < CM_EPI_COLS; ++c) s[c] = wave_sum(s[c]) / (double)E;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, d));
        hi = fmax(hi, __shfl_xor(hi, d));
    }
    // population standard deviation of the reward column, second pass around the mean
    double q = 0.0;
    for (int i = lane; i < E; i += 64) {
        const double x = rows[(size_t)i * CM_EPI_COLS + 1] - s[1];
        q += x * x;
    }
    q = wave_sum(q);
    double out = sqrt(q / (double)E);                           // column 9; the selects below replace it on every other lane
#pragma unroll
    for (int c = 0; c < CM_EPI_COLS; ++c) out = lane == c ? s[c] : out;
    out = lane == 10 ? lo : out;
    out = lane == 11 ? hi : out;
    if (lane < CM_SUM_COLS) summary[(size_t)k * CM_SUM_COLS + lane] = out;
}

}  // namespace epi
}  // namespace cm

using namespace cm;

extern "C" int cm_episode_stats(int32_t T, int32_t B, int32_t N, int32_t scenario, const double *reward_f64, const int32_t *details,
                                const int32_t *success, const int32_t *path_len, const float *dist_adj, int32_t group_size,
                                int32_t take, int32_t episodes_per_group, int32_t row0, double *episodes, void *stream) {
    if (T < 1 || B < 0) return set_error(CM_ERR_ARG, "cm_episode_stats: T >= 1 and B >= 0 required");
    if (N < 1 || N > epi::MAX_N) return set_error(CM_ERR_ARG, "cm_episode_stats: 1 <= n_agents <= 255 required");
    if (scenario != CM_PP && scenario != CM_CO) return set_error(CM_ERR_ARG, "cm_episode_stats: scenario must be CM_PP or CM_CO");
    if (group_size < 1 || B % group_size != 0)
        return set_error(CM_ERR_ARG, "cm_episode_stats: group_size >= 1 must divide B");
    if (take < 0 || take > group_size) return set_error(CM_ERR_ARG, "cm_episode_stats: 0 <= take <= group_size required");
    if (row0 < 0 || (int64_t)row0 + take > episodes_per_group)
        return set_error(CM_ERR_ARG, "cm_episode_stats: rows row0 .. row0 + take - 1 must lie in 0 .. episodes_per_group - 1");
    if (B == 0 || take == 0) return CM_OK;
    if (!reward_f64 || !details || !success || !path_len || !episodes) return set_error(CM_ERR_ARG, "cm_episode_stats: null argument");
    const int64_t rows = (int64_t)(B / group_size) * take;
    const int n_rows = (int)rows;                               // <= B
    const int grid = (n_rows + epi::WAVES - 1) / epi::WAVES;
    const bool vec = (N * N) % 4 == 0 && ((uintptr_t)dist_adj & 15u) == 0;
    const hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(epi::episode_stats_kernel<4>, dim3(grid), dim3(epi::TPB), 0, st, T, B, N, scenario, reward_f64, details,
                           success, path_len, dist_adj, group_size, take, episodes_per_group, row0, n_rows, episodes);
    else
        hipLaunchKernelGGL(epi::episode_stats_kernel<1>, dim3(grid), dim3(epi::TPB), 0, st, T, B, N, scenario, reward_f64, details,
                           success, path_len, dist_adj, group_size, take, episodes_per_group, row0, n_rows, episodes);
    CM_HIP(hipGetLastError());
    return CM_OK;
}

extern "C" int cm_episode_means(int32_t K, int32_t E, const double *episodes, double *summary, void *stream) {
    if (K < 1 || E < 1) return set_error(CM_ERR_ARG, "cm_episode_means: K >= 1 and E >= 1 required");
    if (!episodes || !summary) return set_error(CM_ERR_ARG, "cm_episode_means: null argument");
    const int grid = (K + epi::WAVES - 1) / epi::WAVES;
    hipLaunchKernelGGL(epi::episode_means_kernel, dim3(grid), dim3(epi::TPB), 0, (hipStream_t)stream, K, E, episodes, summary);
    CM_HIP(hipGetLastError());
    return CM_OK;
}
