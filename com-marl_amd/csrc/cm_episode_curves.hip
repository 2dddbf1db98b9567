// cm_episode_curves.hip - cm_episode_curves, cm_curve_means, cm_comm_curves, cm_comm_curve_means: the evaluation rounds of
// cm_episode_stats / cm_episode_comm reduced over EPISODES with the step axis kept (gfx950): what exp_runners/testing.py:307-324
// pads with zeros to max_env_steps and saves as rewMat3, averaged over the episodes.  The curves kernels write per-step SUMS over a
// group's episodes (an episode that has ended contributes zero: the zero padding); the means kernels divide every sum once.
// cm_comm_curves / cm_comm_curve_means are the shared reductions of csrc/cm_stat_rows.hip on cm_comm_stats' rows of four int32.
// One wave owns one group and one tile of consecutive steps; a 256-thread workgroup holds four independent waves - no LDS, no
// barrier, no atomic, one writer per table entry.  A wave's work on its tile t0 .. t0 + tile - 1, for every chunk of 64 envs of the
// group (lane l owns env l of the chunk):
//   running     a lane's episode runs at step t iff no path_len[t'][b] > 0 for t' < t: rows 0 .. t0-1 of path_len are scanned once
//               per chunk and tile (256 contiguous bytes per row, 32 rows in flight, until no lane is left running), then the
//               tile's own rows are loaded at once and give the lane's last running step of the tile.  Which lanes run at a step
//               and which are at their terminal step (path_len[t][b] > 0 or t = T-1) is thus known before the step's loads: the
//               steps' loads wait on nothing but each other.
//   columns     the [T,B] arrays at step t are contiguous runs over the chunk's envs: every running lane loads its env's entries
//               (integers become doubles, which hold their sums exactly); the lanes' values meet in ONE xor butterfly (32, 16,
//               ..., 1) that leaves column c's total on lanes 8c .. 8c+7 (wave_sum8) - one order for every launch.
//   degree      the chunk's blocks of adjacency slot t+1 (slot t for the envs at their terminal step) are one contiguous run of
//               floats, walked flat: 64 consecutive positions per load instruction and four instructions in flight, a position
//               being 16 bytes where N*N is a multiple of 4 and the buffer 16-byte aligned, else one float.  The env of a position
//               is looked up in the wave's ballot of running lanes; blocks of ended episodes are not read.  The walk is issued
//               behind the column loads of the same step and shares their latency.
//   table       one lane per column adds the chunk's total to the group's entry (step, column): the first chunk of an
//               accumulate = 0 launch starts from zero, every other one from what the table holds (this wave wrote it).
// The tile length is chosen on the host from the number of groups and steps (more waves for few groups, fewer scans of path_len
// for many); it changes no sum's order.  Output columns are chosen by lane through selects, no private array is indexed
// dynamically: no private segment, no flat or scratch addressing.
#include "cm_episode_dev.h"

namespace cm {
namespace crv {

using namespace ep;
typedef unsigned long long u64;
constexpr int TPB = 256, WAVES = TPB / 64, MAX_N = 255, UNROLL = 4;

// Eight columns per lane -> every lane holds the wave's total of ONE column, column lane >> 3: a butterfly that halves the columns
// a lane carries at each of its first stages - a lane keeps the half its lane bit names, sends the other half to its partner and
// adds what it receives - and carries one column through the rest.  10 exchanges instead of 48; the order of every sum is fixed.
// All indices are compile-time: the arrays live in registers.
__device__ __forceinline__ double wave_sum8(const double (&v)[8], int lane) {
    const bool h5 = (lane & 32) != 0, h4 = (lane & 16) != 0, h3 = (lane & 8) != 0;
    double a[4], b[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = (h5 ? v[4 + i] : v[i]) + __shfl_xor(h5 ? v[i] : v[4 + i], 32);
#pragma unroll
    for (int i = 0; i < 2; ++i) b[i] = (h4 ? a[2 + i] : a[i]) + __shfl_xor(h4 ? a[i] : a[2 + i], 16);
    double s = (h3 ? b[1] : b[0]) + __shfl_xor(h3 ? b[0] : b[1], 8);
#pragma unroll
    for (int d = 4; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    return s;
}

template <int VEC>
__device__ __forceinline__ float load_sum(const float *p) {
    if constexpr (VEC == 4) {
        const float4 v = *reinterpret_cast<const float4 *>(p);
        return (v.x + v.y) + (v.z + v.w);
    } else {
        return *p;
    }
}

// The 0 / 1 floats of the N x N blocks of the envs named in `mask` (bit e: the e-th env of the run), summed: `base` is the first
// block of a run of P / Q blocks, Q positions of VEC floats each; lane l walks positions l, l + 64, ... ((e, r): its position's
// env and place in the block, (de, dr): 64 positions on).
template <int VEC>
__device__ __forceinline__ unsigned walk(const float *__restrict__ base, int P, int Q, u64 mask, int lane, int e, int r, int de, int dr) {
    unsigned sum = 0u;
    for (int p0 = 0; p0 < P; p0 += 64 * UNROLL) {
        float v[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int p = p0 + u * 64 + lane;
            const bool on = p < P && ((mask >> min(e, 63)) & 1ull) != 0ull;
            const float x = load_sum<VEC>(base + (size_t)(on ? p : 0) * VEC);
            v[u] = on ? x : 0.0f;
            e += de;
            r += dr;
            if (r >= Q) {
                r -= Q;
                ++e;
            }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) sum += (unsigned)(int)v[u];
    }
    return sum;
}

// VEC: floats per position of the adjacency walk (4: N*N % 4 == 0 and a 16-byte aligned buffer; else 1)
template <int VEC>
__global__ __launch_bounds__(TPB) void episode_curves_kernel(int T, int B, int N, const double *__restrict__ reward,
                                                             const int32_t *__restrict__ details, const int32_t *__restrict__ success,
                                                             const int32_t *__restrict__ path_len, const float *__restrict__ adj,
                                                             int group_size, int take, int tile, int tiles, long long n_waves,
                                                             int accumulate, double *__restrict__ sums) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (w >= n_waves) return;                                   // (wave-uniform: a ragged last workgroup)
    const int k = (int)(w / tiles);
    const int t0 = (int)(w - (long long)k * tiles) * tile, t1 = min(T, t0 + tile);
    const int NN = N * N, Q = NN / VEC;
    const int e0 = lane / Q, r0 = lane - e0 * Q, de = 64 / Q, dr = 64 - de * Q;

    for (int j0 = 0; j0 < take; j0 += 64) {                     // the group's envs, 64 at a time
        const int j = j0 + lane;
        const size_t b0 = (size_t)k * group_size + j0, b = b0 + lane;
        const int P = min(64, take - j0) * Q;
        const bool fresh = j0 == 0 && accumulate == 0;          // this chunk starts the table's entries
        const bool first = running_at(path_len, B, b, t0, j < take);
        const int stop = last_running(path_len, B, b, t0, t1, first);
        for (int t = t0; t < t1; ++t) {
            const bool run = first && t - t0 <= stop, term = run && (t - t0 == stop || t == T - 1);
            const u64 running = __ballot(run);
            if (running == 0ull && !fresh) break;               // nothing more to add
            // the step's columns are issued first and used behind the adjacency walk: one latency for both
            const size_t i = run ? (size_t)t * B + b : (size_t)0;
            const int32_t *__restrict__ d = details + i * 6;
            const double rew = reward[i];
            const int32_t sc = success[i], d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3], d4 = d[4];
            unsigned a = run ? (unsigned)NN : 0u;               // the constant full graph: N per running episode, times N
            if (adj != nullptr) {
                const u64 last = __ballot(term), on = running & ~last;
                a = 0u;
                if (on != 0ull) a += walk<VEC>(adj + ((size_t)(t + 1) * B + b0) * NN, P, Q, on, lane, e0, r0, de, dr);
                if (last != 0ull) a += walk<VEC>(adj + ((size_t)t * B + b0) * NN, P, Q, last, lane, e0, r0, de, dr);
            }
            // table columns 0, 1, 2, 4, 5, 6, 7, 8 (column 3, the running count, comes from the ballot)
            double v[8] = { (double)sc, rew, (double)d0, (double)d1, (double)d2, (double)a, (double)d4, (double)d3 };
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = (run || c == 5) ? v[c] : 0.0;
            double out = wave_sum8(v, lane);                    // column lane >> 3 of the eight
            int col = (lane >> 3) + ((lane >> 3) >= 3 ? 1 : 0);
            if (lane == 1) {
                out = (double)__popcll(running);
                col = 3;
            }
            if ((lane & 7) == 0 || lane == 1) {
                double *__restrict__ at = sums + ((size_t)k * T + t) * CM_EPI_COLS + col;
                *at = (fresh ? 0.0 : *at) + out;
            }
        }
    }
}

// every entry of a sums table divided once by its column's exact product; one thread per entry
__global__ __launch_bounds__(TPB) void curve_means_kernel(long long n, int n_episodes, int scenario, int N, const double *__restrict__ sums,
                                                          double *__restrict__ curves) {
    const double nE = (double)n_episodes, nNE = (double)N * nE;  // exact: both factors below 2^31
    const bool pp = scenario == CM_PP;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long long)gridDim.x * TPB) {
        const int c = (int)(i % CM_EPI_COLS);
        const bool whole = c == 0 || c == 1 || c == 3 || (pp && (c == 2 || c == 5));
        const double v = sums[i] / (whole ? nE : nNE);
        curves[i] = (pp && c == 8) ? 0.0 : v;
    }
}

static unsigned means_grid(long long n) {
    const long long g = (n + TPB - 1) / TPB;
    return (unsigned)(g < 65536 ? g : 65536);
}

}  // namespace crv
}  // namespace cm

using namespace cm;

extern "C" int cm_episode_curves(int32_t T, int32_t B, int32_t N, int32_t scenario, const double *reward_f64, const int32_t *details,
                                 const int32_t *success, const int32_t *path_len, const float *dist_adj, int32_t group_size,
                                 int32_t take, int32_t accumulate, double *sums, void *stream) {
    if (T < 1 || B < 0) return set_error(CM_ERR_ARG, "cm_episode_curves: T >= 1 and B >= 0 required");
    if (N < 1 || N > crv::MAX_N) return set_error(CM_ERR_ARG, "cm_episode_curves: 1 <= n_agents <= 255 required");
    if (scenario != CM_PP && scenario != CM_CO) return set_error(CM_ERR_ARG, "cm_episode_curves: scenario must be CM_PP or CM_CO");
    if (group_size < 1 || B % group_size != 0)
        return set_error(CM_ERR_ARG, "cm_episode_curves: group_size >= 1 must divide B");
    if (take < 0 || take > group_size) return set_error(CM_ERR_ARG, "cm_episode_curves: 0 <= take <= group_size required");
    if (accumulate != 0 && accumulate != 1) return set_error(CM_ERR_ARG, "cm_episode_curves: accumulate must be 0 or 1");
    if (B == 0 || take == 0) return CM_OK;
    if (!reward_f64 || !details || !success || !path_len || !sums) return set_error(CM_ERR_ARG, "cm_episode_curves: null argument");
    const int groups = B / group_size, tile = crv::tile_of(groups, T), tiles = (T + tile - 1) / tile;
    const long long n_waves = (long long)groups * tiles;        // <= B T
    const long long grid = (n_waves + crv::WAVES - 1) / crv::WAVES;
    if (grid > INT32_MAX) return set_error(CM_ERR_ARG, "cm_episode_curves: too many (group, step) pairs for one launch");
    const bool vec = (N * N) % 4 == 0 && ((uintptr_t)dist_adj & 15u) == 0;
    const hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(crv::episode_curves_kernel<4>, dim3((unsigned)grid), dim3(crv::TPB), 0, st, T, B, N, reward_f64, details,
                           success, path_len, dist_adj, group_size, take, tile, tiles, n_waves, accumulate, sums);
    else
        hipLaunchKernelGGL(crv::episode_curves_kernel<1>, dim3((unsigned)grid), dim3(crv::TPB), 0, st, T, B, N, reward_f64, details,
                           success, path_len, dist_adj, group_size, take, tile, tiles, n_waves, accumulate, sums);
    CM_HIP(hipGetLastError());
    return CM_OK;
}

extern "C" int cm_curve_means(int32_t cells, int32_t T, int32_t n_episodes, int32_t scenario, int32_t N, const double *sums,
                              double *curves, void *stream) {
    if (cells < 1 || T < 1 || n_episodes < 1) return set_error(CM_ERR_ARG, "cm_curve_means: cells, T and n_episodes >= 1 required");
    if (scenario != CM_PP && scenario != CM_CO) return set_error(CM_ERR_ARG, "cm_curve_means: scenario must be CM_PP or CM_CO");
    if (N < 1 || N > crv::MAX_N) return set_error(CM_ERR_ARG, "cm_curve_means: 1 <= n_agents <= 255 required");
    if (!sums || !curves) return set_error(CM_ERR_ARG, "cm_curve_means: null argument");
    const long long n = (long long)cells * T * CM_EPI_COLS;
    hipLaunchKernelGGL(crv::curve_means_kernel, dim3(crv::means_grid(n)), dim3(crv::TPB), 0, (hipStream_t)stream, n, n_episodes,
                       scenario, N, sums, curves);
    CM_HIP(hipGetLastError());
    return CM_OK;
}

extern "C" int cm_comm_curves(int32_t T, int32_t B, int32_t N, int32_t L, const int32_t *path_len, const int32_t *stats,
                              int32_t group_size, int32_t take, int32_t accumulate, double *sums, void *stream) {
    return rows::curve_sums<int32_t, CM_COMM_COLS>("cm_comm_curves", T, B, { N, L, rows::COMM_L_COLS }, path_len, stats, group_size, take,
                                                   accumulate, sums, stream);
}

extern "C" int cm_comm_curve_means(int32_t cells, int32_t T, int32_t n_episodes, int32_t N, int32_t L, const double *sums,
                                   double *curves, void *stream) {
    return rows::curve_means<CM_COMM_COLS>("cm_comm_curve_means", cells, T, n_episodes, { N, L, rows::COMM_L_COLS }, sums, curves, stream);
}
