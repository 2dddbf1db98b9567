// cm_listen_stats.hip - cm_listen_stats, cm_episode_listen, cm_listen_means, cm_listen_curves, cm_listen_curve_means: whether the
// messages changed what the agents did (gfx950).  cm_listen_stats compares, for S recorded graphs of N agents, the action
// probabilities the policy acted on (probs [N,A] f32) with the ones it would have had under two counterfactual channels: mute
// (every agent hears only itself) and lossless (everything in range is delivered).  Per graph CM_LISTEN_COLS doubles: mute_kl,
// mute_tv, mute_flip, loss_kl, loss_tv, loss_flip (include/commarl.h), each the sum over the N agent rows of
//   kl   = sum over a with p[a] > 0 of p[a] (ln p[a] - ln max(q[a], FLT_MIN))      (not clamped at 0)
//   tv   = 0.5 sum_a |p[a] - q[a]|
//   flip = argmax(p) != argmax(q), the first index on ties, compared on the f32 values
// All arithmetic is f64 on the f32 inputs; ln p[a] is formed once and serves both counterfactuals.  A NULL counterfactual is
// "identical to probs": its three columns are written as exact 0 and nothing is read.  A streaming kernel: every input float is
// loaded once, no atomic.  The decomposition is cm_attn_stats.hip's:
//   N <= 8    P = 1 / 2 / 4 / 8 lanes own one graph (the power of two >= N), lane i the agent row i;
//   N >= 9    one wave owns one graph, lane i the rows i, i + 64, ... in ascending order;
// the six sums meet in log2 P xor shuffles and lane q stores the columns q, q + P, ....  A row is A <= 8 floats at float offset
// i A of its block: where N A % 4 == 0 and every block starts on a 16-byte boundary the lane loads the aligned 16-byte vectors that
// cover its row (at most three; one past the block's last is clamped onto it and not used) and picks its A values with selects on
// i A % 4; otherwise it loads them one float at a time.  Both paths feed the same values to the same arithmetic in the same order:
// the same bits.  The order depends on (N, A) alone - a row's terms in ascending a, a lane's rows in ascending order, then the xor
// tree - not on S, the grid or the load width.  A and P are template arguments: no private array is indexed dynamically, no
// private segment.
// The four reductions are the shared ones of csrc/cm_stat_rows.hip on rows of six doubles, every column divided by n N.
#include "cm_internal.h"

static_assert(CM_LISTEN_COLS == 6 && CM_EPL_COLS == CM_LISTEN_COLS,
              "cm_stat_rows.hip's <double, 6> rows; an episode row has its step rows' columns");

#include <cfloat>

namespace cm {
namespace ls {

constexpr int TPB = 256, MAX_N = 255, SMALL_N = 8, MIN_A = 2, MAX_A = 8, COLS = CM_LISTEN_COLS;

// the A floats of agent row i of the block at `block` (N rows).  VEC = 4: N A % 4 == 0 and the block 16-byte aligned
template <int A, int VEC>
__device__ __forceinline__ void load_row(const float *__restrict__ block, int i, int N, float (&f)[A]) {
    if constexpr (VEC == 4) {
        constexpr int NQ = A % 4 == 0 ? A / 4 : (A + 6) / 4;       // vectors that cover A floats at any offset 0 .. 3
        const int e0 = i * A, q0 = e0 >> 2, off = e0 & 3, last = ((N * A) >> 2) - 1;
        float w[4 * NQ];
#pragma unroll
        for (int u = 0; u < NQ; ++u) {                             // (a vector past the block's last reads the last again: not used)
            const float4 v = *reinterpret_cast<const float4 *>(block + 4 * (size_t)min(q0 + u, last));
            w[4 * u] = v.x;
            w[4 * u + 1] = v.y;
            w[4 * u + 2] = v.z;
            w[4 * u + 3] = v.w;
        }
#pragma unroll
        for (int a = 0; a < A; ++a) {
            if constexpr (A % 4 == 0)
                f[a] = w[a];
            else
                f[a] = off == 0 ? w[a] : off == 1 ? w[a + 1] : off == 2 ? w[a + 2] : w[a + 3];
        }
    } else {
        const float *__restrict__ row = block + (size_t)i * A;
#pragma unroll
        for (int a = 0; a < A; ++a) f[a] = row[a];
    }
}

// one agent row against one counterfactual row: its kl, tv and flip onto the three sums
template <int A>
__device__ __forceinline__ void add_row(const float (&p)[A], const double (&lnp)[A], int best_p, const float (&q)[A], double &kl, double &tv,
                                        double &flip) {
    double k = 0.0, d = 0.0;
    float bq = q[0];
    int best_q = 0;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const double pa = (double)p[a], qa = (double)q[a];
        k += p[a] > 0.0f ? pa * (lnp[a] - log(fmax(qa, (double)FLT_MIN))) : 0.0;
        d += fabs(pa - qa);
        if (a > 0 && q[a] > bq) {                                   // (strictly greater: the first index on ties)
            bq = q[a];
            best_q = a;
        }
    }
    kl += k;
    tv += 0.5 * d;
    flip += best_p != best_q ? 1.0 : 0.0;
}

template <int A, int P, int VEC>
__global__ __launch_bounds__(TPB) void listen_stats_kernel(int S, int N, const float *__restrict__ probs, long long probs_stride,
                                                           const float *__restrict__ mute, long long mute_stride,
                                                           const float *__restrict__ lossless, long long lossless_stride,
                                                           double *__restrict__ out) {
    const long long gid = (long long)blockIdx.x * TPB + threadIdx.x;
    const long long s_mine = gid / P;
    const int i0 = threadIdx.x & (P - 1);
    // lanes past the last graph walk graph S - 1 again (they take part in the shuffles) and store nothing
    const long long s = s_mine < S ? s_mine : (long long)S - 1;
    const float *__restrict__ pb = probs + s * probs_stride;
    const float *__restrict__ mb = mute != nullptr ? mute + s * mute_stride : nullptr;
    const float *__restrict__ lb = lossless != nullptr ? lossless + s * lossless_stride : nullptr;

    double c[COLS];
#pragma unroll
    for (int q = 0; q < COLS; ++q) c[q] = 0.0;
    for (int i = i0; i < N; i += P) {                               // (P < 64: N <= P, at most one row per lane)
        float p[A], q[A];
        load_row<A, VEC>(pb, i, N, p);
        double lnp[A];
        float bp = p[0];
        int best_p = 0;
#pragma unroll
        for (int a = 0; a < A; ++a) {
            lnp[a] = p[a] > 0.0f ? log((double)p[a]) : 0.0;
            if (a > 0 && p[a] > bp) {
                bp = p[a];
                best_p = a;
            }
        }
        if (mb != nullptr) {                                        // (uniform over the launch)
            load_row<A, VEC>(mb, i, N, q);
            add_row<A>(p, lnp, best_p, q, c[0], c[1], c[2]);
        }
        if (lb != nullptr) {
            load_row<A, VEC>(lb, i, N, q);
            add_row<A>(p, lnp, best_p, q, c[3], c[4], c[5]);
        }
    }
#pragma unroll
    for (int d = 1; d < P; d <<= 1) {
#pragma unroll
        for (int q = 0; q < COLS; ++q) c[q] += __shfl_xor(c[q], d);
    }
    if (s_mine >= S) return;
    double *__restrict__ row = out + s_mine * COLS;
#pragma unroll
    for (int q = 0; q < COLS; ++q)                                  // lane i stores the columns i, i + P, ...
        if ((q & (P - 1)) == i0) row[q] = c[q];
}

struct Args {
    int S, N, A;
    const float *probs;
    long long probs_stride;
    const float *mute;
    long long mute_stride;
    const float *lossless;
    long long lossless_stride;
    double *out;
};

// 16-byte loads: a block is a whole number of them and every block of the arrays that are read starts on a 16-byte boundary
static bool vec_ok(const Args &g) {
    return (g.N * g.A) % 4 == 0 && (((uintptr_t)g.probs | (uintptr_t)g.mute | (uintptr_t)g.lossless) & 15u) == 0 &&
           g.probs_stride % 4 == 0 && g.mute_stride % 4 == 0 && g.lossless_stride % 4 == 0;
}

template <int A, int P>
static int launch_lanes(const Args &g, hipStream_t st) {
    const long long grid = ((long long)g.S * P + TPB - 1) / TPB;    // S <= 2^31 - 1, P <= 64: below 2^37
    if (grid > INT32_MAX) return set_error(CM_ERR_ARG, "cm_listen_stats: too many graphs for one launch");
#define CM_LISTEN_LAUNCH(VEC)                                                                                                      \
    hipLaunchKernelGGL((listen_stats_kernel<A, P, VEC>), dim3((unsigned)grid), dim3(TPB), 0, st, g.S, g.N, g.probs, g.probs_stride, \
                       g.mute, g.mute_stride, g.lossless, g.lossless_stride, g.out)
    if (vec_ok(g))
        CM_LISTEN_LAUNCH(4);
    else
        CM_LISTEN_LAUNCH(1);
#undef CM_LISTEN_LAUNCH
    CM_HIP(hipGetLastError());
    return CM_OK;
}

template <int A>
static int launch(const Args &g, hipStream_t st) {
    if (g.N == 1) return launch_lanes<A, 1>(g, st);
    if (g.N == 2) return launch_lanes<A, 2>(g, st);
    if (g.N <= 4) return launch_lanes<A, 4>(g, st);
    if (g.N <= SMALL_N) return launch_lanes<A, 8>(g, st);
    return launch_lanes<A, 64>(g, st);
}

}  // namespace ls
}  // namespace cm

using namespace cm;

extern "C" int cm_listen_stats(int32_t S, int32_t N, int32_t A, const float *probs, int64_t probs_stride, const float *mute,
                               int64_t mute_stride, const float *lossless, int64_t lossless_stride, double *out, void *stream) {
    if (S < 0 || N < 1 || N > ls::MAX_N) return set_error(CM_ERR_ARG, "cm_listen_stats: S >= 0 and 1 <= n_agents <= 255 required");
    if (A < ls::MIN_A || A > ls::MAX_A) return set_error(CM_ERR_ARG, "cm_listen_stats: 2 <= n_actions <= 8 required");
    const int64_t block = (int64_t)N * A;
    if (probs_stride < block) return set_error(CM_ERR_ARG, "cm_listen_stats: probs_stride must be at least N * A");
    if (mute && mute_stride < block) return set_error(CM_ERR_ARG, "cm_listen_stats: mute_stride must be at least N * A");
    if (lossless && lossless_stride < block) return set_error(CM_ERR_ARG, "cm_listen_stats: lossless_stride must be at least N * A");
    if (S == 0) return CM_OK;
    if (!probs || !out) return set_error(CM_ERR_ARG, "cm_listen_stats: null probs or out");
    const ls::Args g{ S, N, A, probs, probs_stride, mute, mute ? mute_stride : 0, lossless, lossless ? lossless_stride : 0, out };
    const hipStream_t st = (hipStream_t)stream;
    switch (A) {
    case 2: return ls::launch<2>(g, st);
    case 3: return ls::launch<3>(g, st);
    case 4: return ls::launch<4>(g, st);
    case 5: return ls::launch<5>(g, st);
    case 6: return ls::launch<6>(g, st);
    case 7: return ls::launch<7>(g, st);
    default: return ls::launch<8>(g, st);
    }
}

// every column is a mean per agent: divided by n N (rows::Div{ N }), none also by L
extern "C" int cm_episode_listen(int32_t T, int32_t B, int32_t N, const int32_t *path_len, const double *stats, int32_t group_size,
                                 int32_t take, int32_t episodes_per_group, int32_t row0, double *episodes, void *stream) {
    return rows::episode_rows<double, CM_LISTEN_COLS>("cm_episode_listen", T, B, { N }, path_len, stats,
                                   group_size, take, episodes_per_group, row0, episodes, stream);
}

extern "C" int cm_listen_means(int32_t K, int32_t E, const double *episodes, double *summary, void *stream) {
    return rows::group_means<CM_LISTEN_COLS>("cm_listen_means", K, E, episodes, summary, stream);
}

extern "C" int cm_listen_curves(int32_t T, int32_t B, int32_t N, const int32_t *path_len, const double *stats, int32_t group_size,
                                int32_t take, int32_t accumulate, double *sums, void *stream) {
    return rows::curve_sums<double, CM_LISTEN_COLS>("cm_listen_curves", T, B, { N }, path_len, stats,
                                   group_size, take, accumulate, sums, stream);
}

extern "C" int cm_listen_curve_means(int32_t cells, int32_t T, int32_t n_episodes, int32_t N, const double *sums, double *curves,
                                     void *stream) {
    return rows::curve_means<CM_LISTEN_COLS>("cm_listen_curve_means", cells, T, n_episodes, { N }, sums, curves, stream);
}
