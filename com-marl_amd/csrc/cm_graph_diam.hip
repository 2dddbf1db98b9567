// cm_graph_diam.hip - cm_graph_diameter: the hop diameter of S range graphs of N <= 255 vertices (gfx950), what the reference's
// get_graph(..., calc_diameter=True) asks networkx for (env_communication.py:235-241): vertices i != j are joined when
// adj[i][j] != 0 OR adj[j][i] != 0, the diagonal is ignored; a connected graph gives its largest shortest-path hop count, a
// disconnected one 0.
// One wave owns one graph, a 256-thread workgroup four.  The adjacency rows live in LDS as bitmasks of W = ceil(N / 64) 64-bit
// words (integer offsets into one array; a wave's table holds 64 W rows: 512 W^2 bytes, 8 KB at W = 4):
//   build       a wave ballot over coalesced f32 reads gives 64 bits of a row (N <= 32: of several rows) per load;
//   transpose   the lane that owns row i ORs in bit i of every row j (word i / 64 of row j: one address for the whole wave);
//   search      level-synchronous BFS from 64 sources per pass, a lane holding the reach set and the frontier of its source in
//               W registers each: next = OR of row[j] over the frontier's j, and-not visited.  At most N - 1 levels.
// A source that does not reach all N vertices makes the graph disconnected; the eccentricity maximum is a wave reduction.
// W is a template argument, so no private array is indexed dynamically: no private segment, no flat or scratch addressing.
#include "cm_internal.h"

namespace cm {
namespace gd {

typedef unsigned long long u64;
constexpr int TPB = 256, WAVES = TPB / 64, MAX_N = 255;

template <int W>
__global__ __launch_bounds__(TPB) void graph_diameter_kernel(int S, int N, const float *__restrict__ adj, int32_t *__restrict__ diameter) {
    __shared__ u64 rows[WAVES * 64 * W * W];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int base = wave * 64 * W * W;
    const int s_mine = blockIdx.x * WAVES + wave;
    // a wave past the last graph of a ragged workgroup walks graph S - 1 again (it meets the same barriers) and stores nothing
    const int s = min(s_mine, S - 1);
    const float *__restrict__ a = adj + (size_t)s * N * N;

    // ---- build: bit j of row i = (adj[i][j] != 0), j != i ----
    if (W == 1 && N <= 32) {
        const int R = 64 / N, NN = N * N;                       // R whole rows per 64-lane load
        const int q = lane / N, c = lane - q * N;
        const u64 row_mask = (1ull << N) - 1ull;
        for (int r0 = 0; r0 < N; r0 += R) {
            const int k = r0 * N + lane;
            const bool in = lane < R * N && k < NN;
            const float v = a[in ? k : NN - 1];
            const u64 m = __ballot(in && c != r0 + q && v != 0.0f);
            if (q < R && r0 + q < N) rows[base + r0 + q] = (m >> ((q * N) & 63)) & row_mask;
        }
    } else {
        for (int i = 0; i < N; ++i) {
            u64 mine = 0ull;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const int col = w * 64 + lane;
                const float v = a[(size_t)i * N + min(col, N - 1)];
                const u64 m = __ballot(col < N && col != i && v != 0.0f);
                if (lane == w) mine = m;
            }
            if (lane < W) rows[base + i * W + lane] = mine;
        }
    }
    __syncthreads();

    // ---- transpose: row i |= column i.  In place: a row rewritten by an earlier pass already holds the union, and ORing the
    // union in again changes nothing ----
#pragma unroll
    for (int p = 0; p < W; ++p) {
        const int i = p * 64 + lane;
        u64 r[W];
#pragma unroll
        for (int w = 0; w < W; ++w) r[w] = i < N ? rows[base + i * W + w] : 0ull;
#pragma unroll
        for (int wj = 0; wj < W; ++wj) {
            const int lim = min(64, N - wj * 64);
            for (int jj = 0; jj < lim; ++jj) {
                const u64 x = rows[base + (wj * 64 + jj) * W + p];
                r[wj] |= ((x >> lane) & 1ull) << jj;
            }
        }
        __syncthreads();
        if (i < N) {
#pragma unroll
            for (int w = 0; w < W; ++w) rows[base + i * W + w] = r[w];
        }
        __syncthreads();
    }

    // ---- search ----
    int ecc = 0;
    bool apart = false;
#pragma unroll
    for (int p = 0; p < W; ++p) {
        const int i = p * 64 + lane;
        const bool src = i < N;
        u64 seen[W], fr[W];
#pragma unroll
        for (int w = 0; w < W; ++w) seen[w] = fr[w] = (src && w == p) ? (1ull << lane) : 0ull;
        for (int level = 1; level < N; ++level) {               // a shortest path has at most N - 1 hops
            u64 nx[W];
#pragma unroll
            for (int w = 0; w < W; ++w) nx[w] = 0ull;
#pragma unroll
            for (int wj = 0; wj < W; ++wj) {
                if (__ballot(fr[wj] != 0ull) == 0ull) continue; // no source of this pass has a frontier vertex in this word
                const int lim = min(64, N - wj * 64);
                for (int jj = 0; jj < lim; ++jj) {
                    const int row = base + (wj * 64 + jj) * W;
                    const u64 sel = 0ull - ((fr[wj] >> jj) & 1ull);
#pragma unroll
                    for (int w = 0; w < W; ++w) nx[w] |= rows[row + w] & sel;
                }
            }
            bool grew = false;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                fr[w] = nx[w] & ~seen[w];
                seen[w] |= fr[w];
                grew = grew || fr[w] != 0ull;
            }
            if (grew) ecc = max(ecc, level);                    // (the lane's largest over the passes' sources)
            if (__ballot(grew) == 0ull) break;
        }
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const int left = N - w * 64;                        // vertices in word w and above
            const u64 full = left >= 64 ? ~0ull : left > 0 ? (1ull << left) - 1ull : 0ull;
            apart = apart || (src && seen[w] != full);
        }
    }
    const bool split = __ballot(apart) != 0ull;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) ecc = max(ecc, __shfl_xor(ecc, d));
    if (lane == 0 && s_mine < S) diameter[s_mine] = split ? 0 : ecc;
}

template <int W>
static int launch(int S, int N, const float *adj, int32_t *diameter, hipStream_t st) {
    const int grid = (S + WAVES - 1) / WAVES;
    hipLaunchKernelGGL(graph_diameter_kernel<W>, dim3(grid), dim3(TPB), 0, st, S, N, adj, diameter);
    CM_HIP(hipGetLastError());
    return CM_OK;
}

}  // namespace gd
}  // namespace cm

using namespace cm;

extern "C" int cm_graph_diameter(int32_t S, int32_t N, const float *dist_adj, int32_t *diameter, void *stream) {
    if (S < 0 || N < 1 || N > gd::MAX_N) return set_error(CM_ERR_ARG, "cm_graph_diameter: S >= 0 and 1 <= n_agents <= 255 required");
    if (S == 0) return CM_OK;
    if (!dist_adj || !diameter) return set_error(CM_ERR_ARG, "cm_graph_diameter: null argument");
    const hipStream_t st = (hipStream_t)stream;
    switch ((N + 63) / 64) {
    case 1: return gd::launch<1>(S, N, dist_adj, diameter, st);
    case 2: return gd::launch<2>(S, N, dist_adj, diameter, st);
    case 3: return gd::launch<3>(S, N, dist_adj, diameter, st);
    default: return gd::launch<4>(S, N, dist_adj, diameter, st);
    }
}
