// cm_comm_stats.hip - cm_comm_stats, cm_episode_comm, cm_comm_means: how much of the offered communication got through (gfx950).
// cm_comm_stats turns S recorded graphs (dist_adj [N,N], channels [L,N,N], f32, "set" = != 0) into CM_COMM_COLS int32 each:
// in_range, delivered, reach, range_reach (include/commarl.h).  The Comm-DP net hears j at hop l iff adj[i][j] * chan[l][i][j] != 0
// (comm_base_net.py:101-103), so reach is the number of (i, k) whose information can arrive within the L hops, hop 0 first.
// A streaming kernel: every float is loaded once, compared at once and kept as one bit of a row mask; the hop products are ORs of
// row masks in registers.  No atomic.  The decomposition is chosen per team-size class:
//   N <= 8    P = 1 / 2 / 4 / 8 lanes own one graph (the power of two >= N), lane i its row i: a 64-lane wave holds 64 / P graphs.
//             A row is N <= 8 bits; the whole N x N matrix fits one 64-bit word, which the P lanes assemble with log2 P xor
//             shuffles per hop.  N = 4 and N = 8 on 16-byte aligned inputs load a row as one / two 16-byte vectors: at N = 4
//             consecutive lanes read consecutive 16 bytes of dist_adj, and the L loads of a channels block (L x 64 bytes per graph)
//             each cover 64 of every L x 64 bytes, the instructions of one wave together every byte of every line.
//   N >= 9    one wave owns one graph, lane i the rows i, i + 64, ... (W = ceil(N / 64) words each).  A block is walked flat, 64
//             consecutive 16-byte positions per load instruction (one-float positions and a wave ballot where N*N % 4 != 0 or the
//             buffer is not 16-byte aligned) and four instructions in flight; the compares' bits go to LDS as the block's N*N-bit
//             stream (N*N / 8 bytes per wave), from which the lane that owns row i reads its N bits with a funnel shift.  The
//             product of hop l reads source row j from its owner with v_readlane (j is wave-uniform) and ORs it into every row that
//             hears j.
// W and P are template arguments, so no private array is indexed dynamically: no private segment, no flat or scratch addressing.
// cm_episode_comm / cm_comm_means are the shared reductions of csrc/cm_stat_rows.hip on rows of four int32: integer sums, every column
// divided by n N, `delivered` (rows::COMM_L_COLS) by n N L.
#include "cm_internal.h"

static_assert(CM_COMM_COLS == 4 && CM_EPC_COLS == CM_COMM_COLS,
              "cm_stat_rows.hip's <int32_t, 4> rows; an episode row has its step rows' columns");

namespace cm {
namespace cs {

typedef unsigned long long u64;
constexpr int TPB = 256, WAVES = TPB / 64, MAX_N = 255, MAX_L = 8, SMALL_N = 8;

template <typename V>
__device__ __forceinline__ V wave_sum(V v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// ---- N <= 8 --------------------------------------------------------------------------------------------------------------------
// the N floats at p -> their "set" bits.  VEC = 4: N % 4 == 0 and p 16-byte aligned
template <int VEC>
__device__ __forceinline__ unsigned row_bits(const float *__restrict__ p, int N) {
    unsigned r = 0u;
    if constexpr (VEC == 4) {
        for (int q = 0; q < N; q += 4) {
            const float4 v = *reinterpret_cast<const float4 *>(p + q);
            const unsigned b = (v.x != 0.0f ? 1u : 0u) | (v.y != 0.0f ? 2u : 0u) | (v.z != 0.0f ? 4u : 0u) | (v.w != 0.0f ? 8u : 0u);
            r |= b << q;
        }
    } else {
        for (int j = 0; j < N; ++j) r |= (p[j] != 0.0f ? 1u : 0u) << j;
    }
    return r;
}

// every lane's row (N bits, at bit i N) of the P lanes that share a graph -> the N x N matrix in one word, on every lane
template <int P>
__device__ __forceinline__ u64 gather_rows(unsigned row, int shift, bool valid) {
    u64 f = valid ? (u64)row << shift : 0ull;
#pragma unroll
    for (int d = 1; d < P; d <<= 1) f |= __shfl_xor(f, d);
    return f;
}

template <int P, int VEC>
__global__ __launch_bounds__(TPB) void comm_stats_small_kernel(int S, int N, int L, const float *__restrict__ adj, long long adj_stride,
                                                               const float *__restrict__ chan, long long chan_stride,
                                                               int32_t *__restrict__ stats) {
    const long long gid = (long long)blockIdx.x * TPB + threadIdx.x;
    const long long s_mine = gid / P;
    const int i = threadIdx.x & (P - 1);
    // lanes past the last graph walk graph S - 1 again (they take part in the shuffles) and store nothing
    const long long s = s_mine < S ? s_mine : (long long)S - 1;
    const bool valid = i < N;
    const int ir = valid ? i : 0;                                   // (a lane without a row reads row 0 and drops it)
    const unsigned full = (1u << N) - 1u, self = 1u << i, others = full & ~self;

    unsigned a = others;
    if (adj != nullptr) a = row_bits<VEC>(adj + s * adj_stride + ir * N, N) & others;
    unsigned x = self, y = self;
    int delivered = 0;
    const float *__restrict__ crow = chan != nullptr ? chan + s * chan_stride + ir * N : nullptr;
    unsigned next = crow != nullptr ? row_bits<VEC>(crow, N) : full;
    for (int l = 0; l < L; ++l) {
        const unsigned m = a & next;
        if (crow != nullptr && l + 1 < L) next = row_bits<VEC>(crow + (size_t)(l + 1) * N * N, N);    // in flight over this hop's product
        delivered += __popc(m);
        if (l == 0) {                                               // X_0 = I: the first hop adds the heard agents themselves
            x |= m;
            y |= a;
        } else {
            const u64 fx = gather_rows<P>(x, i * N, valid), fy = gather_rows<P>(y, i * N, valid);
            unsigned nx = x, ny = y;
            for (int j = 0; j < N; ++j) {
                nx |= (unsigned)(fx >> (j * N)) & (0u - ((m >> j) & 1u));
                ny |= (unsigned)(fy >> (j * N)) & (0u - ((a >> j) & 1u));
            }
            x = nx & full;
            y = ny & full;
        }
    }
    int c0 = valid ? __popc(a) : 0, c1 = valid ? delivered : 0, c2 = valid ? __popc(x) - 1 : 0, c3 = valid ? __popc(y) - 1 : 0;
#pragma unroll
    for (int d = 1; d < P; d <<= 1) {
        c0 += __shfl_xor(c0, d);
        c1 += __shfl_xor(c1, d);
        c2 += __shfl_xor(c2, d);
        c3 += __shfl_xor(c3, d);
    }
    if (s_mine >= S) return;
    int32_t *__restrict__ out = stats + s_mine * CM_COMM_COLS;
    if constexpr (P == 4) {                                         // a wave's 16 graphs: 64 consecutive ints
        int v = c0;
        v = i == 1 ? c1 : v;
        v = i == 2 ? c2 : v;
        v = i == 3 ? c3 : v;
        out[i] = v;
    } else if (i == 0) {
        out[0] = c0;
        out[1] = c1;
        out[2] = c2;
        out[3] = c3;
    }
}

// ---- N >= 9 --------------------------------------------------------------------------------------------------------------------
// bits of word w that name a vertex
__device__ __forceinline__ u64 word_mask(int N, int w) {
    const int left = N - w * 64;
    return left >= 64 ? ~0ull : left > 0 ? (1ull << left) - 1ull : 0ull;
}

// words of a wave's bit stream in LDS: the N*N bits of one block, plus the W + 1 words a row's read may run past them
__host__ __device__ __forceinline__ int stream_words(int N, int W) { return (N * N + 63) / 64 + W + 1; }

// r[p][w] = bits w*64 .. w*64+63 of row p*64 + lane of the N x N block at `a` (NULL: all ones); the diagonal and the bits past N
// clear, rows past N zero.  The block is walked FLAT, 64 consecutive positions per load instruction and UNR instructions in flight
// (VEC = 4: a position is 16 bytes - N*N % 4 == 0 and a 16-byte aligned block; else one float), each float becomes one bit of
// the block's N*N-bit stream in `bits` (LDS, this wave's own words), and the lane that owns row i then reads bits i N .. i N + N - 1
// of the stream: W + 1 words and a funnel shift.  Every wave of the workgroup makes the same calls: the barriers are uniform.
template <int W, int VEC>
__device__ __forceinline__ void load_rows(const float *__restrict__ a, int N, int lane, u64 *__restrict__ bits, u64 (&r)[W][W]) {
#pragma unroll
    for (int p = 0; p < W; ++p)
#pragma unroll
        for (int w = 0; w < W; ++w) r[p][w] = 0ull;
    if (a == nullptr) {
#pragma unroll
        for (int p = 0; p < W; ++p)
#pragma unroll
            for (int w = 0; w < W; ++w)
                if (p * 64 + lane < N) r[p][w] = word_mask(N, w) & ~(w == p ? 1ull << lane : 0ull);
        return;
    }
    const int NN = N * N;
    if constexpr (VEC == 4) {
        constexpr int UNR = 4;
        const int Q = NN / 4;                                       // 16-byte positions
        unsigned char *__restrict__ bytes = reinterpret_cast<unsigned char *>(bits);
        for (int q0 = 0; q0 < Q; q0 += 64 * UNR) {
            float4 v[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u)                           // (a lane past the end reads the last position again and drops it)
                v[u] = *reinterpret_cast<const float4 *>(a + 4 * (size_t)min(q0 + u * 64 + lane, Q - 1));
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                if (q0 + u * 64 >= Q) break;
                const int q = q0 + u * 64 + lane;
                const unsigned nib = q < Q ? (v[u].x != 0.0f ? 1u : 0u) | (v[u].y != 0.0f ? 2u : 0u) | (v[u].z != 0.0f ? 4u : 0u) |
                                                 (v[u].w != 0.0f ? 8u : 0u)
                                           : 0u;
                const unsigned up = __shfl_down(nib, 1);            // the next lane's four bits: an even lane stores eight
                if ((lane & 1) == 0 && q < Q) bytes[q >> 1] = (unsigned char)(nib | (up << 4));
            }
        }
    } else {
        constexpr int UNR = 8;
        const int C = (NN + 63) / 64;                               // stream words
        for (int c0 = 0; c0 < C; c0 += UNR) {
            float v[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) v[u] = a[min((c0 + u) * 64 + lane, NN - 1)];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                if (c0 + u >= C) break;
                const u64 m = __ballot((c0 + u) * 64 + lane < NN && v[u] != 0.0f);
                if (lane == 0) bits[c0 + u] = m;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < W; ++p) {
        const int i = p * 64 + lane;
        if (i < N) {
            const int b0 = i * N, w0 = b0 >> 6, sh = b0 & 63;
            u64 t[W + 1];
#pragma unroll
            for (int w = 0; w <= W; ++w) t[w] = bits[w0 + w];       // (words past the stream are in this wave's range and masked off)
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const u64 word = sh ? (t[w] >> sh) | (t[w + 1] << (64 - sh)) : t[w];
                r[p][w] = word & word_mask(N, w) & ~(w == p ? 1ull << lane : 0ull);
            }
        }
    }
    __syncthreads();                                                // the next block's bits overwrite these
}

__device__ __forceinline__ u64 read_lane(u64 v, int lane) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
    return ((u64)hi << 32) | lo;
}

template <int W, int VEC>
__global__ __launch_bounds__(TPB) void comm_stats_wave_kernel(int S, int N, int L, const float *__restrict__ adj, long long adj_stride,
                                                              const float *__restrict__ chan, long long chan_stride,
                                                              int32_t *__restrict__ stats) {
    extern __shared__ u64 lds_bits[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 *__restrict__ bits = lds_bits + wave * stream_words(N, W);
    const long long s_mine = (long long)blockIdx.x * WAVES + wave;
    // a wave past the last graph of a ragged workgroup walks graph S - 1 again (it meets the same barriers) and stores nothing
    const long long s = s_mine < S ? s_mine : (long long)S - 1;
    u64 a[W][W], m[W][W], x[W][W], y[W][W];
    load_rows<W, VEC>(adj != nullptr ? adj + s * adj_stride : nullptr, N, lane, bits, a);
    int in_range = 0, delivered = 0;
#pragma unroll
    for (int p = 0; p < W; ++p)
#pragma unroll
        for (int w = 0; w < W; ++w) in_range += __popcll(a[p][w]);

    for (int l = 0; l < L; ++l) {
        if (chan != nullptr) {
            load_rows<W, VEC>(chan + s * chan_stride + (size_t)l * N * N, N, lane, bits, m);
#pragma unroll
            for (int p = 0; p < W; ++p)
#pragma unroll
                for (int w = 0; w < W; ++w) m[p][w] &= a[p][w];
        } else {
#pragma unroll
            for (int p = 0; p < W; ++p)
#pragma unroll
                for (int w = 0; w < W; ++w) m[p][w] = a[p][w];
        }
#pragma unroll
        for (int p = 0; p < W; ++p)
#pragma unroll
            for (int w = 0; w < W; ++w) delivered += __popcll(m[p][w]);
        if (l == 0) {                                               // X_0 = I: the first hop adds the heard agents themselves
#pragma unroll
            for (int p = 0; p < W; ++p)
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const u64 me = (w == p && p * 64 + lane < N) ? 1ull << lane : 0ull;
                    x[p][w] = m[p][w] | me;
                    y[p][w] = a[p][w] | me;
                }
            continue;
        }
        u64 nx[W][W], ny[W][W];
#pragma unroll
        for (int p = 0; p < W; ++p)
#pragma unroll
            for (int w = 0; w < W; ++w) {
                nx[p][w] = x[p][w];
                ny[p][w] = y[p][w];
            }
#pragma unroll
        for (int pj = 0; pj < W; ++pj) {                            // source rows j = pj*64 + jj, held by lane jj
            const int lim = min(64, N - pj * 64);
            for (int jj = 0; jj < lim; ++jj) {
                u64 sx[W], sy[W];
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    sx[w] = read_lane(x[pj][w], jj);
                    sy[w] = read_lane(y[pj][w], jj);
                }
#pragma unroll
                for (int p = 0; p < W; ++p) {
                    const u64 hx = 0ull - ((m[p][pj] >> jj) & 1ull), hy = 0ull - ((a[p][pj] >> jj) & 1ull);
#pragma unroll
                    for (int w = 0; w < W; ++w) {
                        nx[p][w] |= sx[w] & hx;
                        ny[p][w] |= sy[w] & hy;
                    }
                }
            }
        }
#pragma unroll
        for (int p = 0; p < W; ++p)
#pragma unroll
            for (int w = 0; w < W; ++w) {
                x[p][w] = nx[p][w];
                y[p][w] = ny[p][w];
            }
    }
    int reach = 0, range_reach = 0;
#pragma unroll
    for (int p = 0; p < W; ++p) {
        if (p * 64 + lane < N) {
            reach -= 1;                                             // (the agent itself)
            range_reach -= 1;
        }
#pragma unroll
        for (int w = 0; w < W; ++w) {
            reach += __popcll(x[p][w]);
            range_reach += __popcll(y[p][w]);
        }
    }
    in_range = wave_sum(in_range);
    delivered = wave_sum(delivered);
    reach = wave_sum(reach);
    range_reach = wave_sum(range_reach);
    int v = in_range;
    v = lane == 1 ? delivered : v;
    v = lane == 2 ? reach : v;
    v = lane == 3 ? range_reach : v;
    if (lane < CM_COMM_COLS && s_mine < S) stats[s_mine * CM_COMM_COLS + lane] = v;
}

struct Args {
    int S, N, L;
    const float *adj;
    long long adj_stride;
    const float *chan;
    long long chan_stride;
    int32_t *stats;
};

// 16-byte loads: every block of both arrays starts on a 16-byte boundary and is a whole number of them (the rows too where a row is
// what a lane loads: N % 4 == 0 implies N*N % 4 == 0)
static bool vec_ok(const Args &g, bool rows = false) {
    return (rows ? g.N % 4 == 0 : g.N * g.N % 4 == 0) && ((uintptr_t)g.adj & 15u) == 0 && ((uintptr_t)g.chan & 15u) == 0 &&
           g.adj_stride % 4 == 0 && g.chan_stride % 4 == 0;
}

template <int P>
static int launch_small(const Args &g, hipStream_t st) {
    const long long lanes = (long long)g.S * P;
    const unsigned grid = (unsigned)((lanes + TPB - 1) / TPB);
    if (vec_ok(g, true))
        hipLaunchKernelGGL((comm_stats_small_kernel<P, 4>), dim3(grid), dim3(TPB), 0, st, g.S, g.N, g.L, g.adj, g.adj_stride, g.chan,
                           g.chan_stride, g.stats);
    else
        hipLaunchKernelGGL((comm_stats_small_kernel<P, 1>), dim3(grid), dim3(TPB), 0, st, g.S, g.N, g.L, g.adj, g.adj_stride, g.chan,
                           g.chan_stride, g.stats);
    CM_HIP(hipGetLastError());
    return CM_OK;
}

template <int W>
static int launch_wave(const Args &g, hipStream_t st) {
    const unsigned grid = (unsigned)(((long long)g.S + WAVES - 1) / WAVES);
    const size_t lds = (size_t)WAVES * stream_words(g.N, W) * sizeof(u64);      // at most 4 x 1022 words: 32 KB
    if (vec_ok(g))
        hipLaunchKernelGGL((comm_stats_wave_kernel<W, 4>), dim3(grid), dim3(TPB), lds, st, g.S, g.N, g.L, g.adj, g.adj_stride, g.chan,
                           g.chan_stride, g.stats);
    else
        hipLaunchKernelGGL((comm_stats_wave_kernel<W, 1>), dim3(grid), dim3(TPB), lds, st, g.S, g.N, g.L, g.adj, g.adj_stride, g.chan,
                           g.chan_stride, g.stats);
    CM_HIP(hipGetLastError());
    return CM_OK;
}

}  // namespace cs
}  // namespace cm

using namespace cm;

extern "C" int cm_comm_stats(int32_t S, int32_t N, int32_t L, const float *dist_adj, int64_t adj_stride, const float *channels,
                             int64_t chan_stride, int32_t *stats, void *stream) {
    if (S < 0 || N < 1 || N > cs::MAX_N) return set_error(CM_ERR_ARG, "cm_comm_stats: S >= 0 and 1 <= n_agents <= 255 required");
    if (L < 1 || L > cs::MAX_L) return set_error(CM_ERR_ARG, "cm_comm_stats: 1 <= n_hops <= 8 required");
    const int64_t a_block = (int64_t)N * N, c_block = (int64_t)L * N * N;
    if (dist_adj && adj_stride != 0 && adj_stride < a_block)
        return set_error(CM_ERR_ARG, "cm_comm_stats: adj_stride must be 0 (one graph for all) or at least N * N");
    if (channels && chan_stride != 0 && chan_stride < c_block)
        return set_error(CM_ERR_ARG, "cm_comm_stats: chan_stride must be 0 (one block for all) or at least L * N * N");
    if (S == 0) return CM_OK;
    if (!stats) return set_error(CM_ERR_ARG, "cm_comm_stats: null stats");
    const cs::Args g{ S, N, L, dist_adj, dist_adj ? adj_stride : 0, channels, channels ? chan_stride : 0, stats };
    const hipStream_t st = (hipStream_t)stream;
    if (N <= cs::SMALL_N) {
        if (N == 1) return cs::launch_small<1>(g, st);
        if (N == 2) return cs::launch_small<2>(g, st);
        if (N <= 4) return cs::launch_small<4>(g, st);
        return cs::launch_small<8>(g, st);
    }
    switch ((N + 63) / 64) {
    case 1: return cs::launch_wave<1>(g, st);
    case 2: return cs::launch_wave<2>(g, st);
    case 3: return cs::launch_wave<3>(g, st);
    default: return cs::launch_wave<4>(g, st);
    }
}

extern "C" int cm_episode_comm(int32_t T, int32_t B, int32_t N, int32_t L, const int32_t *path_len, const int32_t *stats,
                               int32_t group_size, int32_t take, int32_t episodes_per_group, int32_t row0, double *episodes,
                               void *stream) {
    return rows::episode_rows<int32_t, CM_COMM_COLS>("cm_episode_comm", T, B, { N, L, rows::COMM_L_COLS }, path_len, stats, group_size, take,
                                                     episodes_per_group, row0, episodes, stream);
}

extern "C" int cm_comm_means(int32_t K, int32_t E, const double *episodes, double *summary, void *stream) {
    return rows::group_means<CM_COMM_COLS>("cm_comm_means", K, E, episodes, summary, stream);
}
