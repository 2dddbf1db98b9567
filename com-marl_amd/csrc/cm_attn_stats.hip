// cm_attn_stats.hip - cm_attn_stats, cm_episode_attn, cm_attn_means, cm_attn_curves, cm_attn_curve_means: what the policy did with
// what the channel delivered (gfx950).  cm_attn_stats turns S recorded graphs (attn [N,N] f32, row i = agent i's softmax weights M;
// dist_adj [N,N], channels [L,N,N], f32, "set" = != 0, NULL = ones, the diagonals used as recorded) into CM_ATTN_COLS doubles each:
// self, entropy, range_mass, kept_mass, eff_self, eff_entropy (include/commarl.h).  At hop l the net uses A_l = M * Range * L_l
// renormalised per row (comm_base_net.py:101-103); with K_l = the kept links of hop l and W_l[i] = sum_j M[i][j] K_l[i][j], columns 4
// and 5 are the self weight and the row entropy of A_l[i] / W_l[i] - defined WITHOUT the 1e-12 the net adds to the divisor: a row
// whose kept set is empty adds 0, every other row is divided by W_l[i] itself.
// All arithmetic is f64 on the f32 inputs (the products with the 0 / 1 masks are selects, exact); one log per attention value -
// M ln M is formed once and reused by every hop - and one log per row and hop.  A streaming kernel: every input float is loaded once,
// no atomic.  The decomposition mirrors csrc/cm_comm_stats.hip:
//   N <= 8    P = 1 / 2 / 4 / 8 lanes own one graph (the power of two >= N), lane i its row i.  The row of M stays in registers
//             (P doubles and their P values of M ln M); a row of a mask is N <= 8 bits and the L hops' kept rows share one 64-bit
//             word.  N = 4 and N = 8 on 16-byte aligned inputs load a row as one / two 16-byte vectors.  The six sums meet in
//             log2 P xor shuffles and a graph's 48 output bytes are stored by its own lanes (lane i the columns i, i + P, ...).
//   N >= 9    one wave owns one graph, lane i the rows i, i + 64, ... (W = ceil(N / 64) rows each).  The masks' blocks are walked
//             flat and coalesced, their compares' bits go through LDS as the block's N*N-bit stream, and the lane that owns a
//             row reads its N bits from there (load_rows, as in cm_comm_stats.hip but the diagonal kept); the kept rows of all
//             hops stay in registers (LC x W x W words, LC = 2 / 4 / 8 the hop class), so that the walk over a row of M - by the
//             lane that owns it, 16 floats in flight - feeds the sums of every hop from one value and one log.
// The summation order is fixed by (N, L) alone: a row's terms in ascending j (a position past the row adds +0.0 in both load
// paths), a lane's rows in ascending order with the hops inside, then the xor tree - not by S, the grid or the load width: the
// 16-byte and the one-float paths give the same bits.
// W, P and LC are template arguments, so no private array is indexed dynamically: no private segment.
// cm_episode_attn / cm_attn_means and cm_attn_curves / cm_attn_curve_means are the shared reductions of csrc/cm_stat_rows.hip on rows
// of six doubles: columns 0-2 divided by n N, columns 3-5 (at::L_COLS) by n N L.
#include "cm_internal.h"

namespace cm {
namespace at {

typedef unsigned long long u64;
constexpr int TPB = 256, WAVES = TPB / 64, MAX_N = 255, MAX_L = 8, SMALL_N = 8, COLS = CM_ATTN_COLS;
constexpr unsigned L_COLS = 0b111000u;                              // kept_mass, eff_self, eff_entropy: summed over the hops too
static_assert(CM_ATTN_COLS == 6 && CM_EPA_COLS == CM_ATTN_COLS,
              "cm_stat_rows.hip's <double, 6> rows; an episode row has its step rows' columns");

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__device__ __forceinline__ double m_ln_m(double m) { return m != 0.0 ? m * log(m) : 0.0; }

// one row's share of columns 3, 4, 5 at one hop: W = its kept mass, Sx = its kept sum of M ln M
__device__ __forceinline__ void add_hop(double W, double Sx, double self, bool self_kept, double &kept, double &eff_self,
                                        double &eff_ent) {
    const bool some = W != 0.0;
    const double Ws = some ? W : 1.0;
    kept += W;
    eff_self += (some && self_kept) ? self / Ws : 0.0;
    eff_ent += some ? log(Ws) - Sx / Ws : 0.0;
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

template <int P, int VEC>
__global__ __launch_bounds__(TPB) void attn_stats_small_kernel(int S, int N, int L, const float *__restrict__ attn, long long attn_stride,
                                                               const float *__restrict__ adj, long long adj_stride,
                                                               const float *__restrict__ chan, long long chan_stride,
                                                               double *__restrict__ stats) {
    const long long gid = (long long)blockIdx.x * TPB + threadIdx.x;
    const long long s_mine = gid / P;
    const int i = threadIdx.x & (P - 1);
    // lanes past the last graph walk graph S - 1 again (they take part in the shuffles) and store nothing
    const long long s = s_mine < S ? s_mine : (long long)S - 1;
    const bool valid = i < N;
    const int ir = valid ? i : 0;                                   // (a lane without a row reads row 0 and drops it)
    const unsigned full = (1u << N) - 1u;

    // ---- loads: the row of M, the row of the range mask, the L rows of the channel ----
    const float *__restrict__ mrow = attn + s * attn_stride + ir * N;
    float f[P];
    if constexpr (VEC == 4) {                                       // N == P
#pragma unroll
        for (int q = 0; q < P; q += 4) {
            const float4 v = *reinterpret_cast<const float4 *>(mrow + q);
            f[q] = v.x;
            f[q + 1] = v.y;
            f[q + 2] = v.z;
            f[q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < P; ++j) f[j] = mrow[min(j, N - 1)];     // (a position past the row reads its last entry and drops it)
    }
    unsigned a = full;
    if (adj != nullptr) a = row_bits<VEC>(adj + s * adj_stride + ir * N, N);
    u64 kept_rows = 0ull;                                           // hop l's kept row at bits 8 l .. 8 l + 7
    for (int l = 0; l < L; ++l) {
        const unsigned c = chan != nullptr ? row_bits<VEC>(chan + s * chan_stride + (size_t)l * N * N + ir * N, N) : full;
        kept_rows |= (u64)(a & c) << (8 * l);
    }

    // ---- the row's values: M and M ln M in f64, once ----
    double m[P], e[P];
    double self = 0.0, ent = 0.0, range_mass = 0.0;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        m[j] = (valid && j < N) ? (double)f[j] : 0.0;
        e[j] = m_ln_m(m[j]);
        self = j == i ? m[j] : self;
        ent -= e[j];
        range_mass += ((a >> j) & 1u) ? m[j] : 0.0;
    }
    double kept = 0.0, eff_self = 0.0, eff_ent = 0.0;
    for (int l = 0; l < L; ++l) {
        const unsigned k = (unsigned)(kept_rows >> (8 * l)) & 0xffu;
        double W = 0.0, Sx = 0.0;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const bool on = ((k >> j) & 1u) != 0u;
            W += on ? m[j] : 0.0;
            Sx += on ? e[j] : 0.0;
        }
        add_hop(W, Sx, self, ((k >> i) & 1u) != 0u, kept, eff_self, eff_ent);
    }
    double c[COLS] = { self, ent, range_mass, kept, eff_self, eff_ent };
#pragma unroll
    for (int d = 1; d < P; d <<= 1) {
#pragma unroll
        for (int q = 0; q < COLS; ++q) c[q] += __shfl_xor(c[q], d);
    }
    if (s_mine >= S) return;
    double *__restrict__ out = stats + s_mine * COLS;
#pragma unroll
    for (int q = 0; q < COLS; ++q)                                  // lane i stores the columns i, i + P, ...
        if ((q & (P - 1)) == i) out[q] = c[q];
}

// ---- N >= 9 --------------------------------------------------------------------------------------------------------------------
// bits of word w that name a vertex
__device__ __forceinline__ u64 word_mask(int N, int w) {
    const int left = N - w * 64;
    return left >= 64 ? ~0ull : left > 0 ? (1ull << left) - 1ull : 0ull;
}

// words of a wave's bit stream in LDS: the N*N bits of one block, plus the W + 1 words a row's read may run past them
__host__ __device__ __forceinline__ int stream_words(int N, int W) { return (N * N + 63) / 64 + W + 1; }

// r[p][w] = bits w*64 .. w*64+63 of row p*64 + lane of the N x N block at `a` (NULL: all ones); the bits past N clear, rows past N
// zero, the diagonal as recorded.  The block is walked FLAT, 64 consecutive positions per load instruction and UNR instructions in
// flight (VEC = 4: a position is 16 bytes; else one float), each float becomes one bit of the block's N*N-bit stream in `bits` (LDS,
// this wave's own words), and the lane that owns row i then reads bits i N .. i N + N - 1 of the stream: W + 1 words and a funnel
// shift.  Every wave of the workgroup makes the same calls: the barriers are uniform.
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
                if (p * 64 + lane < N) r[p][w] = word_mask(N, w);
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
                r[p][w] = word & word_mask(N, w);
            }
        }
    }
    __syncthreads();                                                // the next block's bits overwrite these
}

constexpr int BATCH = 16;                                           // floats of a row of M in flight per lane

// Row PR*64 + lane of the block of M at `block`, walked by the lane that owns it, BATCH floats in flight: its share of the six
// columns onto c.  a / k: the lane's rows of the range mask and of the hops' kept links.  PR is a template argument: every index of
// a, k and the per-hop sums is a compile-time constant.
template <int W, int LC, int VEC, int PR>
__device__ __forceinline__ void add_row(const float *__restrict__ block, int N, int lane, const u64 (&a)[W][W], const u64 (&k)[LC][W][W],
                                        double (&c)[COLS]) {
    const int i = PR * 64 + lane;
    const bool valid = i < N;
    const float *__restrict__ row = block + (size_t)(valid ? i : 0) * N;           // (a lane without a row reads row 0 and drops it)
    double self = 0.0, ent = 0.0, range_mass = 0.0, Wl[LC], Sl[LC];
#pragma unroll
    for (int l = 0; l < LC; ++l) Wl[l] = Sl[l] = 0.0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const int lim = min(64, N - w * 64);                        // the row's entries in word w (uniform)
        u64 aw = a[PR][w], kw[LC];
#pragma unroll
        for (int l = 0; l < LC; ++l) kw[l] = k[l][PR][w];
        for (int j0 = 0; j0 < lim; j0 += BATCH) {
            float f[BATCH];
            const int base = w * 64 + j0;
            if constexpr (VEC == 4) {
#pragma unroll
                for (int u = 0; u < BATCH; u += 4) {                // (a position past the row reads its last one again and drops it)
                    const float4 v = *reinterpret_cast<const float4 *>(row + min(base + u, N - 4));
                    f[u] = v.x;
                    f[u + 1] = v.y;
                    f[u + 2] = v.z;
                    f[u + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int u = 0; u < BATCH; ++u) f[u] = row[min(base + u, N - 1)];
            }
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const double m = (valid && j0 + u < lim) ? (double)f[u] : 0.0;
                const double e = m_ln_m(m);
                self = base + u == i ? m : self;
                ent -= e;
                range_mass += ((aw >> u) & 1ull) ? m : 0.0;
#pragma unroll
                for (int l = 0; l < LC; ++l) {
                    const bool on = ((kw[l] >> u) & 1ull) != 0ull;
                    Wl[l] += on ? m : 0.0;
                    Sl[l] += on ? e : 0.0;
                }
            }
            aw >>= BATCH;
#pragma unroll
            for (int l = 0; l < LC; ++l) kw[l] >>= BATCH;
        }
    }
    c[0] += self;
    c[1] += ent;
    c[2] += range_mass;
#pragma unroll
    for (int l = 0; l < LC; ++l) add_hop(Wl[l], Sl[l], self, ((k[l][PR][PR] >> lane) & 1ull) != 0ull, c[3], c[4], c[5]);
}

// LC: the hop class (L <= LC); VEC = 4: N % 4 == 0, every block 16-byte aligned
template <int W, int LC, int VEC>
__global__ __launch_bounds__(TPB) void attn_stats_wave_kernel(int S, int N, int L, const float *__restrict__ attn, long long attn_stride,
                                                              const float *__restrict__ adj, long long adj_stride,
                                                              const float *__restrict__ chan, long long chan_stride,
                                                              double *__restrict__ stats) {
    extern __shared__ u64 lds_bits[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 *__restrict__ bits = lds_bits + wave * stream_words(N, W);
    const long long s_mine = (long long)blockIdx.x * WAVES + wave;
    // a wave past the last graph of a ragged workgroup walks graph S - 1 again (it meets the same barriers) and stores nothing
    const long long s = s_mine < S ? s_mine : (long long)S - 1;
    u64 a[W][W], k[LC][W][W];
    load_rows<W, VEC>(adj != nullptr ? adj + s * adj_stride : nullptr, N, lane, bits, a);
#pragma unroll
    for (int l = 0; l < LC; ++l) {
        if (l < L && chan != nullptr) {                             // (uniform over the workgroup)
            load_rows<W, VEC>(chan + s * chan_stride + (size_t)l * N * N, N, lane, bits, k[l]);
#pragma unroll
            for (int p = 0; p < W; ++p)
#pragma unroll
                for (int w = 0; w < W; ++w) k[l][p][w] &= a[p][w];
        } else {
#pragma unroll
            for (int p = 0; p < W; ++p)
#pragma unroll
                for (int w = 0; w < W; ++w) k[l][p][w] = l < L ? a[p][w] : 0ull;     // (a hop past L keeps nothing and adds 0)
        }
    }

    const float *__restrict__ block = attn + s * attn_stride;
    double c[COLS];
#pragma unroll
    for (int q = 0; q < COLS; ++q) c[q] = 0.0;
    add_row<W, LC, VEC, 0>(block, N, lane, a, k, c);
    if constexpr (W > 1) add_row<W, LC, VEC, 1>(block, N, lane, a, k, c);
    if constexpr (W > 2) add_row<W, LC, VEC, 2>(block, N, lane, a, k, c);
    if constexpr (W > 3) add_row<W, LC, VEC, 3>(block, N, lane, a, k, c);
    double c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], c4 = c[4], c5 = c[5];
    c0 = wave_sum(c0);
    c1 = wave_sum(c1);
    c2 = wave_sum(c2);
    c3 = wave_sum(c3);
    c4 = wave_sum(c4);
    c5 = wave_sum(c5);
    double v = c0;
    v = lane == 1 ? c1 : v;
    v = lane == 2 ? c2 : v;
    v = lane == 3 ? c3 : v;
    v = lane == 4 ? c4 : v;
    v = lane == 5 ? c5 : v;
    if (lane < COLS && s_mine < S) stats[s_mine * COLS + lane] = v;
}

struct Args {
    int S, N, L;
    const float *attn;
    long long attn_stride;
    const float *adj;
    long long adj_stride;
    const float *chan;
    long long chan_stride;
    double *stats;
};

// 16-byte loads: a row is a whole number of them and every block of the three arrays starts on a 16-byte boundary
static bool vec_ok(const Args &g) {
    return g.N % 4 == 0 && (((uintptr_t)g.attn | (uintptr_t)g.adj | (uintptr_t)g.chan) & 15u) == 0 && g.attn_stride % 4 == 0 &&
           g.adj_stride % 4 == 0 && g.chan_stride % 4 == 0;
}

#define CM_ATTN_LAUNCH(kernel, grid, lds)                                                                                          \
    hipLaunchKernelGGL((kernel), dim3(grid), dim3(TPB), lds, st, g.S, g.N, g.L, g.attn, g.attn_stride, g.adj, g.adj_stride, g.chan, \
                       g.chan_stride, g.stats)

template <int P>
static int launch_small(const Args &g, hipStream_t st) {
    const long long lanes = (long long)g.S * P;
    const unsigned grid = (unsigned)((lanes + TPB - 1) / TPB);
    if (vec_ok(g))
        CM_ATTN_LAUNCH((attn_stats_small_kernel<P, P >= 4 ? 4 : 1>), grid, 0);
    else
        CM_ATTN_LAUNCH((attn_stats_small_kernel<P, 1>), grid, 0);
    CM_HIP(hipGetLastError());
    return CM_OK;
}

template <int W, int LC>
static int launch_wave_hops(const Args &g, hipStream_t st) {
    const unsigned grid = (unsigned)(((long long)g.S + WAVES - 1) / WAVES);
    const size_t lds = (size_t)WAVES * stream_words(g.N, W) * sizeof(u64);      // at most 4 x 1022 words: 32 KB
    if (vec_ok(g))
        CM_ATTN_LAUNCH((attn_stats_wave_kernel<W, LC, 4>), grid, lds);
    else
        CM_ATTN_LAUNCH((attn_stats_wave_kernel<W, LC, 1>), grid, lds);
    CM_HIP(hipGetLastError());
    return CM_OK;
}

template <int W>
static int launch_wave(const Args &g, hipStream_t st) {
    if (g.L <= 2) return launch_wave_hops<W, 2>(g, st);
    if (g.L <= 4) return launch_wave_hops<W, 4>(g, st);
    return launch_wave_hops<W, 8>(g, st);
}

}  // namespace at
}  // namespace cm

using namespace cm;

extern "C" int cm_attn_stats(int32_t S, int32_t N, int32_t L, const float *attn, int64_t attn_stride, const float *dist_adj,
                             int64_t adj_stride, const float *channels, int64_t chan_stride, double *stats, void *stream) {
    if (S < 0 || N < 1 || N > at::MAX_N) return set_error(CM_ERR_ARG, "cm_attn_stats: S >= 0 and 1 <= n_agents <= 255 required");
    if (L < 1 || L > at::MAX_L) return set_error(CM_ERR_ARG, "cm_attn_stats: 1 <= n_hops <= 8 required");
    const int64_t a_block = (int64_t)N * N, c_block = (int64_t)L * N * N;
    if (attn_stride < a_block) return set_error(CM_ERR_ARG, "cm_attn_stats: attn_stride must be at least N * N");
    if (dist_adj && adj_stride != 0 && adj_stride < a_block)
        return set_error(CM_ERR_ARG, "cm_attn_stats: adj_stride must be 0 (one graph for all) or at least N * N");
    if (channels && chan_stride != 0 && chan_stride < c_block)
        return set_error(CM_ERR_ARG, "cm_attn_stats: chan_stride must be 0 (one block for all) or at least L * N * N");
    if (S == 0) return CM_OK;
    if (!attn || !stats) return set_error(CM_ERR_ARG, "cm_attn_stats: null attn or stats");
    const at::Args g{ S, N, L, attn, attn_stride, dist_adj, dist_adj ? adj_stride : 0, channels, channels ? chan_stride : 0, stats };
    const hipStream_t st = (hipStream_t)stream;
    if (N <= at::SMALL_N) {
        if (N == 1) return at::launch_small<1>(g, st);
        if (N == 2) return at::launch_small<2>(g, st);
        if (N <= 4) return at::launch_small<4>(g, st);
        return at::launch_small<8>(g, st);
    }
    switch ((N + 63) / 64) {
    case 1: return at::launch_wave<1>(g, st);
    case 2: return at::launch_wave<2>(g, st);
    case 3: return at::launch_wave<3>(g, st);
    default: return at::launch_wave<4>(g, st);
    }
}

extern "C" int cm_episode_attn(int32_t T, int32_t B, int32_t N, int32_t L, const int32_t *path_len, const double *stats,
                               int32_t group_size, int32_t take, int32_t episodes_per_group, int32_t row0, double *episodes,
                               void *stream) {
    return rows::episode_rows<double, CM_ATTN_COLS>("cm_episode_attn", T, B, { N, L, at::L_COLS }, path_len, stats,
                                   group_size, take, episodes_per_group, row0, episodes, stream);
}

extern "C" int cm_attn_means(int32_t K, int32_t E, const double *episodes, double *summary, void *stream) {
    return rows::group_means<CM_ATTN_COLS>("cm_attn_means", K, E, episodes, summary, stream);
}

extern "C" int cm_attn_curves(int32_t T, int32_t B, int32_t N, int32_t L, const int32_t *path_len, const double *stats,
                              int32_t group_size, int32_t take, int32_t accumulate, double *sums, void *stream) {
    return rows::curve_sums<double, CM_ATTN_COLS>("cm_attn_curves", T, B, { N, L, at::L_COLS }, path_len, stats,
                                   group_size, take, accumulate, sums, stream);
}

extern "C" int cm_attn_curve_means(int32_t cells, int32_t T, int32_t n_episodes, int32_t N, int32_t L, const double *sums,
                                   double *curves, void *stream) {
    return rows::curve_means<CM_ATTN_COLS>("cm_attn_curve_means", cells, T, n_episodes, { N, L, at::L_COLS }, sums, curves, stream);
}
