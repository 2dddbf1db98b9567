// cm_boot.hip - cm_boot_means, cm_boot_quantiles: bootstrap intervals and paired contrasts of the evaluation scores (gfx950).  The
// episode tables [cells, n, cols] of doubles the reductions of cm_episode.hip / cm_stat_rows.hip fill are resampled over the
// episodes on the device (include/commarl.h):
//   boot_means      one lane per resample r, one workgroup per cell and block of TPB resamples.  The lane draws its n row indices from
//                   Philox (counter (r, j / 4, SITE_BOOT, 0): four draws a call, the stream a function of (seed, r, j) alone - every
//                   cell, column and table sees the same resamples) and sums the cols columns of the drawn rows in registers, j
//                   ascending, then divides once.  The cell's table is staged in LDS when it fits STAGE_BYTES - every lane reads
//                   rows scattered over it, n * cols reads a lane - and read from global memory otherwise: the same sums in the
//                   same order, the same bits.
//   boot_quantiles  one workgroup per (cell, key): the key's R values (minus the reference cell's for a contrast) into an LDS tile
//                   padded with +inf to a power of two; the sum, the sum of squared distances to the mean and the two counts by
//                   lane-strided partial sums in ascending r, the xor tree, then the waves' partials in wave order; a bitonic
//                   network sorts the tile; thread 0 writes the four doubles.
// A key is computed from the columns it needs, loaded one by one under the (workgroup-uniform) switch on the key: no private array,
// no dynamic index, no private segment.  No atomics, one writer per output, the same inputs give the same bits.
#include "cm_internal.h"
#include "cm_rng.h"

#include <cmath>
#include <cstdlib>

static_assert(CM_BOOT_OUT == 4, "lo, hi, se, p_gt");

namespace cm {
namespace boot {

constexpr int TPB = 256, WAVES = TPB / 64;
// the staging budget of boot_means: 32 KB of the CU's 160 KB LDS - four workgroups' tiles a CU, and 100 episodes x 9 columns
// (7200 bytes) fit with room to spare.  A table of 9 columns is staged up to n = 455 episodes.
constexpr int STAGE_BYTES = 32 * 1024;
constexpr int MAX_R = CM_BOOT_MAX_R;            // the sort's tile: 4096 doubles = 32 KB

template <int COLS, bool STAGED>
__global__ __launch_bounds__(TPB) void boot_means_kernel(int n, int R, int blocks_per_cell, const double *__restrict__ table,
                                                         uint32_t seed_lo, uint32_t seed_hi, double *__restrict__ means) {
    __shared__ double tile[STAGED ? STAGE_BYTES / 8 : 1];
    const int g = blockIdx.x / blocks_per_cell;
    const int r = (blockIdx.x - g * blocks_per_cell) * TPB + threadIdx.x;
    const double *__restrict__ rows = table + (size_t)g * n * COLS;
    if constexpr (STAGED) {                                     // (the host launches this form only when n * COLS * 8 <= STAGE_BYTES)
        for (int i = threadIdx.x; i < n * COLS; i += TPB) tile[i] = rows[i];
        __syncthreads();
    }
    if (r >= R) return;
    double s[COLS];
#pragma unroll
    for (int c = 0; c < COLS; ++c) s[c] = 0.0;
    for (int j0 = 0; j0 < n; j0 += 4) {                         // (n is uniform: so is every branch below)
        const u32x4 w = philox4x32_10((uint32_t)r, (uint32_t)(j0 >> 2), SITE_BOOT, 0u, seed_lo, seed_hi);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (j0 + u >= n) break;
            const uint32_t wj = u == 0 ? w.x : u == 1 ? w.y : u == 2 ? w.z : w.w;
            const uint32_t idx = (uint32_t)(((uint64_t)wj * (uint64_t)(uint32_t)n) >> 32);      // < n
#pragma unroll
            for (int c = 0; c < COLS; ++c) {
                if constexpr (STAGED)
                    s[c] += tile[idx * COLS + c];
                else
                    s[c] += rows[(size_t)idx * COLS + c];
            }
        }
    }
    double *__restrict__ out = means + ((size_t)g * R + r) * COLS;
    const double dn = (double)n;
#pragma unroll
    for (int c = 0; c < COLS; ++c) out[c] = s[c] / dn;
}

// ---- the keys: what evaluate.py's _named / _comm_keys / _value_keys / _explained do on the point estimates, operation by operation ----
__device__ __forceinline__ double key_of(int kind, int k, const double *__restrict__ m) {
    if (kind == CM_BOOT_COMM && k == 4) {                       // delivery = heard_degree / range_degree, 1.0 where nobody is in range
        const double range = m[0], heard = m[1];
        return range != 0.0 ? heard / range : 1.0;
    }
    if (kind == CM_BOOT_VALUE) {
        if (k < 2) return m[k];
        if (k >= 5) return m[k - 1];                            // msg_value, loss_value
        if (k == 3) return sqrt(m[2]);                          // value_rmse
        const double mean = m[0], ret = m[1];
        const double bias = mean - ret;
        if (k == 2) return bias;
        const double sq_err = m[2], ret_sq = m[3];              // value_ev (_explained)
        const double resid = sq_err - bias * bias, var = ret_sq - ret * ret;
        const double eps = 1e-12 * ((ret_sq > 1.0 || ret_sq != ret_sq) ? ret_sq : 1.0);        // np.maximum(1.0, ret_sq): a NaN stays
        if (var <= eps) return resid <= eps ? 1.0 : 0.0;
        return 1.0 - resid / var;
    }
    return m[k];                                                // a column
}

// the workgroup's total of one double per thread: the xor tree per wave, then the waves' totals in wave order; every thread returns it
__device__ __forceinline__ double block_sum(double v, double *__restrict__ part) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    __syncthreads();                                            // (part may still be read from the call before)
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = part[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s += part[w];
    return s;
}

__global__ __launch_bounds__(TPB) void boot_quantiles_kernel(int kind, int cells, int R, int P, int cols, int keys,
                                                             const double *__restrict__ means, const int32_t *__restrict__ ref_cell,
                                                             int lo_rank, int hi_rank, double *__restrict__ out) {
    __shared__ double v[MAX_R];
    __shared__ double part[WAVES];
    const int g = blockIdx.x / keys, k = blockIdx.x - g * keys;
    int ref = -1;
    if (ref_cell) {
        ref = ref_cell[g];
        ref = (ref < 0 || ref >= cells) ? g : ref;              // (the caller checks the table; never out of bounds)
    }
    const double *__restrict__ mine = means + (size_t)g * R * cols;
    const double *__restrict__ other = means + (size_t)(ref < 0 ? g : ref) * R * cols;

    // ---- the values, r ascending per thread; the tile's padding ----
    double sum = 0.0;
    int gt = 0, eq = 0;
    for (int r = threadIdx.x; r < P; r += TPB) {
        double x = INFINITY;
        if (r < R) {
            x = key_of(kind, k, mine + (size_t)r * cols);
            if (ref >= 0) x = x - key_of(kind, k, other + (size_t)r * cols);
            sum += x;
            gt += x > 0.0 ? 1 : 0;
            eq += x == 0.0 ? 1 : 0;
        }
        v[r] = x;
    }
    const double mean = block_sum(sum, part) / (double)R;
    double sq = 0.0;
    for (int r = threadIdx.x; r < R; r += TPB) {                // (each thread reads back what it wrote)
        const double d = v[r] - mean;
        sq += d * d;
    }
    const double ss = block_sum(sq, part);
    // the counts: exact in a double (<= 4096), through the same tree
    const double n_gt = block_sum((double)gt, part), n_eq = block_sum((double)eq, part);

    // ---- bitonic sort of the P values, ascending ----
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < (P >> 1); t += TPB) {        // pair t: i without the stride's bit, j = i with it (< P)
                const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), j = i | stride;
                const double a = v[i], b = v[j];
                const bool up = (i & size) == 0;
                if (up ? a > b : a < b) {
                    v[i] = b;
                    v[j] = a;
                }
            }
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) {
        double *__restrict__ o = out + ((size_t)g * keys + k) * CM_BOOT_OUT;
        o[0] = v[lo_rank];
        o[1] = v[hi_rank];
        o[2] = sqrt(ss / (double)(R - 1));
        o[3] = (n_gt + 0.5 * n_eq) / (double)R;
    }
}

static int refuse(const char *who, const char *what) { return set_error(CM_ERR_ARG, std::string(who) + ": " + what); }

// the staging budget in force: STAGE_BYTES, or what COMMARL_BOOT_STAGE_BYTES lowers it to (read at every call: a debugging switch)
static long stage_budget() {
    const char *e = getenv("COMMARL_BOOT_STAGE_BYTES");
    if (!e || !*e) return STAGE_BYTES;
    const long v = strtol(e, nullptr, 10);
    return v < 0 ? 0 : v > STAGE_BYTES ? STAGE_BYTES : v;
}

template <int COLS>
static int means(int cells, int n, const double *table, int R, uint32_t seed_lo, uint32_t seed_hi, double *out, void *stream) {
    const int blocks_per_cell = (R + TPB - 1) / TPB;
    const long long grid = (long long)cells * blocks_per_cell;
    if (grid > INT32_MAX) return refuse("cm_boot_means", "too many (cell, resample block) pairs for one launch");
    const bool staged = (long long)n * COLS * 8 <= stage_budget();
    if (staged)
        hipLaunchKernelGGL((boot_means_kernel<COLS, true>), dim3((unsigned)grid), dim3(TPB), 0, (hipStream_t)stream, n, R, blocks_per_cell,
                           table, seed_lo, seed_hi, out);
    else
        hipLaunchKernelGGL((boot_means_kernel<COLS, false>), dim3((unsigned)grid), dim3(TPB), 0, (hipStream_t)stream, n, R, blocks_per_cell,
                           table, seed_lo, seed_hi, out);
    CM_HIP(hipGetLastError());
    return CM_OK;
}

}  // namespace boot
}  // namespace cm

using namespace cm;

extern "C" int cm_boot_means(int32_t cells, int32_t n, int32_t cols, const double *table, int32_t R, uint32_t seed_lo, uint32_t seed_hi,
                             double *means, void *stream) {
    const char *who = "cm_boot_means";
    if (cells < 1 || n < 1) return boot::refuse(who, "cells >= 1 and n >= 1 required");
    if (cols != 4 && cols != 6 && cols != 9) return boot::refuse(who, "cols must be 4, 6 or 9");
    if (R < 2 || R > boot::MAX_R) return boot::refuse(who, "2 <= R <= 4096 required");
    if (!table || !means) return boot::refuse(who, "null argument");
    if (cols == 4) return boot::means<4>(cells, n, table, R, seed_lo, seed_hi, means, stream);
    if (cols == 6) return boot::means<6>(cells, n, table, R, seed_lo, seed_hi, means, stream);
    return boot::means<9>(cells, n, table, R, seed_lo, seed_hi, means, stream);
}

extern "C" int cm_boot_quantiles(int32_t kind, int32_t cells, int32_t R, int32_t cols, const double *means, const int32_t *ref_cell,
                                 int32_t lo_rank, int32_t hi_rank, double *out, void *stream) {
    const char *who = "cm_boot_quantiles";
    int keys;
    if (kind == CM_BOOT_COLUMNS) {
        if (cols != 4 && cols != 6 && cols != 9) return boot::refuse(who, "CM_BOOT_COLUMNS: cols must be 4, 6 or 9");
        keys = cols;
    } else if (kind == CM_BOOT_COMM) {
        if (cols != 4) return boot::refuse(who, "CM_BOOT_COMM: cols must be 4");
        keys = 5;
    } else if (kind == CM_BOOT_VALUE) {
        if (cols != 6) return boot::refuse(who, "CM_BOOT_VALUE: cols must be 6");
        keys = 7;
    } else {
        return boot::refuse(who, "kind must be CM_BOOT_COLUMNS, CM_BOOT_COMM or CM_BOOT_VALUE");
    }
    if (cells < 1) return boot::refuse(who, "cells >= 1 required");
    if (R < 2 || R > boot::MAX_R) return boot::refuse(who, "2 <= R <= 4096 required");
    if (lo_rank < 0 || lo_rank > hi_rank || hi_rank >= R) return boot::refuse(who, "0 <= lo_rank <= hi_rank < R required");
    if (!means || !out) return boot::refuse(who, "null argument");
    const long long grid = (long long)cells * keys;
    if (grid > INT32_MAX) return boot::refuse(who, "too many (cell, key) pairs for one launch");
    int P = 2;
    while (P < R) P <<= 1;                                      // <= 4096
    hipLaunchKernelGGL(boot::boot_quantiles_kernel, dim3((unsigned)grid), dim3(boot::TPB), 0, (hipStream_t)stream, kind, cells, R, P, cols,
                       keys, means, ref_cell, lo_rank, hi_rank, out);
    CM_HIP(hipGetLastError());
    return CM_OK;
}
