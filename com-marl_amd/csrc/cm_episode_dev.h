// cm_episode_dev.h - device helpers about an env's FIRST episode of a round, read off path_len [T,B] (an episode ends at the first
// t with path_len[t][b] > 0): its length, and whether it still runs at a step.  Shared by the per-episode reductions
// (cm_episode.hip, cm_stat_rows.hip) and the per-step ones (cm_episode_curves.hip, cm_stat_rows.hip), with the tile rule of the latter.
#pragma once
#include "cm_internal.h"

namespace cm {
namespace ep {

constexpr int SCAN = 32, MAX_TILE = 16, MIN_TILE = 4, MIN_WAVES = 1024;

template <typename V>
__device__ __forceinline__ V wave_sum(V v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// The length of env b's first episode, by a whole wave: n = t + 1 for the first t with path_len[t][b] > 0, else T.  Lane l looks
// at t = l, l + 64, ...; the scan stops at the first round of 64 steps that holds an end, and every lane returns the wave minimum.
__device__ __forceinline__ int episode_len(const int32_t *__restrict__ path_len, int T, int B, size_t b, int lane) {
    int first = T;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        if (t < T && path_len[(size_t)t * B + b] > 0) first = t;
        if (__ballot(first < T) != 0ull) break;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) first = min(first, __shfl_xor(first, d));
    return first < T ? first + 1 : T;
}

// Loads that a lane may have no use for are not branched around (a branch per load makes every load wait for the one before):
// such a lane reads element 0 of the array instead - in bounds, one cache line for all of them - and drops the value.

// does the first episode of env b (valid: the lane has one) still run at step t0?
__device__ __forceinline__ bool running_at(const int32_t *__restrict__ path_len, int B, size_t b, int t0, bool valid) {
    bool run = valid;
    for (int t = 0; t < t0 && __ballot(run) != 0ull; t += SCAN) {
        int32_t e[SCAN];
#pragma unroll
        for (int u = 0; u < SCAN; ++u) e[u] = path_len[(run && t + u < t0) ? (size_t)(t + u) * B + b : (size_t)0];
#pragma unroll
        for (int u = 0; u < SCAN; ++u) run = run & ((t + u >= t0) | (e[u] <= 0));
    }
    return run;
}

// The last step of the tile t0 .. t1-1 at which a lane that runs at t0 still runs, as an offset from t0: that of its first
// path_len > 0, or MAX_TILE when there is none.  One load per row, all in flight.
__device__ __forceinline__ int last_running(const int32_t *__restrict__ path_len, int B, size_t b, int t0, int t1, bool run) {
    int32_t e[MAX_TILE];
#pragma unroll
    for (int u = 0; u < MAX_TILE; ++u) e[u] = path_len[(run && t0 + u < t1) ? (size_t)(t0 + u) * B + b : (size_t)0];
    int last = MAX_TILE;
#pragma unroll
    for (int u = MAX_TILE - 1; u >= 0; --u) last = ((t0 + u < t1) & (e[u] > 0)) ? u : last;
    return last;
}

// steps per wave of a per-step reduction: MAX_TILE where that leaves MIN_WAVES waves, else halved down to MIN_TILE
inline int tile_of(int groups, int T) {
    int tile = MAX_TILE;
    while (tile > MIN_TILE && (long long)groups * ((T + tile - 1) / tile) < MIN_WAVES) tile >>= 1;
    return tile;
}

}  // namespace ep
}  // namespace cm
