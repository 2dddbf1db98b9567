// cm_rollout_w_dev.h - what the wave-owned rollout kernels of teams of 4 share besides their step loop (cm_rollout_w_body.h):
// rollout_w_kernel (cm_rollout_w.hip, one weight image per launch), rollout_wm_kernel (cm_rollout_wm.hip, a workgroup picks its
// policy's image at entry) and their twins for a handle with per-env comm conditions (cm_rollout_wc.hip).  The three translation
// units are built with -fno-slp-vectorize (Makefile).
#pragma once
#include <stdio.h>

#include <type_traits>

#include "cm_env_dev.h"
#include "cm_env_pp10_dev.h"
#include "cm_policy_host.h"

namespace cm {

// diagnostic (COMMARL_ENV_STOP=-2): shader clocks of workgroup 0 / thread 0, summed over the launch's steps: [0] steps, [1] policy
// tile, [2] env phase, [3] weight staging
static __device__ unsigned long long g_w_probe[5];

// ---- teams of 4, wave-owned rows (cm_policy_w_dev.h): a workgroup = 16 envs = four waves, ONE per SIMD; a wave carries its four
// envs through policy forward, sample AND env step by itself - the actions go through LDS words only that wave touches, the env
// phase's 16-lane groups are the wave's own envs - so no workgroup barrier exists after the one behind the weight staging, and
// with n_steps > 1 the wave simply loops (weights stay where they are: LDS image + the register-resident 128 -> 64 layer).
// LDS: [policy image | 64 actions | 16 env areas].
// Scalar registers are the scarce resource of this kernel (every kernel argument lives in SGPRs for the whole step loop; what does not
// fit is spilled to VGPR lanes and comes back through v_readlane): the per-step strides travel as 32-bit element counts and the
// RNG tape - test-only, single-step launches - is a compile-time variant.
// folded chunk tail (CARRY builds): after its last step a wave writes its envs' next observation into slot 0 and takes a ticket;
// the wave that takes the last one advances the sampler's Philox base - every other wave has read it for the last time
struct TailW { float *obs_dst; uint32_t *base; unsigned int *ticket; int on; };
struct StridesW { int n_steps, obs, actions, probs, attn, reward, reward_f64, done, details, dist_adj, channels, prey_alive, success, path_len; };

namespace mw {
// the policy set as rollout_wm_kernel / rollout_wcm_kernel see it: read at entry only, so nothing of it stays live through the step
// loop but n_act (as WeightsW)
struct PolicySetW {
    const float *const *packs;                           // [K] cm_policy_pack() outputs
    const int32_t *wg_policy;                            // [n_wg] policy of each workgroup
    int wave_off;                                        // bytes from a pack's start to its wave-owned section (one shape: one offset)
    int n_act;
};
}  // namespace mw

// ---- host: what the rollout entry points share (cm_fused.hip: cm_rollout_step / _chunk / _chunk_tail; cm_rollout_wm.hip:
// cm_rollout_chunk_multi), besides cm_policy_host.h.  The helpers defined here are static: the library exports every external symbol,
// and these are not ABI ----
// handle, weights and buffers are there and of one shape; `who` (the entry point) opens the error text
static inline int check_rollout_args(const char *who, const cm_env *h, const cm_policy_weights *w, const void *obs, const cm_step_out *out) {
    if (!h || !w || !obs || !out) return set_error(CM_ERR_ARG, std::string(who) + ": null argument");
    if (w->n_agents != h->dev.N || w->d != h->dev.d || w->n_hops != h->dev.L)
        return set_error(CM_ERR_ARG, std::string(who) + ": policy shape (n_agents, d, n_hops) does not match the env handle");
    return CM_OK;
}
// the multi-step forms: strides, at least min_steps (0 or 1) steps, and no RNG tape
static inline int check_chunk_args(const char *who, const cm_env *h, const cm_chunk_strides *st, int n_steps, int min_steps) {
    if (!st) return set_error(CM_ERR_ARG, std::string(who) + ": null strides");
    if (n_steps < min_steps) return set_error(CM_ERR_ARG, std::string(who) + (min_steps ? ": at least one step" : ": negative step count"));
    if (h && h->cfg.rng_mode == CM_RNG_TAPE) return set_error(CM_ERR_ARG, std::string(who) + ": tape mode steps one launch at a time");
    return CM_OK;
}

// diagnostic (COMMARL_ENV_STOP < 0): phase clocks of workgroup 0's env phase (ENV_PROBE, cm_env_dev.h).  The caller passes
// HIP_SYMBOL(g_env_probe): the array is each translation unit's own, and a unit that never names it on the host side keeps no
// stores to it in its kernels
static void env_probe_dump(const char *tag, const void *probe, void *stream) {
    unsigned long long hp[16];
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return;
    if (hipMemcpyFromSymbol(hp, probe, sizeof(hp), 0, hipMemcpyDeviceToHost) != hipSuccess) return;
    fprintf(stderr, "[%s env probe] clk since env entry:", tag);
    for (int i = 1; i < 10; ++i) fprintf(stderr, " p%d=%lld", i, (long long)(hp[i] - hp[0]));
    fprintf(stderr, "\n");
}

// ---- host: how a launch of the wave-owned rollout runs (cm_rollout_w.hip: plan_rollout_w) ----
struct RolloutWPlan {
    int n_act;                                           // in: the policy's action count and the launch's outputs (what map10 folds)
    const cm_step_out *out;
    size_t lds;                                          // dynamic LDS bytes: policy image | actions | 16 env areas
    int blocks;                                          // workgroups of 16 envs
    StridesW c;
    TailW tl;
    bool pre, full, carry, map10;                        // env prefetch / every workgroup full / carried form / its map-10 shape build
    bool probes;                                         // map10 under COMMARL_ENV_STOP < 0: the build that has the diagnostic clocks
};
int plan_rollout_w(const mf::FwdArgs &a, const cm_env *h, bool use_tape, const ChunkArgs *chunk, RolloutWPlan &pl);
// cm_rollout_w.hip: single step, or a persistent chunk; 1 = not available for this handle
int launch_rollout_w(mf::FwdArgs a, const cm_policy_weights *w, const void *w_pack, const cm_env *h, const cm_rng_tape &t, const cm_step_out &out,
                     void *stream, const ChunkArgs *chunk);
// cm_rollout_wc.hip: the same for a handle with a condition table (cm_env_set_conditions) - rollout_wc_kernel with one weight image
// (`set` NULL), rollout_wcm_kernel with a policy set; 1 = not available for this handle
int launch_rollout_wc(mf::FwdArgs a, const cm_policy_weights *w, const void *w_pack, const cm_policy_set *set, const cm_env *h,
                      const cm_step_out &out, void *stream, const ChunkArgs *chunk);

// The one ladder from a plan to a build of a wave-owned kernel: f(LHOPS, PRE, FULLWG, TAPE, CARRY, SHAPE), each a
// std::integral_constant.  Per hop count: the tape variant, and {plain, env prefetch, carried, carried map10} x {ragged, full}.
// What f does with its kernel: launch_lds (cm_internal.h) on pl.blocks workgroups of 256 lanes with pl.lds bytes of LDS.
template <class F>
static int for_rollout_w_variant(int L, bool use_tape, const RolloutWPlan &pl, F &&f) {
    using T = std::true_type;
    using N = std::false_type;
    using S0 = std::integral_constant<int, 0>;
    auto hops = [&](auto LH) {
        auto fill = [&](auto PR, auto CA, auto SH) { return pl.full ? f(LH, PR, T{}, N{}, CA, SH) : f(LH, PR, N{}, N{}, CA, SH); };
        if (use_tape) return f(LH, N{}, N{}, T{}, N{}, S0{});
        if (pl.carry) return pl.map10 ? fill(T{}, T{}, std::integral_constant<int, 1>{}) : fill(T{}, T{}, S0{});
        return pl.pre ? fill(T{}, N{}, S0{}) : fill(N{}, N{}, S0{});
    };
    return L == 1 ? hops(std::integral_constant<int, 1>{}) : hops(std::integral_constant<int, 2>{});
}

}  // namespace cm
