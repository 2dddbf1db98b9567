// cm_rollout_w_dev.h - what the wave-owned rollout kernels of teams of 4 share besides their step loop (cm_rollout_w_body.h):
// rollout_w_kernel (cm_rollout_w.hip, one weight image per launch) and rollout_wm_kernel (cm_rollout_wm.hip, a workgroup picks its
// policy's image at entry).  Both translation units are built with -fno-slp-vectorize (Makefile).
#pragma once
#include "cm_env_dev.h"
#include "cm_env_pp10_dev.h"
#include "cm_policy_w_dev.h"

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

// host: how a launch of the wave-owned rollout runs (cm_rollout_w.hip: plan_rollout_w)
struct RolloutWPlan {
    size_t lds;                                          // dynamic LDS bytes: policy image | actions | 16 env areas
    int blocks;                                          // workgroups of 16 envs
    StridesW c;
    TailW tl;
    bool pre, full, carry, map10;                        // env prefetch / every workgroup full / carried form / its map-10 shape build
};
int plan_rollout_w(const mf::FwdArgs &a, const cm_env *h, bool use_tape, const ChunkArgs *chunk, RolloutWPlan &pl);
bool shape_ok_rollout_w(int N, int d, int L, int n_act);   // cm_rollout_w.hip: teams of 4 on the wave-owned kernel, where enabled

}  // namespace cm
