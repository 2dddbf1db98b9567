// cm_rollout_wc.hip - the wave-owned rollout of teams of 4 for a handle with PER-ENV COMM CONDITIONS (cm_env_set_conditions, switched
// on per handle by cm_env_fuse_conditions): the twins of rollout_w_kernel (cm_rollout_w.hip, one weight image per launch) and
// rollout_wm_kernel (cm_rollout_wm.hip, a workgroup picks its policy's pack at entry) with one more argument, the handle's device
// table of one 32-byte record per env.  The step loop is theirs (cm_rollout_w_body.h, COND): a 16-lane env group loads its env's
// record once per launch and its env phase runs on a by-value copy of the launch's EnvDev that carries the record's range,
// channel parameters and Philox env id - exactly what env_cond_kernel (cm_env_cond.hip) does per launch, so a step here is bit
// for bit the policy launch + cm_env_step of such a handle.  The policy tile does not know the table: it reads dist_adj /
// channels of step t from the slot the env phase of step t - 1 wrote, and its sampler's Philox id stays env_id_offset + the
// physical env.
// A handle with a table has adj_const off, so plan_rollout_w never chooses the carried form or the map-10 shape build for it: the
// twins are the non-carried builds only (release / acquire workgroup fence between steps, no folded tail - the caller's tail is a
// cm_chunk_tail launch) and, tape mode being refused for such a handle, have no tape variant: {1, 2 hops} x {env prefetch, plain}
// x {full, ragged last workgroup} per kernel, less the two-hop plain builds.  The plain form is for the grids env_prefetch_ok
// refuses: a side above 16 (more than 10 preys means more than 8, and then cm_env_create gives an env 64 lanes, not 16), whose 16
// env areas fit the 160 KB beside the one-hop image only (map 17: 161536 bytes; beside the two-hop image 177920).  A build that
// no handle reaches by default is not shipped: launch_rollout_wc answers 1 for it.  No host of these kernels reads the diagnostic
// clocks of COMMARL_ENV_STOP = -2: PROBES is off.
// Its own translation unit, built with -fno-slp-vectorize like its siblings (Makefile).
#include "cm_rollout_w_dev.h"

namespace cm {

template <int LHOPS, bool PRE, bool FULLWG>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void rollout_wc_kernel(mf::FwdArgs a, mw::WeightsW w, EnvDev p, const EnvCondDev *__restrict__ cond, cm_step_out out, StridesW c) {
    constexpr bool TAPE = false, CARRY = false, COND = true, PROBES = false;
    constexpr int SHAPE = 0;
    const cm_rng_tape tape_arg{};
    const TailW tl{};
#include "cm_rollout_w_body.h"
}

template <int LHOPS, bool PRE, bool FULLWG>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void rollout_wcm_kernel(mf::FwdArgs a, mw::PolicySetW ps, EnvDev p, const EnvCondDev *__restrict__ cond, cm_step_out out, StridesW c) {
    constexpr bool TAPE = false, CARRY = false, COND = true, PROBES = false;
    constexpr int SHAPE = 0;
    const cm_rng_tape tape_arg{};
    const TailW tl{};
    // uniform per workgroup: one lookup of the policy, one of its pack, the address uniform and global (as rollout_wm_kernel)
    const int k = __builtin_amdgcn_readfirstlane(ps.wg_policy[blockIdx.x]);
    const mw::WeightsW w{ reinterpret_cast<const uint4 *>(uniform_global(reinterpret_cast<const char *>(ps.packs[k])) + ps.wave_off), ps.n_act };
#include "cm_rollout_w_body.h"
}

// Launch for a handle with a condition table: the plan and the ladder of the uniform kernels (a table means adj_const off: never
// carried, never the map-10 build), the table handed over.  `set` NULL: one weight image (w_pack), single step or chunk; else the
// policy set of cm_rollout_chunk_multi.  1 = not available for this shape / handle.
int launch_rollout_wc(mf::FwdArgs a, const cm_policy_weights *w, const void *w_pack, const cm_policy_set *set, const cm_env *h,
                      const cm_step_out &out, void *stream, const ChunkArgs *chunk) {
    const EnvDev &d = h->dev;
    const EnvCondDev *cond = (const EnvCondDev *)h->cond;
    RolloutWPlan pl;
    pl.n_act = w->n_act; pl.out = &out;
    if (!cond || plan_rollout_w(a, h, false, chunk, pl) || pl.carry) return 1;
    if (set) {
        const mw::PolicySetW ps{ set->packs, set->wg_policy, (int)pack_sections(w).w_off, w->n_act };
        return for_rollout_w_variant(d.L, false, pl, [&](auto LH, auto PR, auto FU, auto, auto, auto) {
            if constexpr (LH.value == 2 && !PR.value) return 1;          // two hops, plain: not built (header)
            else return launch_lds<&rollout_wcm_kernel<LH.value, PR.value, FU.value>>(dim3(pl.blocks), dim3(256), pl.lds, stream, a, ps, d, cond, out, pl.c);
        });
    }
    const mw::WeightsW ww = weights_w(w, w_pack);
    return for_rollout_w_variant(d.L, false, pl, [&](auto LH, auto PR, auto FU, auto, auto, auto) {
        if constexpr (LH.value == 2 && !PR.value) return 1;
        else return launch_lds<&rollout_wc_kernel<LH.value, PR.value, FU.value>>(dim3(pl.blocks), dim3(256), pl.lds, stream, a, ww, d, cond, out, pl.c);
    });
}

}  // namespace cm
