// cm_rollout_wm.hip - the wave-owned rollout of teams of 4 with SEVERAL policies in one launch (cm_rollout_chunk_multi): K policies of
// one architecture, each owning a contiguous range of whole workgroups (16 envs).  A workgroup's LDS image and its register-resident
// 128 -> 64 layer are its only per-policy state, and both are read through one pointer at kernel entry: the workgroup looks up its
// policy once, points the weight staging at that policy's pack, and from there runs rollout_w_kernel's step loop unchanged
// (cm_rollout_w_body.h) - every env's arithmetic and Philox draws are those of a single-policy launch at the same global env id.
// Its own translation unit, built with -fno-slp-vectorize like cm_rollout_w.hip (Makefile).
#include "cm_rollout_w_dev.h"

namespace cm {

// No tape variant (tape mode steps one launch at a time) and no folded tail (the caller's tail is a cm_chunk_tail launch).
template <int LHOPS, bool PRE, bool FULLWG, bool CARRY = false, int SHAPE = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void rollout_wm_kernel(mf::FwdArgs a, mw::PolicySetW ps, EnvDev p, cm_step_out out, StridesW c) {
    constexpr bool TAPE = false;
    constexpr bool PROBES = SHAPE != 1;                  // the host of this entry never reads the clocks: no probe twin of its SHAPE 1 builds
    constexpr bool COND = false;                         // per-env comm conditions: rollout_wcm_kernel (cm_rollout_wc.hip)
    constexpr const EnvCondDev *cond = nullptr;
    // uniform per workgroup: one lookup of the policy, one of its pack.  The pack address is made uniform (both halves through
    // readfirstlane) and global explicitly: a pointer as loaded from memory is generic and not known uniform, and then the staging's
    // loads become flat loads and its batch of chunks goes to scratch (304 bytes per lane)
    const int k = __builtin_amdgcn_readfirstlane(ps.wg_policy[blockIdx.x]);
    const unsigned long long u = (unsigned long long)ps.packs[k];
    const unsigned long long pk = ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(u >> 32)) << 32) |
                                  (unsigned)__builtin_amdgcn_readfirstlane((unsigned)u);
    const mw::WeightsW w{ (const uint4 *)(const __attribute__((address_space(1))) uint4 *)(pk + ps.wave_off), ps.n_act };
    const cm_rng_tape tape_arg{};
    const TailW tl{};
#include "cm_rollout_w_body.h"
}

}  // namespace cm

using namespace cm;

extern "C" int cm_rollout_chunk_multi(cm_env_t h, const cm_policy_weights *w, const cm_policy_set *set, int32_t n_steps,
                                      const cm_chunk_strides *st, const float *obs, const float *dist_adj, const float *channels,
                                      uint64_t seed, int32_t env_id_offset, uint32_t policy_step, const uint32_t *policy_step_base,
                                      int32_t greedy, int32_t *actions, float *probs, float *attn, const cm_step_out *out, void *stream) {
    const char *who = "cm_rollout_chunk_multi";
    if (int rc = check_chunk_args(who, h, st, n_steps, 0)) return rc;
    if (int rc = check_rollout_args(who, h, w, obs, out)) return rc;
    const EnvDev &d = h->dev;
    if (!set || set->n_policies < 1 || !set->packs || !set->wg_policy)
        return set_error(CM_ERR_ARG, "cm_rollout_chunk_multi: empty policy set or null table");
    if (set->n_wg != (d.B + mw::WG_ENVS - 1) / mw::WG_ENVS)
        return set_error(CM_ERR_ARG, "cm_rollout_chunk_multi: n_wg must be ceil(B / 16) of the env handle");
    if (n_steps == 0) return CM_OK;
    if (h->cond && !h->cond_fused) return 1;         // per-env comm conditions: fused on request only (cm_env_fuse_conditions)
    if (!policy_shape_ok(w) || !policy_w_enabled() || !shape_ok_rollout_w(d.N, d.d, d.L, w->n_act)) return 1;
    // the policy forward's arguments: shape from the env handle, the rest as the entry point received it
    const mf::FwdArgs a = fwd_args(FwdShape{ d.B, d.N, d.d, d.L, w->no_residual }, obs, dist_adj, channels, attn,
                                   FwdSampler{ nullptr, seed, env_id_offset, policy_step, policy_step_base, greedy, actions, probs });
    const ChunkArgs c = chunk_args(n_steps, *st);
    RolloutWPlan pl;
    pl.n_act = w->n_act; pl.out = out;
    if (h->cond) return launch_rollout_wc(a, w, nullptr, set, h, *out, stream, &c);   // rollout_wcm_kernel, or 1
    if (plan_rollout_w(a, h, false, &c, pl)) return 1;
    const mw::PolicySetW ps{ set->packs, set->wg_policy, (int)pack_sections(w).w_off, w->n_act };
    // no tape variant here: the ladder never takes that branch without a tape
    return for_rollout_w_variant(d.L, false, pl, [&](auto LH, auto PR, auto FU, auto, auto CA, auto SH) {
        return launch_lds<&rollout_wm_kernel<LH.value, PR.value, FU.value, CA.value, SH.value>>(dim3(pl.blocks), dim3(256), pl.lds, stream, a, ps, d, *out, pl.c);
    });
}
