// cm_rollout_wm.hip - the wave-owned rollout of teams of 4 with SEVERAL policies in one launch (cm_rollout_chunk_multi): K policies of
// one architecture, each owning a contiguous range of whole workgroups (16 envs).  A workgroup's LDS image and its register-resident
// 128 -> 64 layer are its only per-policy state, and both are read through one pointer at kernel entry: the workgroup looks up its
// policy once, points the weight staging at that policy's pack, and from there runs rollout_w_kernel's step loop unchanged
// (cm_rollout_w_body.h) - every env's arithmetic and Philox draws are those of a single-policy launch at the same global env id.
// Its own translation unit, built with -fno-slp-vectorize like cm_rollout_w.hip (Makefile).
#include "cm_rollout_w_dev.h"

namespace cm {

bool policy_w_enabled();                                 // cm_policy_w.hip
size_t policy_pack_h_bytes(int d, int L, bool policy);   // cm_policy_h.hip: size of the f16 pack the wave-owned fragments sit behind

namespace mw {
// the policy set as the kernel sees it: read at entry only, so nothing of it stays live through the step loop but n_act (as WeightsW)
struct PolicySetW {
    const float *const *packs;                           // [K] cm_policy_pack() outputs
    const int32_t *wg_policy;                            // [n_wg] policy of each workgroup
    int wave_off;                                        // bytes from a pack's start to its wave-owned section (one shape: one offset)
    int n_act;
};
}  // namespace mw

// No tape variant (tape mode steps one launch at a time) and no folded tail (the caller's tail is a cm_chunk_tail launch).
template <int LHOPS, bool PRE, bool FULLWG, bool CARRY = false, int SHAPE = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void rollout_wm_kernel(mf::FwdArgs a, mw::PolicySetW ps, EnvDev p, cm_step_out out, StridesW c) {
    constexpr bool TAPE = false;
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
    if (!h || !w || !set || !st || !obs || !out) return set_error(CM_ERR_ARG, "cm_rollout_chunk_multi: null argument");
    if (n_steps < 0) return set_error(CM_ERR_ARG, "cm_rollout_chunk_multi: negative step count");
    if (h->cfg.rng_mode == CM_RNG_TAPE) return set_error(CM_ERR_ARG, "cm_rollout_chunk_multi: tape mode steps one launch at a time");
    const EnvDev &d = h->dev;
    if (w->n_agents != d.N || w->d != d.d || w->n_hops != d.L)
        return set_error(CM_ERR_ARG, "cm_rollout_chunk_multi: policy shape (n_agents, d, n_hops) does not match the env handle");
    if (set->n_policies < 1 || !set->packs || !set->wg_policy)
        return set_error(CM_ERR_ARG, "cm_rollout_chunk_multi: empty policy set or null table");
    if (set->n_wg != (d.B + mw::WG_ENVS - 1) / mw::WG_ENVS)
        return set_error(CM_ERR_ARG, "cm_rollout_chunk_multi: n_wg must be ceil(B / 16) of the env handle");
    if (n_steps == 0) return CM_OK;
    if (!policy_shape_ok(w) || !policy_w_enabled() || !shape_ok_rollout_w(d.N, d.d, d.L, w->n_act)) return 1;
    mf::FwdArgs a{};
    a.S = d.B; a.N = d.N; a.d = d.d; a.L = d.L;
    a.obs = obs; a.adj = dist_adj; a.chan = channels;
    a.key0 = (uint32_t)seed; a.key1 = (uint32_t)(seed >> 32); a.policy_step = policy_step; a.step_base = policy_step_base;
    a.env_id_offset = env_id_offset; a.greedy = greedy; a.no_residual = w->no_residual;
    a.actions = actions; a.probs = probs; a.attn = attn;
    const ChunkArgs c{ n_steps, st->obs, st->actions, st->probs, st->attn, st->reward, st->reward_f64, st->done, st->details,
                       st->dist_adj, st->channels, st->prey_alive, st->success, st->path_len };
    RolloutWPlan pl;
    if (plan_rollout_w(a, h, false, &c, pl)) return 1;
    // the wave-owned section of a pack: behind the all-f32 fragments and the f16-split pack (as rollout_impl, cm_fused.hip)
    const size_t off = (size_t)mf::pack_layout(mf::kpad_of(d.d), d.L, true).total * sizeof(float) + policy_pack_h_bytes(d.d, d.L, true);
    const mw::PolicySetW ps{ set->packs, set->wg_policy, (int)off, w->n_act };
    const int blocks = pl.blocks;
    const size_t lds = pl.lds;
    const StridesW &sw = pl.c;
    const cm_step_out o = *out;
#define CM_RWM_(LH, PR, FU, CA, SH)                                                                                             \
    do {                                                                                                                        \
        static unsigned long long done = 0;                                                                                     \
        if (cm::dev_first(done))                                                                                                \
            CM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&rollout_wm_kernel<LH, PR, FU, CA, SH>),                  \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));                                \
        hipLaunchKernelGGL((rollout_wm_kernel<LH, PR, FU, CA, SH>), dim3(blocks), dim3(256), lds, (hipStream_t)stream, a, ps, d, o, sw); \
    } while (0)
#define CM_RWM(LH, PR, FU, CA) do { if (CA && pl.map10) CM_RWM_(LH, PR, FU, CA, (CA ? 1 : 0)); else CM_RWM_(LH, PR, FU, CA, 0); } while (0)
#define CM_RWM2(LH) do { if (pl.carry) { if (pl.full) CM_RWM(LH, true, true, true); else CM_RWM(LH, true, false, true); }         \
                         else if (pl.pre) { if (pl.full) CM_RWM(LH, true, true, false); else CM_RWM(LH, true, false, false); }   \
                         else { if (pl.full) CM_RWM(LH, false, true, false); else CM_RWM(LH, false, false, false); } } while (0)
    if (d.L == 1) CM_RWM2(1); else CM_RWM2(2);
#undef CM_RWM2
#undef CM_RWM
#undef CM_RWM_
    CM_HIP(hipGetLastError());
    return CM_OK;
}
