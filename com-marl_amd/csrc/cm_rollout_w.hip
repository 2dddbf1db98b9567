// cm_rollout_w.hip - the rollout step of teams of 4 on WAVE-OWNED rows: Comm-DP policy forward + sample (cm_policy_w_dev.h) and
// the env step (cm_env_dev.h) of a wave's four envs, by that wave alone, for one step or a whole chunk of steps per launch
// (reference: centralized_ma_on_policy_vectorized_sampler.py:119-232 - get_actions, vec_env.step, obses = next_obses).
// Its own translation unit: built with -fno-slp-vectorize (Makefile), which the older kernels of cm_fused.hip are not.
#include "cm_rollout_w_dev.h"

namespace cm {

template <int LHOPS, bool PRE, bool FULLWG, bool TAPE, bool CARRY = false, int SHAPE = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void rollout_w_kernel(mf::FwdArgs a, mw::WeightsW w, EnvDev p, cm_rng_tape tape_arg, cm_step_out out, StridesW c, TailW tl) {
#include "cm_rollout_w_body.h"
}

bool shape_ok_rollout_w(int N, int d, int L, int n_act) { return policy_w_enabled() && mw::shape_ok_w(N, d, L, n_act); }

// Launch plan of the wave-owned rollout kernels (rollout_w_kernel here, rollout_wm_kernel in cm_rollout_wm.hip); 1 = not available for
// this handle / chunk.  Sets *chunk->tail_folded when the carried form will take the chunk's tail.
int plan_rollout_w(const mf::FwdArgs &a, const cm_env *h, bool use_tape, const ChunkArgs *chunk, RolloutWPlan &pl) {
    const EnvDev &d = h->dev;
    if (d.scen != CM_PP || d.lpe != 16 || d.M > 16 || d.N != 4) return 1;
    pl.lds = mw::lds_policy_bytes(d.L) + (size_t)d.lds_env * mw::WG_ENVS;
    if (pl.lds > 160 * 1024) return 1;                                   // larger maps: the env areas do not fit beside the weights
    StridesW &c = pl.c;
    c = StridesW{};
    c.n_steps = 1;
    if (chunk) {
        const long long st[13] = { chunk->obs, chunk->actions, chunk->probs, chunk->attn, chunk->reward, chunk->reward_f64, chunk->done, chunk->details,
                                   chunk->dist_adj, chunk->channels, chunk->prey_alive, chunk->success, chunk->path_len };
        for (long long v : st) if (v < 0 || v > 0x7fffffffLL) return 1;   // strides beyond 2^31 elements: the workgroup-tiled kernels take it
        c = StridesW{ chunk->n_steps, (int)st[0], (int)st[1], (int)st[2], (int)st[3], (int)st[4], (int)st[5], (int)st[6], (int)st[7], (int)st[8],
                      (int)st[9], (int)st[10], (int)st[11], (int)st[12] };
    }
    pl.blocks = (a.S + mw::WG_ENVS - 1) / mw::WG_ENVS;
    pl.pre = env_prefetch_ok<CM_PP, 16>(d);
    pl.full = a.S % mw::WG_ENVS == 0;
    // carried form (state and observation from step to step inside the wave, no fence between steps): multi-step launches on
    // a constant adjacency without a channel model; the observation copy needs 4 rows x 24 floats in the env area's claim table
    pl.carry = pl.pre && !use_tape && c.n_steps > 1 && d.adj_const && d.ch_const && !a.adj && !a.chan &&
               a.d <= OBS_COPY_STRIDE && 4 * d.S * d.S >= 4 * OBS_COPY_STRIDE * 4;
    pl.tl = TailW{};
    if (pl.carry && chunk && chunk->tail_obs && chunk->tail_base && chunk->tail_folded) {
        pl.tl = TailW{ chunk->tail_obs, chunk->tail_base, d.tail_ticket, 1 };
        *chunk->tail_folded = 1;
    }
    pl.map10 = pl.carry && d.S == 10 && d.M == 4 && d.R == 1 && d.W == 3 && d.d == 21 && d.lds_env == lds_env_bytes(10, 4, 4);
    return 0;
}

// Launch of the wave-owned rollout kernel; 1 = not available for this shape / handle.
int launch_rollout_w(mf::FwdArgs a, const cm_policy_weights *w, const void *w_pack, const cm_env *h, const cm_rng_tape &t, const cm_step_out &out,
                    void *stream, const ChunkArgs *chunk) {
    const EnvDev &d = h->dev;
    const bool use_tape = t.prey || t.spawn || t.iid_u || t.ge_u || t.ge_init_u;
    RolloutWPlan pl;
    if (plan_rollout_w(a, h, use_tape, chunk, pl)) return 1;
    const mw::WeightsW ww{ reinterpret_cast<const uint4 *>(w_pack), w->n_act };
    const int rc = for_rollout_w_variant(d.L, use_tape, pl, [&](auto LH, auto PR, auto FU, auto TP, auto CA, auto SH) {
        return launch_rollout_w_variant<&rollout_w_kernel<LH.value, PR.value, FU.value, TP.value, CA.value, SH.value>>(pl, stream, a, ww, d, t, out, pl.c, pl.tl);
    });
    if (rc != CM_OK) return rc;
    if (d.stop == -1) env_probe_dump("rollout_w", HIP_SYMBOL(g_env_probe), stream);
    if (d.stop == -2) {
        unsigned long long hp[5];
        if (hipStreamSynchronize((hipStream_t)stream) == hipSuccess && hipMemcpyFromSymbol(hp, HIP_SYMBOL(g_w_probe), sizeof(hp)) == hipSuccess && hp[0])
            fprintf(stderr, "[rollout_w probe] steps=%llu staging=%llu clk; per step: policy=%llu env=%llu clk (of which the closing fence %llu)\n", hp[0],
                    hp[3], hp[1] / hp[0], hp[2] / hp[0], hp[4] / hp[0]);
    }
    return CM_OK;
}

}  // namespace cm
