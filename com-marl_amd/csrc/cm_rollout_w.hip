// cm_rollout_w.hip - the rollout step of teams of 4 on WAVE-OWNED rows: Comm-DP policy forward + sample (cm_policy_w_dev.h) and
// the env step (cm_env_dev.h) of a wave's four envs, by that wave alone, for one step or a whole chunk of steps per launch
// (reference: centralized_ma_on_policy_vectorized_sampler.py:119-232 - get_actions, vec_env.step, obses = next_obses).
// Its own translation unit: built with -fno-slp-vectorize (Makefile), which the older kernels of cm_fused.hip are not.
#include "cm_rollout_w_dev.h"

namespace cm {

template <int LHOPS, bool PRE, bool FULLWG, bool TAPE, bool CARRY = false, int SHAPE = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void rollout_w_kernel(mf::FwdArgs a, mw::WeightsW w, EnvDev p, cm_rng_tape tape_arg, cm_step_out out, StridesW c, TailW tl) {
    constexpr bool PROBES = SHAPE != 1;                  // generic builds: gated at run time as ever; SHAPE 1: none (the entry below has them)
    constexpr bool COND = false;                         // per-env comm conditions: the twins of cm_rollout_wc.hip
    constexpr const EnvCondDev *cond = nullptr;
#include "cm_rollout_w_body.h"
}

// The headline build (two hops, full workgroups, carried, SHAPE 1) WITH the diagnostic clocks of COMMARL_ENV_STOP < 0 (g_w_probe, ENV_PROBE):
// what the launcher takes instead of rollout_w_kernel<2, true, true, false, true, 1> when the handle asks for them, so that the
// production build carries neither the s_memtime sites nor the branches around them.  Its timing is this build's, not that one's.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void rollout_w_probe_kernel(mf::FwdArgs a, mw::WeightsW w, EnvDev p, cm_rng_tape tape_arg, cm_step_out out, StridesW c, TailW tl) {
    constexpr int LHOPS = 2, SHAPE = 1;
    constexpr bool PRE = true, FULLWG = true, TAPE = false, CARRY = true, PROBES = true, COND = false;
    constexpr const EnvCondDev *cond = nullptr;
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
    // ... and what the SHAPE 1 build folds besides the grid: five actions sampled without an avail mask, every output the
    // engine passes by default (a constant adjacency without channel model has no dist_adj / channels output), and byte offsets
    // that fit 32 bits - per buffer, n_steps slots plus one step's rows below 2^31 bytes; the state arrays likewise
    if (pl.map10) {
        const cm_step_out *o = pl.out;
        pl.map10 = pl.n_act == 5 && !a.avail && !a.greedy && a.actions && a.probs && a.attn && o && o->obs && o->reward && o->reward_f64 &&
                   o->done && o->details && o->prey_alive && o->success && o->path_len;
        const long long B = d.B, lim = 0x7fffffffLL;
        auto fits = [&](int stride, long long row_elems, long long bytes) { return ((long long)c.n_steps * stride + B * row_elems) * bytes < lim; };
        pl.map10 = pl.map10 && fits(c.obs, 4 * 21, 4) && fits(c.actions, 4, 4) && fits(c.probs, 4 * 5, 4) && fits(c.attn, 16, 4) &&
                   fits(c.reward, 1, 4) && fits(c.reward_f64, 1, 8) && fits(c.done, 1, 1) && fits(c.details, 6, 4) &&
                   fits(c.prey_alive, 4, 1) && fits(c.success, 1, 4) && fits(c.path_len, 1, 4) && fits(0, 4, 8);
    }
    pl.probes = pl.map10 && d.stop < 0 && pl.full && d.L == 2;          // the one build that has the clocks (rollout_w_probe_kernel)
    return 0;
}

// Launch of the wave-owned rollout kernel; 1 = not available for this shape / handle.
int launch_rollout_w(mf::FwdArgs a, const cm_policy_weights *w, const void *w_pack, const cm_env *h, const cm_rng_tape &t, const cm_step_out &out,
                    void *stream, const ChunkArgs *chunk) {
    const EnvDev &d = h->dev;
    const bool use_tape = t.prey || t.spawn || t.iid_u || t.ge_u || t.ge_init_u;
    RolloutWPlan pl;
    pl.n_act = w->n_act; pl.out = &out;
    if (plan_rollout_w(a, h, use_tape, chunk, pl)) return 1;
    const mw::WeightsW ww = weights_w(w, w_pack);
    const int rc = pl.probes ? launch_lds<&rollout_w_probe_kernel>(dim3(pl.blocks), dim3(256), pl.lds, stream, a, ww, d, t, out, pl.c, pl.tl) : for_rollout_w_variant(d.L, use_tape, pl, [&](auto LH, auto PR, auto FU, auto TP, auto CA, auto SH) {
        return launch_lds<&rollout_w_kernel<LH.value, PR.value, FU.value, TP.value, CA.value, SH.value>>(dim3(pl.blocks), dim3(256), pl.lds, stream, a, ww, d, t, out, pl.c, pl.tl);
    });
    if (rc != CM_OK) return rc;
    if (pl.map10 && !pl.probes) return CM_OK;                            // a SHAPE 1 build without the clocks: nothing to print
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
