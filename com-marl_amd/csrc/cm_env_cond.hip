// cm_env_cond.hip - the env step of cm_env.hip with a per-env comm condition (cm_env_set_conditions, include/commarl.h).
//
// A handle's communication range and channel parameters are scalars of EnvDev: every env of a launch shares them.  The
// robustness curves of the paper (success / return against a shrinking range and a lossier channel: the runners' --teRcom,
// --tepl, --Pgb, --Pbg) want many conditions in ONE batch.  The kernels here are the twins of env_kernel / env_kernel_wide
// with one more argument, a device table of one 32-byte record per env: a sub-wave group loads its env's record once, ahead
// of the state loads, and runs the unchanged bodies of cm_env_dev.h on a by-value copy of the launch's EnvDev in which rc2,
// ploss, pgb, pbg and env_id_offset are that env's values.  The copy is taken apart by the compiler: the five fields live in
// VGPRs (with 16 lanes per env the four envs of a wave differ), everything else stays the launch's scalar argument - no
// private segment, LDS through integer offsets as everywhere in the env step.
// Tape mode is refused for such a handle on the host, so rng_mode is the constant CM_RNG_PHILOX here and the tape branches
// of the bodies fold away.
#include "cm_internal.h"
#include "cm_rng.h"
#include "cm_env_dev.h"

namespace cm {

// The launch's EnvDev with env b's record in place of the handle's comm scalars.  The Philox env id of env b becomes
// rec.rng_id: the bodies compute it as env_id_offset + b (load_cond / apply_cond, cm_env_dev.h).
__device__ __forceinline__ EnvDev with_cond(const EnvDev &p, const EnvCondDev *__restrict__ cond, int b) {
    return apply_cond(p, load_cond(cond, b));
}

template <int SCEN, int LPE>
__global__ __launch_bounds__(WAVE) void env_cond_kernel(EnvDev p, const EnvCondDev *__restrict__ cond,
                                                       const int32_t *__restrict__ actions, cm_step_out out, int reset_only) {
    constexpr int G = WAVE / LPE;
    const int grp = threadIdx.x / LPE, b_raw = blockIdx.x * G + grp;
    const int b = b_raw < p.B ? b_raw : p.B - 1;                                 // idle groups shadow the last env, as env_body does
    const EnvDev q = with_cond(p, cond, b);
    const cm_rng_tape no_tape{};
    env_body<SCEN, LPE>(q, actions, nullptr, no_tape, out, reset_only, grp, b_raw, true, 0);
}

// Wide form (env_kernel_wide: wave 0 steps, all four waves emit).  One env per workgroup: both phases read the same record.
template <int SCEN, int LPE>
__global__ __launch_bounds__(256) void env_cond_kernel_wide(EnvDev p, const EnvCondDev *__restrict__ cond,
                                                           const int32_t *__restrict__ actions, cm_step_out out, int reset_only) {
    static_assert(LPE == WAVE, "the wide form is built for one env per workgroup");
    constexpr int EL = 256;
    __shared__ int hand[4];                            // [0] emit?  [1] step count  [2] comm slot  [3] Philox step
    if (threadIdx.x < 4) hand[threadIdx.x] = 0;
    __syncthreads();
    const int b = blockIdx.x;                          // the grid is exactly B workgroups
    const EnvDev q = with_cond(p, cond, b);
    const cm_rng_tape no_tape{};
    if (threadIdx.x < WAVE) env_body<SCEN, LPE>(q, actions, nullptr, no_tape, out, reset_only, 0, b, true, 0, hand);
    __syncthreads();
    if (b >= q.B || !hand[0]) return;
    Grp<EL> g;
    g.sub = 0; g.sl = threadIdx.x % EL;
    const Lds l = make_lds(q.S, q.N, q.M, 0, q.status);
    const Rng rng{ (uint32_t)(q.env_id_offset + b), (uint32_t)hand[3], q.key0, q.key1 };
    emit<SCEN, EL>(q, l, rng, no_tape, out, b, g, hand[1], hand[2]);
}

// cm_env.hip's launch() made the narrow / wide choice; d.lpe is the handle's.
int launch_env_cond(const cm_env *h, bool wide, const int32_t *actions, const cm_step_out &out, hipStream_t st, int reset_only) {
    const EnvDev &d = h->dev;
    const EnvCondDev *cond = (const EnvCondDev *)h->cond;
    if (wide) {
        const dim3 grid(d.B), block(256);
#define CM_WIDE(SC) hipLaunchKernelGGL((env_cond_kernel_wide<SC, 64>), grid, block, h->lds_bytes, st, d, cond, actions, out, reset_only)
        if (d.scen == CM_PP) CM_WIDE(CM_PP); else CM_WIDE(CM_CO);
#undef CM_WIDE
        CM_HIP(hipGetLastError());
        return CM_OK;
    }
    const int G = WAVE / d.lpe;
    const dim3 grid((d.B + G - 1) / G), block(WAVE);
#define CM_LAUNCH(SC, LP) hipLaunchKernelGGL((env_cond_kernel<SC, LP>), grid, block, h->lds_bytes, st, d, cond, actions, out, reset_only)
    if (d.scen == CM_PP) { if (d.lpe == 16) CM_LAUNCH(CM_PP, 16); else if (d.lpe == 32) CM_LAUNCH(CM_PP, 32); else CM_LAUNCH(CM_PP, 64); }
    else { if (d.lpe == 16) CM_LAUNCH(CM_CO, 16); else if (d.lpe == 32) CM_LAUNCH(CM_CO, 32); else CM_LAUNCH(CM_CO, 64); }
#undef CM_LAUNCH
    CM_HIP(hipGetLastError());
    return CM_OK;
}

}  // namespace cm
