// cm_policy_host.h - the host code the units of the default-shape Comm-DP forward share (cm_policy.hip, cm_policy_mfma.hip,
// cm_policy_h.hip, cm_policy_hm.hip, cm_policy_w.hip, cm_fused.hip and, through cm_rollout_w_dev.h, cm_rollout_w*.hip): the
// prototypes of what they call across units, the COMMARL_POLICY_KERNEL switch, the builder of the forward's argument block, the
// sections of an operand pack, the weight-pointer structs and the team-size / observation-width ladder.  Host only: nothing here
// is device code.  The helpers are static inline: the library exports every external symbol, and these are not ABI.
#pragma once
#include <type_traits>

#include "cm_policy_w_dev.h"   // (-> cm_policy_h_dev.h -> cm_policy_mfma_dev.h)

namespace cm {

// ---- COMMARL_POLICY_KERNEL: read once per process (cm_policy.hip), first letter only; anything but h / f / v is `wave` ----
//
//  value         | cm_policy_forward,         | cm_policy_forward_multi | cm_rollout_step / _chunk      | *_forward_saved   | *_forward_saved_wave
//                | cm_critic_forward          | (and its planner)       | (_chunk_tail, _chunk_multi)   |                   |
//  --------------+----------------------------+-------------------------+-------------------------------+-------------------+---------------------
//  unset, "w..." | teams of 4: wave-owned     | f16-split set kernel    | teams of 4: wave-owned rollout| f16-split kernel  | wave-owned training
//   (wave)       | (policy); else f16-split   |                         | (_multi: that one only);      |                   | forward (teams of 4)
//                |                            |                         | else fused step, f16-split    |                   |
//  "h..."  (h)   | f16-split, every team size | f16-split set kernel    | fused step, f16-split         | f16-split kernel  | 1 (not covered)
//  "f..."  (f32) | all-f32 matrix-core kernel | 0 / 1 (no set kernel)   | fused step, all-f32           | f16-split kernel  | 1 (not covered)
//  "v..."  (valu)| generic VALU kernel        | 0 / 1 (no set kernel)   | fused step, f16-split         | f16-split kernel  | 1 (not covered)
//
// Every row falls through to the next older kernel where a shape has no instantiation (f16-split -> all-f32 -> VALU for the
// stand-alone forwards; the rollout entry points answer 1).  Two oddities are kept as they are: `valu` turns off the matrix-core
// route of the stand-alone forward and of the set forward only - the fused rollout still takes the f16-split body - and the
// *_saved entry points call the f16-split kernel whatever the switch says.  cm_rollout_chunk_multi has the wave-owned kernels
// only and answers 1 for h / f32 / valu.  The size of the critic's wave-owned pack section follows the switch too
// (critic_pack_w_bytes is 0 unless `wave`).
enum class PolicyKernel { wave, h, f32, valu };
PolicyKernel policy_kernel();                                                                    // cm_policy.hip
static inline bool policy_w_enabled() { return policy_kernel() == PolicyKernel::wave; }          // wave-owned teams-of-4 kernels
static inline bool policy_h_enabled() { return policy_kernel() != PolicyKernel::f32; }           // f16-split dense layers, else all-f32
static inline bool policy_mfma_enabled() { return policy_kernel() != PolicyKernel::valu; }       // stand-alone forward: matrix-core route
static inline bool policy_set_enabled() { return policy_kernel() <= PolicyKernel::h; }          // cm_policy_forward_multi: wave or h

// ---- what the units call across each other: 1 = the shape / switch is not covered (the caller runs its next kernel) ----
// cm_policy_mfma.hip
bool policy_shape_ok(const cm_policy_weights *w);
int policy_forward_mfma(const cm_policy_weights *w, mf::FwdArgs a, void *stream);
int critic_forward_mfma(const cm_critic_weights *w, mf::FwdArgs a, void *stream);
// cm_policy_h.hip: the f16-split kernel and its operand pack; h_pack / dst = the pack's f16-split section
int policy_forward_h(const cm_policy_weights *w, const void *h_pack, mf::FwdArgs a, void *stream);
int critic_forward_h(const cm_critic_weights *w, const void *h_pack, mf::FwdArgs a, void *stream);
size_t policy_pack_h_bytes(int d, int L, bool policy);
int policy_pack_h(const cm_policy_weights *w, void *dst, int sections, void *stream);
int critic_pack_h(const cm_critic_weights *w, void *dst, int sections, void *stream);
// cm_policy_w.hip: the wave-owned teams-of-4 kernel; w_pack / dst = the pack's wave-owned section, `bad` = the caller's range
// flag (a weight the f16 pair cannot carry), may be null
int policy_forward_w(const cm_policy_weights *w, const void *w_pack, mf::FwdArgs a, void *stream);
int policy_forward_w_train(const cm_policy_weights *w, const void *w_pack, mf::FwdArgs a, void *stream);
int critic_forward_w_train(const cm_critic_weights *w, const void *w_pack, mf::FwdArgs a, void *stream);
size_t policy_pack_w_bytes(const cm_policy_weights *w);
size_t critic_pack_w_bytes(const cm_critic_weights *w);
int policy_pack_w(const cm_policy_weights *w, void *dst, void *stream, int *bad);
int critic_pack_w(const cm_critic_weights *w, void *dst, void *stream, int *bad);
// cm_rollout_w.hip: teams of 4 on the wave-owned rollout kernel, where enabled
bool shape_ok_rollout_w(int N, int d, int L, int n_act);

static inline mw::WeightsW weights_w(const cm_policy_weights *w, const void *w_pack) {
    return mw::WeightsW{ reinterpret_cast<const uint4 *>(w_pack), w->n_act };
}

template <class W>
constexpr bool is_policy_v = std::is_same_v<W, cm_policy_weights>;   // the other weights struct is cm_critic_weights

// ---- the forward's argument block.  Args = mf::FwdArgs, or the VALU kernel's own (cm_policy.hip) ----
struct FwdShape { int S, N, d, L, no_residual; };
template <class W>
static inline FwdShape fwd_shape(const W *w, int S) { return FwdShape{ S, w->n_agents, w->d, w->n_hops, w->no_residual }; }
// the sampler's part (policy, acting form)
struct FwdSampler {
    const float *avail;
    uint64_t seed;
    int32_t env_id_offset;
    uint32_t policy_step;
    const uint32_t *step_base;
    int32_t greedy;
    int32_t *actions;
    float *probs;
};
// shape, graph inputs and outputs (values: the critic's)
template <class Args = mf::FwdArgs>
static inline Args fwd_args(const FwdShape &s, const float *obs, const float *adj, const float *chan, float *attn, float *values = nullptr) {
    Args a{};
    a.S = s.S; a.N = s.N; a.d = s.d; a.L = s.L; a.no_residual = s.no_residual;
    a.obs = obs; a.adj = adj; a.chan = chan; a.attn = attn; a.values = values;
    return a;
}
template <class Args = mf::FwdArgs>
static inline Args fwd_args(const FwdShape &s, const float *obs, const float *adj, const float *chan, float *attn, const FwdSampler &sm) {
    Args a = fwd_args<Args>(s, obs, adj, chan, attn);
    a.avail = sm.avail;
    a.key0 = (uint32_t)sm.seed; a.key1 = (uint32_t)(sm.seed >> 32); a.policy_step = sm.policy_step; a.step_base = sm.step_base;
    a.env_id_offset = sm.env_id_offset; a.greedy = sm.greedy;
    a.actions = sm.actions; a.probs = sm.probs;
    return a;
}

// ---- one cm_policy_pack / cm_critic_pack buffer: [all-f32 fragments | f16-split pack | wave-owned pack] ----
// Offsets in bytes from the buffer's start; h_bytes / w_bytes are 0 for a shape without that section.  Policy or critic: the type of w.
struct PackSections {
    const char *base;                                    // the pack (may be null: sizes and offsets only)
    size_t h_off, w_off, h_bytes, w_bytes, total;
    const float *f32() const { return reinterpret_cast<const float *>(base); }
    const uint4 *h() const { return reinterpret_cast<const uint4 *>(base + h_off); }
    const uint4 *w() const { return reinterpret_cast<const uint4 *>(base + w_off); }
};
template <class W>
static inline mf::PackLayout layout_f32(const W *w) { return mf::pack_layout(mf::kpad_of(w->d), w->n_hops, is_policy_v<W>); }
template <class W>
static inline mh::PackLayoutH layout_h(const W *w) { return mh::pack_layout_h(mh::kh_of(w->d), w->n_hops, is_policy_v<W>); }
template <class W>
static inline PackSections pack_sections(const W *w, const void *pack) {
    PackSections s{};
    s.base = reinterpret_cast<const char *>(pack);
    s.h_off = layout_f32(w).total * sizeof(float);
    s.h_bytes = policy_pack_h_bytes(w->d, w->n_hops, is_policy_v<W>);
    s.w_off = s.h_off + s.h_bytes;
    if constexpr (is_policy_v<W>) s.w_bytes = policy_pack_w_bytes(w);
    else s.w_bytes = critic_pack_w_bytes(w);
    s.total = s.w_off + s.w_bytes;
    return s;
}
template <class W>
static inline PackSections pack_sections(const W *w) { return pack_sections(w, w->mfma_pack); }

// ---- the weight-pointer structs: fragments from a pack section (P, its layout), biases and the critic's 64 -> 1 row plain ----
template <class W>
static inline mf::TrunkW trunk_w(const float *P, const mf::PackLayout &lo, const W *w) {
    return mf::TrunkW{ P + lo.enc1, w->enc_b1, P + lo.enc2, w->enc_b2, P + lo.attn, P + lo.gcn, w->gcn_b };
}
static inline mf::PolHead pol_head(const float *P, const mf::PackLayout &lo, const cm_policy_weights *w) {
    return mf::PolHead{ P + lo.x1, w->hd_b1, P + lo.h2, w->hd_b2, P + lo.h3, w->hd_b3, P + lo.h4, w->hd_b4, w->n_act };
}
static inline mf::CritHead crit_head(const float *P, const mf::PackLayout &lo, const cm_critic_weights *w) {
    return mf::CritHead{ P + lo.x1, w->dec_b1, w->dec_w2t, w->dec_b2 };
}
template <class W>
static inline mh::TrunkH trunk_h(const uint4 *P, const mh::PackLayoutH &lo, const W *w) {
    return mh::TrunkH{ P + lo.enc1, w->enc_b1, P + lo.enc2, w->enc_b2, P + lo.attn, P + lo.gcn, w->gcn_b };
}
static inline mh::PolHeadH pol_head_h(const uint4 *P, const mh::PackLayoutH &lo, const cm_policy_weights *w) {
    return mh::PolHeadH{ P + lo.x1, w->hd_b1, P + lo.h2, w->hd_b2, P + lo.h3, w->hd_b3, P + lo.h4, w->hd_b4, w->n_act };
}
static inline mh::CritHeadH crit_head_h(const uint4 *P, const mh::PackLayoutH &lo, const cm_critic_weights *w) {
    return mh::CritHeadH{ P + lo.x1, w->dec_b1, w->dec_w2t, w->dec_b2 };
}

// ---- the one ladder from (observation width, team size) to a build of a workgroup-tiled forward: f(K, MAXMK, NW), each a
// std::integral_constant; 1 = no instantiation.  MAXMK: -1 = teams of 4 (register-resident attention / aggregation), 0 = below 16
// agents, else the N x N products on MFMA tiles ((row blocks) x (column blocks) of 16) ----
struct FwdTile {
    int mk;                                              // 0 | 25 | 64: N < 16, N <= 80, N <= 128
    bool quad;                                           // teams of 4: the MAXMK = -1 build
    bool w8;                                             // 8-wave workgroups (every team with mk == 64): one workgroup per CU fits in LDS,
};                                                       // two waves per SIMD hide each other's latencies; N = 24 is faster on 4 waves
static inline FwdTile fwd_tile(int N) {
    return FwdTile{ N < 16 ? 0 : (N <= 80 ? 25 : 64), N == 4 && mf::pick_epb(4) * 4 <= 32, N >= 32 };
}
// k = mf::kpad_of(d) with K2 = 80 (the all-f32 family) or mh::kh_of(d) with K2 = 96 (the f16-split families); QUAD = false: a
// family without a teams-of-4 build (the set kernel), which the caller does not reach with N = 4
template <int K2, bool QUAD = true, class F>
static inline int for_fwd_variant(int k, int N, F &&f) {
    if (N > 128) return 1;                               // the N x N MFMA tiles are built for teams of up to 128 agents
    const FwdTile t = fwd_tile(N);
    auto tile = [&](auto K) {
        using std::integral_constant;
        if constexpr (QUAD) {
            if (t.quad) return f(K, integral_constant<int, -1>{}, integral_constant<int, 4>{});
        }
        if (t.mk == 0) return f(K, integral_constant<int, 0>{}, integral_constant<int, 4>{});
        if (t.mk == 25)
            return t.w8 ? f(K, integral_constant<int, 15>{}, integral_constant<int, 8>{}) : f(K, integral_constant<int, 25>{}, integral_constant<int, 4>{});
        return f(K, integral_constant<int, 32>{}, integral_constant<int, 8>{});
    };
    switch (k) {      // obs dims of the reference scenarios: PP sen1 21, CO sen1 29, PP sen2 53, CO sen2 77 (+clock 78)
    case 32: return tile(std::integral_constant<int, 32>{});
    case 64: return tile(std::integral_constant<int, 64>{});
    case K2: return tile(std::integral_constant<int, K2>{});
    default: return 1;
    }
}

}  // namespace cm
