// cm_policy_mfma.hip - fused Comm-DP policy / critic forward on the gfx950 matrix cores.
//
// Same computation and C-ABI as cm_policy.hip (reference:
// com_marl/torch/policies/comm_categorical_mlp_policy.py:48-119, modules/comm_base_net.py:80-108,
// attention_module.py:26-51, graph_conv_module.py:51-72, baselines/comm_base_critic.py:91-114),
// with every dense per-agent layer on v_mfma_f32_16x16x4_f32 (f32 in / f32 accumulate: exact
// f32, needed for the 1e-5 parity bar; this is the 157 TFLOP/s roof the kernel is priced on).
//
// Work decomposition (256 threads = 4 waves per workgroup, EPB whole envs = rows agent rows):
//   * activations live in LDS [rows_pad][stride] with stride == 2 (mod 32) words, so the A-operand
//     read  A[row = lane&15][k = 4*kk + (lane>>4)]  is bank-conflict free;
//   * a wave owns 1-2 column tiles (16 outputs) of a layer and ALL row tiles: its B fragments
//     (weights, k-major [in][out], read from L2 once per layer per wave) sit in registers for the
//     whole layer, two row tiles are accumulated alternately so the 40-cycle dependent-accumulator
//     latency of the 16x16x4 instruction is covered by the 32-cycle issue of the other tile;
//   * the tiny per-env parts (N x N attention softmax, mask + renorm, A.(HW), 32->5 head,
//     categorical sample) stay on the VALU against the same LDS tiles.
// HBM traffic is the algorithmic minimum: obs (+ masks) in, actions / probs / attention out.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "cm_internal.h"
#include "cm_rng.h"
#include "cm_policy_host.h"

namespace cm {
namespace mf {

template <int HEAD, int KPAD, int MAXMK, int NW>
__global__ __launch_bounds__(64 * NW) void fwd_mfma_kernel(FwdArgs a, TrunkW tw, PolHead ph, CritHead chd) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    fwd_body<HEAD, KPAD, MAXMK, NW>(a, tw, ph, chd, lds, blockIdx.x, nullptr);
}


template <int HEAD, int KPAD, int MAXMK, int NW>
static int launch(FwdArgs a, const TrunkW &tw, const PolHead &ph, const CritHead &chd, void *stream) {
    a.EPB = pick_epb(a.N);
    const int rows_cap = (a.EPB * a.N + 15) & ~15;
    const size_t lds = lds_floats(rows_cap, a.EPB, a.N) * sizeof(float);
    if (lds > 160 * 1024) return set_error(CM_ERR_ARG, "policy forward: n_agents too large for the 160 KB LDS tile");
    const int blocks = (a.S + a.EPB - 1) / a.EPB;
    constexpr auto KERN = &fwd_mfma_kernel<HEAD, KPAD, MAXMK, NW>;
    static const bool want_probe = getenv("COMMARL_FWD_PROBE") != nullptr;
    if (want_probe) {                                    // diagnostic: per-phase shader clocks, averaged over workgroups
        unsigned long long *dbuf = nullptr;
        const size_t nb = (size_t)blocks * NPROBE * sizeof(unsigned long long);
        CM_HIP(hipMalloc(&dbuf, nb));
        CM_HIP(hipMemset(dbuf, 0, nb));
        a.probe = dbuf;
        for (int rep = 0; rep < 3; ++rep)
            if (int rc = launch_lds<KERN>(dim3(blocks), dim3(64 * NW), lds, stream, a, tw, ph, chd)) return rc;
        CM_HIP(hipDeviceSynchronize());
        std::vector<unsigned long long> h((size_t)blocks * NPROBE);
        CM_HIP(hipMemcpy(h.data(), dbuf, nb, hipMemcpyDeviceToHost));
        CM_HIP(hipFree(dbuf));
        double sum[NPROBE] = { 0 }; int cnt[NPROBE] = { 0 };
        unsigned long long tmin = ~0ull, tmax = 0;
        for (int b = 0; b < blocks; ++b) {
            int prev = 0;
            tmin = std::min(tmin, h[(size_t)b * NPROBE]);
            for (int i = 1; i < NPROBE; ++i) {
                const unsigned long long t = h[(size_t)b * NPROBE + i];
                if (!t) continue;
                sum[i] += (double)(t - h[(size_t)b * NPROBE + prev]); ++cnt[i]; prev = i; tmax = std::max(tmax, t);
            }
        }
        fprintf(stderr, "[fwd probe] HEAD=%d blocks=%d span=%llu clk; mean clk per phase:", HEAD, blocks, tmax - tmin);
        for (int i = 1; i < NPROBE; ++i) if (cnt[i]) fprintf(stderr, " p%d=%.0f", i, sum[i] / cnt[i]);
        fprintf(stderr, "\n");
        return CM_OK;
    }
    return launch_lds<KERN>(dim3(blocks), dim3(64 * NW), lds, stream, a, tw, ph, chd);
}

// 1 = no instantiation: the caller falls back to the generic VALU kernel
template <int HEAD>
static int dispatch(const FwdArgs &a, const TrunkW &tw, const PolHead &ph, const CritHead &chd, void *stream) {
    return for_fwd_variant<80>(kpad_of(a.d), a.N, [&](auto K, auto MK, auto NW) { return launch<HEAD, K.value, MK.value, NW.value>(a, tw, ph, chd, stream); });
}

// ---- operand pack ---------------------------------------------------------------------------------------------
// dst[((ct*KQ + kq)*64 + lane)*4 + j] = Wt[k = 16kq + 4(lane>>4) + j][col = 16ct + (lane&15)], zero outside [K, OUT]
__global__ void pack_layer_kernel(const float *__restrict__ Wt, int K, int OUT, int KQ, int CT, float *__restrict__ dst) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= CT * KQ * 256) return;
    const int j = idx & 3, lane = (idx >> 2) & 63, blk = idx >> 8, kq = blk % KQ, ct = blk / KQ;
    const int k = 16 * kq + 4 * (lane >> 4) + j, col = 16 * ct + (lane & 15);
    dst[idx] = (k < K && col < OUT) ? Wt[(size_t)k * OUT + col] : 0.0f;
}



int pack_one(const float *Wt, int K, int OUT, int kpad, int out_pad, float *dst, void *stream) {
    if (!Wt) return set_error(CM_ERR_ARG, "weight pack: null layer weight");
    const int KQ = kpad / 16, CT = out_pad / 16, total = CT * KQ * 256;
    hipLaunchKernelGGL(pack_layer_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, Wt, K, OUT, KQ, CT, dst);
    CM_HIP(hipGetLastError());
    return CM_OK;
}

static int pack_trunk(int d, int L, const float *w1t, const float *w2t, const float *wat, const float *gw, int kpad,
                      const PackLayout &lo, float *pack, void *stream) {
    if (int rc = pack_one(w1t, d, EH, kpad, EH, pack + lo.enc1, stream)) return rc;
    if (int rc = pack_one(w2t, EH, EMB, EH, EMB, pack + lo.enc2, stream)) return rc;
    if (int rc = pack_one(wat, EMB, EMB, EMB, EMB, pack + lo.attn, stream)) return rc;
    for (int l = 0; l < L; ++l)
        if (int rc = pack_one(gw ? gw + (size_t)l * EMB * EMB : nullptr, EMB, EMB, EMB, EMB, pack + lo.gcn + (size_t)l * EMB * EMB, stream)) return rc;
    return CM_OK;
}

}  // namespace mf

bool policy_shape_ok(const cm_policy_weights *w) {
    return w && w->enc_hidden == mf::EH && w->emb == mf::EMB && w->h1 == mf::H1 && w->h2 == mf::H2 && w->h3 == mf::H3 &&
           w->n_act >= 1 && w->n_act <= mf::MAX_ACT && w->n_agents >= 1 && w->n_agents <= 128 && w->n_hops >= 0 &&
           mf::kpad_of(w->d) != 0;
}
static bool critic_shape_ok(const cm_critic_weights *w) {
    return w && w->enc_hidden == mf::EH && w->emb == mf::EMB && w->dec_hidden == mf::DH && w->n_agents >= 1 &&
           w->n_agents <= 128 && w->n_hops >= 0 && mf::kpad_of(w->d) != 0;
}

// entry points used by cm_policy.hip's C-ABI functions; return 1 when the shape has no MFMA instantiation or the
// caller supplied no operand pack (the generic VALU kernel then runs)
int policy_forward_mfma(const cm_policy_weights *w, mf::FwdArgs a, void *stream) {
    if (!w->mfma_pack || !policy_shape_ok(w)) return 1;
    { const char *e = getenv("COMMARL_FWD_STOP"); a.stop = e ? atoi(e) : 0; }
    const PackSections s = pack_sections(w);
    if (s.w_bytes) {
        const int rc = policy_forward_w(w, s.w(), a, stream);
        if (rc <= 0) return rc;
    }
    if (policy_h_enabled()) {
        const int rc = policy_forward_h(w, s.h(), a, stream);
        if (rc <= 0) return rc;
    }
    const mf::PackLayout lo = layout_f32(w);
    return mf::dispatch<0>(a, trunk_w(s.f32(), lo, w), pol_head(s.f32(), lo, w), mf::CritHead{}, stream);
}

int critic_forward_mfma(const cm_critic_weights *w, mf::FwdArgs a, void *stream) {
    if (!w->mfma_pack || !critic_shape_ok(w)) return 1;
    const PackSections s = pack_sections(w);
    if (policy_h_enabled()) {
        const int rc = critic_forward_h(w, s.h(), a, stream);
        if (rc <= 0) return rc;
    }
    const mf::PackLayout lo = layout_f32(w);
    return mf::dispatch<1>(a, trunk_w(s.f32(), lo, w), mf::PolHead{}, crit_head(s.f32(), lo, w), stream);
}

static bool saved_shape_ok(int N, int L, int d) { return N >= 1 && N <= 128 && L <= 4 && L >= 0 && d <= 96; }
// the training forward's arguments: no sampler, every activation the backward needs stored (probs: the policy's)
static mf::FwdArgs saved_args(const FwdShape &s, const float *obs, const float *adj, const float *chan, float *attn, float *values,
                              const cm_fwd_saves *sv, float *probs) {
    mf::FwdArgs a = fwd_args(s, obs, adj, chan, attn, values);
    a.sv_on = 1;
    a.sv_a1 = sv->a1; a.sv_e = sv->e; a.sv_q = sv->q; a.sv_x1 = sv->x1; a.sv_x2 = sv->x2; a.sv_x3 = sv->x3; a.sv_out = sv->out;
    for (int l = 0; l < 4; ++l) { a.sv_hw[l] = sv->hw[l]; a.sv_h[l] = sv->h[l]; }
    a.probs = probs;
    return a;
}

}  // namespace cm

using namespace cm;

extern "C" int cm_policy_forward_saved(const cm_policy_weights *w, int32_t S, const float *obs, const float *adj, const float *chan,
                                       float *attn, const cm_fwd_saves *sv, void *stream) {
    if (!w || !obs || !sv) return set_error(CM_ERR_ARG, "cm_policy_forward_saved: null argument");
    if (S <= 0) return CM_OK;
    if (!w->mfma_pack || !policy_shape_ok(w) || !saved_shape_ok(w->n_agents, w->n_hops, w->d)) return 1;
    return policy_forward_h(w, pack_sections(w).h(), saved_args(fwd_shape(w, S), obs, adj, chan, attn, nullptr, sv, sv->probs), stream);
}

extern "C" int cm_policy_forward_saved_wave(const cm_policy_weights *w, int32_t S, const float *obs, const float *adj, const float *chan,
                                            float *attn, const cm_fwd_saves *sv, void *stream) {
    if (!w || !obs || !sv) return set_error(CM_ERR_ARG, "cm_policy_forward_saved_wave: null argument");
    if (S <= 0) return CM_OK;
    if (!w->mfma_pack || !policy_shape_ok(w)) return 1;
    const PackSections s = pack_sections(w);
    if (s.w_bytes == 0) return 1;
    return policy_forward_w_train(w, s.w(), saved_args(fwd_shape(w, S), obs, adj, chan, attn, nullptr, sv, sv->probs), stream);
}

extern "C" int cm_critic_forward_saved(const cm_critic_weights *w, int32_t S, const float *obs, const float *adj, const float *chan,
                                       float *attn, float *values, const cm_fwd_saves *sv, void *stream) {
    if (!w || !obs || !sv || !values) return set_error(CM_ERR_ARG, "cm_critic_forward_saved: null argument");
    if (S <= 0) return CM_OK;
    if (!w->mfma_pack || !critic_shape_ok(w) || !saved_shape_ok(w->n_agents, w->n_hops, w->d)) return 1;
    return critic_forward_h(w, pack_sections(w).h(), saved_args(fwd_shape(w, S), obs, adj, chan, attn, values, sv, nullptr), stream);
}

extern "C" int cm_critic_forward_saved_wave(const cm_critic_weights *w, int32_t S, const float *obs, const float *adj, const float *chan,
                                            float *attn, float *values, const cm_fwd_saves *sv, void *stream) {
    if (!w || !obs || !sv) return set_error(CM_ERR_ARG, "cm_critic_forward_saved_wave: null argument");
    if (S <= 0) return CM_OK;
    if (!w->mfma_pack || !critic_shape_ok(w)) return 1;
    const PackSections s = pack_sections(w);
    if (s.w_bytes == 0) return 1;
    return critic_forward_w_train(w, s.w(), saved_args(fwd_shape(w, S), obs, adj, chan, attn, values, sv, nullptr), stream);
}

extern "C" size_t cm_policy_pack_bytes(const cm_policy_weights *w) { return policy_shape_ok(w) ? pack_sections(w).total : 0; }

extern "C" int cm_policy_pack_sections(const cm_policy_weights *w, float *pack, int32_t sections, void *stream) {
    if (!w || !pack) return set_error(CM_ERR_ARG, "cm_policy_pack: null argument");
    if (!policy_shape_ok(w)) return set_error(CM_ERR_ARG, "cm_policy_pack: this shape has no matrix-core instantiation (cm_policy_pack_bytes() == 0)");
    const int kpad = mf::kpad_of(w->d);
    const mf::PackLayout lo = layout_f32(w);
    if (sections & CM_PACK_F32) {
        if (int rc = mf::pack_trunk(w->d, w->n_hops, w->enc_w1t, w->enc_w2t, w->attn_wt, w->gcn_w, kpad, lo, pack, stream)) return rc;
        if (int rc = mf::pack_one(w->hd_w1t, mf::EMB, mf::H1, mf::EMB, mf::H1, pack + lo.x1, stream)) return rc;
        if (int rc = mf::pack_one(w->hd_w2t, mf::H1, mf::H2, mf::H1, mf::H2, pack + lo.h2, stream)) return rc;
        if (int rc = mf::pack_one(w->hd_w3t, mf::H2, mf::H3, mf::H2, mf::H3, pack + lo.h3, stream)) return rc;
        if (int rc = mf::pack_one(w->hd_w4t, mf::H3, w->n_act, mf::H3, 16, pack + lo.h4, stream)) return rc;
    }
    // the f16 (hi, lo) fragments (+ the wave-owned section), behind the f32 ones
    return policy_pack_h(w, reinterpret_cast<char *>(pack) + pack_sections(w, pack).h_off, sections, stream);
}

extern "C" int cm_policy_pack(const cm_policy_weights *w, float *pack, void *stream) {
    return cm_policy_pack_sections(w, pack, CM_PACK_ALL, stream);
}

extern "C" size_t cm_critic_pack_bytes(const cm_critic_weights *w) { return critic_shape_ok(w) ? pack_sections(w).total : 0; }

extern "C" int cm_critic_pack_sections(const cm_critic_weights *w, float *pack, int32_t sections, void *stream) {
    if (!w || !pack) return set_error(CM_ERR_ARG, "cm_critic_pack: null argument");
    if (!critic_shape_ok(w)) return set_error(CM_ERR_ARG, "cm_critic_pack: this shape has no matrix-core instantiation (cm_critic_pack_bytes() == 0)");
    const int kpad = mf::kpad_of(w->d);
    const mf::PackLayout lo = layout_f32(w);
    if (sections & CM_PACK_F32) {
        if (int rc = mf::pack_trunk(w->d, w->n_hops, w->enc_w1t, w->enc_w2t, w->attn_wt, w->gcn_w, kpad, lo, pack, stream)) return rc;
        if (int rc = mf::pack_one(w->dec_w1t, mf::EMB, mf::DH, mf::EMB, mf::DH, pack + lo.x1, stream)) return rc;
    }
    return critic_pack_h(w, reinterpret_cast<char *>(pack) + pack_sections(w, pack).h_off, sections, stream);
}

extern "C" int cm_critic_pack(const cm_critic_weights *w, float *pack, void *stream) {
    return cm_critic_pack_sections(w, pack, CM_PACK_ALL, stream);
}
