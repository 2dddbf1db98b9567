// cm_policy_g.hip - Comm-DP policy forward + sample for nets of ANY layer sizes, in one launch (gfx950).
//
// cm_policy_forward (cm_policy*.hip) is built for the reference's default shape (128 | 64 | 128,64,32) and carries its
// weights as pre-packed fragments.  The runners take the shape from the command line (--encoder_hidden_sizes,
// --embedding_dim, --categorical_mlp_hidden_sizes, exp_runners/env_uitils.py:83-90): this unit runs every such shape -
// 1..3 encoder hidden layers, 1..4 head hidden layers, every width and the embedding in 1..128 - with run-time sizes and
// the plain [in,out] weights.  Kernel and LDS map: cm_policy_g_dev.h.
#include "cm_policy_g_dev.h"

using namespace cm;

static bool width_ok(int w) { return w >= 1 && w <= pg::MAX_W; }

extern "C" int cm_policy_forward_any(const cm_net_weights *w, int32_t n_samples, const float *obs, const float *avail,
                                     const float *dist_adj, const float *channels, uint64_t seed, int32_t env_id_offset,
                                     uint32_t policy_step, const uint32_t *policy_step_base, int32_t greedy,
                                     int32_t *actions, float *probs, float *attn, void *stream) {
    if (!w || !obs) return set_error(CM_ERR_ARG, "cm_policy_forward_any: null weights / obs");
    if (n_samples <= 0) return CM_OK;
    // outside the bounds the kernel is written for: "not for this shape", nothing launched
    if (w->n_enc < 1 || w->n_enc > pg::MAX_ENC || w->n_head < 1 || w->n_head > pg::MAX_HEAD) return 1;
    if (!width_ok(w->emb) || !width_ok(w->d) || w->n_act < 1 || w->n_act > pg::MAX_ACT || w->n_agents < 1 || w->n_hops < 0) return 1;
    int widest = w->emb;
    for (int i = 0; i < w->n_enc; ++i) { if (!width_ok(w->enc_hidden[i])) return 1; widest = widest > w->enc_hidden[i] ? widest : w->enc_hidden[i]; }
    for (int i = 0; i < w->n_head; ++i) { if (!width_ok(w->head_hidden[i])) return 1; widest = widest > w->head_hidden[i] ? widest : w->head_hidden[i]; }
    const pg::Plan p = pg::plan(w->n_agents, w->d, w->emb, widest);
    if (p.lds_bytes > pg::LDS_LIMIT) return 1;
    for (int i = 0; i <= w->n_enc; ++i)
        if (!w->enc_wt[i]) return set_error(CM_ERR_ARG, "cm_policy_forward_any: null encoder weight");
    for (int i = 0; i <= w->n_head; ++i)
        if (!w->head_wt[i]) return set_error(CM_ERR_ARG, "cm_policy_forward_any: null head weight");
    if (w->n_hops > 0 && !w->gcn_w) return set_error(CM_ERR_ARG, "cm_policy_forward_any: null gcn_w");

    pg::Args a{};
    a.S = n_samples; a.N = w->n_agents; a.d = w->d; a.L = w->n_hops; a.A = w->n_act; a.emb = w->emb;
    a.no_residual = w->no_residual;
    a.n_enc = w->n_enc; a.n_head = w->n_head;
    for (int i = 0; i < w->n_enc; ++i) { a.enc_h[i] = w->enc_hidden[i]; a.enc_w[i] = w->enc_wt[i]; a.enc_b[i] = w->enc_b[i]; }
    a.enc_wo = w->enc_wt[w->n_enc]; a.enc_bo = w->enc_b[w->n_enc];
    for (int i = 0; i < w->n_head; ++i) { a.head_h[i] = w->head_hidden[i]; a.head_w[i] = w->head_wt[i]; a.head_b[i] = w->head_b[i]; }
    a.head_wo = w->head_wt[w->n_head]; a.head_bo = w->head_b[w->n_head];
    a.attn_wt = w->attn_wt; a.gcn_w = w->gcn_w; a.gcn_b = w->gcn_b;
    a.EPB = p.EPB; a.R16 = p.R16; a.SE = p.SE; a.SW = p.SW; a.NP = p.NP;
    a.obs = obs; a.avail = avail; a.adj = dist_adj; a.chan = channels;
    a.key0 = (uint32_t)seed; a.key1 = (uint32_t)(seed >> 32); a.policy_step = policy_step; a.step_base = policy_step_base;
    a.env_id_offset = env_id_offset; a.greedy = greedy;
    a.actions = actions; a.probs = probs; a.attn = attn;

    static unsigned long long attr_set = 0;
    if (dev_first(attr_set))
        CM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&pg::fwd_any_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)pg::LDS_LIMIT));
    const int blocks = (a.S + a.EPB - 1) / a.EPB;
    hipLaunchKernelGGL(pg::fwd_any_kernel, dim3(blocks), dim3(pg::TPB), p.lds_bytes, (hipStream_t)stream, a);
    CM_HIP(hipGetLastError());
    return CM_OK;
}
