// cm_policy_g.hip - Comm-DP policy forward + sample for nets of ANY layer sizes, in one launch (gfx950).
//
// cm_policy_forward (cm_policy*.hip) is built for the reference's default shape (128 | 64 | 128,64,32) and carries its
// weights as pre-packed fragments.  The runners take the shape from the command line (--encoder_hidden_sizes,
// --embedding_dim, --categorical_mlp_hidden_sizes, exp_runners/env_uitils.py:83-90): this unit runs every such shape -
// 1..3 encoder hidden layers, 1..4 head hidden layers, every width and the embedding in 1..128 - with run-time sizes and
// the plain [in,out] weights.  Kernel and LDS map: cm_policy_g_dev.h.
#include "cm_policy_g_dev.h"

using namespace cm;

extern "C" int cm_policy_forward_any(const cm_net_weights *w, int32_t n_samples, const float *obs, const float *avail,
                                     const float *dist_adj, const float *channels, uint64_t seed, int32_t env_id_offset,
                                     uint32_t policy_step, const uint32_t *policy_step_base, int32_t greedy,
                                     int32_t *actions, float *probs, float *attn, void *stream) {
    if (!w || !obs) return set_error(CM_ERR_ARG, "cm_policy_forward_any: null weights / obs");
    if (n_samples <= 0) return CM_OK;
    pg::Args a{};
    pg::Plan p;
    if (const int rc = pg::fill("cm_policy_forward_any", w, n_samples, a, p)) return rc;
    a.obs = obs; a.avail = avail; a.adj = dist_adj; a.chan = channels;
    a.key0 = (uint32_t)seed; a.key1 = (uint32_t)(seed >> 32); a.policy_step = policy_step; a.step_base = policy_step_base;
    a.env_id_offset = env_id_offset; a.greedy = greedy;
    a.actions = actions; a.probs = probs; a.attn = attn;

    return launch_lds<&pg::fwd_any_kernel<false>>(dim3((a.S + a.EPB - 1) / a.EPB), dim3(pg::TPB), p.lds_bytes, stream, a);
}
