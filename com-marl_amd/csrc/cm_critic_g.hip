// cm_critic_g.hip - Comm-DP critic forward ('sum' aggregator) for nets of ANY layer sizes, in one launch (gfx950).
//
// The critic's trunk is the policy's (cm_policy_g.hip); its head is the decoder baseline_aggregator._mean_module with one
// output column, and values[s] is the sum of the env's per-agent outputs, taken in agent order by one thread per env.  The
// kernel is the CRITIC instantiation of fwd_any_kernel (cm_policy_g_dev.h): same LDS map, same dense layers.
#include "cm_policy_g_dev.h"

using namespace cm;

extern "C" int cm_critic_forward_any(const cm_net_weights *w, int32_t n_samples, const float *obs, const float *dist_adj,
                                     const float *channels, float *values, void *stream) {
    if (!w || !obs || !values) return set_error(CM_ERR_ARG, "cm_critic_forward_any: null weights / obs / values");
    if (w->n_act != 1) return set_error(CM_ERR_ARG, "cm_critic_forward_any: n_act must be 1 (slot n_head is the [K,1] output layer)");
    if (n_samples <= 0) return CM_OK;
    pg::Args a{};
    pg::Plan p;
    if (const int rc = pg::fill("cm_critic_forward_any", w, n_samples, a, p)) return rc;
    a.obs = obs; a.adj = dist_adj; a.chan = channels;
    a.values = values;

    return launch_lds<&pg::fwd_any_kernel<true>>(dim3((a.S + a.EPB - 1) / a.EPB), dim3(pg::TPB), p.lds_bytes, stream, a);
}
