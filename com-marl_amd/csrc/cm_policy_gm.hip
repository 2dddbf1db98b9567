// cm_policy_gm.hip - the run-time-sized Comm-DP policy forward (cm_policy_g_dev.h) for SEVERAL policies in one launch
// (cm_policy_forward_any_multi): K policies that share the team, the observation, the hops and the actions but NOT the layer
// sizes, each acting on its own contiguous range of the envs.  fwd_any_kernel is sized from its argument block and a workgroup
// owns whole envs, so a workgroup only has to be told whose net to run: it reads (member, block inside the member's group) and
// the member's record - sizes, plane strides, weight pointers - from a device table through scalar loads, builds its own
// argument block, points it at the group and from there runs trunk(), head() and the sampler tail (cm_policy_g_tail.h) unchanged.  Every env's
// arithmetic and Philox draws are those of a cm_policy_forward_any launch on the group's rows with env_id_offset + the
// group's first env.  This is cm_policy_hm.hip's move for the default shape, with the shape in the record as well.
#include <stddef.h>

#include <vector>

#include "cm_policy_g_dev.h"

namespace cm {
namespace pgm {

// the table's records as the kernel reads them (the ABI's cm_forward_set_wg / cm_any_set_member, include/commarl.h)
struct SetWg { int32_t member, block; };
struct SetMember {
    int32_t first_env, n_envs;
    int32_t emb, no_residual;
    int32_t n_enc, enc_h[pg::MAX_ENC];
    int32_t n_head, head_h[pg::MAX_HEAD];
    int32_t SE, SW;
    int32_t _pad;
    const float *enc_w[pg::MAX_ENC], *enc_b[pg::MAX_ENC], *enc_wo, *enc_bo;
    const float *attn_wt, *gcn_w, *gcn_b;
    const float *head_w[pg::MAX_HEAD], *head_b[pg::MAX_HEAD], *head_wo, *head_bo;
};
static_assert(sizeof(SetWg) == sizeof(cm_forward_set_wg) && sizeof(SetMember) == sizeof(cm_any_set_member), "table records are the ABI's");
static_assert(offsetof(SetMember, enc_w) == offsetof(cm_any_set_member, enc_w) && offsetof(SetMember, head_bo) == offsetof(cm_any_set_member, head_bo),
              "table records are the ABI's");

// `a` carries what the members share (N, d, L, A, the plan's EPB / R16 / NP, the batch's pointers and sampler counters); the
// sizes, strides and weights come from the member's record.  Every slot of the record is named by a constant index (the loops
// are unrolled), so the rebuilt argument block stays in registers.
__global__ __launch_bounds__(pg::TPB) void fwd_any_set_kernel(pg::Args a, const SetWg *__restrict__ wgs, const SetMember *__restrict__ members) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const SetWg wg = wgs[blockIdx.x];
    const int k = __builtin_amdgcn_readfirstlane(wg.member), blk = __builtin_amdgcn_readfirstlane(wg.block);
    const SetMember &m = members[k];
    const int first = __builtin_amdgcn_readfirstlane(m.first_env);
    a.emb = __builtin_amdgcn_readfirstlane(m.emb);
    a.no_residual = __builtin_amdgcn_readfirstlane(m.no_residual);
    a.n_enc = __builtin_amdgcn_readfirstlane(m.n_enc);
    a.n_head = __builtin_amdgcn_readfirstlane(m.n_head);
    a.SE = __builtin_amdgcn_readfirstlane(m.SE);
    a.SW = __builtin_amdgcn_readfirstlane(m.SW);
#pragma unroll
    for (int i = 0; i < pg::MAX_ENC; ++i) {
        a.enc_h[i] = __builtin_amdgcn_readfirstlane(m.enc_h[i]);
        a.enc_w[i] = uniform_global(m.enc_w[i]);
        a.enc_b[i] = uniform_global(m.enc_b[i]);
    }
    a.enc_wo = uniform_global(m.enc_wo); a.enc_bo = uniform_global(m.enc_bo);
    a.attn_wt = uniform_global(m.attn_wt); a.gcn_w = uniform_global(m.gcn_w); a.gcn_b = uniform_global(m.gcn_b);
#pragma unroll
    for (int i = 0; i < pg::MAX_HEAD; ++i) {
        a.head_h[i] = __builtin_amdgcn_readfirstlane(m.head_h[i]);
        a.head_w[i] = uniform_global(m.head_w[i]);
        a.head_b[i] = uniform_global(m.head_b[i]);
    }
    a.head_wo = uniform_global(m.head_wo); a.head_bo = uniform_global(m.head_bo);
    // the group as a batch of its own: every pointer the body indexes by env advanced to the group's first env
    const size_t rows0 = (size_t)first * a.N, nn0 = rows0 * a.N;
    a.obs += rows0 * a.d;
    if (a.avail) a.avail += rows0 * a.A;
    if (a.adj) a.adj += nn0;
    if (a.chan) a.chan += nn0 * a.L;
    if (a.actions) a.actions += rows0;
    if (a.probs) a.probs += rows0 * a.A;
    if (a.attn) a.attn += nn0;
    a.S = __builtin_amdgcn_readfirstlane(m.n_envs);
    a.env_id_offset += first;
    using namespace pg;                                  // (the tail names TPB, MAX_ACT and the Philox helpers as the header does)
    const int tid = threadIdx.x, N = a.N, SW = a.SW;
    const Tile t = trunk(a, lds, tid, blk);
    const int s0 = t.s0, rows = t.rows;
    const int nxt = head(a, lds, t, tid);
#include "cm_policy_g_tail.h"
}

}  // namespace pgm
}  // namespace cm

using namespace cm;

extern "C" int64_t cm_policy_forward_any_multi_plan(const cm_net_weights *members, const int32_t *group_sizes, int32_t n_policies,
                                                    int32_t n_envs, void *image, size_t image_bytes, int32_t *n_wg_out,
                                                    size_t *lds_bytes_out) {
    const char *who = "cm_policy_forward_any_multi_plan";
    if (!members || !group_sizes || !n_wg_out || !lds_bytes_out) return set_error(CM_ERR_ARG, std::string(who) + ": null argument");
    if (n_policies < 1) return set_error(CM_ERR_ARG, std::string(who) + ": a policy set has at least one member");
    const cm_net_weights &w0 = members[0];
    long long sum = 0;
    for (int k = 0; k < n_policies; ++k) {
        const cm_net_weights &w = members[k];
        if (group_sizes[k] < 1) return set_error(CM_ERR_ARG, std::string(who) + ": every member needs at least one env");
        if (w.n_agents != w0.n_agents || w.d != w0.d || w.n_hops != w0.n_hops || w.n_act != w0.n_act)
            return set_error(CM_ERR_ARG, std::string(who) + ": the members differ in n_agents, d, n_hops or n_act");
        sum += group_sizes[k];
    }
    if (sum != n_envs) return set_error(CM_ERR_ARG, std::string(who) + ": the group sizes must sum to n_envs");
    // every member through the single launch's own fill(): its bounds, its LDS need, its null checks
    std::vector<pg::Args> args((size_t)n_policies);
    bool fits = true;
    size_t lds = 0;
    for (int k = 0; k < n_policies; ++k) {
        pg::Plan p{};
        const int rc = pg::fill(who, &members[k], group_sizes[k], args[(size_t)k], p);
        if (rc < 0) return rc;
        if (rc == 1) fits = false;
        lds = p.lds_bytes > lds ? p.lds_bytes : lds;        // (an out-of-bounds member leaves its plan at 0)
    }
    if (!fits) { *n_wg_out = 0; *lds_bytes_out = lds > pg::LDS_LIMIT ? lds : 0; return 0; }
    const int epb = args[0].EPB;
    long long n_wg = 0;
    for (int k = 0; k < n_policies; ++k) n_wg += (group_sizes[k] + epb - 1) / epb;   // a ragged last workgroup per group: none is shared
    const size_t need = (size_t)n_wg * sizeof(cm_forward_set_wg) + (size_t)n_policies * sizeof(cm_any_set_member);
    *n_wg_out = (int32_t)n_wg;
    *lds_bytes_out = lds;
    if (!image) return (int64_t)need;
    if (image_bytes < need) return set_error(CM_ERR_ARG, std::string(who) + ": image buffer too small");
    cm_forward_set_wg *wg = reinterpret_cast<cm_forward_set_wg *>(image);
    cm_any_set_member *mem = reinterpret_cast<cm_any_set_member *>(wg + n_wg);
    int32_t first = 0;
    for (int k = 0; k < n_policies; ++k) {
        const pg::Args &a = args[(size_t)k];
        const int blocks = (group_sizes[k] + epb - 1) / epb;
        for (int b = 0; b < blocks; ++b) *wg++ = cm_forward_set_wg{ k, b };
        cm_any_set_member r{};
        r.first_env = first; r.n_envs = group_sizes[k];
        r.emb = a.emb; r.no_residual = a.no_residual;
        r.n_enc = a.n_enc; r.n_head = a.n_head;
        for (int i = 0; i < pg::MAX_ENC; ++i) { r.enc_h[i] = a.enc_h[i]; r.enc_w[i] = a.enc_w[i]; r.enc_b[i] = a.enc_b[i]; }
        for (int i = 0; i < pg::MAX_HEAD; ++i) { r.head_h[i] = a.head_h[i]; r.head_w[i] = a.head_w[i]; r.head_b[i] = a.head_b[i]; }
        r.SE = a.SE; r.SW = a.SW;
        r.enc_wo = a.enc_wo; r.enc_bo = a.enc_bo;
        r.attn_wt = a.attn_wt; r.gcn_w = a.gcn_w; r.gcn_b = a.gcn_b;
        r.head_wo = a.head_wo; r.head_bo = a.head_bo;
        mem[k] = r;
        first += group_sizes[k];
    }
    return (int64_t)need;
}

extern "C" int cm_policy_forward_any_multi(const cm_net_weights *shape, const void *table_dev, int32_t n_wg, int32_t n_envs,
                                           size_t lds_bytes, const float *obs, const float *avail, const float *dist_adj,
                                           const float *channels, uint64_t seed, int32_t env_id_offset, uint32_t policy_step,
                                           const uint32_t *policy_step_base, int32_t greedy, int32_t *actions, float *probs,
                                           float *attn, void *stream) {
    const char *who = "cm_policy_forward_any_multi";
    if (!shape || !obs) return set_error(CM_ERR_ARG, std::string(who) + ": null weights / obs");
    if (n_envs <= 0) return CM_OK;
    pg::Args a{};
    pg::Plan p{};
    if (const int rc = pg::fill(who, shape, n_envs, a, p)) return rc;
    if (lds_bytes == 0 || lds_bytes > pg::LDS_LIMIT) return 1;          // the planner's answer for a set it declines
    if (!table_dev || n_wg < (n_envs + p.EPB - 1) / p.EPB || n_wg > n_envs)
        return set_error(CM_ERR_ARG, std::string(who) + ": null table, or n_wg is not the planner's for n_envs");
    if (lds_bytes < p.lds_bytes) return set_error(CM_ERR_ARG, std::string(who) + ": lds_bytes is below the need of `shape` itself");
    a.obs = obs; a.avail = avail; a.adj = dist_adj; a.chan = channels;
    a.key0 = (uint32_t)seed; a.key1 = (uint32_t)(seed >> 32); a.policy_step = policy_step; a.step_base = policy_step_base;
    a.env_id_offset = env_id_offset; a.greedy = greedy;
    a.actions = actions; a.probs = probs; a.attn = attn;

    const pgm::SetWg *wgs = reinterpret_cast<const pgm::SetWg *>(table_dev);
    return launch_lds<&pgm::fwd_any_set_kernel>(dim3(n_wg), dim3(pg::TPB), lds_bytes, stream, a, wgs, reinterpret_cast<const pgm::SetMember *>(wgs + n_wg));
}
