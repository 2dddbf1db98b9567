// cm_policy_hm.hip - the f16-split policy forward (cm_policy_h_dev.h) for SEVERAL policies in one launch (cm_policy_forward_multi): K
// policies of one architecture, each acting on its own contiguous range of the envs.  The workgroup-tiled body already owns whole
// envs per workgroup, so a workgroup only has to be told whose weights to use: it reads (member, block inside the member's group)
// from a device table, points the argument block at the group and the weight pointers at the member's operand pack, and from there
// runs fwd_h_kernel's body unchanged - every env's arithmetic and Philox draws are those of a cm_policy_forward launch on the
// group's rows with env_id_offset + the group's first env.  Teams of 4 keep cm_rollout_chunk_multi (cm_rollout_wm.hip).
#include "cm_internal.h"
#include "cm_rng.h"
#include "cm_policy_host.h"

namespace cm {
namespace mh {

// the table's records as the kernel reads them (the ABI's cm_forward_set_wg / cm_forward_set_member, include/commarl.h)
struct SetWg { int32_t member, block; };
struct SetMember {
    int32_t first_env, n_envs;
    const uint4 *pack;                                   // the member's f16-split fragments (pack_layout_h offsets from here)
    const float *enc_b1, *enc_b2, *gcn_b, *hd_b1, *hd_b2, *hd_b3, *hd_b4;   // biases live in the member's flat weight copy
};
static_assert(sizeof(SetWg) == sizeof(cm_forward_set_wg) && sizeof(SetMember) == sizeof(cm_forward_set_member), "table records are the ABI's");
// pack_layout_h of the shared shape, in uint4 units (enc1 sits at 0)
struct SetOffs { unsigned enc2, attn, gcn, x1, h2, h3, h4; };

// Policy head only.  SAVES = false: the acting forward stores no activations, and the rebased copy of the argument block then has
// no dynamically indexed member (it stays in registers).
template <int KH, int MAXMK, int NW>
__global__ __launch_bounds__(64 * NW) void fwd_h_set_kernel(FwdArgs a, const SetWg *__restrict__ wgs, const SetMember *__restrict__ members,
                                                           SetOffs o, int n_act) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_h[];
    const SetWg wg = wgs[blockIdx.x];
    const int k = __builtin_amdgcn_readfirstlane(wg.member), blk = __builtin_amdgcn_readfirstlane(wg.block);
    const SetMember &m = members[k];
    const int first = __builtin_amdgcn_readfirstlane(m.first_env);
    const uint4 *P = uniform_global(m.pack);
    const TrunkH tw{ P, uniform_global(m.enc_b1), P + o.enc2, uniform_global(m.enc_b2), P + o.attn, P + o.gcn, uniform_global(m.gcn_b) };
    const PolHeadH ph{ P + o.x1, uniform_global(m.hd_b1), P + o.h2, uniform_global(m.hd_b2), P + o.h3, uniform_global(m.hd_b3),
                       P + o.h4, uniform_global(m.hd_b4), n_act };
    // the group as a batch of its own: every pointer the body indexes by env advanced to the group's first env
    const size_t rows0 = (size_t)first * a.N, nn0 = rows0 * a.N;
    a.obs += rows0 * a.d;
    if (a.avail) a.avail += rows0 * n_act;
    if (a.adj) a.adj += nn0;
    if (a.chan) a.chan += nn0 * a.L;
    if (a.actions) a.actions += rows0;
    if (a.probs) a.probs += rows0 * n_act;
    if (a.attn) a.attn += nn0;
    a.S = __builtin_amdgcn_readfirstlane(m.n_envs);
    a.env_id_offset += first;
    fwd_body_h<0, KH, MAXMK, NW, false>(a, tw, ph, CritHeadH{}, lds_h, blk, nullptr);
}

// the families dispatch_h (cm_policy_h.hip) selects for teams that are not 4, policy head
static int dispatch_set(const FwdArgs &a, const SetWg *wgs, const SetMember *members, int n_wg, const SetOffs &o, int n_act, size_t lds,
                        void *stream) {
    return for_fwd_variant<96, false>(kh_of(a.d), a.N, [&](auto K, auto MK, auto NW) {
        return launch_lds<&fwd_h_set_kernel<K.value, MK.value, NW.value>>(dim3(n_wg), dim3(64 * NW.value), lds, stream, a, wgs, members, o, n_act);
    });
}

}  // namespace mh

// The shapes with a set kernel: what cm_policy_forward runs on fwd_h_kernel's non-quad families, up to 80 agents.  Larger teams are
// the ones a host runs layer by layer (nets.py: one env's planes and scores exceed the LDS tile from 84 agents on), so a set launch
// would have no member-by-member twin to equal there.  0 = no set kernel; else the LDS bytes of a workgroup.
static size_t forward_set_lds(const cm_policy_weights *w) {
    if (!policy_set_enabled() || !policy_shape_ok(w) || !mh::kh_of(w->d)) return 0;
    const int N = w->n_agents;
    if (N == 4 || N > 80) return 0;
    const int epb = mf::pick_epb(N), rows_cap = (epb * N + 15) & ~15;
    const size_t lds = mh::lds_map(rows_cap, epb, N, N < 16 ? 0 : 1).total;
    return lds > 160 * 1024 ? 0 : lds;
}

}  // namespace cm

using namespace cm;

static bool same_shape(const cm_policy_weights &x, const cm_policy_weights &y) {
    return x.d == y.d && x.n_agents == y.n_agents && x.n_hops == y.n_hops && x.enc_hidden == y.enc_hidden && x.emb == y.emb && x.h1 == y.h1 &&
           x.h2 == y.h2 && x.h3 == y.h3 && x.n_act == y.n_act && x.no_residual == y.no_residual;
}

extern "C" int64_t cm_policy_forward_multi_plan(const cm_policy_weights *members, const int32_t *group_sizes, int32_t n_policies, int32_t n_envs,
                                                void *image, size_t image_bytes, int32_t *n_wg_out) {
    const char *who = "cm_policy_forward_multi_plan";
    if (!members || !group_sizes || !n_wg_out) return set_error(CM_ERR_ARG, std::string(who) + ": null argument");
    if (n_policies < 1) return set_error(CM_ERR_ARG, std::string(who) + ": a policy set has at least one member");
    long long sum = 0, n_wg = 0;
    const int epb = mf::pick_epb(members[0].n_agents > 0 ? members[0].n_agents : 1);
    for (int k = 0; k < n_policies; ++k) {
        if (group_sizes[k] < 1) return set_error(CM_ERR_ARG, std::string(who) + ": every member needs at least one env");
        if (!same_shape(members[k], members[0])) return set_error(CM_ERR_ARG, std::string(who) + ": the members differ in shape");
        if (!members[k].mfma_pack) return set_error(CM_ERR_ARG, std::string(who) + ": a member has no operand pack (cm_policy_pack)");
        if (!members[k].enc_b1 || !members[k].enc_b2 || !members[k].hd_b1 || !members[k].hd_b2 || !members[k].hd_b3 || !members[k].hd_b4)
            return set_error(CM_ERR_ARG, std::string(who) + ": a member has a null bias");
        sum += group_sizes[k];
        n_wg += (group_sizes[k] + epb - 1) / epb;        // a ragged last workgroup per group: none is shared with the next member
    }
    if (sum != n_envs) return set_error(CM_ERR_ARG, std::string(who) + ": the group sizes must sum to n_envs");
    if (!forward_set_lds(&members[0])) { *n_wg_out = 0; return 0; }
    const size_t need = (size_t)n_wg * sizeof(cm_forward_set_wg) + (size_t)n_policies * sizeof(cm_forward_set_member);
    *n_wg_out = (int32_t)n_wg;
    if (!image) return (int64_t)need;
    if (image_bytes < need) return set_error(CM_ERR_ARG, std::string(who) + ": image buffer too small");
    cm_forward_set_wg *wg = reinterpret_cast<cm_forward_set_wg *>(image);
    cm_forward_set_member *mem = reinterpret_cast<cm_forward_set_member *>(wg + n_wg);
    int32_t first = 0;
    for (int k = 0; k < n_policies; ++k) {
        const cm_policy_weights &w = members[k];
        const int blocks = (group_sizes[k] + epb - 1) / epb;
        for (int b = 0; b < blocks; ++b) *wg++ = cm_forward_set_wg{ k, b };
        mem[k] = cm_forward_set_member{ first, group_sizes[k], pack_sections(&w).h(), w.enc_b1, w.enc_b2, w.gcn_b, w.hd_b1, w.hd_b2, w.hd_b3, w.hd_b4 };
        first += group_sizes[k];
    }
    return (int64_t)need;
}

extern "C" int cm_policy_forward_multi(const cm_policy_weights *shape, const void *table_dev, int32_t n_wg, int32_t n_envs, const float *obs,
                                       const float *avail, const float *dist_adj, const float *channels, uint64_t seed, int32_t env_id_offset,
                                       uint32_t policy_step, const uint32_t *policy_step_base, int32_t greedy, int32_t *actions, float *probs,
                                       float *attn, void *stream) {
    if (!shape || !obs) return set_error(CM_ERR_ARG, "cm_policy_forward_multi: null weights / obs");
    if (n_envs <= 0) return CM_OK;
    if (!shape->mfma_pack) return 1;
    const size_t lds = forward_set_lds(shape);
    if (!lds) return 1;
    const int epb = mf::pick_epb(shape->n_agents);
    if (!table_dev || n_wg < (n_envs + epb - 1) / epb || n_wg > n_envs)
        return set_error(CM_ERR_ARG, "cm_policy_forward_multi: null table, or n_wg is not the planner's for n_envs");
    mf::FwdArgs a = fwd_args(fwd_shape(shape, n_envs), obs, dist_adj, channels, attn,
                             FwdSampler{ avail, seed, env_id_offset, policy_step, policy_step_base, greedy, actions, probs });
    a.EPB = epb;
    const mh::PackLayoutH lo = layout_h(shape);
    const mh::SetOffs o{ (unsigned)lo.enc2, (unsigned)lo.attn, (unsigned)lo.gcn, (unsigned)lo.x1, (unsigned)lo.h2, (unsigned)lo.h3, (unsigned)lo.h4 };
    const mh::SetWg *wgs = reinterpret_cast<const mh::SetWg *>(table_dev);
    return mh::dispatch_set(a, wgs, reinterpret_cast<const mh::SetMember *>(wgs + n_wg), n_wg, o, shape->n_act, lds, stream);
}
