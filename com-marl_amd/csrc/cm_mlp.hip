// cm_mlp.hip - fused row-wise MLP forward on the gfx950 matrix cores for the two non-communicating
// policies of the reference and the plain Gaussian baseline:
//   * DecCategoricalMLPPolicy.get_actions  (com_marl/torch/policies/dec_categorical_mlp_policy.py:106-176):
//       per agent row  obs[d] -> 128 tanh -> 64 tanh | 32 tanh -> 5 logits -> softmax * avail, renorm, sample
//   * CentralizedCategoricalMLPPolicy.get_actions (centralized_categorical_mlp_policy.py:61-118):
//       per env row  obs[N*d] -> 128 tanh -> 64 tanh -> 32 tanh -> N*5 logits -> per-agent softmax ..., sample
//   * GaussianMLPBaseline.forward (com_marl/torch/baselines/gaussian_mlp_baseline.py:100-115):
//       per env row  obs[N*d] -> 64 tanh -> 64 tanh -> 64 tanh -> 1
// With hidden_nonlinearity=F.relu the policies' hidden layers (Obs-DP: the head's 32, CENT: all three) take ReLU instead
// of tanh: per layer, bit l of relu_mask selects it.
// Layer sizes are run-time values (cm_mlp_weights); every layer is  v_mfma_f32_16x16x4_f32  (f32 in, f32
// accumulate - the 1e-5 parity bar), 32 rows (two 16-row tiles) per 256-thread workgroup, activations ping-pong
// between two LDS tiles, the first layer streams its (possibly thousands of columns wide) input through LDS in
// 128-column chunks with the accumulators held in registers.  HBM traffic = input rows in, actions / probs /
// values out; weights are read from L2.
#include "cm_internal.h"
#include "cm_rng.h"

namespace cm {
namespace mlp {

constexpr int TPB = 256, ROWS = 32, CHUNK = 128, MAXL = CM_MLP_MAX_LAYERS, MAX_ACT = 8;
typedef float v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float fast_tanh(float x) {      // same form as cm_policy_mfma.hip (abs err <= 2e-7)
    const float t = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(t + 1.0f);
}

struct Args {
    int rows, in_dim, n_layers, tanh_mask, relu_mask, sw;
    int out_dim[MAXL];
    const float *wt[MAXL], *b[MAXL];
    const float *pk[MAXL];          // per-layer B fragments (cm_mlp_pack) or NULL: [ct][kq][lane][4], kq over ceil(K/16)
    const float *x, *avail;
    int groups, n_act, agents_per_env, env_id_offset, greedy;
    uint32_t key0, key1, policy_step;
    const uint32_t *step_base;
    int32_t *actions;
    float *probs, *values;
};

extern __shared__ float smem[];

// activation after layer l: 1 = tanh (bit l of tanh_mask), 2 = ReLU (bit l of relu_mask), 0 = none
__device__ __forceinline__ int layer_act(const Args &a, int l) {
    return ((a.tanh_mask >> l) & 1) ? 1 : (((a.relu_mask >> l) & 1) ? 2 : 0);
}

// k-slot mapping shared by A and B: lane group g = lane>>4 supplies k = 16*kq + 4*g + j at MFMA (kq, j), so a
// lane's four A words per kq are contiguous (one ds_read_b128).  ReLU as torch.relu: v < 0 ? 0 : v lets a NaN through
// (fmaxf would turn it into 0).
__device__ __forceinline__ void store_tile(float *out, int sw, int rt, int ct, int lane, const v4f &acc, float bias,
                                           int act) {
    const int c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float v = acc[r] + bias;
        out[(size_t)(rt * 16 + 4 * g + r) * sw + ct * 16 + c] = act == 1 ? fast_tanh(v) : (act == 2 ? (v < 0.0f ? 0.0f : v) : v);
    }
}

__global__ __launch_bounds__(TPB) void mlp_kernel(Args a) {
#define CM_MLP_ROW0 (blockIdx.x * ROWS)
#define CM_MLP_ROWS_LEFT (a.rows - row0)
#define CM_MLP_LAYER(l)
#define CM_MLP_HAS_PK(l) (a.pk[l])
#define CM_MLP_PK(l) (a.pk[l])
#define CM_MLP_WT(l) (a.wt[l])
#define CM_MLP_B(l) (a.b[l])
#include "cm_mlp_body.h"
#undef CM_MLP_ROW0
#undef CM_MLP_ROWS_LEFT
#undef CM_MLP_LAYER
#undef CM_MLP_HAS_PK
#undef CM_MLP_PK
#undef CM_MLP_WT
#undef CM_MLP_B
}

// ---- the same body for SEVERAL policies of one shape in one launch (cm_mlp_policy_forward_multi) ---------------------------------
// The table's records as the kernel reads them (the ABI's cm_forward_set_wg / cm_mlp_set_member, include/commarl.h).
struct SetWg { int32_t member, block; };
struct SetMember {
    int32_t first_row, n_rows, first_env, pad;
    const float *b[MAXL];                                // biases live in the member's flat weight copy
    const float *pk[MAXL];                               // per-layer B fragments inside the member's cm_mlp_pack output
};
static_assert(sizeof(SetWg) == sizeof(cm_forward_set_wg) && sizeof(SetMember) == sizeof(cm_mlp_set_member), "table records are the ABI's");

// A workgroup reads whose rows it has - (member, block inside the member's rows) - and runs mlp_kernel's body on them with the
// member's operands.  `a` is the shared shape and the whole batch's pointers and is not modified: rows are indexed in the whole
// batch (row0 = the member's first row + 32 * block), so x / avail / outputs and the Philox env id need no rebasing - a member's
// first row times `groups` is its first env times agents_per_env.  The per-layer pointers are read from the table by `l` where the
// layer starts (a copy of them per workgroup would be a dynamically indexed array: scratch), each made uniform and global.  Every
// member has a pack (the planner's condition), so there is no plain-weight gather here.
__global__ __launch_bounds__(TPB) void mlp_set_kernel(Args a, const SetWg *__restrict__ wgs, const SetMember *__restrict__ members) {
    const SetWg wg = wgs[blockIdx.x];
    const int member = __builtin_amdgcn_readfirstlane(wg.member), blk = __builtin_amdgcn_readfirstlane(wg.block);
    const SetMember &m = members[member];
    const int first_row = __builtin_amdgcn_readfirstlane(m.first_row), n_rows = __builtin_amdgcn_readfirstlane(m.n_rows);
#define CM_MLP_ROW0 (first_row + blk * ROWS)
#define CM_MLP_ROWS_LEFT (n_rows - blk * ROWS)
#define CM_MLP_LAYER(l) const float *const pk_l = uniform_global(m.pk[l]), *const b_l = uniform_global(m.b[l]);
#define CM_MLP_HAS_PK(l) true
#define CM_MLP_PK(l) pk_l
#define CM_MLP_WT(l) nullptr
#define CM_MLP_B(l) b_l
#include "cm_mlp_body.h"
#undef CM_MLP_ROW0
#undef CM_MLP_ROWS_LEFT
#undef CM_MLP_LAYER
#undef CM_MLP_HAS_PK
#undef CM_MLP_PK
#undef CM_MLP_WT
#undef CM_MLP_B
}

static size_t pack_floats(int K, int OUT) { return (size_t)((OUT + 15) >> 4) * ((K + 15) >> 4) * 256; }

// the LDS row stride of a chain (a.sw) -> the two tiles' bytes, or 0 when they exceed the 160 KB a workgroup can have
static size_t lds_tiles(Args &a) {
    int maxw = CHUNK;
    for (int l = 0; l < a.n_layers; ++l) maxw = max(maxw, (a.out_dim[l] + 15) & ~15);
    a.sw = maxw + 4;                                         // +4 words: rows skewed across LDS banks, 16-byte aligned
    const size_t lds = 2ull * ROWS * a.sw * sizeof(float);
    return lds > 160 * 1024 ? 0 : lds;
}

static int launch(Args a, void *stream) {
    const size_t lds = lds_tiles(a);
    if (!lds) return set_error(CM_ERR_ARG, "mlp forward: layer too wide for the 160 KB LDS tile");
    if (a.rows == 0) return CM_OK;
    return launch_lds<&mlp_kernel>(dim3((a.rows + ROWS - 1) / ROWS), dim3(TPB), lds, stream, a);
}

static int fill(Args &a, const cm_mlp_weights *w, int32_t rows, const float *x) {
    if (!w || !x) return set_error(CM_ERR_ARG, "mlp forward: null weights / input");
    if (rows < 0) return set_error(CM_ERR_ARG, "mlp forward: negative row count");
    if (w->n_layers < 1 || w->n_layers > MAXL) return set_error(CM_ERR_ARG, "mlp forward: 1..6 linear layers supported");
    if (w->in_dim < 1) return set_error(CM_ERR_ARG, "mlp forward: in_dim < 1");
    if (w->out_dim[0] > 128) return set_error(CM_ERR_ARG, "mlp forward: first layer wider than 128 outputs");
    if (w->tanh_mask & w->relu_mask) return set_error(CM_ERR_ARG, "mlp forward: a layer has both its tanh_mask and relu_mask bit set");
    a.rows = rows; a.in_dim = w->in_dim; a.n_layers = w->n_layers; a.tanh_mask = w->tanh_mask; a.relu_mask = w->relu_mask; a.x = x;
    for (int l = 0; l < w->n_layers; ++l) {
        if (w->out_dim[l] < 1 || w->out_dim[l] > 1024) return set_error(CM_ERR_ARG, "mlp forward: layer width outside 1..1024");
        if (!w->wt[l]) return set_error(CM_ERR_ARG, "mlp forward: null layer weight");
        a.out_dim[l] = w->out_dim[l]; a.wt[l] = w->wt[l]; a.b[l] = w->b[l];
    }
    size_t off = 0;
    for (int l = 0; l < w->n_layers; ++l) {
        a.pk[l] = w->mfma_pack ? w->mfma_pack + off : nullptr;
        off += pack_floats(l == 0 ? w->in_dim : w->out_dim[l - 1], w->out_dim[l]);
    }
    return CM_OK;
}

static int launch_set(Args a, const SetWg *wgs, const SetMember *members, int n_wg, void *stream) {
    const size_t lds = lds_tiles(a);
    if (!lds) return set_error(CM_ERR_ARG, "mlp forward: layer too wide for the 160 KB LDS tile");
    return launch_lds<&mlp_set_kernel>(dim3(n_wg), dim3(TPB), lds, stream, a, wgs, members);
}

// what the policy entry points ask of the sampler's shape
static int check_sampler(const char *who, const cm_mlp_weights *w, int groups, int n_act, int agents_per_env) {
    if (groups < 1 || n_act < 1 || n_act > MAX_ACT || agents_per_env < 1)
        return set_error(CM_ERR_ARG, std::string(who) + ": groups >= 1, 1 <= n_act <= 8, agents_per_env >= 1");
    if (w->out_dim[w->n_layers - 1] != groups * n_act)
        return set_error(CM_ERR_ARG, std::string(who) + ": last layer width != groups * n_act");
    return CM_OK;
}

static bool same_shape(const cm_mlp_weights &x, const cm_mlp_weights &y) {
    if (x.in_dim != y.in_dim || x.n_layers != y.n_layers || x.tanh_mask != y.tanh_mask || x.relu_mask != y.relu_mask) return false;
    for (int l = 0; l < x.n_layers && l < MAXL; ++l)
        if (x.out_dim[l] != y.out_dim[l]) return false;
    return true;
}

}  // namespace mlp
}  // namespace cm

extern "C" {

int64_t cm_mlp_forward_multi_plan(const cm_mlp_weights *members, const int32_t *group_sizes, int32_t n_policies, int32_t n_envs,
                                  int32_t groups, int32_t n_act, int32_t agents_per_env, void *image, size_t image_bytes,
                                  int32_t *n_wg_out) {
    using namespace cm::mlp;
    const std::string who = "cm_mlp_forward_multi_plan";
    if (!members || !group_sizes || !n_wg_out) return cm::set_error(CM_ERR_ARG, who + ": null argument");
    if (n_policies < 1) return cm::set_error(CM_ERR_ARG, who + ": a policy set has at least one member");
    static const float no_input = 0.0f;                      // fill() wants an input pointer; the planner reads none
    Args a{};
    if (int rc = fill(a, &members[0], 0, &no_input)) return rc;
    if (groups != 1 && groups != agents_per_env)
        return cm::set_error(CM_ERR_ARG, who + ": groups is 1 (a row per agent) or agents_per_env (a row per env)");
    if (int rc = check_sampler(who.c_str(), &members[0], groups, n_act, agents_per_env)) return rc;
    if (!lds_tiles(a)) return cm::set_error(CM_ERR_ARG, "mlp forward: layer too wide for the 160 KB LDS tile");
    const int rows_per_env = agents_per_env / groups;
    long long sum = 0, n_wg = 0;
    bool packed = true;
    for (int k = 0; k < n_policies; ++k) {
        if (group_sizes[k] < 1) return cm::set_error(CM_ERR_ARG, who + ": every member needs at least one env");
        if (!same_shape(members[k], members[0])) return cm::set_error(CM_ERR_ARG, who + ": the members differ in shape");
        packed = packed && members[k].mfma_pack;
        sum += group_sizes[k];
        n_wg += ((long long)group_sizes[k] * rows_per_env + ROWS - 1) / ROWS;   // a ragged last workgroup per member: none is shared with the next
    }
    if (sum != n_envs) return cm::set_error(CM_ERR_ARG, who + ": the group sizes must sum to n_envs");
    if (sum * rows_per_env > INT32_MAX) return cm::set_error(CM_ERR_ARG, who + ": more than 2^31 - 1 rows in one launch");
    if (!packed) { *n_wg_out = 0; return 0; }
    const size_t need = (size_t)n_wg * sizeof(cm_forward_set_wg) + (size_t)n_policies * sizeof(cm_mlp_set_member);
    *n_wg_out = (int32_t)n_wg;
    if (!image) return (int64_t)need;
    if (image_bytes < need) return cm::set_error(CM_ERR_ARG, who + ": image buffer too small");
    cm_forward_set_wg *wg = reinterpret_cast<cm_forward_set_wg *>(image);
    cm_mlp_set_member *mem = reinterpret_cast<cm_mlp_set_member *>(wg + n_wg);
    int32_t first = 0;
    for (int k = 0; k < n_policies; ++k) {
        const cm_mlp_weights &w = members[k];
        const int32_t rows = group_sizes[k] * rows_per_env;
        for (int b = 0; b < (rows + ROWS - 1) / ROWS; ++b) *wg++ = cm_forward_set_wg{ k, b };
        cm_mlp_set_member r{};
        r.first_row = first * rows_per_env; r.n_rows = rows; r.first_env = first;
        size_t off = 0;
        for (int l = 0; l < w.n_layers; ++l) {               // the layers' fragments lie in the pack as fill() walks them
            r.b[l] = w.b[l];
            r.pack[l] = w.mfma_pack + off;
            off += pack_floats(l == 0 ? w.in_dim : w.out_dim[l - 1], w.out_dim[l]);
        }
        mem[k] = r;
        first += group_sizes[k];
    }
    return (int64_t)need;
}

int cm_mlp_policy_forward_multi(const cm_mlp_weights *shape, const void *table_dev, int32_t n_wg, int32_t n_envs, int32_t groups,
                                int32_t n_act, int32_t agents_per_env, const float *x, const float *avail, uint64_t seed,
                                int32_t env_id_offset, uint32_t policy_step, const uint32_t *policy_step_base, int32_t greedy,
                                int32_t *actions, float *probs, void *stream) {
    using namespace cm::mlp;
    const char *who = "cm_mlp_policy_forward_multi";
    Args a{};
    if (n_envs < 0) return cm::set_error(CM_ERR_ARG, std::string(who) + ": negative env count");
    if (int rc = fill(a, shape, 0, x)) return rc;
    if (groups != 1 && groups != agents_per_env)
        return cm::set_error(CM_ERR_ARG, std::string(who) + ": groups is 1 (a row per agent) or agents_per_env (a row per env)");
    if (int rc = check_sampler(who, shape, groups, n_act, agents_per_env)) return rc;
    if (!actions && !probs) return cm::set_error(CM_ERR_ARG, std::string(who) + ": no output requested");
    if (n_envs == 0) return CM_OK;
    if (!shape->mfma_pack) return 1;
    const long long rows = (long long)n_envs * (agents_per_env / groups);
    if (!table_dev || n_wg < (rows + ROWS - 1) / ROWS || n_wg > rows || rows > INT32_MAX)
        return cm::set_error(CM_ERR_ARG, std::string(who) + ": null table, or n_wg is not the planner's for n_envs");
    a.rows = (int)rows;
    a.groups = groups; a.n_act = n_act; a.agents_per_env = agents_per_env; a.avail = avail;
    a.key0 = (uint32_t)seed; a.key1 = (uint32_t)(seed >> 32); a.policy_step = policy_step; a.step_base = policy_step_base;
    a.env_id_offset = env_id_offset; a.greedy = greedy; a.actions = actions; a.probs = probs;
    const SetWg *wgs = reinterpret_cast<const SetWg *>(table_dev);
    return launch_set(a, wgs, reinterpret_cast<const SetMember *>(wgs + n_wg), n_wg, stream);
}

int cm_mlp_policy_forward(const cm_mlp_weights *w, int32_t rows, int32_t groups, int32_t n_act, int32_t agents_per_env,
                          const float *x, const float *avail, uint64_t seed, int32_t env_id_offset,
                          uint32_t policy_step, const uint32_t *policy_step_base, int32_t greedy, int32_t *actions,
                          float *probs, void *stream) {
    cm::mlp::Args a{};
    if (int rc = cm::mlp::fill(a, w, rows, x)) return rc;
    if (int rc = cm::mlp::check_sampler("mlp policy forward", w, groups, n_act, agents_per_env)) return rc;
    if (!actions && !probs) return cm::set_error(CM_ERR_ARG, "mlp policy forward: no output requested");
    a.groups = groups; a.n_act = n_act; a.agents_per_env = agents_per_env; a.avail = avail;
    a.key0 = (uint32_t)seed; a.key1 = (uint32_t)(seed >> 32); a.policy_step = policy_step; a.step_base = policy_step_base;
    a.env_id_offset = env_id_offset; a.greedy = greedy; a.actions = actions; a.probs = probs;
    return cm::mlp::launch(a, stream);
}

int cm_mlp_value_forward(const cm_mlp_weights *w, int32_t rows, const float *x, float *values, void *stream) {
    cm::mlp::Args a{};
    if (int rc = cm::mlp::fill(a, w, rows, x)) return rc;
    if (!values) return cm::set_error(CM_ERR_ARG, "mlp value forward: null output");
    if (w->out_dim[w->n_layers - 1] != 1) return cm::set_error(CM_ERR_ARG, "mlp value forward: last layer width != 1");
    a.values = values;
    return cm::mlp::launch(a, stream);
}

size_t cm_mlp_pack_bytes(const cm_mlp_weights *w) {
    if (!w || w->n_layers < 1 || w->n_layers > cm::mlp::MAXL || w->in_dim < 1) return 0;
    size_t n = 0;
    for (int l = 0; l < w->n_layers; ++l) {
        if (w->out_dim[l] < 1) return 0;
        n += cm::mlp::pack_floats(l == 0 ? w->in_dim : w->out_dim[l - 1], w->out_dim[l]);
    }
    return n * sizeof(float);
}

int cm_mlp_pack(const cm_mlp_weights *w, float *pack, void *stream) {
    if (!w || !pack || !cm_mlp_pack_bytes(w)) return cm::set_error(CM_ERR_ARG, "cm_mlp_pack: null / malformed argument");
    size_t off = 0;
    for (int l = 0; l < w->n_layers; ++l) {
        const int K = l == 0 ? w->in_dim : w->out_dim[l - 1], OUT = w->out_dim[l];
        if (int rc = cm::mf::pack_one(w->wt[l], K, OUT, (K + 15) & ~15, (OUT + 15) & ~15, pack + off, stream)) return rc;
        off += cm::mlp::pack_floats(K, OUT);
    }
    return CM_OK;
}

}  // extern "C"
