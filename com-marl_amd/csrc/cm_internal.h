// cm_internal.h - shared between the translation units of libcommarl_hip.so
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/commarl.h"

namespace cm {

int set_error(int code, const std::string &msg);   // stores thread-local text, returns code
int hip_fail(hipError_t e, const char *what);      // -> CM_ERR_HIP

#define CM_HIP(call)                                          \
    do {                                                      \
        hipError_t _e = (call);                               \
        if (_e != hipSuccess) return ::cm::hip_fail(_e, #call); \
    } while (0)

// Function attributes (hipFuncAttributeMaxDynamicSharedMemorySize) and CU counts belong to a DEVICE, not to the process:
// a launcher's `static unsigned long long done` carries one bit per device ordinal, so a process that moves on to a second
// GPU sets the attribute there too.  (Host launch paths are single-threaded per handle, include/commarl.h.)
inline bool dev_first(unsigned long long &done) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    const unsigned long long bit = 1ull << (dev & 63);
    if (done & bit) return false;
    done |= bit;
    return true;
}
// A launch with dynamic LDS: the 160 KB attribute on KERN once per device, the launch, its error.  (CM_HIP is defined above;
// the static is per kernel and argument types - a kernel launched from two sites sets its attribute at most twice.)
template <auto KERN, class... A>
static inline int launch_lds(dim3 grid, dim3 block, size_t lds_bytes, void *stream, const A &...args) {
    static unsigned long long done = 0;
    if (dev_first(done)) CM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL(KERN, grid, block, lds_bytes, (hipStream_t)stream, args...);
    CM_HIP(hipGetLastError());
    return CM_OK;
}
inline int cu_count() {
    static int cached[64] = { 0 };
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    int &n = cached[dev & 63];
    if (n <= 0) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
        n = v;
    }
    return n;
}

// threadIdx.x through an opaque register: inside the step loop of the persistent rollout kernel the compiler otherwise
// hoists every lane-derived address computation of both bodies out of the loop (several hundred live VGPRs: one
// workgroup per CU, or 256 spilled registers when held to two).  Costs one move in the single-step kernels.
__device__ __forceinline__ int thread_x() {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}

// A pointer as loaded from memory is generic and not known uniform: loads through it become flat loads and what they feed may go
// to scratch (DESIGN.md §5 "Multi-policy rollouts").  Both halves through readfirstlane, and global explicitly.
template <typename T>
__device__ __forceinline__ const T *uniform_global(const T *p) {
    const unsigned long long u = (unsigned long long)p;
    const unsigned long long v = ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(u >> 32)) << 32) |
                                 (unsigned)__builtin_amdgcn_readfirstlane((unsigned)u);
    return (const T *)(const __attribute__((address_space(1))) T *)v;
}

// Device-side view of one batched env set (passed to kernels by value).
struct EnvDev {
    int scen, B, N, M, S, R, W, d, load, max_steps, mpl, L, rc2, channel, add_clock, n_empty, rng_mode, env_id_offset;
    int adj_const, ch_const;
    int ge_flags;             // cm_env_cfg.ge_flags (bit 0: one GE transition per env step; bits 1-2: initial state)
    int lpe, lds_env;         // lanes per env (16/32/64) and LDS bytes per env
    int stop;                 // diagnostic (COMMARL_ENV_STOP): return after phase `stop`; 0 = run everything
    int no_small;             // COMMARL_ENV_SMALL=0: tile walk also for small PP teams (A/B of pp_small_step)
    float rcp_d, rcp_W, rcp_N, rcp_WW, rcp_NN;   // float reciprocals for the exact fast division in the emit loops
    float ploss, pgb, pbg;
    double cap_rew, step_cost, move_cost, penalty, lazy, revisit, final_reward;
    uint32_t key0, key1;
    // SoA state in HBM
    int2 *agent_pos;          // [B,N]  (row, col)
    int2 *prey_pos;           // [B,M]
    uint8_t *alive;           // [B,M]
    uint32_t *visited;        // [B,S]  row bitmasks (CO)
    int32_t *step_count;      // [B]
    int32_t *total_capture;   // [B]
    int32_t *success;         // [B]
    uint8_t *ge_state;        // [B,N,N]
    uint32_t *rng_step;       // [B]
    uint8_t *agent_cond;      // [B,N] PP agent_condition (predator_prey.py:74,152,258): 0 = the agent cannot move
    int32_t *status;          // [1] first kernel-side error
    unsigned int *tail_ticket;  // [1] zero at rest: waves that finished a chunk whose tail is folded into the kernel (cm_rollout_w.hip)
    // read-only tables
    const uint8_t *base_grid; // [S*S] CO walls (0 empty / 3 wall)
    const float *lut_row;     // [S]   obs row coordinate
    const float *lut_col;     // [S]
    const float *lut_step;    // [max_steps+1] clock
    const double *rew_lut;    // count-indexed f64 reward terms (no f64 division on the device)
};

// Device image of one cm_env_cond record (cm_env_set_conditions): the same 32 bytes, with the range already squared
// (EnvDev.rc2; INT32_MAX for a fully connected env) so that the kernel patches EnvDev without arithmetic.
struct EnvCondDev {
    int32_t rc2;
    float ploss, pgb, pbg;
    int32_t rng_id;
    int32_t reserved[3];
};
static_assert(sizeof(EnvCondDev) == sizeof(cm_env_cond) && sizeof(EnvCondDev) == 32, "one 32-byte record per env");

}  // namespace cm

struct cm_env {
    cm_env_cfg cfg;
    cm::EnvDev dev;
    size_t lds_bytes;
    void *arena;              // one hipMalloc for all state
    size_t arena_bytes;
    // cm_env_set_conditions: the [B] device table (NULL = none: every env has the handle's comm scalars), the pinned host
    // image later calls copy from, and the event behind the last copy (the image is not rewritten before that copy has run)
    void *cond;
    void *cond_host;
    hipEvent_t cond_copied;
    bool cond_fused;          // cm_env_fuse_conditions: the rollout entry points run such a handle on the kernels of cm_rollout_wc.hip
    bool started;             // a reset / step was launched: the first cm_env_set_conditions comes too late
};

namespace cm {
// Per-step element strides of the time-major trajectory buffers, for the kernels that run several rollout steps per launch
// (cm_rollout_chunk): step t reads / writes base + t * stride.
struct ChunkArgs {
    int n_steps;
    long long obs, actions, probs, attn, reward, reward_f64, done, details, dist_adj, channels, prey_alive, success, path_len;
    // cm_rollout_chunk_tail: the tail the caller wants behind the chunk - the last step's observation into `tail_obs` (slot 0) and
    // *tail_base += n_steps.  A kernel that does it itself sets *tail_folded (host) to 1; otherwise the entry point launches cm_chunk_tail.
    float *tail_obs = nullptr;
    uint32_t *tail_base = nullptr;
    int *tail_folded = nullptr;
};
static inline ChunkArgs chunk_args(int n_steps, const cm_chunk_strides &st) {
    return ChunkArgs{ n_steps, st.obs, st.actions, st.probs, st.attn, st.reward, st.reward_f64, st.done, st.details,
                      st.dist_adj, st.channels, st.prey_alive, st.success, st.path_len };
}

int check_tape(const cm_env *h, const cm_rng_tape *tape, bool is_reset);   // cm_env.hip: tape pointers the config needs
// cm_env_cond.hip: the env step of a handle with a condition table; `wide` is launch()'s narrow / wide choice
int launch_env_cond(const cm_env *h, bool wide, const int32_t *actions, const cm_step_out &out, hipStream_t st, int reset_only);
namespace mf {
// cm_policy_mfma.hip: one layer's weights [K,OUT] -> MFMA B fragments [out_pad/16][kpad/16][64 lanes][4], zero padded
int pack_one(const float *Wt, int K, int OUT, int kpad, int out_pad, float *dst, void *stream);
}
}

namespace cm {
// ---- deterministic merges (include/commarl.h "Deterministic update mode") ----
// In slab mode a workgroup plain-stores its partial sums into row blockIdx.x of a slab instead of adding them into the
// output with float atomics; slab_reduce then sums the rows in index order.  The number of rows is the launch's grid
// size, a function of the shape and the device's CU count only.
template <bool DET>
__device__ __forceinline__ void merge_add(float *p, float v) {
    if constexpr (DET) *p = v;
    else atomicAdd(p, v);
}

// out[i] += sum_{b < rows} slab[b * row_len + off + i], b ascending, for up to four segments of a slab row
struct SlabSeg { float *out; int off, n; };
struct SlabSegs { SlabSeg s[4]; int n_seg; };
int slab_reduce(const float *slab, int rows, int row_len, const SlabSegs &segs, hipStream_t st);
// a workspace of `need` bytes is present (else -1 with cm_last_error text naming `what`)
int slab_check(const void *ws, size_t ws_bytes, size_t need, const char *what);

// ---- backward launchers called across translation units: return 1 when the shape / alignment is not covered (the caller
// runs its generic kernel), else the launch status.  det: slab mode - the gradient outputs address their segments of slab
// row 0 and *grid (when given) receives the number of rows written ----
// cm_linear_bwd.hip: one dense layer, widths 32 / 64 / 128
int linear_bwd_stream(bool det, long R, int K, int O, const float *x, const float *w, int layout, const float *dy, const float *dy2,
                      const float *y, int act, float *dx, float *dw, float *db, void *stream, int *grid = nullptr);
// cm_linear_bwd.hip: both encoder layers in one pass (slab row: dW2 | db2 | dW1 | db1, lin2_slab_row(d) floats)
int encoder_bwd_chain(bool det, long R, int d, const float *obs, const float *a1, const float *e, const float *w2, const float *dy,
                      const float *dy2, float *dw2, float *db2, float *dw1, float *db1, void *stream, int *grid = nullptr);
size_t lin2_slab_row(int d);
// cm_graph_ops_mfma.hip: teams of 8 .. 128 on the matrix cores (slab row: d_bias, 64 floats)
int agg_bwd_mfma(bool det, int S, int N, const float *attn, const float *adj, const float *chan, long ch_stride, const float *hw,
                 const float *out, const float *out_minus, const float *d_out, float *d_attn, float *d_hw, float *d_bias, void *stream,
                 int *grid = nullptr);
int attn_bwd_mfma(int S, int N, const float *q, const float *e, const float *m, const float *d_m, const float *add0, const float *add1,
                  float *d_q, float *d_e, void *stream);

// ---- cm_stat_rows.hip: the four reductions of a statistics family's per-step rows, behind cm_episode_<family>, cm_<family>_means,
// cm_<family>_curves and cm_<family>_curve_means of comm, attn, listen and value.  Instantiated for the two row kinds there are:
// <int32_t, CM_COMM_COLS> and <double, 6>.  `who` names the entry point in the refusals' texts ----
namespace rows {
// what a family's columns are divided by, next to the number of steps or episodes: N (the agents; 1 for one value per step), and
// for the columns set in l_cols also L (the hops)
struct Div {
    int N, L = 1;
    unsigned l_cols = 0u;
};
constexpr unsigned COMM_L_COLS = 0b0010u;   // cm_comm_stats' `delivered` is counted per hop
template <typename V, int COLS>
int episode_rows(const char *who, int T, int B, Div d, const int32_t *path_len, const V *stats, int group_size, int take,
                 int episodes_per_group, int row0, double *episodes, void *stream);
template <int COLS>
int group_means(const char *who, int K, int E, const double *episodes, double *summary, void *stream);
template <typename V, int COLS>
int curve_sums(const char *who, int T, int B, Div d, const int32_t *path_len, const V *stats, int group_size, int take, int accumulate,
               double *sums, void *stream);
template <int COLS>
int curve_means(const char *who, int cells, int T, int n_episodes, Div d, const double *sums, double *curves, void *stream);
}
}
