/*
 * commarl.h - C ABI of libcommarl_hip.so: the MI355X (gfx950) batched rollout + GNN-PPO
 * hot path of Com-MARL.
 *
 * The reference (cnuns/Com-MARL) is pure Python and has no FFI of its own; the drop-in
 * boundary is the set of Python classes its runner scripts import by name
 * (exp_runners/predatorprey/runner_pp_commDP.py:22-28).  Those classes are re-provided by
 * the host package (com-marl_amd/) as thin veneers over THIS C ABI.  Each entry point
 * below cites the reference interface it replaces (file:line relative to the reference
 * tree).  Conventions:
 *   - every function returns 0 on success, <0 on error; cm_last_error() gives the text;
 *     no exception ever crosses the ABI;
 *   - all data pointers are DEVICE pointers unless the name ends in _host; buffers are
 *     caller-owned (torch-allocated in the Python veneer) except the env state, which the
 *     handle owns;
 *   - `stream` is a hipStream_t passed as void*; NULL = the default stream.  Launches are
 *     asynchronous; nothing here synchronises except get/set_state and cm_env_status;
 *   - one handle is not thread-safe; distinct handles are independent (one process per GPU).
 */
#ifndef COMMARL_H
#define COMMARL_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CM_ABI_VERSION 3

enum { CM_PP = 0, CM_CO = 1 };                                  /* scenario */
enum { CM_CH_FC = 0, CM_CH_FL = 1, CM_CH_IID = 2, CM_CH_GE = 3 }; /* channel model */
enum { CM_RNG_PHILOX = 0, CM_RNG_TAPE = 1 };

enum {
    CM_OK = 0,
    CM_ERR_ARG = -1,        /* bad argument / unsupported config */
    CM_ERR_TAPE = -2,       /* RNG tape exhausted (parity mode) */
    CM_ERR_TAPE_PREY = -3,
    CM_ERR_ACTION = -4,     /* action outside 0..4: predator_prey.py:255, coverage.py:347 raise */
    CM_ERR_LOAD = -5,       /* PP load not in {2,3,4}: capv undefined (predator_prey.py:77-79) */
    CM_ERR_HIP = -6,
    CM_ERR_NOMEM = -7
};

/* Env configuration = the `params` dict the reference envs read
 * (predator_prey.py:52-82, coverage.py:40-96, env_communication.py:10-75) after the arg
 * post-processing of exp_runners/env_uitils.py:174-217. */
typedef struct cm_env_cfg {
    int32_t scenario;        /* CM_PP / CM_CO */
    int32_t n_envs;          /* B independent envs owned by this handle */
    int32_t n_agents;        /* N */
    int32_t n_preys;         /* M (PP) */
    int32_t grid;            /* PP: G = --map; CO: m = --map (grid side m+2 incl. wall ring) */
    int32_t rsen;            /* --sen: window (2R+1)^2 */
    int32_t load;            /* --cap: 2 reward_default, 3/4 reward_individual */
    int32_t max_steps;       /* env time limit (PP max_env_steps; CO ctor max_steps=400) */
    int32_t max_path_length; /* VecEnvExecutor truncation (vec_env_executor.py:33-34) */
    int32_t n_hops;          /* n_gcn_layers L */
    int32_t rcom;            /* trRcom (rule Rcom+1>=map -> fully connected applied inside) */
    int32_t channel;         /* CM_CH_* */
    int32_t obst_hard;       /* CO obstComplex: 0 Easy / 1 Hard */
    int32_t add_clock;       /* CO */
    int32_t rng_mode;        /* CM_RNG_PHILOX production / CM_RNG_TAPE parity */
    int32_t env_id_offset;   /* global id of local env 0: rank r of k owns [r*B, (r+1)*B) */
    float ploss, pgb, pbg;
    int32_t ge_flags;        /* GE channel variants (env_communication.py:106-157), 0 = the runners' defaults:
                                bit 0 set  = loss_apply 0: ONE state transition per env step shared by all hops (else one per hop);
                                bits 1-2   = GE_INIT: 0 all links good, 1 all bad, 2 random with the stationary bad rate
                                             Pgb/(Pgb+Pbg) (not together with bit 0: the reference's state is shape-
                                             inconsistent for that pair, :121) */
    double capture_reward, step_cost, move_cost, penalty, lazy_penalty, revisit_penalty, final_reward;
    uint64_t seed;
} cm_env_cfg;

/* Recorded draws for parity mode (device pointers, any may be NULL when unused):
 * SURVEY.md App. A-6 call sites.  slot 0 = the step's comm update, slot 1 = the reset's. */
typedef struct cm_rng_tape {
    const uint8_t *prey;     /* [B,M,5]  np.random.choice outcomes (predator_prey.py:401), 255 unused */
    const int32_t *spawn;    /* [B,cap,2] random.randint pairs (predator_prey.py:156,165; coverage.py:185) */
    int32_t spawn_cap;
    int32_t _pad;
    const float *iid_u;      /* [B,2,L,N,N]   torch.rand (env_communication.py:212) */
    const float *ge_u;       /* [B,2,L,2,N,N] torch.rand (gilbert_elliot_loss_model.py:138,142) */
    const float *ge_init_u;  /* [B,N,N] torch.rand of get_init_state (:84-87), GE_INIT random only */
} cm_rng_tape;

/* What VecEnvExecutor.step returns + the env attributes the sampler reads each step
 * (centralized_ma_on_policy_vectorized_sampler.py:123-141).  Any pointer may be NULL to
 * skip that output; dist_adj / channels are skipped automatically when constant
 * (fully connected / FC / FL: filled once by cm_env_fill_constants). */
typedef struct cm_step_out {
    float *obs;              /* [B,N,d]   next observation (reset obs where done) */
    float *reward;           /* [B]       f32 view of the reward */
    double *reward_f64;      /* [B]       reward as the Python float the reference produces */
    uint8_t *done;           /* [B] */
    int32_t *details;        /* [B,6] capture, move, penalty, lazy, revisit|watching, final (sums over agents) */
    float *dist_adj;         /* [B,N,N] */
    float *channels;         /* [B,L,N,N] */
    uint8_t *prey_alive;     /* [B,M] env_infos['prey_alive'] (pre-reset) */
    int32_t *success;        /* [B] env.success after the step */
    int32_t *path_len;       /* [B] length of the path that ended at this step (0 = still running):
                                what the sampler adds to n_samples, x N (sampler.py:225) */
} cm_step_out;

/* Host-side snapshot of the SoA state (for parity fixtures / checkpoints). */
typedef struct cm_env_state {
    int32_t *agent_pos;      /* [B,N,2] */
    int32_t *prey_pos;       /* [B,M,2] */
    uint8_t *prey_alive;     /* [B,M] */
    uint32_t *visited;       /* [B,S,W] row bitmasks (CO): W = ceil(S / 32) words per grid row - [B,S] up to map 30; cell (r, c) =
                              * bit c & 31 of word (r, c >> 5) */
    int32_t *step_count;     /* [B] */
    int32_t *total_capture;  /* [B] */
    int32_t *success;        /* [B] */
    uint8_t *ge_state;       /* [B,N,N] */
    uint32_t *rng_step;      /* [B] */
} cm_env_state;

typedef struct cm_env *cm_env_t;

int cm_abi_version(void);
const char *cm_last_error(void);

/* PredatorPreyWrapper(...)/CoverageWrapper(...) construction (predatorprey_wrapper.py:23-44,
 * coverage_wrapper.py:16-33) for B envs at once. */
int cm_env_create(const cm_env_cfg *cfg, cm_env_t *out);
int cm_env_destroy(cm_env_t h);
int cm_env_obs_dim(cm_env_t h);          /* d per agent */
int cm_env_n_empty_cells(cm_env_t h);    /* coverage.py:228-230 */
int cm_env_adj_is_const(cm_env_t h);     /* 1 when Rcom rule gives fully connected (env_communication.py:71-72) */
int cm_env_channels_are_const(cm_env_t h);
/* write the constant dist_adj [B,N,N] / channels [B,L,N,N] once */
int cm_env_fill_constants(cm_env_t h, float *dist_adj, float *channels, void *stream);

/* VecEnvExecutor.reset (vec_env_executor.py:47-54): reset every env, emit obs + comm state. */
int cm_env_reset(cm_env_t h, const cm_rng_tape *tape, const cm_step_out *out, void *stream);
/* VecEnvExecutor.step (vec_env_executor.py:19-45) over env.step (predator_prey.py:494-519,
 * coverage.py:319-401): actions int32 [B,N]. */
int cm_env_step(cm_env_t h, const int32_t *actions, const cm_rng_tape *tape, const cm_step_out *out, void *stream);
/* synchronises; returns the first kernel-side error (CM_ERR_TAPE / CM_ERR_ACTION ...) or 0 */
int cm_env_status(cm_env_t h);
int cm_env_get_state(cm_env_t h, const cm_env_state *host);
int cm_env_set_state(cm_env_t h, const cm_env_state *host);

/* Per-env comm conditions: every env of the handle gets its own communication range, channel parameters and Philox env id -
 * what the reference's runners sweep one run at a time with --teRcom / --tepl / --Pgb / --Pbg, and what a curriculum over the
 * packet loss changes between epochs.  HOST table of n_envs records; the handle owns a device copy. */
typedef struct cm_env_cond {      /* 32 bytes */
    int32_t rcom;                 /* as cm_env_cfg.rcom; the rule of cm_env_create - rcom == 0 or rcom + 1 >= grid means fully
                                     connected (env_communication.py:71-72) - is applied per env */
    float   ploss, pgb, pbg;      /* read where the handle's channel is IID / GE; otherwise ignored */
    int32_t rng_id;               /* the Philox env id this env draws with (without a table: cfg.env_id_offset + b) */
    int32_t reserved[3];          /* 0 */
} cm_env_cond;
/* The FIRST call is allowed only before the handle's first cm_env_reset / cm_env_step (CM_ERR_ARG afterwards): it allocates the
 * table and turns cm_env_adj_is_const off - every env's dist_adj is computed and written from then on, all ones for a fully
 * connected env - while cm_env_channels_are_const stays what the channel kind (a property of the handle, not of a record)
 * dictates.  Query the two once after it and size buffers by the answers.  LATER calls overwrite the same device memory with a
 * copy ordered on `stream`: steps launched on that stream afterwards, replays of a captured hipGraph included, read the new
 * values.  The host table may be freed on return.  Not to be called while `stream` is being captured.
 * With a table cm_env_reset / cm_env_step launch the kernels of csrc/cm_env_cond.hip (the same narrow / wide / lanes-per-env
 * choice): env b does exactly what env 0 of a handle created with the record's rcom / ploss / pgb / pbg and env_id_offset =
 * rng_id would do, bit for bit.  Entry points that run the env phase inside another kernel - cm_rollout_step,
 * cm_rollout_chunk, cm_rollout_chunk_tail, cm_rollout_chunk_multi - return 1 (nothing done) for such a handle, and the caller
 * takes the policy launch + cm_env_step, unless cm_env_fuse_conditions (below) switched them on.  cm_env_agent_fault and cm_comm_delays are out of
 * scope: the fault draws stay keyed by the physical env id cfg.env_id_offset + b, whatever rng_id says.
 * CM_ERR_ARG (text in cm_last_error) before anything is launched or copied: a NULL table, a CM_RNG_TAPE handle (a tape holds
 * draws recorded under one condition), rcom < 0, a probability the channel kind reads outside [0, 1], a non-zero reserved
 * word. */
int cm_env_set_conditions(cm_env_t h, const cm_env_cond *host_table /* [n_envs] */, void *stream);
int cm_env_has_conditions(cm_env_t h);   /* 1 once a table was set */
/* on != 0: the four rollout entry points above run a handle with a table where the wave-owned rollout kernel covers its shape
 * (Predator-Prey, teams of 4, 16 lanes per env, at most 16 preys, LDS within 160 KB: the kernels of csrc/cm_rollout_wc.hip, whose
 * env phase reads the table) - bit for bit what the policy launch + cm_env_step give; every other shape still returns 1.  Off by
 * default.  Allowed before or after the table is set; without a table it has no effect.  CM_ERR_ARG on a NULL handle. */
int cm_env_fuse_conditions(cm_env_t h, int32_t on);

/* PP agent_condition (predator_prey.py:74,152,258): [B,N] bytes, 0 = the agent's moves are not applied; every env reset
 * puts its row back to ones.  HOST pointers; either may be NULL.  Synchronises. */
int cm_env_agent_condition(cm_env_t h, const uint8_t *set_host, uint8_t *get_host);
/* The reference's dormant agent-fault models, applied to agent_condition (custom_implement/env_communication.py:290-301;
 * never called by the reference's own code): mode 1 = iid_fault(n, p_fault = p); mode 2 = GE_fault(condition, p, r) as
 * written (ONE draw for all good agents, ONE for all bad ones).  tape_u (DEVICE, [B,N] for mode 1, [B,2] for mode 2):
 * the uniforms np.random.choice would consume, or NULL = Philox site 9 at (global env id, fault_step). */
int cm_env_agent_fault(cm_env_t h, int32_t mode, float p, float r, const float *tape_u, uint32_t fault_step, void *stream);
/* Link-delay counters (env_communication.py:271-286), a pure function of DEVICE arrays: init != 0 = delays_init(adjacency
 * [B,N,N], link_loss [B,L,N,N], delay_th); init == 0 = calc_delays(adjacency, link_loss, old_delays [B,N,N]).
 * delays [B,L,N,N] int32.  NULL adjacency / link_loss = ones. */
int cm_comm_delays(int32_t B, int32_t L, int32_t N, const float *dist_adj, const float *link_loss, const int32_t *old_delays,
                   int32_t delay_th, int32_t init, int32_t *delays, void *stream);

/* Hop diameter of S graphs of N vertices (env_communication.py:235-241: what get_graph asks networkx for with
 * calc_diameter), a pure function of a DEVICE array: vertices i != j are joined when dist_adj[s][i][j] != 0 OR
 * dist_adj[s][j][i] != 0 (any non-zero value is an edge, the diagonal is ignored).  diameter[s] = the largest shortest-path
 * hop count of a connected graph (0 for N = 1), 0 for a disconnected one; exactly S ints are written.  1 <= N <= 255;
 * anything else, or a NULL pointer with S > 0, is CM_ERR_ARG.  S = 0 launches nothing. */
int cm_graph_diameter(int32_t S, int32_t N, const float *dist_adj, int32_t *diameter, void *stream);

/* Episode statistics of an evaluation round, reduced on the device: what the reference's eval loop accumulates per episode
 * (eval_pp.py:60-91) and exp_runners/testing.py:329-335 averages into one CSV row per checkpoint.  Pure functions of DEVICE
 * arrays: the time-major trajectory buffers of a T-step rollout over B envs (the cm_step_out arrays, one slot per step).
 *
 * cm_episode_stats summarises the FIRST episode of selected envs into rows of CM_EPI_COLS doubles.  Env b belongs to group
 * k = b / group_size and has index j = b % group_size in it; envs with j >= take are not read and nothing is written for them;
 * every other env's row is episodes[k * episodes_per_group + row0 + j].  The episode's length n is t + 1 for the first t with
 * path_len[t][b] > 0, or T when there is none (the step limit cut it); later episodes of an auto-reset env are ignored.
 * Over steps 0 .. n-1, with nA = N and d = details[t][b]:
 *   column 0 success     = success[n-1][b]
 *          1 reward      = sum of reward_f64 (f64)
 *          2 capture_cnt = sum d[0]        (CM_CO: / nA)
 *          3 step_cnt    = n
 *          4 move_cnt    = sum d[1] / nA
 *          5 penalty_cnt = sum d[2]        (CM_CO: / nA)
 *          6 nodeDeg     = N when dist_adj is NULL (the constant full graph); else the mean of the n entries deg[1], ...,
 *                          deg[n-1], deg[n-1] (n = 1: the single entry deg[0]), deg[t] = (sum of the N x N floats of
 *                          dist_adj[t][b]) / N: the graph after the step, and for the terminal step the one before it (the env
 *                          auto-resets on done, so the post-step graph of a finished episode is never materialised)
 *          7 variable    = sum d[4] / nA
 *          8 vars2       = 0               (CM_CO: sum d[3] / nA)
 * The detail columns are summed as integers and divided once; adjacency entries are 0 or 1 and summed as integers.
 *
 * cm_episode_means reduces each of K groups of E consecutive rows to CM_SUM_COLS doubles: the mean of every column, then for
 * the reward column the population standard deviation sqrt(mean((x - mean)^2)) (second pass around the mean), the minimum and
 * the maximum.
 *
 * Both: no atomics - every sum has one fixed order, so two launches on the same inputs write the same bits; exactly the named
 * rows are written (B / group_size * take rows of `episodes`, K rows of `summary`).  B = 0 or take = 0 launches nothing.
 * CM_ERR_ARG (text in cm_last_error) before anything is launched: T < 1, N outside 1..255, a scenario other than CM_PP / CM_CO,
 * group_size < 1 or not a divisor of B, take > group_size, row0 < 0 or row0 + take > episodes_per_group, K < 1, E < 1, or a
 * NULL pointer other than dist_adj where there is work to do. */
#define CM_EPI_COLS 9    /* success, then the reference's VECTORS in order (testing.py:209): reward, capture_cnt, step_cnt,
                            move_cnt, penalty_cnt, nodeDeg, variable, vars2 */
#define CM_SUM_COLS 12   /* the 9 column means, then std (population), min, max of the reward column */
int cm_episode_stats(int32_t T, int32_t B, int32_t N, int32_t scenario,      /* CM_PP / CM_CO */
                     const double *reward_f64,   /* [T,B]   */
                     const int32_t *details,     /* [T,B,6] */
                     const int32_t *success,     /* [T,B]   */
                     const int32_t *path_len,    /* [T,B]   */
                     const float *dist_adj,      /* [T+1,B,N,N], or NULL = constant full graph */
                     int32_t group_size, int32_t take, int32_t episodes_per_group, int32_t row0,
                     double *episodes,           /* [B/group_size * episodes_per_group, CM_EPI_COLS] */
                     void *stream);
int cm_episode_means(int32_t K, int32_t E, const double *episodes /* [K*E, CM_EPI_COLS] */,
                     double *summary /* [K, CM_SUM_COLS] */, void *stream);

/* Communication statistics: how much of the offered communication was delivered, and how much of the team an agent can hear
 * through the L hops of the Comm-DP net.  At hop l agent i hears j iff dist_adj[i][j] * channels[l][i][j] != 0
 * (comm_base_net.py:101-103).  Pure functions of DEVICE arrays.
 *
 * cm_comm_stats turns S graphs into rows of CM_COMM_COLS int32.  Graph s reads the N*N floats at dist_adj + s*adj_stride and the
 * L*N*N floats at channels + s*chan_stride (strides in floats).  A NULL array means all ones.  A stride of 0 means every graph
 * reads the same block (a constant FL channel - the identity - is passed this way); any other stride must be at least the block
 * size (N*N, L*N*N).  An entry is "set" when it is != 0.0f (-0.0 is not set).  The diagonal of both inputs is ignored and taken
 * as set.  With a[i][j] = (dist_adj[i][j] set) and m_l[i][j] = a[i][j] && (channels[l][i][j] set), for i != j:
 *   column 0 in_range    = #{(i,j), i != j : a[i][j]}
 *          1 delivered   = sum over l of #{(i,j), i != j : m_l[i][j]}
 *          2 reach       = #{(i,k), i != k : X_L[i][k]},  X_0 = I,  X_{l+1}[i] = X_l[i] OR (OR over j with m_l[i][j] of X_l[j]):
 *                          hop 0 is applied first, and the order matters
 *          3 range_reach = reach with every channel taken as ones (the geometry's share alone)
 * Integer arithmetic, no atomics: two launches on the same inputs write the same bits.  Exactly S rows are written; S = 0 launches
 * nothing.  CM_ERR_ARG (text in cm_last_error) before anything is launched: S < 0, N outside 1..255, L outside 1..8, a stride of a
 * non-NULL array that is neither 0 nor at least the block size, or NULL stats with S > 0.
 *
 * cm_episode_comm sums the rows of the slots an episode's policy acted through into one row of CM_EPC_COLS doubles per episode.
 * The env-to-row mapping (group_size, take, episodes_per_group, row0), the first-episode rule and the episode length n are
 * cm_episode_stats's; the slots summed are 0 .. n-1 (the forward of step t reads slot t).  With c = the int64 column sums:
 *   column 0 range_degree = c[in_range]    / (n N)      mean number of agents in range
 *          1 heard_degree = c[delivered]   / (n N L)    mean number of agents heard per hop
 *          2 reach        = c[reach]       / (n N)      mean number of team mates whose information can arrive within L hops
 *          3 range_reach  = c[range_reach] / (n N)      the same on loss-free channels
 * each sum divided once.  Refusals as cm_episode_stats (T < 1, N outside 1..255, group_size < 1 or not a divisor of B,
 * take > group_size, row0 < 0 or row0 + take > episodes_per_group, a NULL pointer where there is work to do), and L outside 1..8.
 * B = 0 or take = 0 launches nothing.
 *
 * cm_comm_means reduces each of K groups of E consecutive rows to their CM_EPC_COLS column means, summed in one fixed order
 * (the order of cm_episode_means).  K < 1, E < 1 or a NULL pointer is CM_ERR_ARG. */
#define CM_COMM_COLS 4   /* in_range, delivered, reach, range_reach */
#define CM_EPC_COLS 4    /* range_degree, heard_degree, reach, range_reach */
int cm_comm_stats(int32_t S, int32_t N, int32_t L,
                  const float *dist_adj, int64_t adj_stride,     /* graph s: dist_adj + s*adj_stride, N*N floats; NULL = ones */
                  const float *channels, int64_t chan_stride,    /* graph s: channels + s*chan_stride, L*N*N floats; NULL = ones */
                  int32_t *stats,                                /* [S, CM_COMM_COLS] */
                  void *stream);
int cm_episode_comm(int32_t T, int32_t B, int32_t N, int32_t L,
                    const int32_t *path_len,    /* [T,B] */
                    const int32_t *stats,       /* [T+1,B,CM_COMM_COLS] */
                    int32_t group_size, int32_t take, int32_t episodes_per_group, int32_t row0,
                    double *episodes,           /* [B/group_size * episodes_per_group, CM_EPC_COLS] */
                    void *stream);
int cm_comm_means(int32_t K, int32_t E, const double *episodes /* [K*E, CM_EPC_COLS] */,
                  double *summary /* [K, CM_EPC_COLS] */, void *stream);

/* Attention statistics: what the policy did with what the channel delivered.  The Comm-DP net records its attention matrix M
 * (row i = agent i's softmax weights over the team, before any mask: the reference's attention_weights); at hop l it uses
 * A_l = M * dist_adj * channels[l], renormalised per row (comm_base_net.py:101-103).  Pure functions of DEVICE arrays.
 *
 * cm_attn_stats turns S graphs into rows of CM_ATTN_COLS doubles.  Graph s reads the N*N floats at attn + s*attn_stride (required;
 * attn_stride >= N*N), and dist_adj / channels as cm_comm_stats does: strides in floats, a NULL array means all ones, a stride of 0
 * one block for every graph, any other stride at least the block size, an entry "set" when it is != 0.0f.  Unlike cm_comm_stats the
 * DIAGONAL of both masks is used as recorded, because the net uses it.  With K_l[i][j] = (dist_adj[i][j] set) && (channels[l][i][j]
 * set) and W_l[i] = sum_j M[i][j] K_l[i][j], each column a sum over the N rows i, the last three also over the L hops:
 *   column 0 self        = sum_i M[i][i]
 *          1 entropy     = sum_i -sum_j M[i][j] ln M[i][j]                 (nats; a term with M == 0 is 0)
 *          2 range_mass  = sum_i sum_j M[i][j] (dist_adj[i][j] set)
 *          3 kept_mass   = sum_l sum_i W_l[i]
 *          4 eff_self    = sum_l sum_i K_l[i][i] M[i][i] / W_l[i]          (a row with W_l[i] == 0 adds 0)
 *          5 eff_entropy = sum_l sum_i ( ln W_l[i] - (sum_j K_l[i][j] M[i][j] ln M[i][j]) / W_l[i] )      (W_l[i] == 0 adds 0)
 * Columns 4 and 5 are the self weight and the row entropy of the renormalised A_l - defined WITHOUT the 1e-12 the net adds to the
 * divisor.  f64 arithmetic on the f32 inputs, one log per attention value and one per row and hop, no atomics; the summation order
 * depends on (N, L) alone - not on S, the grid or the alignment of the buffers: the same inputs give the same bits.  Exactly S
 * rows are written; S = 0 launches nothing.  CM_ERR_ARG (text in cm_last_error) before anything is launched: S < 0, N outside
 * 1..255, L outside 1..8, attn_stride < N*N, a stride of a non-NULL mask that is neither 0 nor at least the block size, or NULL attn
 * or stats with S > 0.
 *
 * cm_episode_attn sums the rows of the slots an episode's policy acted through (0 .. n-1) into one row of CM_EPA_COLS doubles per
 * episode: cm_episode_comm's arguments, mapping and length rule, `stats` being the [T,B,CM_ATTN_COLS] rows of cm_attn_stats.
 * Columns 0-2 are divided by n N (means per agent), columns 3-5 by n N L (means per agent and hop), each sum divided once.
 * cm_attn_means reduces each of K groups of E consecutive rows to their column means, as cm_comm_means does.
 * cm_attn_curves / cm_attn_curve_means are cm_comm_curves / cm_comm_curve_means for these rows: per group and step the sum over the
 * running episodes of slot t's row (an ended episode counts as zero; accumulate = 1 adds to the table), then every sum divided
 * once by N * n_episodes (columns 0-2) or N * L * n_episodes (columns 3-5).  Their refusals are those of their comm twins.
 * All sums are f64 in one fixed order (lane-strided, then an xor tree; chunks of 64 envs in ascending order). */
#define CM_ATTN_COLS 6   /* self, entropy, range_mass, kept_mass, eff_self, eff_entropy: sums over a graph's rows (and hops) */
#define CM_EPA_COLS 6    /* the same names: means per agent (columns 0-2), per agent and hop (columns 3-5) */
int cm_attn_stats(int32_t S, int32_t N, int32_t L,
                  const float *attn, int64_t attn_stride,        /* graph s: attn + s*attn_stride, N*N floats */
                  const float *dist_adj, int64_t adj_stride,     /* graph s: dist_adj + s*adj_stride, N*N floats; NULL = ones */
                  const float *channels, int64_t chan_stride,    /* graph s: channels + s*chan_stride, L*N*N floats; NULL = ones */
                  double *stats,                                 /* [S, CM_ATTN_COLS] */
                  void *stream);
int cm_episode_attn(int32_t T, int32_t B, int32_t N, int32_t L,
                    const int32_t *path_len,    /* [T,B] */
                    const double *stats,        /* [T,B,CM_ATTN_COLS] */
                    int32_t group_size, int32_t take, int32_t episodes_per_group, int32_t row0,
                    double *episodes,           /* [B/group_size * episodes_per_group, CM_EPA_COLS] */
                    void *stream);
int cm_attn_means(int32_t K, int32_t E, const double *episodes /* [K*E, CM_EPA_COLS] */,
                  double *summary /* [K, CM_EPA_COLS] */, void *stream);
int cm_attn_curves(int32_t T, int32_t B, int32_t N, int32_t L,
                   const int32_t *path_len,    /* [T,B] */
                   const double *stats,        /* [T,B,CM_ATTN_COLS] */
                   int32_t group_size, int32_t take, int32_t accumulate,
                   double *sums,               /* [B/group_size, T, CM_ATTN_COLS] */
                   void *stream);
int cm_attn_curve_means(int32_t cells, int32_t T, int32_t n_episodes, int32_t N, int32_t L,
                        const double *sums /* [cells, T, CM_ATTN_COLS] */, double *curves /* [cells, T, CM_EPA_COLS] */,
                        void *stream);

/* Listening statistics: whether the messages changed what the agents did.  For one agent row let p be the action probabilities
 * the policy acted on and q the ones the same net gives on the same observations and range graph under a counterfactual channel
 * - mute (the identity: every agent hears only itself) or lossless (all ones: everything in range is delivered); both f32 of
 * length A.  In f64 on those f32 values:
 *   kl   = sum over a with p[a] > 0 of p[a] * (ln p[a] - ln max(q[a], FLT_MIN))     (FLT_MIN = 2^-126; not clamped: f32 rows sum to
 *                                                                                     1 only within rounding, so a hair below 0 is possible)
 *   tv   = 0.5 * sum_a |p[a] - q[a]|
 *   flip = 1 if argmax(p) != argmax(q) else 0                                        (the first index on ties, compared as f32)
 * Pure functions of DEVICE arrays.
 *
 * cm_listen_stats turns S graphs of N agents into rows of CM_LISTEN_COLS doubles, each column the sum over the N agent rows in
 * agent order: mute_kl, mute_tv, mute_flip, loss_kl, loss_tv, loss_flip.  Graph s reads the N*A floats at probs + s*probs_stride
 * and, for each counterfactual that is given, at mute + s*mute_stride / lossless + s*lossless_stride (strides in floats, at least
 * N*A).  A NULL counterfactual means "identical to probs": its three columns are written as exact 0 and nothing is read.  No
 * atomics; the summation order depends on (N, A) alone - not on S, the grid, the strides or the alignment of the buffers: the same
 * inputs give the same bits.  Exactly S rows are written; S = 0 launches nothing.  CM_ERR_ARG (text in cm_last_error) before
 * anything is launched: S < 0, N outside 1..255, A outside 2..8, a stride of a non-NULL array below N*A, or NULL probs or out with
 * S > 0.
 *
 * cm_episode_listen / cm_listen_means / cm_listen_curves / cm_listen_curve_means are cm_episode_attn / cm_attn_means /
 * cm_attn_curves / cm_attn_curve_means for these rows - the same arguments without n_hops, the same mapping, length rule, refusals
 * and fixed summation order - with ALL six columns divided by n N (N * n_episodes for the curves): there is no per-hop factor. */
#define CM_LISTEN_COLS 6   /* mute_kl, mute_tv, mute_flip, loss_kl, loss_tv, loss_flip: sums over a graph's agent rows */
#define CM_EPL_COLS 6      /* the same names: means per agent */
int cm_listen_stats(int32_t S, int32_t N, int32_t A,
                    const float *probs, int64_t probs_stride,        /* graph s: probs + s*probs_stride, N*A floats */
                    const float *mute, int64_t mute_stride,          /* graph s: mute + s*mute_stride, N*A floats; NULL = probs */
                    const float *lossless, int64_t lossless_stride,  /* graph s: lossless + s*lossless_stride; NULL = probs */
                    double *out,                                     /* [S, CM_LISTEN_COLS] */
                    void *stream);
int cm_episode_listen(int32_t T, int32_t B, int32_t N,
                      const int32_t *path_len,    /* [T,B] */
                      const double *stats,        /* [T,B,CM_LISTEN_COLS] */
                      int32_t group_size, int32_t take, int32_t episodes_per_group, int32_t row0,
                      double *episodes,           /* [B/group_size * episodes_per_group, CM_EPL_COLS] */
                      void *stream);
int cm_listen_means(int32_t K, int32_t E, const double *episodes /* [K*E, CM_EPL_COLS] */,
                    double *summary /* [K, CM_EPL_COLS] */, void *stream);
int cm_listen_curves(int32_t T, int32_t B, int32_t N,
                     const int32_t *path_len,    /* [T,B] */
                     const double *stats,        /* [T,B,CM_LISTEN_COLS] */
                     int32_t group_size, int32_t take, int32_t accumulate,
                     double *sums,               /* [B/group_size, T, CM_LISTEN_COLS] */
                     void *stream);
int cm_listen_curve_means(int32_t cells, int32_t T, int32_t n_episodes, int32_t N,
                          const double *sums /* [cells, T, CM_LISTEN_COLS] */, double *curves /* [cells, T, CM_EPL_COLS] */,
                          void *stream);

/* Critic statistics: how well the values of the critic trained with a policy explain the returns its episodes went on to collect,
 * and what that critic believes the messages are worth.  For env b over T recorded steps let n be the length of its first episode -
 * n = t + 1 for the first t with path_len[t][b] > 0, else T (the rule of cm_episode_stats) - and G the discounted return-to-go of
 * its f64 rewards r:
 *   G[n-1] = r[n-1],   G[t] = r[t] + gamma * G[t+1]     (f64, descending t, product and sum rounded separately; no bootstrap at
 *                                                        an episode cut at T, as cm_discount_returns and the update's returns)
 * With v = (double)values[t][b], row (t, b) for t < n holds CM_VALUE_COLS doubles:
 *   0 value = v   1 ret = G[t]   2 sq_err = (v - G[t])^2   3 ret_sq = G[t]^2
 *   4 msg_value = v - mute[t][b]          what the critic believes the messages are worth (mute: its value under the identity channel)
 *   5 loss_value = lossless[t][b] - v     what it believes the channel loss costs (lossless: its value under the all-ones channel)
 * and rows with t >= n are written as exact zeros.  Pure functions of DEVICE arrays.
 *
 * cm_value_stats writes exactly T*B rows.  A NULL counterfactual means "identical to values": its column is written as exact +0.0
 * and nothing is read.  One lane per env; no atomics; the order of operations of a row depends on (T, n) alone - not on B or the
 * grid: the same inputs give the same bits.  T = 0 or B = 0 launches nothing.  CM_ERR_ARG (text in cm_last_error) before anything
 * is launched: T < 0 or B < 0, gamma outside [0, 1] or not finite, or NULL rewards, path_len, values or stats with T*B > 0.
 *
 * cm_episode_value / cm_value_means / cm_value_curves / cm_value_curve_means are cm_episode_listen / cm_listen_means /
 * cm_listen_curves / cm_listen_curve_means for these rows - the same arguments without n_agents, the same mapping, length rule,
 * refusals and fixed summation order - with ALL six columns divided by n (n_episodes for the curves): means per step.  From an
 * episode's (or a cell's) means m: bias = m0 - m1, rmse = sqrt(m2), explained variance = 1 - (m2 - bias^2) / (m3 - m1^2). */
#define CM_VALUE_COLS 6   /* value, ret, sq_err, ret_sq, msg_value, loss_value: per recorded step */
#define CM_EPV_COLS 6     /* the same names: means per step */
int cm_value_stats(int32_t T, int32_t B,
                   const double *rewards,     /* [T,B] */
                   const int32_t *path_len,   /* [T,B] */
                   const float *values,       /* [T,B] */
                   const float *mute,         /* [T,B]; NULL = values */
                   const float *lossless,     /* [T,B]; NULL = values */
                   double gamma,
                   double *stats,             /* [T,B,CM_VALUE_COLS] */
                   void *stream);
int cm_episode_value(int32_t T, int32_t B,
                     const int32_t *path_len,    /* [T,B] */
                     const double *stats,        /* [T,B,CM_VALUE_COLS] */
                     int32_t group_size, int32_t take, int32_t episodes_per_group, int32_t row0,
                     double *episodes,           /* [B/group_size * episodes_per_group, CM_EPV_COLS] */
                     void *stream);
int cm_value_means(int32_t K, int32_t E, const double *episodes /* [K*E, CM_EPV_COLS] */,
                   double *summary /* [K, CM_EPV_COLS] */, void *stream);
int cm_value_curves(int32_t T, int32_t B,
                    const int32_t *path_len,    /* [T,B] */
                    const double *stats,        /* [T,B,CM_VALUE_COLS] */
                    int32_t group_size, int32_t take, int32_t accumulate,
                    double *sums,               /* [B/group_size, T, CM_VALUE_COLS] */
                    void *stream);
int cm_value_curve_means(int32_t cells, int32_t T, int32_t n_episodes,
                         const double *sums /* [cells, T, CM_VALUE_COLS] */, double *curves /* [cells, T, CM_EPV_COLS] */,
                         void *stream);

/* Bootstrap intervals and paired contrasts of the evaluation scores: the episode tables the reductions above fill - table
 * [cells, n, cols] doubles, row e of a cell one episode - resampled over the EPISODES on the device.  Pure functions of DEVICE
 * arrays.
 *
 * cm_boot_means forms R resampled means of every cell.  Resample r draws n rows with replacement,
 *   idx_j = ((uint64_t)w_j * n) >> 32,  j = 0 .. n-1,
 *   w_j   = component j & 3 of philox4x32_10(counter = (r, j >> 2, SITE_BOOT = 10, 0), key = (seed_lo, seed_hi))
 * (csrc/cm_rng.h), and means[g][r][c] = (sum_j table[g][idx_j][c]) / n: the sum f64, sequential in ascending j, divided ONCE.  The
 * index stream depends on (seed, r, j) alone - NOT on the cell, the column or the table: resample r of every cell, every column and
 * every table of a call with one seed picks the same episodes.  That is what makes a key derived from several columns a joint
 * resample and the difference of two cells a PAIRED one.  The multiply-high mapping prefers some rows by at most n / 2^32 in
 * probability.  One lane per resample, one workgroup per cell and block of 256 resamples; the cell's table is staged in LDS when
 * n * cols * 8 <= 32768 bytes (the staging budget; the environment variable COMMARL_BOOT_STAGE_BYTES, read at every call, lowers
 * it - a debugging switch) and read from global memory above it, the same sums in the same order either way: the same bits.  No
 * atomics, one writer per output, the same inputs give the same bits.  cols must be 4, 6 or 9 (the row widths there are).
 * CM_ERR_ARG (text in cm_last_error) before anything is launched: cells < 1, n < 1, another cols, R outside 2..CM_BOOT_MAX_R, a
 * NULL table or means.
 *
 * cm_boot_quantiles turns those means into CM_BOOT_OUT doubles per cell and KEY.  `kind` says how a key comes from the cols
 * columns m of a row of means, operation by operation what evaluate.py's host functions do on the point estimates:
 *   CM_BOOT_COLUMNS  cols keys: key k = m[k]                                              (cols 4, 6 or 9)
 *   CM_BOOT_COMM     5 keys: m[0 .. 3], then delivery = m[0] != 0 ? m[1] / m[0] : 1.0     (cols 4: range_degree, heard_degree, ...)
 *   CM_BOOT_VALUE    7 keys: m[0], m[1], bias = m[0] - m[1], rmse = sqrt(m[2]),           (cols 6: value, ret, sq_err, ret_sq,
 *                    ev, m[4], m[5], where with resid = m[2] - bias * bias, var = m[3] - m[1] * m[1] and                msg, loss)
 *                    eps = 1e-12 * max(1.0, m[3]):  ev = var <= eps ? (resid <= eps ? 1.0 : 0.0) : 1.0 - resid / var
 * every product, sum, quotient and root a separately rounded f64 operation.  One workgroup per (cell g, key k) forms
 *   v_r = key_k(means[g][r][:])                                      ref_cell == NULL
 *   v_r = key_k(means[g][r][:]) - key_k(means[ref_cell[g]][r][:])    else: the contrast of cell g against cell ref_cell[g]
 * for r = 0 .. R-1, sorts them ascending in LDS (a bitonic network, padded with +inf to a power of two) and writes out[g][k][:]:
 *   0 lo   = sorted[lo_rank]           1 hi = sorted[hi_rank]        order statistics, not interpolated
 *   2 se   = sqrt(sum_r (v_r - mean)^2 / (R - 1)), mean = (sum_r v_r) / R: two passes, each sum in one fixed order
 *   3 p_gt = (#{v_r > 0} + 0.5 * #{v_r == 0}) / R: integer counts, divided once
 * A cell whose ref_cell is itself holds exact zeros and p_gt = 0.5.  ref_cell[g] must lie in 0 .. cells-1: the CALLER checks that
 * (the table lives on the device); an entry outside is read as g itself, never out of bounds.  No atomics, one writer per output,
 * the same inputs give the same bits.  CM_ERR_ARG (text in cm_last_error) before anything is launched: another kind, a cols the
 * kind does not take, cells < 1, R outside 2..CM_BOOT_MAX_R, not 0 <= lo_rank <= hi_rank < R, a NULL means or out. */
#define CM_BOOT_OUT 4        /* lo, hi, se, p_gt */
#define CM_BOOT_MAX_R 4096   /* resamples per call: the sort's LDS tile */
#define CM_BOOT_COLUMNS 0
#define CM_BOOT_COMM 1
#define CM_BOOT_VALUE 2
int cm_boot_means(int32_t cells, int32_t n, int32_t cols,
                  const double *table,        /* [cells, n, cols] */
                  int32_t R, uint32_t seed_lo, uint32_t seed_hi,
                  double *means,              /* [cells, R, cols] */
                  void *stream);
int cm_boot_quantiles(int32_t kind, int32_t cells, int32_t R, int32_t cols,
                      const double *means,    /* [cells, R, cols] */
                      const int32_t *ref_cell,/* [cells] or NULL */
                      int32_t lo_rank, int32_t hi_rank,
                      double *out,            /* [cells, keys, CM_BOOT_OUT] */
                      void *stream);

/* Per-step evaluation curves: the rounds of cm_episode_stats / cm_episode_comm reduced over the EPISODES with the step axis kept -
 * the mean over episodes of the per-step lists the reference's test loop pads with zeros to max_env_steps and saves as rewMat3
 * (exp_runners/testing.py:307-324, pad_sequence(..., padding_value=0)).  Pure functions of DEVICE arrays.
 *
 * cm_episode_curves takes cm_episode_stats's arguments up to `take`; the env-to-group mapping (group k = b / group_size, envs
 * with b % group_size >= take are not read), the first-episode rule and the episode length n are cm_episode_stats's.  For group k
 * and step t it forms the SUMS over the group's `take` episodes of the per-step values below, into sums[k][t][CM_EPI_COLS]; an
 * episode with n <= t contributes zero to every column (the reference's zero padding).  For a running episode (t < n), with
 * d = details[t][b]:
 *   column 0 success[t][b]
 *          1 reward_f64[t][b]                                              (f64)
 *          2 d[0]          3 the count 1          4 d[1]          5 d[2]          7 d[4]          8 d[3]
 *          6 the sum of the N x N floats of dist_adj[s][b], s = t + 1 for t < n - 1 and s = n - 1 for the terminal step (n = 1:
 *            slot 0) - the slots behind cm_episode_stats's nodeDeg; N * N when dist_adj is NULL (the constant full graph)
 * Columns other than the reward are sums of integers (adjacency entries are 0 or 1), held exactly in a double.  accumulate = 0
 * overwrites group k's [T, CM_EPI_COLS] block, accumulate = 1 adds to it: the rounds of an evaluation land in one table.  Exactly
 * the blocks of the B / group_size groups are written.
 *
 * cm_curve_means turns `cells` such blocks into curves[cells][T][CM_EPI_COLS]: every sum divided ONCE by the exact product that
 * makes it the mean over all n_episodes episodes of the zero-padded per-step value eval_model lists (evaluate._episode) -
 * success, reward, step_cnt by n_episodes; capture_cnt and penalty_cnt by n_episodes (CM_CO: N * n_episodes); move_cnt, nodeDeg,
 * variable by N * n_episodes; vars2 is 0 (CM_CO: column 8 / (N * n_episodes)).  Column order: CM_EPI_COLS's.  Column 3
 * (step_cnt) is therefore the share of episodes still running at step t: another column divided by it is the mean over the
 * RUNNING episodes, where the plain column is the mean over all of them with the ended ones counted as zero.
 *
 * cm_comm_curves does the same for the [T+1,B,CM_COMM_COLS] rows of cm_comm_stats: cm_episode_comm's arguments with
 * (accumulate, sums) in place of the row mapping.  Step t of a running episode adds the row of slot t (the graph the policy
 * acted through, as in cm_episode_comm) to sums[k][t][CM_COMM_COLS].  cm_comm_curve_means turns `cells` blocks into
 * curves[cells][T][CM_EPC_COLS] with cm_episode_comm's divisors, n replaced by n_episodes: range_degree, reach and range_reach
 * by N * n_episodes, heard_degree by N * L * n_episodes.
 *
 * All four: no atomics and one writer per entry.  The integer columns are exact; the reward sums add a round's envs in one fixed
 * order (chunks of 64 envs in ascending order, a chunk's lanes through one xor butterfly) and the rounds in call order, so two
 * runs on the same inputs write the same bits.  B = 0 or take = 0 launches nothing.  CM_ERR_ARG (text in cm_last_error) before anything is launched: what
 * cm_episode_stats / cm_episode_comm refuse for the shared arguments, accumulate other than 0 or 1, cells, T or n_episodes
 * below 1, or a NULL pointer other than dist_adj where there is work to do. */
int cm_episode_curves(int32_t T, int32_t B, int32_t N, int32_t scenario,     /* CM_PP / CM_CO */
                      const double *reward_f64,   /* [T,B]   */
                      const int32_t *details,     /* [T,B,6] */
                      const int32_t *success,     /* [T,B]   */
                      const int32_t *path_len,    /* [T,B]   */
                      const float *dist_adj,      /* [T+1,B,N,N], or NULL = constant full graph */
                      int32_t group_size, int32_t take, int32_t accumulate,
                      double *sums,               /* [B/group_size, T, CM_EPI_COLS] */
                      void *stream);
int cm_curve_means(int32_t cells, int32_t T, int32_t n_episodes, int32_t scenario, int32_t N,
                   const double *sums /* [cells, T, CM_EPI_COLS] */, double *curves /* [cells, T, CM_EPI_COLS] */, void *stream);
int cm_comm_curves(int32_t T, int32_t B, int32_t N, int32_t L,
                   const int32_t *path_len,    /* [T,B] */
                   const int32_t *stats,       /* [T+1,B,CM_COMM_COLS] */
                   int32_t group_size, int32_t take, int32_t accumulate,
                   double *sums,               /* [B/group_size, T, CM_COMM_COLS] */
                   void *stream);
int cm_comm_curve_means(int32_t cells, int32_t T, int32_t n_episodes, int32_t N, int32_t L,
                        const double *sums /* [cells, T, CM_COMM_COLS] */, double *curves /* [cells, T, CM_EPC_COLS] */,
                        void *stream);

/* Comm-DP policy weights (device pointers), reference state_dict names in comments
 * (SURVEY.md §8 a-16).  Linear weights are passed TRANSPOSED [in,out] (contiguous over the
 * output index) - the veneer keeps a transposed device copy; GCN weights are already [in,out]. */
typedef struct cm_policy_weights {
    int32_t d, n_agents, n_hops, enc_hidden, emb, h1, h2, h3, n_act;
    int32_t no_residual;             /* 0 (default): x = E + H_L (comm_categorical_mlp_policy.py:74-77); 1: x = H_L */
    const float *enc_w1t, *enc_b1;   /* encoder._layers.0.linear.{weight^T,bias}          [d,128],[128] */
    const float *enc_w2t, *enc_b2;   /* encoder._output_layers.0.linear.*                 [128,64],[64] */
    const float *attn_wt;            /* attention_layer.linear_in.weight^T                [64,64] */
    const float *gcn_w, *gcn_b;      /* gcn_layers.{l}.{weight,bias}                      [L,64,64],[L,64] */
    const float *hd_w1t, *hd_b1;     /* categorical_output_layer._layers.0.linear.*       [64,128] */
    const float *hd_w2t, *hd_b2;     /* ..._layers.1.linear.*                             [128,64] */
    const float *hd_w3t, *hd_b3;     /* ..._layers.2.linear.*                             [64,32] */
    const float *hd_w4t, *hd_b4;     /* ..._output_layers.0.linear.*                      [32,5] */
    const float *mfma_pack;          /* cm_policy_pack() output, or NULL: without it the generic VALU kernel runs */
} cm_policy_weights;

typedef struct cm_critic_weights {
    int32_t d, n_agents, n_hops, enc_hidden, emb, dec_hidden;
    int32_t no_residual, _pad;
    const float *enc_w1t, *enc_b1, *enc_w2t, *enc_b2, *attn_wt, *gcn_w, *gcn_b;
    const float *dec_w1t, *dec_b1;   /* baseline_aggregator._mean_module._layers.0.linear.*        [64,64] */
    const float *dec_w2t, *dec_b2;   /* baseline_aggregator._mean_module._output_layers.0.linear.* [64,1] */
    const float *mfma_pack;          /* cm_critic_pack() output, or NULL */
} cm_critic_weights;

/* Matrix-core operand pack.  The MFMA forward kernels read every dense layer's weights as ready-made
 * v_mfma_f32_16x16x4_f32 B fragments - [column tile][16-deep k block][lane][4] with the zero padding baked in - so a
 * wave fetches 1 KB per instruction, unconditionally, instead of 4 predicated dword gathers per fragment.
 * cm_*_pack_bytes: size of the pack for this net, 0 when the shape has no matrix-core instantiation (then leave
 * mfma_pack NULL).  cm_*_pack: (re)build it on `stream` from the plain [in,out] weights in *w - call after every
 * weight update; the buffer is caller-owned and may be rewritten in place (captured hipGraphs keep working).
 * The default kernels carry every weight as an (hi, lo) pair of f16 values: a weight with |w| > 65504, inf or NaN cannot
 * be carried, and cm_*_pack REFUSE such a net (CM_ERR_ARG, text in cm_last_error()) instead of packing +-inf planes.  The
 * check costs one 4-byte copy and a wait for the pack kernels on `stream`; it is skipped while `stream` is being captured
 * (a capture cannot wait) and with COMMARL_PACK_CHECK=0.  Observations are expected in the envs' range ([-1, 1]); a
 * foreign caller's |obs| > 65504 saturates the same way and is NOT checked per step. */
size_t cm_policy_pack_bytes(const cm_policy_weights *w);
int cm_policy_pack(const cm_policy_weights *w, float *pack, void *stream);
/* The pack has sections - the all-f32 fragments (COMMARL_POLICY_KERNEL=f32, shapes without an f16 instantiation), the f16-split
 * fragments (every default kernel incl. the training forward), the wave-owned rollout kernel's fragments (teams of 4) - and a
 * caller that knows its next consumer may refresh only what that consumer reads: an optimiser step followed by a training
 * forward needs CM_PACK_F16 alone (10 launches and no wait instead of ~30 and one), the next rollout CM_PACK_ALL.
 * cm_policy_pack / cm_critic_pack = CM_PACK_ALL.  A section that was skipped is STALE until a later call packs it. */
#define CM_PACK_F32 1
#define CM_PACK_F16 2
#define CM_PACK_WAVE 4
#define CM_PACK_CHECK 8           /* the f16 range check (waits for the pack kernels) */
#define CM_PACK_ALL 15
int cm_policy_pack_sections(const cm_policy_weights *w, float *pack, int32_t sections, void *stream);
size_t cm_critic_pack_bytes(const cm_critic_weights *w);
int cm_critic_pack(const cm_critic_weights *w, float *pack, void *stream);
int cm_critic_pack_sections(const cm_critic_weights *w, float *pack, int32_t sections, void *stream);

/* CommCategoricalMLPPolicy.get_actions (comm_categorical_mlp_policy.py:98-119) for S env
 * states in one fused launch: encoder -> attention -> L x (mask, renorm, GCN) -> residual ->
 * head -> softmax x avail -> renorm -> sample (inverse CDF on the Philox stream) or argmax.
 *   obs [S,N,d]; avail [S,N,A] or NULL (= all ones, predatorprey_wrapper.py:46-51);
 *   dist_adj [S,N,N] or NULL (= ones); channels [S,L,N,N] or NULL (= ones);
 *   out: actions int32 [S,N] (or NULL), probs [S,N,A] (or NULL), attn [S,N,N] (or NULL).
 *   The sampler's Philox counter word is policy_step + (policy_step_base ? *policy_step_base : 0);
 *   the device-side base lets a captured hipGraph be replayed with fresh draws. */
int cm_policy_forward(const cm_policy_weights *w, int32_t n_samples, const float *obs, const float *avail,
                      const float *dist_adj, const float *channels, uint64_t seed, int32_t env_id_offset,
                      uint32_t policy_step, const uint32_t *policy_step_base, int32_t greedy, int32_t *actions,
                      float *probs, float *attn, void *stream);

/* CommBaseCritic.forward (comm_base_critic.py:91-114): values [S] = sum over agents. */
int cm_critic_forward(const cm_critic_weights *w, int32_t n_samples, const float *obs, const float *dist_adj,
                      const float *channels, float *values, void *stream);

/* A Comm-DP policy of ANY layer sizes (the runners' --encoder_hidden_sizes, --embedding_dim and
 * --categorical_mlp_hidden_sizes, exp_runners/env_uitils.py:83-90): n_enc = 1..3 encoder hidden layers, n_head = 1..4
 * head hidden layers, every width, emb and d in 1..128.  Weights are plain device pointers, linear weights TRANSPOSED
 * [in,out]; slot n_enc of enc_wt / enc_b is the encoder's output layer (-> emb), slot n_head of head_wt / head_b the
 * logits layer (-> n_act).  attn_wt [emb,emb], NULL = 'dot' attention (Q = E).  gcn_w [L,emb,emb] stacked, gcn_b [L,emb]
 * or NULL (gcn_bias=False). */
typedef struct cm_net_weights {
    int32_t d, n_agents, n_hops, n_act, no_residual, emb;
    int32_t n_enc, enc_hidden[3];
    int32_t n_head, head_hidden[4];
    int32_t _pad;
    const float *enc_wt[4], *enc_b[4];
    const float *attn_wt, *gcn_w, *gcn_b;
    const float *head_wt[5], *head_b[5];
} cm_net_weights;
/* cm_policy_forward for such a net, in one launch (csrc/cm_policy_g.hip: every dense layer on v_mfma_f32_16x16x4_f32,
 * activations in LDS): same inputs, outputs, Philox stream and arithmetic order of the softmax x avail + draw.
 * Returns 1 - nothing launched - when the shape is outside the bounds above or one workgroup's LDS need exceeds 160 KB
 * (large teams of wide nets): the caller then runs layer by layer. */
int cm_policy_forward_any(const cm_net_weights *w, int32_t n_samples, const float *obs, const float *avail,
                          const float *dist_adj, const float *channels, uint64_t seed, int32_t env_id_offset,
                          uint32_t policy_step, const uint32_t *policy_step_base, int32_t greedy, int32_t *actions,
                          float *probs, float *attn, void *stream);

/* CommBaseCritic.forward with aggregator_type='sum' for such a net, in one launch (csrc/cm_critic_g.hip: the policy kernel's
 * trunk, then the decoder): head_* carry baseline_aggregator._mean_module - n_head = 1..4 tanh hidden layers, slot n_head the
 * [K,1] output layer - and n_act must be 1.  values[s] = sum over the env's agents of the decoder's output, summed in agent
 * order by one thread (no atomic: the same bits on every launch).  Returns 1 - nothing launched, nothing written - where
 * cm_policy_forward_any does. */
int cm_critic_forward_any(const cm_net_weights *w, int32_t n_samples, const float *obs, const float *dist_adj,
                          const float *channels, float *values, void *stream);

/* Training forward (PPO update): the same fused forward, which additionally stores every activation the backward pass
 * needs ONCE, as f32 [R = S * n_agents rows, width] (the value the rest of the network saw): what torch's autograd would
 * keep layer by layer through ~20 separate kernels.  Pointers that are NULL are skipped.
 *   a1 [R,128] encoder hidden layer     e [R,64] encoder output E     q [R,64] attention query E.Wa^T
 *   hw[l] [R,64] H_l.Wg_l               h[l] [R,64] hop l's output tanh(A_l.hw[l] + b_l); the LAST hop's entry includes the
 *                                       residual (x = E + H_L, comm_categorical_mlp_policy.py:74-77) unless no_residual
 *   x1, x2, x3  head hidden layers: policy [R,128], [R,64], [R,32]; critic x1 [R,64] only
 *   out         policy: logits [R, n_act] (before softmax / avail mask); critic: per-agent value [R] (before the sum)
 *   probs       policy only: the action probabilities [R, n_act] exactly as cm_policy_forward returns them (no avail mask)
 * attn [S,N,N] is written as in cm_policy_forward.  Returns 1 - nothing done - when there is no saved-forward
 * instantiation for the shape (teams of <= 128 agents, n_hops <= 4, obs dim <= 96): the caller then runs layer by layer. */
typedef struct cm_fwd_saves {
    float *a1, *e, *q, *hw[4], *h[4], *x1, *x2, *x3, *out, *probs;
} cm_fwd_saves;
int cm_policy_forward_saved(const cm_policy_weights *w, int32_t n_samples, const float *obs, const float *dist_adj,
                            const float *channels, float *attn, const cm_fwd_saves *sv, void *stream);
int cm_critic_forward_saved(const cm_critic_weights *w, int32_t n_samples, const float *obs, const float *dist_adj,
                            const float *channels, float *attn, float *values, const cm_fwd_saves *sv, void *stream);
/* cm_policy_forward_saved / cm_critic_forward_saved for teams of 4 on the wave-owned kernel of the rollout (csrc/cm_policy_w_dev.h): one persistent
 * workgroup per CU stages the weights once and walks the batch, a wave carries 16 agent rows through the whole net in registers
 * and stores the saved activations from there.  Needs the CM_PACK_WAVE section of the operand pack to be current (between
 * optimiser steps: cm_policy_pack_sections(..., CM_PACK_F16 | CM_PACK_WAVE, ...)).  Same saves, same values to the f16-split
 * kernels' rounding (1e-6 relative).  Returns 1 - nothing done - for every other shape: call cm_policy_forward_saved / cm_critic_forward_saved. */
int cm_policy_forward_saved_wave(const cm_policy_weights *w, int32_t n_samples, const float *obs, const float *dist_adj,
                                 const float *channels, float *attn, const cm_fwd_saves *sv, void *stream);
int cm_critic_forward_saved_wave(const cm_critic_weights *w, int32_t n_samples, const float *obs, const float *dist_adj,
                                 const float *channels, float *attn, float *values, const cm_fwd_saves *sv, void *stream);

/* One rollout step in ONE launch: cm_policy_forward over the B envs of `h` followed, inside the same workgroups, by
 * cm_env_step on the sampled actions (which travel through LDS and are also written to `actions`): what one iteration
 * of the sampler loop does (centralized_ma_on_policy_vectorized_sampler.py:133-141).  Arguments and results are those
 * of the two calls (n_samples is the handle's B; obs / dist_adj / channels are the CURRENT step's inputs, `out` receives
 * the next step's), bit-identical to calling them back to back.
 * Returns 0 on success, < 0 on error, and 1 - having done nothing - when this (scenario, team size, obs dim) has no
 * fused instantiation or no operand pack was supplied: call the two entry points instead. */
int cm_rollout_step(cm_env_t h, const cm_policy_weights *w, const float *obs, const float *avail,
                    const float *dist_adj, const float *channels, uint64_t seed, int32_t env_id_offset,
                    uint32_t policy_step, const uint32_t *policy_step_base, int32_t greedy, int32_t *actions,
                    float *probs, float *attn, const cm_rng_tape *tape, const cm_step_out *out, void *stream);

/* n_steps consecutive rollout steps in ONE launch: step t = cm_rollout_step with every pointer advanced by t x its
 * per-step stride (time-major trajectory buffers [T(+1), B, ...]: obs / dist_adj / channels are read at slot t and -
 * through `out` - written at slot t + 1) and policy_step + t.  A workgroup keeps its envs for the whole chunk and no
 * grid-wide synchronisation separates the steps, so env phases overlap other workgroups' matrix phases.  Production
 * RNG only (tape mode is refused); no avail mask.  Results are bit-identical to n_steps calls of cm_rollout_step.
 * Strides are in ELEMENTS of the respective buffer; unused outputs may have stride 0.  Returns as cm_rollout_step. */
typedef struct cm_chunk_strides {
    int64_t obs, actions, probs, attn, reward, reward_f64, done, details, dist_adj, channels, prey_alive, success, path_len;
} cm_chunk_strides;
int cm_rollout_chunk(cm_env_t h, const cm_policy_weights *w, int32_t n_steps, const cm_chunk_strides *strides,
                     const float *obs, const float *dist_adj, const float *channels, uint64_t seed,
                     int32_t env_id_offset, uint32_t policy_step, const uint32_t *policy_step_base, int32_t greedy,
                     int32_t *actions, float *probs, float *attn, const cm_step_out *out, void *stream);

/* cm_rollout_chunk with SEVERAL policies of one architecture in the same launch (evaluating many checkpoints at once): the B envs
 * of `h` are split into workgroups of 16 consecutive envs, and workgroup g runs the policy whose pack is packs[wg_policy[g]].
 * `w` gives the shape every member shares (its weight pointers are not read).  Every other argument is that of cm_rollout_chunk, and
 * env b draws what it would draw in a single-policy launch at the same global env id (env_id_offset + b): a workgroup's results
 * are bit-identical to cm_rollout_chunk with its policy.  Preconditions, NOT checked on the device:
 *   - each workgroup's 16 envs belong to one policy, i.e. every policy's env range except the last one's ends on a multiple of 16;
 *   - every wg_policy value lies in [0, n_policies) (build and check the table on the host, then upload it);
 *   - the CM_PACK_WAVE section of every pack is current.
 * Returns 0 when the multi-policy kernel was launched, < 0 on error, and 1 - having done nothing - when the shape is not teams of 4
 * on the wave-owned kernel (or the sizes do not fit it): the caller then runs each policy on its envs (cm_policy_forward on the
 * group's rows) and one cm_env_step per step. */
typedef struct cm_policy_set {
    int32_t n_policies, n_wg;        /* n_wg = ceil(B / 16) */
    const float *const *packs;       /* DEVICE array [n_policies] of cm_policy_pack() outputs */
    const int32_t *wg_policy;        /* DEVICE array [n_wg], values in [0, n_policies) */
} cm_policy_set;
int cm_rollout_chunk_multi(cm_env_t h, const cm_policy_weights *w, const cm_policy_set *set, int32_t n_steps,
                           const cm_chunk_strides *strides, const float *obs, const float *dist_adj, const float *channels,
                           uint64_t seed, int32_t env_id_offset, uint32_t policy_step, const uint32_t *policy_step_base,
                           int32_t greedy, int32_t *actions, float *probs, float *attn, const cm_step_out *out, void *stream);

/* cm_policy_forward for SEVERAL policies of one architecture in ONE launch, each on its own contiguous range of the envs: member k
 * acts on the group_sizes[k] envs behind those of members 0 .. k-1.  Every output is bit-identical to cm_policy_forward with member
 * k's weights on its group's rows and env_id_offset + the group's first env (one seed for the set).  For the teams the f16-split
 * workgroup-tiled kernel serves; teams of 4 have cm_rollout_chunk_multi.
 *
 * cm_policy_forward_multi_plan (host only, no device work): checks the set - n_policies >= 1, every group size >= 1, the sizes sum
 * to n_envs, every member has the shape of members[0], an operand pack (mfma_pack, with a current CM_PACK_F16 section) and its bias
 * pointers - and returns the size in bytes of the table the launch reads, *n_wg = the launch's workgroup count (a group ends in a
 * ragged workgroup of its own, never shared with the next member); with `image` non-NULL (image_bytes >= that size) the table's
 * host image is written there: n_wg cm_forward_set_wg descriptors, then n_policies cm_forward_set_member records.  The caller
 * uploads the image to device memory it owns and rebuilds it when a member's pack or weight buffers move or the groups change.
 * Returns 0 (*n_wg = 0, nothing written) when the shape has no set kernel - teams of 4, more than 80 agents, an observation
 * dim without an f16 instantiation, COMMARL_POLICY_KERNEL=f32 / valu, an LDS need above 160 KB - and < 0 on a refused set.
 *
 * cm_policy_forward_multi: the launch.  `shape` = any member's weights (dims, n_act, no_residual; its weight pointers are not
 * read), table_dev = the uploaded image, n_wg / n_envs = the planner's; every other argument is cm_policy_forward's over the
 * whole batch.  No allocation, copy or synchronisation: it can be captured in a hipGraph.  The kernel trusts the table.  Returns
 * 0 when launched, < 0 on error, and 1 - nothing launched - where the planner returns 0 or `shape` has no operand pack: the
 * caller then runs cm_policy_forward per member. */
typedef struct cm_forward_set_wg {
    int32_t member, block;           /* workgroup -> member, and its block index inside the member's group */
} cm_forward_set_wg;
typedef struct cm_forward_set_member {
    int32_t first_env, n_envs;       /* the member's group */
    const void *pack;                /* the f16-split section of the member's operand pack */
    const float *enc_b1, *enc_b2, *gcn_b, *hd_b1, *hd_b2, *hd_b3, *hd_b4;   /* biases: plain f32, outside the pack */
} cm_forward_set_member;
int64_t cm_policy_forward_multi_plan(const cm_policy_weights *members, const int32_t *group_sizes, int32_t n_policies,
                                     int32_t n_envs, void *image, size_t image_bytes, int32_t *n_wg);
int cm_policy_forward_multi(const cm_policy_weights *shape, const void *table_dev, int32_t n_wg, int32_t n_envs,
                            const float *obs, const float *avail, const float *dist_adj, const float *channels, uint64_t seed,
                            int32_t env_id_offset, uint32_t policy_step, const uint32_t *policy_step_base, int32_t greedy,
                            int32_t *actions, float *probs, float *attn, void *stream);

/* cm_policy_forward_any for SEVERAL Comm-DP policies in ONE launch, each on its own contiguous range of the envs - and the members
 * may differ in their layer sizes: encoder hidden sizes, embedding, head hidden sizes, 'general' / 'dot' attention (attn_wt NULL),
 * residual, GCN bias (gcn_b NULL).  They share n_agents, d, n_hops and n_act.  A workgroup owns whole envs of ONE member, reads
 * that member's sizes and weight pointers from the table and runs cm_policy_forward_any's body on them (csrc/cm_policy_gm.hip):
 * every output is bit-identical to cm_policy_forward_any with member k's weights on its group's rows and env_id_offset + the
 * group's first env (one seed for the set).
 *
 * cm_policy_forward_any_multi_plan (host only, no device work): checks the set and returns the size in bytes of the table the
 * launch reads, *n_wg = the launch's workgroup count = sum over k of ceil(group_sizes[k] / EPB), EPB = max(1, 48 / n_agents) (a
 * group ends in a ragged workgroup of its own, never shared with the next member), *lds_bytes = the launch's dynamic LDS (the
 * largest member's need; every workgroup zeroes and uses its own member's map only).  With `image` non-NULL (image_bytes >= that
 * size) the table's host image is written there: n_wg cm_forward_set_wg descriptors, then n_policies cm_any_set_member records.
 * The caller uploads the image to device memory it owns and rebuilds it when a member's weight buffers move or the groups change;
 * the weights themselves are read at launch time.  Returns
 *   0 (*n_wg = 0, nothing written: no set kernel) when a member is outside cm_policy_forward_any's bounds or needs more than
 *     160 KB of LDS (*lds_bytes = the largest need found, 0 when a member is out of bounds);
 *   CM_ERR_ARG (< 0, cm_last_error set) for a null argument, n_policies < 1, members that differ in n_agents, d, n_hops or
 *     n_act, a group of fewer than 1 env, group sizes that do not sum to n_envs, a null weight cm_policy_forward_any requires, or
 *     an image buffer that is too small.
 *
 * cm_policy_forward_any_multi: the launch.  `shape` = any member's weights (n_agents, d, n_hops, n_act are read, and its layer sizes
 * only to answer 1), table_dev = the uploaded image, n_wg / n_envs / lds_bytes = the planner's; every argument from `obs` on is
 * cm_policy_forward_any's over the whole batch.  No allocation, copy or synchronisation: it can be captured in a hipGraph.  The
 * kernel trusts the table.  Returns 0 when launched; 1 - nothing launched, nothing written - when `shape` is a net
 * cm_policy_forward_any answers 1 for, or lds_bytes is 0 or above 160 KB (the planner's answer for a set it declines): the caller
 * then runs cm_policy_forward_any (or layer by layer) per member; CM_ERR_ARG for a null shape / obs / table, an n_wg outside
 * [ceil(n_envs / EPB), n_envs], or an lds_bytes below `shape`'s own need. */
typedef struct cm_any_set_member {
    int32_t first_env, n_envs;       /* the member's group */
    int32_t emb, no_residual;
    int32_t n_enc, enc_h[3];
    int32_t n_head, head_h[4];
    int32_t SE, SW;                  /* LDS row strides of the member's planes: pad16(emb) + 4, pad16(max(widest layer, d)) + 4 */
    int32_t _pad;
    const float *enc_w[3], *enc_b[3], *enc_wo, *enc_bo;     /* hidden layers (slots >= n_enc NULL), then the output layer (-> emb) */
    const float *attn_wt, *gcn_w, *gcn_b;                   /* attn_wt NULL = 'dot'; gcn_b NULL = no GCN bias */
    const float *head_w[4], *head_b[4], *head_wo, *head_bo; /* hidden layers (slots >= n_head NULL), then the logits layer */
} cm_any_set_member;
int64_t cm_policy_forward_any_multi_plan(const cm_net_weights *members, const int32_t *group_sizes, int32_t n_policies,
                                         int32_t n_envs, void *image, size_t image_bytes, int32_t *n_wg, size_t *lds_bytes);
int cm_policy_forward_any_multi(const cm_net_weights *shape, const void *table_dev, int32_t n_wg, int32_t n_envs,
                                size_t lds_bytes, const float *obs, const float *avail, const float *dist_adj,
                                const float *channels, uint64_t seed, int32_t env_id_offset, uint32_t policy_step,
                                const uint32_t *policy_step_base, int32_t greedy, int32_t *actions, float *probs, float *attn,
                                void *stream);

/* cm_rollout_chunk followed by cm_chunk_tail (below) for the same chunk: the observation (and masks, where the env produces
 * them) the last step wrote - out->obs + (n_steps - 1) * strides->obs, ... - carried into obs_next / dist_adj_next /
 * channels_next (slot 0 of the caller's ring; the mask pointers may be NULL) and *policy_step_base += n_steps.  Where the wave-owned
 * kernel takes the chunk the tail is part of that launch (a wave writes its envs' next observation itself, the last wave to
 * finish advances the counter): one launch per chunk; everywhere else the two launches of the separate calls.  Returns as
 * cm_rollout_chunk (1: nothing was launched, tail included). */
int cm_rollout_chunk_tail(cm_env_t h, const cm_policy_weights *w, int32_t n_steps, const cm_chunk_strides *strides,
                          const float *obs, const float *dist_adj, const float *channels, uint64_t seed,
                          int32_t env_id_offset, uint32_t policy_step, uint32_t *policy_step_base, int32_t greedy,
                          int32_t *actions, float *probs, float *attn, const cm_step_out *out, float *obs_next,
                          float *dist_adj_next, float *channels_next, void *stream);

/* End of a chunk of rollout steps, in ONE launch: what the sampler loop does between two steps that a captured chunk
 * cannot leave to the host - `obses = next_obses` (centralized_ma_on_policy_vectorized_sampler.py:232): the slot the
 * last step wrote (src) becomes slot 0 (dst) for up to three buffers (observations, dist_adj, channels; bytes multiple
 * of 4, pointers 4-byte aligned, a NULL / 0-byte entry is skipped) - and the advance of the device-side Philox counter
 * base of the action sampler by n_steps.  Replaces two framework kernels + a blit per chunk (and the idle gaps
 * around them) by one kernel of this library. */
int cm_chunk_tail(uint32_t *policy_step_base, uint32_t n_steps, const void *src0, void *dst0, size_t bytes0,
                  const void *src1, void *dst1, size_t bytes1, const void *src2, void *dst2, size_t bytes2, void *stream);

/* Plain row-wise MLPs: the non-communicating policies and the Gaussian baseline of the reference's Obs-DP / CENT
 * runners.  Layer l:  y = x . wt[l] + b[l]  (wt TRANSPOSED [in,out] as above), followed by tanh
 * when bit l of tanh_mask is set, by ReLU (torch.relu: y < 0 ? 0 : y, NaN passes) when bit l of relu_mask is set
 * (hidden_nonlinearity=F.relu); a layer with both bits set is refused (CM_ERR_ARG).  First layer at most 128 outputs;
 * any layer at most 624: the two 32-row LDS tiles of max(128, width padded to 16) + 4 words a row must fit a workgroup's
 * 160 KB (2 * 32 * 628 * 4 = 160768 bytes; at 640 + 4 words they do not), and a wider layer is refused (CM_ERR_ARG). */
#define CM_MLP_MAX_LAYERS 6
typedef struct cm_mlp_weights {
    int32_t in_dim, n_layers;
    int32_t out_dim[CM_MLP_MAX_LAYERS];
    int32_t tanh_mask, relu_mask;
    const float *wt[CM_MLP_MAX_LAYERS];
    const float *b[CM_MLP_MAX_LAYERS];   /* NULL = no bias */
    const float *mfma_pack;              /* cm_mlp_pack() output (all layers, B fragments as in cm_policy_pack), or NULL:
                                            the kernel then gathers the plain weights (slower) */
} cm_mlp_weights;
size_t cm_mlp_pack_bytes(const cm_mlp_weights *w);
int cm_mlp_pack(const cm_mlp_weights *w, float *pack, void *stream);

/* DecCategoricalMLPPolicy.get_actions (com_marl/torch/policies/dec_categorical_mlp_policy.py:106-176; encoder 2
 * layers + head 2 layers = one 4-layer chain per AGENT row: rows = S*N, groups = 1) and
 * CentralizedCategoricalMLPPolicy.get_actions (centralized_categorical_mlp_policy.py:61-118; one chain per ENV row
 * with N*n_act logits: rows = S, groups = N).  x [rows,in_dim]; the last layer has groups*n_act outputs; per group:
 * softmax x avail ([rows,groups,n_act] or NULL = ones), renormalise, then argmax (greedy) or inverse-CDF sample on the
 * Philox stream (counter: env = env_id_offset + flat/agents_per_env, step, site 7, agent = flat % agents_per_env with
 * flat = row*groups + group - the same stream cm_policy_forward uses).
 *   out: actions int32 [rows,groups] (or NULL), probs [rows,groups,n_act] (or NULL). */
int cm_mlp_policy_forward(const cm_mlp_weights *w, int32_t rows, int32_t groups, int32_t n_act, int32_t agents_per_env,
                          const float *x, const float *avail, uint64_t seed, int32_t env_id_offset,
                          uint32_t policy_step, const uint32_t *policy_step_base, int32_t greedy, int32_t *actions,
                          float *probs, void *stream);
/* cm_mlp_policy_forward for SEVERAL policies of one shape in ONE launch, each on its own contiguous range of the envs: member k acts
 * on the group_sizes[k] envs behind those of members 0 .. k-1, i.e. on group_sizes[k] * agents_per_env / groups rows of x (agent
 * rows with groups == 1, env rows with groups == agents_per_env; nothing else is accepted).  Every output is bit-identical to
 * cm_mlp_policy_forward with member k's weights on its rows and env_id_offset + the group's first env (one seed for the set): a
 * member's rows end in a ragged 32-row workgroup of their own, never shared with the next member.
 *
 * cm_mlp_forward_multi_plan (host only, no device work): refuses (< 0, text in cm_last_error) an empty set, a group without envs,
 * sizes that do not sum to n_envs, members that differ in in_dim / n_layers / out_dim[] / tanh_mask / relu_mask, a shape
 * cm_mlp_policy_forward refuses (last layer != groups * n_act wide, ...) and an `image` that is too small.  Otherwise returns the
 * size in bytes of the table the launch reads and *n_wg = the launch's workgroup count, the sum over members of
 * ceil(rows / 32); with `image` non-NULL the table's host image is written there: n_wg cm_forward_set_wg descriptors, then
 * n_policies cm_mlp_set_member records.  The caller uploads the image to device memory it owns and rebuilds it when a member's
 * pack or weight buffers move or the groups change.  Returns 0 (*n_wg = 0, nothing written) when a member has no mfma_pack: the
 * set kernel has no plain-weight path, and the caller runs cm_mlp_policy_forward per member.
 *
 * cm_mlp_policy_forward_multi: the launch.  `shape` = any member's weights (dims and masks; its weight pointers are not read),
 * table_dev = the uploaded image, n_wg / n_envs / groups / n_act / agents_per_env = the planner's; every other argument is
 * cm_mlp_policy_forward's over the whole batch.  No allocation, copy or synchronisation: it can be captured in a hipGraph.  The
 * kernel trusts the table.  Returns 0 when launched, < 0 on a bad argument, and 1 - nothing launched - when `shape` has no
 * mfma_pack. */
typedef struct cm_mlp_set_member {       /* 4 * 4 + 2 * CM_MLP_MAX_LAYERS * 8 = 112 bytes */
    int32_t first_row, n_rows;           /* the member's rows of x */
    int32_t first_env, _pad;             /* its first env: first_row * groups == first_env * agents_per_env */
    const float *b[CM_MLP_MAX_LAYERS];   /* biases: in the member's flat weight copy; NULL = none / past n_layers */
    const float *pack[CM_MLP_MAX_LAYERS];/* each layer's B fragments inside the member's cm_mlp_pack output */
} cm_mlp_set_member;
int64_t cm_mlp_forward_multi_plan(const cm_mlp_weights *members, const int32_t *group_sizes /* envs */, int32_t n_policies,
                                  int32_t n_envs, int32_t groups, int32_t n_act, int32_t agents_per_env, void *image,
                                  size_t image_bytes, int32_t *n_wg);
int cm_mlp_policy_forward_multi(const cm_mlp_weights *shape, const void *table_dev, int32_t n_wg, int32_t n_envs,
                                int32_t groups, int32_t n_act, int32_t agents_per_env, const float *x, const float *avail,
                                uint64_t seed, int32_t env_id_offset, uint32_t policy_step, const uint32_t *policy_step_base,
                                int32_t greedy, int32_t *actions, float *probs, void *stream);
/* GaussianMLPBaseline.forward mean (com_marl/torch/baselines/gaussian_mlp_baseline.py:100-115): the last layer has
 * one output; values [rows]. */
int cm_mlp_value_forward(const cm_mlp_weights *w, int32_t rows, const float *x, float *values, void *stream);

/* Adjacency-masked aggregation, one GCN hop, for S samples (comm_base_net.py:101-105 +
 * graph_conv_module.py:63-70):  A = M*R*C; A /= rowsum+1e-12; out = tanh(A.(HW) + b).
 *   attn M [S,N,N]; dist_adj R [S,N,N] or NULL; channel C_l [S,N,N] with element stride
 *   ch_stride between samples (so a [S,L,N,N] tensor can be sliced) or NULL;
 *   hw [S,N,E]; bias [E] or NULL; out [S,N,E].  Saves nothing: backward recomputes A. */
int cm_masked_agg_forward(int32_t S, int32_t N, int32_t E, const float *attn, const float *dist_adj,
                          const float *chan, int64_t ch_stride, const float *hw, const float *bias, float *out,
                          void *stream);
/* grads of the op above: given out and d_out returns d_attn [S,N,N], d_hw [S,N,E], d_bias [E] (accumulated with
 * atomics; caller zeroes).  out_minus (or NULL): the op's output is out - out_minus (the caller holds x = E + H of
 * comm_base_net.py:107 and E: saves the subtraction pass). */
int cm_masked_agg_backward(int32_t S, int32_t N, int32_t E, const float *attn, const float *dist_adj,
                           const float *chan, int64_t ch_stride, const float *hw, const float *out, const float *out_minus,
                           const float *d_out, float *d_attn, float *d_hw, float *d_bias, void *stream);
/* The same with the bias gradient spread over `bias_replicas` >= 1 rows: d_bias [bias_replicas][E], zero on entry like every
 * accumulated gradient; a workgroup adds its column sums into ONE of the rows and the caller sums the rows.  (All workgroups adding
 * into one 256-byte row serialise in the L2: a third of the teams-of-4 kernel's time at a million agent rows.) */
int cm_masked_agg_backward_r(int32_t S, int32_t N, int32_t E, const float *attn, const float *dist_adj,
                             const float *chan, int64_t ch_stride, const float *hw, const float *out, const float *out_minus,
                             const float *d_out, float *d_attn, float *d_hw, float *d_bias, int32_t bias_replicas, void *stream);

/* Attention scores + softmax for the autograd path (attention_module.py:39-49):
 *   m[s,i,:] = softmax_j(q[s,i,:] . e[s,j,:]),  q = linear_in(e) [S,N,E], e [S,N,E], m [S,N,N].
 * backward: d_q, d_e [S,N,E] from d_m [S,N,N] (the d_e returned is only the key-side term) plus, when given, the
 * other gradients that flow into E: d_e = key-side term + d_e_add0 + d_e_add1 (each [S,N,E] or NULL; must not alias d_e). */
int cm_attention_forward(int32_t S, int32_t N, int32_t E, const float *q, const float *e, float *m, void *stream);
int cm_attention_backward(int32_t S, int32_t N, int32_t E, const float *q, const float *e, const float *m,
                          const float *d_m, const float *d_e_add0, const float *d_e_add1, float *d_q, float *d_e, void *stream);

/* The four graph ops above for ANY embedding width E in 1..128 (--embedding_dim; csrc/cm_graph_any.hip): the argument lists and
 * pointer semantics of their E = 64 namesakes (chan + ch_stride, out_minus, d_e_add0 / d_e_add1 and the aliasing refusal), the
 * same arithmetic.  d_bias [E] accumulates (one row: the caller zeroes it).  Return 1 - nothing launched, nothing written -
 * when the planes of one workgroup's envs do not fit 160 KB of LDS (N above 128, or e.g. N = 128 with E = 128): all of them
 * answer from the SAME test, so a shape whose forward runs has its backward.  E outside 1..128 is CM_ERR_ARG. */
int cm_masked_agg_forward_any(int32_t S, int32_t N, int32_t E, const float *attn, const float *dist_adj,
                              const float *chan, int64_t ch_stride, const float *hw, const float *bias, float *out,
                              void *stream);
int cm_masked_agg_backward_any(int32_t S, int32_t N, int32_t E, const float *attn, const float *dist_adj,
                               const float *chan, int64_t ch_stride, const float *hw, const float *out, const float *out_minus,
                               const float *d_out, float *d_attn, float *d_hw, float *d_bias, void *stream);
int cm_attention_forward_any(int32_t S, int32_t N, int32_t E, const float *q, const float *e, float *m, void *stream);
int cm_attention_backward_any(int32_t S, int32_t N, int32_t E, const float *q, const float *e, const float *m,
                              const float *d_m, const float *d_e_add0, const float *d_e_add1, float *d_q, float *d_e, void *stream);

/* Weight gradient of a per-agent dense layer over R rows: c[p][q] += sum_r a[r][p] * b[r][q] (c [P,Q] must be
 * zeroed by the caller; accumulated with float atomics), colsum_a[p] += sum_r a[r][p] (or NULL).
 * nn.Linear backward: a = dY [R,out], b = X [R,in] -> c = dW [out,in], colsum_a = db.
 * GraphConvolutionModule (H.W, graph_conv_module.py:63): a = H [R,in], b = dZ [R,out] -> c = dW [in,out].
 * Alignment: every pointer 4-byte aligned (any float *); 16-byte aligned a / b only select the faster (float4) loads. */
int cm_linear_wgrad(int64_t R, int32_t P, int32_t Q, const float *a, const float *b, float *c, float *colsum_a,
                    void *stream);

/* One dense per-agent layer of the PPO update, one HBM pass each way (csrc/cm_linear.hip).
 * w_layout 0: w is nn.Linear's [out,in] (multi_headed_mlp_module.py:134-149, attention_module.py:36);
 * w_layout 1: w is GraphConvolutionModule's [in,out] (graph_conv_module.py:63).  1 <= in, out <= 128.
 *   forward :  y[r][o] = act(bias[o] + sum_k x[r][k] w(k,o)),  act 0 = identity, 1 = tanh, 2 = ReLU (z < 0 ? 0 : z);
 *              any other act is refused (CM_ERR_ARG); bias may be NULL.
 *   backward:  dz = (dy + dy2) * (1 - y^2) when y != NULL (tanh layer), dz = dy + dy2 when y == NULL; dy2 [R,out] or NULL
 *              is a second gradient flowing into the same output (saves the caller's accumulation pass);
 *              dx[r][k] = sum_o dz[r][o] w(k,o)   (dx may be NULL: first layer);
 *              dw += dz^T.x in w's own layout and db += colsum(dz) (db may be NULL), float atomics:
 *              the caller zeroes dw / db.
 * Alignment: every pointer 4-byte aligned (any float *).  16-byte aligned x / dy / dy2 / y / dx only select the faster
 * path (float4 staging; the streaming kernels of csrc/cm_linear_bwd.hip): the results are the same to rounding. */
int cm_linear_act_forward(int64_t R, int32_t in_dim, int32_t out_dim, const float *x, const float *w, int32_t w_layout,
                          const float *bias, int32_t act, float *y, void *stream);
int cm_linear_act_backward(int64_t R, int32_t in_dim, int32_t out_dim, const float *x, const float *w, int32_t w_layout,
                           const float *dy, const float *dy2, const float *y, float *dx, float *dw, float *db, void *stream);
/* The same with the activation named: act 0 = identity (y unused, may be NULL), 1 = tanh (dz = (dy + dy2) * (1 - y^2)),
 * 2 = ReLU (dz = y > 0 ? dy + dy2 : 0, a select as torch's threshold_backward: an inf / NaN gradient into a dead unit
 * gives 0).  y is required when act != 0; any other act is refused (CM_ERR_ARG). */
int cm_linear_act_backward_ex(int64_t R, int32_t in_dim, int32_t out_dim, const float *x, const float *w, int32_t w_layout,
                              const float *dy, const float *dy2, const float *y, int32_t act, float *dx, float *dw, float *db,
                              void *stream);

/* Backward of the two-layer observation encoder (mlp_encoder_module: obs [R,d] -> a1 = tanh(W1 obs + b1) [R,128] ->
 * e = tanh(W2 a1 + b2) [R,64]; comm_base_net.py:80-84) in ONE pass over the saved activations: dz2 = (dy + dy2) * (1 - e^2),
 * dw2 += dz2^T a1, db2 += colsum(dz2); the gradient wrt a1 stays in the workgroup (times tanh' it overwrites the a1 tile) and
 * gives dw1 += dz1^T obs [128,d], db1 += colsum(dz1).  dy2 / db2 / db1 may be NULL; the caller zeroes dw* / db*.
 * Returns 1 - nothing done - when the shape is not covered (d > 64, tensors not 16-byte aligned): run the two layers with
 * cm_linear_act_backward instead. */
int cm_encoder_backward(int64_t R, int32_t d, const float *obs, const float *a1, const float *e, const float *w2, const float *dy,
                        const float *dy2, float *dw2, float *db2, float *dw1, float *db1, void *stream);

/* n tensors in one launch: src[k] is [rows[k], cols[k]] row-major f32; dst[k] receives its transpose ([cols, rows]) when
 * transpose[k] != 0, else a plain copy.  The veneer refreshes a net's flat [in,out] weight copy with it (one launch instead of
 * one framework copy per tensor).  n <= 40. */
int cm_multi_copy_t(int32_t n, const float *const *src, float *const *dst, const int32_t *rows, const int32_t *cols,
                    const int32_t *transpose, void *stream);
/* Multi-tensor Adam step with optional gradient-norm clip, two launches for a whole net (csrc/cm_optim.hip): the vendored
 * torch-1.9 Adam of the reference (com_marl/torch/algos/my_optimizer/_functional.py:72-98, no weight decay / amsgrad) preceded
 * - when norm_ws != NULL - by torch.nn.utils.clip_grad_norm_(params, max_norm) (centralized_ma_ppo.py:253-255), the clipped
 * gradient written back.  params / grads / exp_avg / exp_avg_sq: HOST arrays of n <= 40 DEVICE pointers, sizes[k] elements
 * each; norm_ws: DEVICE workspace of CM_ADAM_NORM_FLOATS floats, no initial contents required: [0] receives |g|^2 before
 * the clip, the rest holds per-workgroup partial sums added in index order - the norm, and with it the step, is
 * bit-reproducible (data-parallel replicas stay identical).  step = 1, 2, ... (bias correction). */
#define CM_ADAM_NORM_FLOATS 65
int cm_multi_adam_step(int32_t n, float *const *params, float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                       const int64_t *sizes, float *norm_ws, float max_norm, float lr, float beta1,
                       float beta2, float eps, int32_t step, void *stream);
/* The same step for a captured hipGraph that is replayed for SUCCESSIVE optimiser steps (the 10 mini-epochs over one minibatch,
 * centralized_ma_ppo.py:211-268, are the same launches on the same buffers): the bias-correction factors of step `first + *cursor`
 * are read from a DEVICE table [table_steps][2] = (1 - beta1^t, sqrt(1 - beta2^t)) indexed by the DEVICE counter `cursor` (the caller
 * advances it between steps; clamped to the table).  cm_adam_bias_corrections fills a HOST table with exactly the factors
 * cm_multi_adam_step computes for steps first_step .. first_step + n_steps - 1 (same f64 -> f32 arithmetic: the replayed steps
 * are bit-identical to eager ones). */
void cm_adam_bias_corrections(float beta1, float beta2, int32_t first_step, int32_t n_steps, float *table);
int cm_multi_adam_step_dev(int32_t n, float *const *params, float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                           const int64_t *sizes, float *norm_ws, float max_norm, float lr, float beta1, float beta2, float eps,
                           const float *bc_table, const int32_t *cursor, int32_t table_steps, void *stream);
/* cm_multi_adam_step_dev behind a DEVICE gate word (required; the KL early stop of cm_ppo_update_stats below writes it in the
 * launch before).  *gate == 0: cm_multi_adam_step_dev's step, bit for bit.  *gate != 0: the step is not taken - norm_ws[0] still
 * receives the pre-clip |g|^2, and parameters, moments and gradients (not clipped, not written back) stay untouched. */
int cm_multi_adam_step_gated(int32_t n, float *const *params, float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                             const int64_t *sizes, float *norm_ws, float max_norm, float lr, float beta1, float beta2, float eps,
                             const float *bc_table, const int32_t *cursor, int32_t table_steps, const int32_t *gate, void *stream);

/* The critic's loss (comm_base_critic.py:59-89: -Normal(values, std.mean()).log_prob(returns).mean(); values = the per-agent
 * outputs summed over the team, :110-112; std = exp(clamp(log_std, min)) of gaussian_mlp_module.py:62-188) in one launch, its
 * gradient in one more.  per_agent [S,N], returns [S], log_std: the DEVICE scalar parameter; has_min = 0 ignores min_log_std.
 *   forward : out[0] = loss, out[1] = mean_s (returns - values)^2 (read by the backward);  ws: CM_GAUSS_WS_BYTES of DEVICE memory,
 *             zero before the first use - the launch leaves it zero again (f64 sum of squares + a block counter)
 *   backward: d_per_agent [S,N] and d_log_std [1] (may be NULL), both times the DEVICE scalar *g (NULL = 1). */
#define CM_GAUSS_WS_BYTES 16
int cm_gauss_nll_forward(int64_t S, int32_t N, const float *per_agent, const float *returns, const float *log_std, float min_log_std,
                         int32_t has_min, float *out, void *ws, void *stream);
int cm_gauss_nll_backward(int64_t S, int32_t N, const float *per_agent, const float *returns, const float *log_std, float min_log_std,
                          int32_t has_min, const float *out, const float *g, float *d_per_agent, float *d_log_std, void *stream);

/* tensor_utils.discount_cumsum (garage/misc/tensor_utils.py:7-23) per path over a padded
 * [P,T] batch: f64 recurrence, f32 result, zero past lens[p]. */
int cm_discount_returns(int32_t P, int32_t T, const double *rewards, const int32_t *lens, double gamma,
                        float *returns, void *stream);
/* compute_advantages (garage/torch/algos/_utils.py:56-113) + per-path normalisation over the
 * valid steps (centralized_ma_ppo.py:422-426); normalize=0 skips the second part. */
int cm_gae(int32_t P, int32_t T, const float *rewards, const float *baselines, const int32_t *lens, float gamma,
           float lam, int32_t normalize, float eps, float *adv, void *stream);

/* PPO clipped-surrogate loss with entropy bonus over a padded [P,T] batch and its gradient wrt the policy logits
 * [P*T,N,A] (centralized_ma_ppo.py:390-438 _compute_loss, :540-589 _compute_objective; Categorical(probs=...) as built by
 * comm_categorical_mlp_policy.py:48-96, entropy / log_prob :121-137):
 *   *total = - sum over valid steps of [ min(r adv, clamp(r, 1 - clip, 1 + clip) adv) + ent_coeff * mean_i H_i ]   (f64)
 *   *count = number of valid steps (t < lens[p]);  dlogits (nullable) = d total / d logits, zero on padded steps.
 * add_entropy is a bit set (entropy_method == "regularized", centralized_ma_ppo.py:434-435 + :499-538):
 *   CM_ENT_ADD       (1)  add the entropy term; 0 drops it (entropy_method != "regularized")
 *   CM_ENT_SOFTPLUS  (2)  the term is ent_coeff * softplus(mean_i H_i) (use_softplus_entropy)
 *   CM_ENT_STOP_GRAD (4)  the term stays in *total but contributes nothing to dlogits (stop_entropy_gradient)
 * The values 0 and 1 are the kernel's original behaviour. */
#define CM_ENT_ADD 1
#define CM_ENT_SOFTPLUS 2
#define CM_ENT_STOP_GRAD 4
int cm_ppo_surrogate(int32_t P, int32_t T, int32_t N, int32_t A, const float *logits, const int32_t *actions,
                     const float *old_ll, const float *adv, const int32_t *lens, float clip, float ent_coeff,
                     int32_t add_entropy, double *total, int64_t *count, float *dlogits, void *stream);

/* entropy_method == "max" (centralized_ma_ppo.py:415-418 + :499-538): per step of a padded [P,T] batch
 *   H[p,t] = mean_i H(Categorical_i(logits[p*T+t, i, :]))  (padded steps included; same Categorical arithmetic as
 *            cm_ppo_surrogate), softplus(H) when softplus != 0,
 *   r'     = rewards + ent_coeff * H,
 *   adv    = compute_advantages(gamma, lam, r', baselines) over the padded length, no normalisation.
 * logits [P*T,N,A] (1 <= A <= 8), rewards / baselines / adv [P,T].  rewards_out (nullable, may alias rewards) receives r';
 * entropy_out (nullable) receives H [P,T] after the softplus.  T <= CM_ENT_GAE_MAX_T. */
#define CM_ENT_GAE_MAX_T 8192
int cm_entropy_gae(int32_t P, int32_t T, int32_t N, int32_t A, const float *logits, const float *rewards,
                   const float *baselines, float gamma, float lam, float ent_coeff, int32_t softplus, float *rewards_out,
                   float *entropy_out, float *adv, void *stream);

/* ---- Deterministic update mode (com_marl_amd.set_deterministic) ----
 * Twins of the entry points above whose cross-workgroup float sums would otherwise be merged with atomics (an order that
 * changes from run to run).  Each takes a slab workspace `ws` of DEVICE memory, at least cm_*_det_ws_bytes(shape) bytes,
 * contents ignored: every workgroup plain-stores its partial sums into its own row, and a second launch sums the rows in
 * index order.  The number of rows is fixed by the shape and the device's CU count, so two runs on the same GPU type
 * give bit-identical results.  Outputs accumulate like the originals' (zero them on entry).  A NULL or too-small `ws`
 * returns CM_ERR_ARG (text in cm_last_error) before anything is launched.  Concurrent launches need separate slabs. */
size_t cm_linear_act_backward_det_ws_bytes(int64_t R, int32_t K, int32_t O);
int cm_linear_act_backward_det(int64_t R, int32_t K, int32_t O, const float *x, const float *w, int32_t w_layout,
                               const float *dy, const float *dy2, const float *y, float *dx, float *dw, float *db,
                               void *ws, size_t ws_bytes, void *stream);
/* twin of cm_linear_act_backward_ex; the slab size is cm_linear_act_backward_det_ws_bytes(R, K, O) */
int cm_linear_act_backward_ex_det(int64_t R, int32_t K, int32_t O, const float *x, const float *w, int32_t w_layout,
                                  const float *dy, const float *dy2, const float *y, int32_t act, float *dx, float *dw, float *db,
                                  void *ws, size_t ws_bytes, void *stream);
/* db2 and db1 are required here; returns 1 (nothing launched) where cm_encoder_backward does */
size_t cm_encoder_backward_det_ws_bytes(int64_t R, int32_t d);
int cm_encoder_backward_det(int64_t R, int32_t d, const float *obs, const float *a1, const float *e, const float *w2, const float *dy,
                            const float *dy2, float *dw2, float *db2, float *dw1, float *db1, void *ws, size_t ws_bytes, void *stream);
/* d_bias [E] (one row: no replicas) */
size_t cm_masked_agg_backward_det_ws_bytes(int32_t S, int32_t N, int32_t E);
int cm_masked_agg_backward_det(int32_t S, int32_t N, int32_t E, const float *attn, const float *dist_adj,
                               const float *chan, int64_t ch_stride, const float *hw, const float *out, const float *out_minus,
                               const float *d_out, float *d_attn, float *d_hw, float *d_bias, void *ws, size_t ws_bytes, void *stream);
/* twin of cm_masked_agg_backward_any: one E-float row of d_bias per workgroup, summed in index order */
size_t cm_masked_agg_backward_any_det_ws_bytes(int32_t S, int32_t N, int32_t E);
int cm_masked_agg_backward_any_det(int32_t S, int32_t N, int32_t E, const float *attn, const float *dist_adj,
                                   const float *chan, int64_t ch_stride, const float *hw, const float *out, const float *out_minus,
                                   const float *d_out, float *d_attn, float *d_hw, float *d_bias, void *ws, size_t ws_bytes, void *stream);
size_t cm_linear_wgrad_det_ws_bytes(int64_t R, int32_t P, int32_t Q);
int cm_linear_wgrad_det(int64_t R, int32_t P, int32_t Q, const float *a, const float *b, float *c, float *colsum_a,
                        void *ws, size_t ws_bytes, void *stream);
/* *total: f64 block sums summed in a fixed order */
size_t cm_ppo_surrogate_det_ws_bytes(int32_t P, int32_t T);
int cm_ppo_surrogate_det(int32_t P, int32_t T, int32_t N, int32_t A, const float *logits, const int32_t *actions,
                         const float *old_ll, const float *adv, const int32_t *lens, float clip, float ent_coeff,
                         int32_t add_entropy, double *total, int64_t *count, float *dlogits, void *ws, size_t ws_bytes, void *stream);
/* the slab replaces cm_gauss_nll_forward's CM_GAUSS_WS_BYTES workspace (no zero state to keep) */
size_t cm_gauss_nll_forward_det_ws_bytes(int64_t S);
int cm_gauss_nll_forward_det(int64_t S, int32_t N, const float *per_agent, const float *returns, const float *log_std, float min_log_std,
                             int32_t has_min, float *out, void *ws, size_t ws_bytes, void *stream);

/* ---- Per-step PPO update statistics and the device-side KL early stop (csrc/cm_ppo_stats.hip, DESIGN.md "Update statistics") ----
 * One row of CM_UPD_COLS doubles per call, from cm_ppo_surrogate's inputs (padded [P,T] batch, logits [P*T,N,A], 1 <= A <= 8,
 * step (p,t) valid iff t < lens[p]).  Per valid step new_ll and H = mean_i H_i are cm_ppo_surrogate's Categorical arithmetic
 * (the same device function), lr = new_ll - old_ll is taken in f32 as the loss takes it, r = expf(lr) is the ratio the loss
 * clamps; the sums are f64:
 *   CM_UPD_N_VALID    number of valid steps
 *   CM_UPD_APPROX_KL  mean of expm1(lr) - lr        (the k3 estimator of KL(old || new), >= 0)
 *   CM_UPD_KL         mean of -lr                   (k1)
 *   CM_UPD_CLIP_FRAC  share of valid steps with |r - 1| > clip (f32 compare)
 *   CM_UPD_RATIO_MIN / CM_UPD_RATIO_MAX  range of r over the valid steps
 *   CM_UPD_ENTROPY    mean of H (no softplus)
 *   CM_UPD_STOPPED    1.0 if the optimiser step this row precedes is not to be applied, else 0.0
 * rows [max_rows][CM_UPD_COLS], row_cursor [1] (int32), gate [1] (int32, nullable): DEVICE memory.  The call writes
 * rows[clamp(*row_cursor, 0, max_rows - 1)], then *row_cursor += 1.  With was = gate ? *gate : 0,
 *   stop = was || (kl_stop > 0 && n_valid > 0 && approx_kl > kl_stop)
 * (kl_stop <= 0 or NaN never stops; no valid step gives a row of zeros and never stops) and *gate = stop when gate != NULL: the
 * gate is sticky until the host clears it.  cm_multi_adam_step_gated reads it.  ws: at least cm_ppo_update_stats_ws_bytes(P, T)
 * bytes of DEVICE memory, contents ignored (per-workgroup f64 partials, added in a fixed order by a second launch: no float
 * atomics, the row is bit-reproducible, so there is no deterministic twin).  Bad arguments, a NULL or too-small workspace
 * return CM_ERR_ARG before anything is launched. */
#define CM_UPD_COLS 8
#define CM_UPD_N_VALID 0
#define CM_UPD_APPROX_KL 1
#define CM_UPD_KL 2
#define CM_UPD_CLIP_FRAC 3
#define CM_UPD_RATIO_MIN 4
#define CM_UPD_RATIO_MAX 5
#define CM_UPD_ENTROPY 6
#define CM_UPD_STOPPED 7
size_t cm_ppo_update_stats_ws_bytes(int32_t P, int32_t T);
int cm_ppo_update_stats(int32_t P, int32_t T, int32_t N, int32_t A, const float *logits, const int32_t *actions,
                        const float *old_ll, const int32_t *lens, float clip, double kl_stop, double *rows, int32_t max_rows,
                        int32_t *row_cursor, int32_t *gate, void *ws, size_t ws_bytes, void *stream);

/* ---- Fixed-length rollout segments (csrc/cm_segments.hip, DESIGN.md "Rollout segments") ----
 * A batch of P fragments of T steps each, rolled without a reset in between.  None of the entry points below merges floats with
 * atomics: every sum has one order, fixed by the shape, so the bits repeat from run to run on one GPU type and there is no
 * deterministic twin.
 *
 * cm_segment_targets: advantages and critic targets in one launch.  rewards64 (f64) and dones (u8) are read in place: step t of
 * row p is element p * row_stride + t * step_stride of both (the engine's time-major [T,B] buffers: row_stride 1, step_stride B;
 * a [P,T] copy: T and 1).  baselines, adv, returns are [P,T] f32, v_last [P] is the critic's value of the observation after the
 * row's last step.  Per row, backwards, with cm_gae's and cm_discount_returns' arithmetic (f32 delta with gamma and lam rounded
 * to f32, f64 accumulator; f64 return recurrence with gamma as given):
 *   a set dones[t] clears the carried V_{t+1}, the accumulator and the running return before step t is processed (the episode
 *   ended with step t, whatever ended it - the time limit is a terminal state);
 *   at t = T-1 without a done, V_{t+1} = v_last[p] and the running return starts from (double)v_last[p].
 * A null pointer or T <= 0 returns CM_ERR_ARG before any launch. */
int cm_segment_targets(int32_t P, int32_t T, const double *rewards64, const uint8_t *dones, int64_t row_stride, int64_t step_stride,
                       const float *baselines, const float *v_last, double gamma, double lam, float *adv, float *returns,
                       void *stream);

/* Batch-wide advantage normalisation, in place: mean and biased variance over all `count` values in f64, two passes (the second
 * around the mean of the first), then adv = (adv - (float)mean) * (1 / sqrtf((float)var + eps)) - the expression cm_gae applies
 * per path.  ws: cm_adv_normalize_ws_bytes() bytes of DEVICE memory, contents ignored. */
size_t cm_adv_normalize_ws_bytes(void);
int cm_adv_normalize(int64_t count, float *adv, float eps, void *ws, size_t ws_bytes, void *stream);

/* Episode bookkeeping across segments.  One record per env, DEVICE memory the caller zeroes - with rec_f64's third plane at 1 -
 * when the envs are reset:
 *   rec_f64 [3][B]  undiscounted return so far, discounted return so far, gamma^length
 *   rec_i64 [6][B]  length, the sums of details columns 0..4
 * A call scans slots 0 .. n_steps-1 of reward_f64 [T,B], done [T,B] (u8), details [T,B,6] and success [T,B] per env, carries the
 * records on and writes table [CM_SEG_COLS]: the episodes that ended in these slots (done set), summed in a fixed order -
 *   CM_SEG_COUNT      their number
 *   CM_SEG_RET_SUM / _SUMSQ / _MIN / _MAX   of their undiscounted returns (no episode: 0, 0, +inf, -inf)
 *   CM_SEG_DISC_SUM   sum of their discounted returns (sum_k gamma^k r_k from the episode's first step)
 *   CM_SEG_LEN_SUM    sum of their lengths
 *   CM_SEG_SUCCESS    sum of success at their last step
 *   CM_SEG_DETAILS+k  sum of their details column k, k = 0..4 (raw counts)
 * ws: cm_segment_episodes_ws_bytes(B) bytes of DEVICE memory, contents ignored. */
#define CM_SEG_COLS 13
#define CM_SEG_COUNT 0
#define CM_SEG_RET_SUM 1
#define CM_SEG_RET_SUMSQ 2
#define CM_SEG_RET_MIN 3
#define CM_SEG_RET_MAX 4
#define CM_SEG_DISC_SUM 5
#define CM_SEG_LEN_SUM 6
#define CM_SEG_SUCCESS 7
#define CM_SEG_DETAILS 8
size_t cm_segment_episodes_ws_bytes(int32_t B);
int cm_segment_episodes(int32_t n_steps, int32_t B, const double *reward_f64, const uint8_t *done, const int32_t *details,
                        const int32_t *success, double gamma, double *rec_f64, int64_t *rec_i64, double *table, void *ws,
                        size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* COMMARL_H */
