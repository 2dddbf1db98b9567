// cm_env_pp10_dev.h - the env step of the carried headline rollout (rollout_w_kernel SHAPE 1: Predator-Prey on a 10 x 10 grid,
// 4 agents, 4 preys, sensing range 1, 21 observation entries) with the env state in registers from step to step.
// The generic bodies of cm_env_dev.h (env_body / pp_small_step / emit) stay the reference: this is the same step, order and
// Philox counters on another representation, and the parity tests compare the two bit for bit.
//
// Representation: a cell is one byte, (r + 1) * 16 + (c + 1): rows of 16 with a one-cell border on every side, so a target one
// step outside the grid is still a distinct byte (1 .. 186) that no entity can hold, and the four neighbours of a cell are the
// cell +-1 and +-16 without wrapping.  Every lane of an env's 16-lane group holds the whole env in three words:
//   apos  : the 4 agents' cells, byte i = agent i
//   ppos  : the 4 preys' cells, byte j = prey j (a dead prey keeps the cell it was captured on: the state write-back reports it)
//   flags : bits 0-3 prey j alive, bits 4-7 agent i's condition (predator_prey.py:257-261)
// "Is an agent on cell t" is one test of four bytes at once: some byte of apos ^ (t * 0x01010101) is zero.  The live-prey word
// replaces a dead prey's byte by 0xFF, a byte no query reaches.  Three words instead of two occupancy boards: they are carried
// through the policy forward, which already runs at the VGPR limit.  No occupancy tile, no LDS round trip inside the step;
// the tile of the env's LDS area is only used by an auto-reset (do_reset, rare), whose result the group reads back.
//
// Diagnostics: this body does not honour the early-return switch COMMARL_ENV_STOP > 0 (p.stop = 1..7) nor COMMARL_ENV_SMALL=0
// (p.no_small) of env_body - the carried map10 build always runs the whole step.  Its ENV_PROBE stamps (COMMARL_ENV_STOP=-1; they
// exist in rollout_w_probe_kernel only, every other build of this step sets p.stop = 0 at entry and they fold away) mark
// its own phases: p1 = p2 actions read, p3 agents, p8 prey trials, p4 (count, move) exchange and watch count, p5 prey moves,
// p6 reward and per-env stores, p7 reset, p9 emission and state write-back.
#pragma once
#include "cm_env_dev.h"

namespace cm {
namespace pp10 {

constexpr int S = 10, N = 4, M = 4, D = 21;
constexpr uint32_t ONES = 0x01010101u, HIGH = 0x80808080u, LOW7 = 0x7f7f7f7fu, SIXTEENS = 0x10101010u;

__device__ __forceinline__ uint32_t cell_of(int r, int c) { return (uint32_t)((r + 1) * 16 + c + 1); }
__device__ __forceinline__ int row_of(uint32_t ci) { return (int)(ci >> 4) - 1; }
__device__ __forceinline__ int col_of(uint32_t ci) { return (int)(ci & 15u) - 1; }
__device__ __forceinline__ uint32_t byte_at(uint32_t w, int i) { return (w >> (8 * i)) & 0xffu; }
__device__ __forceinline__ uint32_t set_byte(uint32_t w, int i, uint32_t v) { return (w & ~(0xffu << (8 * i))) | (v << (8 * i)); }
__device__ __forceinline__ uint32_t bcast(uint32_t t) { return t * ONES; }
// nonzero iff some byte of x is zero (exact as a test for ANY zero byte)
__device__ __forceinline__ uint32_t any0(uint32_t x) { return (x - ONES) & ~x & HIGH; }
// bit 7 of exactly the bytes of x that are zero
__device__ __forceinline__ uint32_t zero_bytes(uint32_t x) { return ~(((x & LOW7) + LOW7) | x | LOW7); }
__device__ __forceinline__ uint32_t delta_of(int a) { return (uint32_t)(16 * dr_of(a) + dc_of(a)); }
__device__ __forceinline__ int inside(uint32_t t) { return (((t >> 4) - 1u) < 10u) & (((t & 15u) - 1u) < 10u); }
// is `layer` (a word of four cells) free of cell t
__device__ __forceinline__ int lacks(uint32_t layer, uint32_t t) { return any0(layer ^ bcast(t)) == 0u; }
// the live-prey word: dead preys' bytes -> 0xFF
__device__ __forceinline__ uint32_t live_preys(uint32_t ppos, uint32_t flags) {
    uint32_t w = ppos;
#pragma unroll
    for (int j = 0; j < M; ++j) w |= ((flags >> j) & 1u) ? 0u : (0xffu << (8 * j));
    return w;
}
// entities of a layer at cell distance 1 from t (an entity matches at most one of the four neighbours, so the masks OR)
__device__ __forceinline__ int count_next(uint32_t layer, uint32_t t) {
    return __popc(zero_bytes(layer ^ bcast(t - 16u)) | zero_bytes(layer ^ bcast(t - 1u)) | zero_bytes(layer ^ bcast(t + 1u)) |
                  zero_bytes(layer ^ bcast(t + 16u)));
}
// the same for the agent layer from its four shifted copies (agents sit on 17..170: no byte carries), one broadcast per query
struct Shifted { uint32_t m16, m1, p1, p16; };
__device__ __forceinline__ int agents_next(const Shifted &a, uint32_t t) {
    const uint32_t bt = bcast(t);
    return __popc(zero_bytes(a.m16 ^ bt) | zero_bytes(a.m1 ^ bt) | zero_bytes(a.p1 ^ bt) | zero_bytes(a.p16 ^ bt));
}
__device__ __forceinline__ int no_agent_next(const Shifted &a, uint32_t t) {
    const uint32_t bt = bcast(t);
    return (any0(a.m16 ^ bt) | any0(a.m1 ^ bt) | any0(a.p1 ^ bt) | any0(a.p16 ^ bt)) == 0u;
}

struct State { uint32_t apos, ppos, flags; };
// what the next step needs besides the state (EnvPre's scalars).  The row / col tables share one register: lanes 16-31 of the
// wave hold the column entries, lanes 0-15 the row entries, so one wave-wide shuffle reaches either table.
struct Pre { uint32_t rng_step; int step_count_in, succ; float t_rc, t_step0, t_step; double t_rew; };

// Observation element u of a lane (k = 16u + lane < 84, agent i = k / 21, entry f = k % 21), decoded once per launch into 9 bits:
// bits 0-1 agent, bits 2-8 code: 0..34 agent-window cell (wr * 16 + wc = offset from the agent's cell + 17), + 64 for the prey
// window, 35 row, 36 col, 37 clock.  Elements 0-2 in one word, 3-5 in the other, 10 bits apart.
__device__ __forceinline__ uint32_t elem_code(int k) {
    const int i = k / D, f = k - D * i;
    int x;
    if (f < 18) { const int chn = f >= 9, w = f - 9 * chn, wr = w / 3, wc = w - 3 * wr; x = (wr * 16 + wc) | (chn << 6); }
    else x = 35 + (f - 18);
    return (uint32_t)(i | (x << 2));
}
struct Emit { uint32_t e0, e1; };
__device__ __forceinline__ Emit emit_codes(int sl) {
    Emit e{ 0u, 0u };
#pragma unroll
    for (int u = 0; u < 6; ++u) {
        const int k = min(16 * u + sl, N * D - 1);
        const uint32_t c = elem_code(k) << (10 * (u % 3));
        if (u < 3) e.e0 |= c; else e.e1 |= c;
    }
    return e;
}

// launch entry: the env's state from the global arrays (every lane reads all of it) and the scalars env_prefetch reads
__device__ __forceinline__ State load_state(const EnvDev &p, int b) {
    State s{ 0u, 0u, 0u };
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int2 q = p.agent_pos[(size_t)b * N + i];
        s.apos |= cell_of(q.x, q.y) << (8 * i);
        s.flags |= (p.agent_cond[(size_t)b * N + i] != 0 ? 16u : 0u) << i;
    }
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const int2 q = p.prey_pos[(size_t)b * M + j];
        s.ppos |= cell_of(q.x, q.y) << (8 * j);
        s.flags |= (p.alive[(size_t)b * M + j] != 0 ? 1u : 0u) << j;
    }
    return s;
}
__device__ __forceinline__ Pre load_pre(const EnvDev &p, int b, int sl, int tx) {
    Pre e;
    e.step_count_in = p.step_count[b];
    e.succ = p.success[b];
    e.rng_step = p.rng_step[b];
    const int s0 = sl < S ? sl : S - 1;
    e.t_rc = (tx & 16) ? p.lut_col[s0] : p.lut_row[s0];
    e.t_step0 = p.lut_step[0];
    e.t_rew = p.rew_lut[sl < (M + 1) + (N + 1) ? sl : 0];
    const int sc = e.step_count_in + 1;
    e.t_step = p.lut_step[sc <= p.max_steps ? sc : p.max_steps];
    return e;
}

// What the launcher (plan_rollout_w) has established for this build: every cm_step_out member stored below is non-null, and every
// trajectory buffer and state array stays below 2^31 bytes over the launch.  So the stores take the LAUNCH's base pointer as a
// scalar operand plus one 32-bit byte offset per lane (global saddr + voffset), and a step's slot is an element offset
// t * stride (StepOff, one scalar multiply per buffer) instead of a rebuilt 64-bit pointer.
struct StepOff { uint32_t obs, reward, reward_f64, done, details, prey_alive, success, path_len; };
template <class T>
__device__ __forceinline__ T *at32(T *base, uint32_t elem) { return reinterpret_cast<T *>(reinterpret_cast<char *>(base) + (uint32_t)(elem * (uint32_t)sizeof(T))); }

// the env's record in the global state arrays (lane j < 4: agent j, prey j; lane 0: the per-env scalars)
__device__ __forceinline__ void write_back(const EnvDev &p, uint32_t b, int sl, uint32_t apos, uint32_t ppos, uint32_t flags, int step_count,
                                           int succ, uint32_t rng_step) {
    if (sl == 0) {
        *at32(p.rng_step, b) = rng_step;
        *at32(p.step_count, b) = step_count;
        *at32(p.success, b) = succ;
    }
    if (sl < M) {
        const uint32_t ca = byte_at(apos, sl), cp = byte_at(ppos, sl);
        *at32(p.agent_pos, b * N + sl) = make_int2(row_of(ca), col_of(ca));
        *at32(p.prey_pos, b * M + sl) = make_int2(row_of(cp), col_of(cp));
        *at32(p.alive, b * M + sl) = (uint8_t)((flags >> sl) & 1u);
    }
}

// The draw stage of the carried map-10 step loop.  A step's common path needs 16 action words (site 7: env, policy step, agent)
// and 16 prey trial blocks (site 2: env, rng_step, 2 * prey) per wave, and none of their counters depends on anything a step
// computes (rng_step advances by one per step, reset or not): one 64-lane Philox4x32-10 call therefore serves TWO steps.  The wave
// runs it on every even step of the loop (paired by the loop index, so a chunk draws the same whatever base it starts at) -
//   lane >> 5 : step t / t + 1     (lane >> 4) & 1 : action / prey     lane & 15 : policy row c (env c >> 2, agent c & 3) resp.
//   (env idx >> 2, prey idx & 3)
// - and each lane leaves its four words in the wave's LDS buffer (`buf`: byte offset, 64 x 16 bytes, this wave's only).  LDS is in
// order per wave: the readers (policy_tile_w: word x of an action entry; step below: a prey entry) need no barrier.  Same counters,
// same keys, same words as the per-step calls of the generic builds.  `rng_step`: the lane's group's, at step t.  `act_step`: the
// sampler's Philox step of step t.  Idle groups of a ragged workgroup draw for env B - 1, as their step shadows it.
// The rounds are written out here instead of calling philox4x32_10: an instance of its own (see Frags::fetch).
__device__ __forceinline__ void draw_stage(const EnvDev &p, uint32_t rng_step, int32_t act_gid0, uint32_t act_step, uint32_t act_k0,
                                           uint32_t act_k1, int envs, bool all_valid, int buf) {
    const int tx = thread_x(), lane = tx & (WAVE - 1), idx = lane & 15;
    const bool prey = (lane & 16) != 0;
    const uint32_t half = (uint32_t)(lane >> 5);
    const int tgt = (tx >> 6) * 4 + (idx >> 2);                          // the entry's env inside the workgroup
    const int b_raw = blockIdx.x * 16 + tgt;
    const bool valid = all_valid || (tgt < envs && b_raw < p.B);
    const int b = valid ? b_raw : p.B - 1;
    const uint32_t rs = (uint32_t)__shfl((int)rng_step, (idx >> 2) * 16, WAVE);
    uint32_t c0 = prey ? (uint32_t)(p.env_id_offset + b) : (uint32_t)(act_gid0 + b_raw);
    uint32_t c1 = (prey ? rs : act_step) + half;
    uint32_t c2 = prey ? (uint32_t)SITE_PREY : (uint32_t)SITE_ACTION;
    uint32_t c3 = prey ? 2u * (uint32_t)(idx & 3) : (uint32_t)(idx & 3);
    uint32_t k0 = prey ? p.key0 : act_k0, k1 = prey ? p.key1 : act_k1;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    *reinterpret_cast<uint4 *>(smem + buf + 16 * lane) = make_uint4(c0, c1, c2, c3);
}

// One env step of a 16-lane group: env_stage + env_body + env_pre_carry of the generic carried form.  `act_off`: byte offset of
// the group's four action words in LDS; `obs_copy`: byte offset of the env's LDS observation copy.  Updates `st` and `pre`.
// `draw`: byte offset in LDS of the wave's 16 prey entries of this step (draw_stage), 16 bytes apart.
// `out`: the launch's bases, `off`: this step's element offsets into them.  `last`: the launch's last step - the only one whose
// state write-back anything reads (no load of the launch reads the state arrays: the next launch and the host see what the last
// step left), so the others keep the state in registers only.
// `ahead`: called once, every lane of the wave active, behind the emission's last scalar load and in front of its stores - what the
// caller wants requested from LDS for the next step (a scalar load's lgkmcnt(0) behind it would drain the request at once).
// Reference lines as in env_body / pp_small_step.
template <class AHEAD>
__device__ __forceinline__ void step(const EnvDev &p, State &st, Pre &pre, const Emit em, int act_off, const cm_step_out &out,
                                     const StepOff &off, bool last, int grp, int b_raw, bool grp_live, int lds_base, bool all_valid,
                                     int obs_copy, int draw, AHEAD ahead) {
    Grp<16> g;
    const int tx = thread_x();
    g.sub = (tx & (WAVE - 1)) / 16; g.sl = tx % 16;
    const int sl = g.sl;
    ENV_PROBE(0);
    const bool valid = all_valid || (grp_live && b_raw < p.B);
    const int b = valid ? b_raw : p.B - 1;             // idle groups shadow the last env and never commit
    const Rng rng{ (uint32_t)(p.env_id_offset + b), pre.rng_step, p.key0, p.key1 };
    const bool mine = sl < M;                          // lane j < 4: prey j's move, agent j's watch test and write-back
    // the prey's first four trial words come from the draw stage's buffer: requested first.  Lane sl of a group runs trial sl >> 2
    // of prey sl & 3 (16 lanes, 16 (prey, trial) pairs): word sl >> 2 of the prey's entry, one 4-byte read
    const uint32_t xw = *reinterpret_cast<const uint32_t *>(smem + draw + 16 * (4 * g.sub + (sl & 3)) + 4 * (sl >> 2));
    const int4 araw = *reinterpret_cast<const int4 *>(smem + act_off);
    const int ain[4] = { araw.x, araw.y, araw.z, araw.w };
    int act[4], bad = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int a = ain[i];
        const int bi = (unsigned)a > 4u;
        bad |= bi;
        const int faulty = ((st.flags >> (4 + i)) & 1u) == 0u;          // pseudo-action 5, as env_stage encodes it
        act[i] = bi ? 4 : ((faulty & (a != 4)) ? 5 : a);
    }
    if (bad && valid) {
        if (sl == 0) raise(p, CM_ERR_ACTION);                           // the reference raises (predator_prey.py:255)
        // a step that does not commit stores no state, so memory keeps the record of the step before it.  With the write-back
        // deferred to the launch's last step that record may never have been stored: stored here, from the registers the step
        // came in with.  (Not reached in this kernel: the action words were written 0..4 by the sampler of the same step.)
        write_back(p, (uint32_t)b, sl, st.apos, st.ppos, st.flags, pre.step_count_in, pre.succ, pre.rng_step);
    }
    const bool commit = valid && !bad;
    ENV_PROBE(1);
    ENV_PROBE(2);                                      // no tile to build: p2 = p1

    // ---- agents move in index order (predator_prey.py:497-500, :240-261): the target must be inside the grid and hold no
    // agent (earlier agents at their new cells) and no live prey.  Pseudo-action 5: target = own cell, which agent i holds ----
    uint32_t apos = st.apos, ppos = st.ppos, flags = st.flags;
    uint32_t plive = live_preys(ppos, flags);
    int moving = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int a = act[i];
        const int active = a != 4;
        moving += active;
        const uint32_t t = byte_at(apos, i) + delta_of(a);
        const int ok = active & inside(t) & lacks(apos, t) & lacks(plive, t);
        apos = ok ? set_byte(apos, i, t) : apos;
    }
    ENV_PROBE(3);
    // ---- per-prey work against the (now static) agent layer: one lane per prey (:396-407) ----
    const Shifted ag{ apos - SIXTEENS, apos - ONES, apos + ONES, apos + SIXTEENS };
    int pk;
    {
        const uint32_t my = byte_at(ppos, sl & 3);
        const int my_alive = mine & (int)((flags >> (sl & 3)) & 1u);
        const int cnt = my_alive ? agents_next(ag, my) : 0;
        // first of <= 5 draws whose target has no predator neighbour.  A trial's test depends on no other trial, only "the first
        // that passes" orders them: this lane's trial as a 3-bit code (its move, 7 = failed), and lane j takes the codes of
        // lanes j + 4, j + 8, j + 12 of its row by row-shift DPP moves (a wave's rows of 16 are the groups, and the whole wave
        // is active here; the old value 7 stands where a shift reaches past the row: lanes >= 4, which discard it)
        const int m0 = prey_move_from_u32(xw);
        const int c0 = no_agent_next(ag, my + delta_of(m0)) ? m0 : 7;
        const int c1 = __builtin_amdgcn_update_dpp(7, c0, 0x104, 0xf, 0xf, false);   // row_shl:4
        const int c2 = __builtin_amdgcn_update_dpp(7, c0, 0x108, 0xf, 0xf, false);   // row_shl:8
        const int c3 = __builtin_amdgcn_update_dpp(7, c0, 0x10c, 0xf, 0xf, false);   // row_shl:12
        const int first = c0 != 7 ? c0 : (c1 != 7 ? c1 : (c2 != 7 ? c2 : c3));
        const int none = (my_alive ^ 1) | ((p.load == 2) & (cnt >= 2));  // dead, or captured this step: no trial
        int mv = (none | (first == 7)) ? 4 : first;
        const int found = none | (first != 7);
        if (!found) {                                  // fifth draw: second Philox call, rare
            const u32x4 x1 = rng.at(SITE_PREY, (uint32_t)(2 * sl + 1));
            const int m = prey_move_from_u32(x1.x);
            mv = no_agent_next(ag, my + delta_of(m)) ? m : mv;
        }
        pk = cnt | (mv << 3);
    }
    ENV_PROBE(8);
    // prey_watching (:419-423): agents 4-adjacent to a live prey (prey layer at start-of-phase positions)
    const int wsum = g.count(mine && count_next(plive, byte_at(apos, sl & 3)) != 0);
    int pks[M];                                        // every lane: prey j's (count, move), from lane j
#pragma unroll
    for (int j = 0; j < M; ++j) pks[j] = __shfl(pk, j, 16);
    ENV_PROBE(4);
    // ---- captures + prey moves in index order (:416-432 / :460-478, :276-301) ----
    int capture = 0, penalty = 0, alive_any = 0;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const uint32_t c = byte_at(ppos, j);
        const int alive = (int)((flags >> j) & 1u), cnt = pks[j] & 7, mv = pks[j] >> 3;
        int need = p.load;
        if (p.load != 2) {                                                       // reward_individual :467-470 (uniform branch)
            const uint32_t rf = c >> 4, cf = c & 15u;
            const int on_r = (rf == 1u) | (rf == (uint32_t)S), on_c = (cf == 1u) | (cf == (uint32_t)S);
            const int adj = (on_r & on_c) ? 2 : ((on_r | on_c) ? 3 : p.load);    // __create_edges :123-144
            const int avail = adj - count_next(plive, c);
            need = p.load < avail ? p.load : avail;
        }
        const int hit = alive & (cnt >= 1), captured = hit & (need <= cnt);
        capture += captured; penalty += hit & (captured ^ 1);
        const int stays = alive & (captured ^ 1);                                // :301 otherwise
        const uint32_t t = c + delta_of(mv);
        const int ok = stays & (mv != 4) & inside(t) & lacks(apos, t) & lacks(plive, t);
        ppos = ok ? set_byte(ppos, j, t) : ppos;
        plive = stays ? (ok ? set_byte(plive, j, t) : plive) : (plive | (0xffu << (8 * j)));
        flags = stays ? flags : (flags & ~(1u << j));
        alive_any |= stays;
    }
    ENV_PROBE(5);
    // reward in f64 exactly as the Python expression evaluates (:434 / :480), from the host tables (as env_body)
    double reward = __shfl(pre.t_rew, capture, 16) + __shfl(pre.t_rew, (M + 1) + moving, 16);
    if (p.load == 2) reward = reward + p.penalty * (double)penalty;
    const cm_step_out &o = out;
    const uint32_t ub = (uint32_t)b;
    if (commit && mine) *at32(o.prey_alive, off.prey_alive + ub * M + sl) = (uint8_t)((flags >> sl) & 1u);
    int step_count = pre.step_count_in + 1, succ = pre.succ;
    int done = (step_count >= p.max_steps) || !alive_any;                       // :511-517
    if (done) succ = alive_any ? 0 : 1;
    if (step_count >= p.mpl) done = 1;                                           // vec_env_executor.py:33-34
    if (sl == 0 && commit) {
        *at32(o.reward, off.reward + ub) = (float)reward;
        *at32(o.reward_f64, off.reward_f64 + ub) = reward;
        *at32(o.done, off.done + ub) = (uint8_t)done;
        *at32(o.path_len, off.path_len + ub) = done ? step_count : 0;
        int2 *dd = reinterpret_cast<int2 *>(at32(o.details, off.details + ub * 6));   // 24-byte rows: three 8-byte stores
        dd[0] = make_int2(capture, moving); dd[1] = make_int2(penalty, 0); dd[2] = make_int2(wsum, 0);
    }
    ENV_PROBE(6);
    // auto-reset (:36-43): rare, so it keeps the tile-based spawn of the generic body.  A resetting group's do_reset clears its
    // tile, spawns against it and leaves the positions in the LDS arrays, which the group reads back.  do_reset's loop is
    // wave-wide: the wave enters it if any of its groups resets.
    if (__any(done)) {
        const Lds l = make_lds(S, N, M, lds_base + p.lds_env * grp, p.status);
        do_reset<CM_PP, 16>(p, l, rng, cm_rng_tape{}, b, g, done != 0);
        if (done) {
            uint32_t a = 0u, q = 0u;
#pragma unroll
            for (int i = 0; i < N; ++i) { a |= cell_of(AR(l, i), AC(l, i)) << (8 * i); q |= cell_of(PR(l, i), PC(l, i)) << (8 * i); }
            apos = a; ppos = q;
            flags |= 0x0fu;
        }
    }
    if (done) step_count = 0;
    ENV_PROBE(7);
    const float t_clock = done ? pre.t_step0 : pre.t_step;
    // ---- emission (get_neighbors, predator_prey.py:173-181; row / col / clock :195-196): a window entry is a presence test of
    // one cell on the agent or live-prey word; same global stores and LDS copy as emit<CM_PP, 16>.  The values are formed here,
    // with every lane of the wave active: the table shuffle reads lanes 0-31 of the wave (groups 0 and 1), and a bpermute from a
    // lane that has left (an idle group of a ragged batch, a group whose step did not commit) would return 0.  Only the stores
    // below wait for `commit`. ----
    plive = live_preys(ppos, flags);
    float vv[6];
    int ci_copy[6];
#pragma unroll
    for (int u = 0; u < 6; ++u) {
        const uint32_t code = ((u < 3 ? em.e0 : em.e1) >> (10 * (u % 3))) & 0x1ffu;
        const uint32_t i = code & 3u, x = code >> 2, w = x & 63u;
        const uint32_t ci = (apos >> (8u * i)) & 0xffu;
        const uint32_t t = ci + w - 17u;
        const int hit = !lacks((x & 64u) ? plive : apos, t);
        const float tab = __shfl(pre.t_rc, x == 36u ? 16 + col_of(ci) : row_of(ci), 64);
        vv[u] = w < 35u ? (hit ? 1.0f : 0.0f) : (x == 37u ? t_clock : tab);
        ci_copy[u] = 16 * u + sl + 3 * (int)i;         // row i * OBS_COPY_STRIDE + entry f, f = k - 21 i
    }
    // the next step's record (env_pre_carry): positions always; step count, success and the agent conditions re-armed by the
    // reset only when the step committed, as the generic carried form leaves them
    st.apos = apos; st.ppos = ppos; st.flags = (commit && done) ? (flags | 0xf0u) : flags;
    pre.rng_step += 1u;
    if (commit) { pre.step_count_in = step_count; pre.succ = succ; }
    {
        const int sc = pre.step_count_in + 1;
        pre.t_step = p.lut_step[sc <= p.max_steps ? sc : p.max_steps];
    }
    if (sl == 0 && commit) *at32(o.success, off.success + ub) = succ;
    ahead();
    if (!commit) return;
    const uint32_t ob = off.obs + ub * (N * D) + (uint32_t)sl;
    float *oc = reinterpret_cast<float *>(smem + obs_copy);
#pragma unroll
    for (int u = 0; u < 6; ++u) {
        if (16 * u + sl < N * D) {
            *at32(o.obs, ob + 16u * u) = vv[u];
            oc[ci_copy[u]] = vv[u];
        }
    }
    static_assert(OBS_COPY_STRIDE == D + 3, "the copy index k + 3i assumes rows of 24 floats");
    // ---- state write-back: the launch's last step only ----
    if (last) write_back(p, ub, sl, apos, ppos, flags, step_count, succ, rng.step + 1);
    ENV_PROBE(9);
}

}  // namespace pp10
}  // namespace cm
