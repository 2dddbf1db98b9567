// cm_rollout_w_body.h - the BODY of the wave-owned rollout kernels (no include guard: it is included inside a kernel's braces).
// The including kernel provides the template parameters <int LHOPS, bool PRE, bool FULLWG, bool TAPE, bool CARRY, int SHAPE> and
// the locals  mf::FwdArgs a, mw::WeightsW w, EnvDev p, cm_rng_tape tape_arg, cm_step_out out, StridesW c, TailW tl  (a and p are
// modified) and  constexpr bool PROBES  (whether the diagnostic clocks of COMMARL_ENV_STOP < 0 exist in this build: always in the
// generic builds, where they are gated at run time; in the SHAPE 1 builds only in the probe entry).  A textual include rather than an inlined device function: it leaves rollout_w_kernel's code exactly what it was
// when the loop was written in place (an inlined call reorders the IR enough to move the register allocation).
// CARRY (PRE builds, constant adjacency, no channel model, no tape): a wave's envs hand observation and state from step to step
// through LDS and registers (EnvCarry, env_pre_carry, the observation copy in the env area's unused claim table); no load of a
// step depends on a store of the launch, so the fence between two steps goes and the trajectory stores of step t drain under
// the policy forward of step t + 1.
// SHAPE 1 (carried builds): the grid of BASELINE config 2 - 10 x 10 cells, 4 preys, sensing range 1 (3 x 3 window, 21 observation
// entries) - as compile-time constants: index divisions by constants, constant LDS offsets, unrolled element loops; and what else
// plan_rollout_w has established for it: five actions, no avail mask, sampling (not greedy), every output the engine passes by
// default present, every trajectory buffer below 2^31 bytes.  The sampling tail is straight-line code, a step's slot in a
// buffer is a 32-bit element offset from the launch's base (no per-step pointer rebuild, no null test at a store), and the
// state arrays are written by the launch's last step only.  The step's common Philox draws (the sampler's action word, the preys'
// first four trial words) are computed for two steps at once on every even step of the loop (pp10::draw_stage) and handed over
// through a per-wave LDS buffer in the image's h3 / h4 slots, which these builds do not stage.  The first encoder layer's fragments and
// biases of step t + 1 are requested in the env phase of step t (mw::E1Ahead; step 0's behind the staging barrier, the last step's are
// discarded): at the top of a step nothing runs that could cover their 24 LDS reads.
// constexpr bool COND (true in cm_rollout_wc.hip only; the non-carried, tape-less builds: a handle with a condition table has adj_const off): the including
// kernel also provides  const EnvCondDev *cond  - the handle's device table (cm_env_set_conditions).  A 16-lane env group loads its
// env's record ONCE, ahead of the step loop (the table cannot change under a running launch), and its env phase runs on a
// by-value copy of p that carries the record's rc2, ploss, pgb, pbg and Philox env id (apply_cond, cm_env_dev.h): five VGPRs
// per lane, everything else of p stays the scalar argument.  The policy tile is untouched.  The other kernels set COND to false
// and cond to a constant nullptr: everything of it is behind `if constexpr`.
    static_assert(!COND || (!CARRY && !TAPE && SHAPE == 0), "the conditions twins are the non-carried, tape-less builds");
    static_assert(SHAPE == 0 || CARRY, "shape constants are built into the carried form only");
    if constexpr (SHAPE == 1) {
        p.S = 10; p.M = 4; p.R = 1; p.W = 3; p.d = 21; p.rcp_d = 1.0f / 21.0f; p.rcp_W = 1.0f / 3.0f; p.rcp_WW = 1.0f / 9.0f;
        p.lds_env = lds_env_bytes(10, 4, 4);
        a.N = 4; a.d = 21; a.L = LHOPS;
        a.avail = nullptr; a.greedy = 0; a.adj = nullptr; a.chan = nullptr; a.probe = nullptr;
        __builtin_assume(a.actions != nullptr); __builtin_assume(a.probs != nullptr); __builtin_assume(a.attn != nullptr);
        if constexpr (!PROBES) p.stop = 0;                               // ENV_PROBE folds away
        // the sampler's Philox base is constant for the launch (the folded tail advances it behind every wave's last read): once, here
        a.policy_step += a.step_base ? *a.step_base : 0u;
        a.step_base = nullptr;
    }
    const int n_act = SHAPE == 1 ? 5 : w.n_act;
    static_assert(!CARRY || (PRE && !TAPE), "the carried form is the prefetching, tape-less build");
    const cm_rng_tape tape = TAPE ? tape_arg : cm_rng_tape{};
    // what the launcher has already established, as compile-time constants of the by-value config: the branches on them fold away
    if constexpr (!TAPE) p.rng_mode = CM_RNG_PHILOX;                     // no tape pointers
    p.scen = CM_PP; p.N = 4; p.lpe = 16; p.rcp_N = 0.25f; p.rcp_NN = 0.0625f;
    if constexpr (CARRY) { p.adj_const = 1; p.ch_const = 1; p.channel = CM_CH_FC; }   // constant adjacency, no channel model
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_w[];
    constexpr int LPE = 16;
    constexpr int ACT_OFF = mw::pack_w(LHOPS).lds_u4 * 16, ENV_BASE = ACT_OFF + mw::WG_ROWS * 4;
    constexpr int DRAW_OFF = mw::draw_lds_off(LHOPS);                    // SHAPE 1: the draw buffers, in the image's unstaged h3 / h4 slots
    int32_t *act = reinterpret_cast<int32_t *>(lds_w + ACT_OFF);
    const bool probe = PROBES && p.stop == -2 && blockIdx.x == 0 && thread_x() == 0;
    const unsigned long long t_in = probe ? __builtin_amdgcn_s_memtime() : 0ull;
    mw::stage_w<LHOPS, SHAPE == 1>(w, lds_w, thread_x());
    mw::ResidentW<SHAPE == 1> res;
    res.template fetch<LHOPS>(w, thread_x() & 63);
    __syncthreads();                                                     // the only workgroup barrier of the launch
    if (probe) { g_w_probe[3] = __builtin_amdgcn_s_memtime() - t_in; g_w_probe[0] = g_w_probe[1] = g_w_probe[2] = g_w_probe[4] = 0; }
    const int envs = FULLWG ? mw::WG_ENVS : min(mw::WG_ENVS, a.S - (int)blockIdx.x * mw::WG_ENVS);
    mw::E1Ahead<SHAPE == 1> e1a;                                         // SHAPE 1: step t + 1's first-layer reads, requested in step t
    if constexpr (SHAPE == 1) { e1a.template init<LHOPS>(lds_w, thread_x() & 63); e1a.template fetch<LHOPS>(); }
    EnvPre pre{};
    pp10::State st{};                                                    // SHAPE 1: the env in registers (cm_env_pp10_dev.h)
    pp10::Pre pp{};
    pp10::Emit em{};
    int obs_row = 0, obs_env = -1;                                       // LDS copy: this lane's row (policy) / this group's env (emission)
    if constexpr (CARRY) {
        const int tx = thread_x(), grp = tx / LPE, lane = tx & 63, cc = lane & 15;
        const bool live = FULLWG || grp < envs;
        const Lds l0 = make_lds(p.S, p.N, p.M, ENV_BASE + p.lds_env * grp, p.status);
        obs_env = l0.win;                                                // teams of 4 never run agents_parallel: its claim table is free
        const int env_l = (tx >> 6) * 4 + (cc >> 2);                     // env of the policy's row c
        obs_row = make_lds(p.S, p.N, p.M, ENV_BASE + p.lds_env * env_l, p.status).win + (cc & 3) * OBS_COPY_STRIDE * 4;
        // step 0: the observation of slot 0 into the copy (rows of this group's env; zeros behind the d entries), the env
        // state from the global arrays - the only loads of the launch that read what an earlier launch wrote
        float *oc = reinterpret_cast<float *>(lds_w + obs_env);
        const int b0 = blockIdx.x * mw::WG_ENVS + (live ? grp : 0);
        const bool ok = live && b0 < a.S;
        for (int k = tx % LPE; k < 4 * OBS_COPY_STRIDE; k += LPE) {
            const int i = k / OBS_COPY_STRIDE, f = k - i * OBS_COPY_STRIDE;
            oc[k] = (ok && f < a.d) ? a.obs[((size_t)b0 * 4 + i) * a.d + f] : 0.0f;
        }
        if constexpr (SHAPE == 1) {                                      // the state as three words per lane from here on
            const int b = (live && b0 < p.B) ? b0 : p.B - 1;             // as env_prefetch
            st = pp10::load_state(p, b);
            pp = pp10::load_pre(p, b, tx % LPE, tx);
            em = pp10::emit_codes(tx % LPE);
        } else pre = env_prefetch<CM_PP, LPE>(p, b0, live);
    }
    EnvCondVals cv{};                                                    // COND: this group's record, for the whole launch
    if constexpr (COND) {
        const int grp = thread_x() / LPE;
        const int b0 = blockIdx.x * mw::WG_ENVS + ((FULLWG || grp < envs) ? grp : 0);
        cv = load_cond(cond, ((FULLWG || grp < envs) && b0 < p.B) ? b0 : p.B - 1);   // idle groups shadow env B - 1, as env_body
    }
    for (int t = 0; t < c.n_steps; ++t) {
        asm volatile("" ::: "memory");                                   // keep each step's loads inside the step
        const int tx = thread_x(), grp = tx / LPE;
        const bool live = FULLWG || grp < envs;
        bool env_wave = FULLWG || (tx & ~63) / LPE < envs;              // a wave with an env of its own
        // SHAPE 1: as a scalar, so that the env phase and the idle wave's request below are two branches and not two masked passes
        if constexpr (SHAPE == 1 && !FULLWG) env_wave = __builtin_amdgcn_readfirstlane(tx >> 6) * (64 / LPE) < envs;
        const int b_raw = blockIdx.x * mw::WG_ENVS + (live ? grp : 0);
        mf::FwdArgs at = a;
        at.policy_step = a.policy_step + (uint32_t)t;
        const uint32_t ut = (uint32_t)t;
        if constexpr (SHAPE != 1) {
        at.obs = a.obs + (size_t)t * c.obs;
        at.adj = a.adj ? a.adj + (size_t)t * c.dist_adj : nullptr;
        at.chan = a.chan ? a.chan + (size_t)t * c.channels : nullptr;
        at.actions = a.actions ? a.actions + (size_t)t * c.actions : nullptr;
        at.probs = a.probs ? a.probs + (size_t)t * c.probs : nullptr;
        at.attn = a.attn ? a.attn + (size_t)t * c.attn : nullptr;
        }
        const unsigned long long t0 = probe ? __builtin_amdgcn_s_memtime() : 0ull;
        // SHAPE 1: the Philox words of steps t and t + 1, on even t (pp10::draw_stage); entry 32 h + 16 k + i of the wave's buffer
        const int draw = DRAW_OFF + __builtin_amdgcn_readfirstlane(tx >> 6) * mw::DRAW_WAVE_BYTES + (t & 1) * (mw::DRAW_WAVE_BYTES / 2);   // wave-uniform: a scalar
        if constexpr (SHAPE == 1) {
            if ((t & 1) == 0) pp10::draw_stage(p, pp.rng_step, a.env_id_offset, at.policy_step, a.key0, a.key1, envs, FULLWG, draw);
            asm volatile("" ::: "memory");
        }
        if constexpr (COND) { if constexpr (PRE) pre = env_prefetch<CM_PP, LPE>(apply_cond(p, cv), b_raw, live); }
        else
        if constexpr (PRE && !CARRY) pre = env_prefetch<CM_PP, LPE>(p, b_raw, live);   // env state requested in front of the policy forward
        if constexpr (SHAPE == 1)
            mw::policy_tile_w<LHOPS, true, false, 0, true, true>(at, n_act, res, lds_w, blockIdx.x, act, obs_row,
                                                           mw::StepOff{ ut * (uint32_t)c.actions, ut * (uint32_t)c.probs, ut * (uint32_t)c.attn }, draw, &e1a);
        else mw::policy_tile_w<LHOPS, CARRY>(at, n_act, res, lds_w, blockIdx.x, act, obs_row);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");               // this wave's action words are in LDS
        const unsigned long long t1 = probe ? __builtin_amdgcn_s_memtime() : 0ull;
        cm_step_out ot = out;
        if constexpr (SHAPE != 1) {
        if (ot.obs) ot.obs += (size_t)t * c.obs;
        if (ot.reward) ot.reward += (size_t)t * c.reward;
        if (ot.reward_f64) ot.reward_f64 += (size_t)t * c.reward_f64;
        if (ot.done) ot.done += (size_t)t * c.done;
        if (ot.details) ot.details += (size_t)t * c.details;
        if (ot.dist_adj) ot.dist_adj += (size_t)t * c.dist_adj;
        if (ot.channels) ot.channels += (size_t)t * c.channels;
        if (ot.prey_alive) ot.prey_alive += (size_t)t * c.prey_alive;
        if (ot.success) ot.success += (size_t)t * c.success;
        if (ot.path_len) ot.path_len += (size_t)t * c.path_len;
        }
        if (SHAPE == 1 && !FULLWG ? __builtin_expect(env_wave, true) : env_wave) {
            const int32_t *my_act = act + (live ? grp : 0) * 4;
            if constexpr (COND) {                                        // the non-carried forms below, on the env's own comm scalars
                const EnvDev q = apply_cond(p, cv);
                if constexpr (PRE) {
                    const bool bad = env_stage<CM_PP, LPE>(q, pre, my_act, grp, ENV_BASE);
                    env_body<CM_PP, LPE>(q, nullptr, my_act, tape, ot, 0, grp, b_raw, live, ENV_BASE, nullptr, true, pre.rng_step, pre.step_count_in,
                                         pre.succ, pre.t_row, pre.t_col, pre.t_step0, pre.t_step, pre.t_rew, bad, FULLWG);
                } else env_body<CM_PP, LPE>(q, nullptr, my_act, tape, ot, 0, grp, b_raw, live, ENV_BASE);
            } else if constexpr (CARRY && SHAPE == 1) {
                const pp10::StepOff so{ ut * (uint32_t)c.obs, ut * (uint32_t)c.reward, ut * (uint32_t)c.reward_f64, ut * (uint32_t)c.done,
                                        ut * (uint32_t)c.details, ut * (uint32_t)c.prey_alive, ut * (uint32_t)c.success, ut * (uint32_t)c.path_len };
                pp10::step(p, st, pp, em, ACT_OFF + (live ? grp : 0) * 16, ot, so, t == c.n_steps - 1, grp, b_raw, live, ENV_BASE, FULLWG, obs_env, draw + mw::DRAW_WAVE_BYTES / 4,
                           [&] { e1a.template fetch<LHOPS>(); });
            } else if constexpr (CARRY) {
                const bool bad = env_stage<CM_PP, LPE>(p, pre, my_act, grp, ENV_BASE);
                EnvCarry carry{ pre.step_count_in, pre.succ, 0 };
                env_body<CM_PP, LPE>(p, nullptr, my_act, tape, ot, 0, grp, b_raw, live, ENV_BASE, nullptr, true, pre.rng_step, pre.step_count_in,
                                     pre.succ, pre.t_row, pre.t_col, pre.t_step0, pre.t_step, pre.t_rew, bad, FULLWG, &carry, obs_env);
                pre = env_pre_carry<CM_PP, LPE>(p, pre, carry, grp, ENV_BASE);
            } else if constexpr (PRE) {
                const bool bad = env_stage<CM_PP, LPE>(p, pre, my_act, grp, ENV_BASE);
                env_body<CM_PP, LPE>(p, nullptr, my_act, tape, ot, 0, grp, b_raw, live, ENV_BASE, nullptr, true, pre.rng_step, pre.step_count_in,
                                     pre.succ, pre.t_row, pre.t_col, pre.t_step0, pre.t_step, pre.t_rew, bad, FULLWG);
            } else env_body<CM_PP, LPE>(p, nullptr, my_act, tape, ot, 0, grp, b_raw, live, ENV_BASE);
        } else e1a.template fetch<LHOPS>();                               // SHAPE 1, a wave without an env: no step that requests them
        // step t + 1 reads what this WAVE wrote (observation, masks, env state): its stores are performed before its next loads;
        // the CU's vector L1 is write-through and shared, so workgroup scope needs no cache maintenance (as rollout_chunk_kernel)
        const unsigned long long tf = probe ? __builtin_amdgcn_s_memtime() : 0ull;
        if constexpr (!CARRY) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
        if (probe) { const unsigned long long t2 = __builtin_amdgcn_s_memtime(); g_w_probe[0] += 1; g_w_probe[1] += t1 - t0; g_w_probe[2] += t2 - t1; g_w_probe[4] += t2 - tf; }
    }
    if constexpr (CARRY) {
        if (tl.on) {                                                     // `obses = next_obses` + the counter advance (cm_chunk_tail) in here
            const int tx = thread_x(), grp = tx / LPE, sl = tx % LPE;
            const int b0 = blockIdx.x * mw::WG_ENVS + grp;
            if ((FULLWG || grp < envs) && b0 < a.S) {
                const float *oc = reinterpret_cast<const float *>(lds_w + obs_env);
                float *dst = tl.obs_dst + (size_t)b0 * 4 * a.d;
                const float rcp_d = p.rcp_d;
                for (int k = sl; k < 4 * a.d; k += LPE) { const int i = fdiv(k, a.d, rcp_d), f = k - i * a.d; dst[k] = oc[i * OBS_COPY_STRIDE + f]; }
            }
            if ((tx & 63) == 0) {
                const unsigned int last = gridDim.x * (blockDim.x >> 6) - 1;
                if (atomicAdd(tl.ticket, 1u) == last) { *tl.base += (uint32_t)c.n_steps; *tl.ticket = 0u; }
            }
        }
    }
