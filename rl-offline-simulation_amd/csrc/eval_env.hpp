// eval_env.hpp -- the reference's tabular drivers evalMC, qlearn and expSARSA (offsim4rl/agents/tabular.py:247-270, :71-139, :141-191) on its
// own grid worlds MyGridNavi, MyGridNaviNoise and MyGridNaviModuloCounter (offsim4rl/envs/gridworld.py:14-184), many rollouts per launch:
// offsim_eval_env / offsim_eval_env_pop (include/offsim.h).  The ground truth the *_psrs and *_queue drivers are judged against.
//
// k_eval_queue (eval_queue.hpp) with the grid's dynamics in the place of the queue pop.  There is no table, no queue and no cursor: an
// environment never runs dry, every episode begins with a reset, and the carried state of a rollout is its action stream, its tie stream
// and its Q.  Per step
//   o      x + num_cells * y + num_cells^2 * extra  (external_state; extra: the random bits of NOISE, the counter of COUNTER, 0 for PLAIN)
//   p      pi[o], or td_behaviour on Q[o]
//   A      queue_draw's rule on one next_double of the rollout's PCG64 action stream (Generator.choice(5, p=p))
//   extra  NOISE: Generator.integers(factor) of the episode's stream, BEFORE the move (gridworld.py:145); COUNTER: (extra + 1) % factor (:174)
//   move   MyGridNavi.step (:87-121) to the letter: done if already on the goal, the clamped move, step_count, then reward 0 if done, 1 and
//          done on reaching the goal, else -0.1 -- in f64, as the reference's Python floats
//   TD     the update of k_eval_queue on Q[o, A] with Q[o'], the same arithmetic and order
// The exogenous stream is default_rng(episode0 + e), created again at the reset of every episode e (gridworld.py:139, :168: the drivers call
// env.reset(seed=episode)); NOISE and COUNTER draw integers(factor) from it at the reset.  integers(n) is NumPy's scalar path: nothing drawn
// for n = 1, else Lemire's bounded 32-bit draw on the buffered halves of the 64-bit outputs (PcgSeq::next32).  Its redraw loop is the one
// data-dependent loop here; every other loop is bounded by num_steps * max_episodes.
//
// Two launch shapes:
//   k_eval_env<TD, POP>   one wavefront per rollout, wave-uniform control flow: the learner drivers (Q, the behaviour row and the tie stream
//                         per rollout in LDS, shared pi in LDS; the carve of k_eval_queue without seg_off and cursors), and a population of
//                         learners under csrc/td_pop.hpp's index rule.  <false, false> is evalMC in that shape, kept for the comparison
//                         tools/bench_env_drivers.py records (OFFSIM_ENV_EVALMC_WAVE=1 routes evalMC of one policy to it).
//   k_eval_env_mc<PI_LDS> evalMC: no table and no per-rollout LDS state, so the ROLLOUT IS THE LANE (as the learner is in replay_td.hpp);
//                         the five-term cdf runs serially per lane with queue_draw's expressions.  A stack of L policies [L, nS, 5] sits in
//                         LDS when it fits 64 KiB, else it is read from global memory; rollout r = l * S + j reads stack row l.  A lane
//                         that has finished its episodes idles until the last lane of its wave has.
//
// Included by offsim_hip.hip behind eval_queue.hpp: mt_seed_lds, queue_draw, td_behaviour, check_evalmc_out, check_td, check_td_pop,
// td_of_pop, launch_shape, discount_at and allow_big_lds are that file's and its includes'.
#pragma once

#define ENV_NA 5  // noop, up, right, down, left

// Generator.integers(n), 0 < n < 2^31, scalar path (numpy/random/_bounded_integers: _rand_int64 -> random_bounded_uint64 with rng = n - 1,
// unmasked: nothing for rng = 0, else buffered_bounded_lemire_uint32 on next_uint32)
__device__ __forceinline__ int grid_integers(PcgSeq &g, uint32_t n) {
    if (n <= 1u) return 0;
    uint64_t m = (uint64_t)g.next32() * (uint64_t)n;
    uint32_t leftover = (uint32_t)m;
    if (leftover < n) {
        const uint32_t threshold = (0xffffffffu - (n - 1u)) % n;
        while (leftover < threshold) {
            m = (uint64_t)g.next32() * (uint64_t)n;
            leftover = (uint32_t)m;
        }
    }
    return (int)(m >> 32);
}

// env.reset(seed): the exogenous stream and its first draw (NOISE, COUNTER); returns extra
__device__ __forceinline__ int grid_reset_extra(const offsim_grid_env &E, PcgSeq &g, uint64_t seed) {
    if (E.kind == OFFSIM_GRID_PLAIN) return 0;
    g.init(pcg_seed(seed));
    return grid_integers(g, (uint32_t)E.factor);
}

// the exogenous part of step(a), before the move
__device__ __forceinline__ int grid_step_extra(const offsim_grid_env &E, PcgSeq &g, int extra) {
    if (E.kind == OFFSIM_GRID_NOISE) return grid_integers(g, (uint32_t)E.factor);
    if (E.kind == OFFSIM_GRID_COUNTER) return (extra + 1) % E.factor;
    return 0;
}

// MyGridNavi.step(a): the move on (x, y, step_count); returns done
__device__ __forceinline__ bool grid_move(const offsim_grid_env &E, int &x, int &y, int &sc, int a, double &reward) {
    bool done = x == E.goal_x && y == E.goal_y;
    const int hi = E.num_cells - 1;
    if (a == 1) y = y + 1 < hi ? y + 1 : hi;
    else if (a == 2) x = x + 1 < hi ? x + 1 : hi;
    else if (a == 3) y = y - 1 > 0 ? y - 1 : 0;
    else if (a == 4) x = x - 1 > 0 ? x - 1 : 0;
    sc++;
    if (sc >= E.num_steps) done = true;
    if (done) reward = 0.0;
    else if (x == E.goal_x && y == E.goal_y) {
        reward = 1.0;
        done = true;
    } else reward = -0.1;
    return done;
}

struct EnvArgs {
    int32_t tie_reseed;
    uint32_t tie_episode0;  // np.random.seed takes the episode modulo 2^32
    uint64_t episode0;
};
struct EnvPopArgs : EnvArgs, TdPopFields {};
static_assert(td_pop_layout<EnvPopArgs>(96, 16, 88), "kernel arguments of k_eval_env<TD, POP>");
template <bool POP>
using EnvKernelArgs = std::conditional_t<POP, EnvPopArgs, EnvArgs>;

// The learner blocks around the step (POP prologue and index, tie stream, TD update, episode close, outputs) are written out here as in each of
// the three rollout kernels (see the note above k_eval_queue).
template <bool TD, bool POP = false>
__global__ void __launch_bounds__(256, 4) k_eval_env(offsim_grid_env E, offsim_env_rollouts ro, const double *__restrict__ pi, double gamma,
                                                  const double *__restrict__ gamma_pow, int64_t n_gamma_pow, int64_t max_episodes,
                                                  offsim_evalmc_out out, offsim_td td, EnvKernelArgs<POP> ea) {
    static_assert(!POP || TD, "a population is a population of learners");
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int waves = blockDim.x / WAVE;
    int pop_l = 0, pop_nb = 1;  // POP: this workgroup's learner, workgroups per learner
    if constexpr (POP) {
        pop_nb = (ea.S + waves - 1) / waves;
        pop_l = blockIdx.x / pop_nb;
        td.alpha = ea.alpha[pop_l];
        td.epsilon = ea.epsilon[pop_l];
        td.behaviour = ea.behaviour[pop_l];
        td.alpha_ep = ea.alpha_ep ? ea.alpha_ep + (int64_t)pop_l * td.n_sched : nullptr;
        td.epsilon_ep = ea.epsilon_ep ? ea.epsilon_ep + (int64_t)pop_l * td.n_sched : nullptr;
        gamma = ea.gamma[pop_l];
        gamma_pow = ea.gamma_pow + (int64_t)pop_l * n_gamma_pow;
        pi = ea.pi ? ea.pi + (int64_t)pop_l * ea.pi_stride : nullptr;
    }
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE), lane = threadIdx.x & (WAVE - 1);  // uniform -> SGPR
    constexpr int nA = ENV_NA;
    const int ncc = E.num_cells * E.num_cells;
    const int n = ncc * E.factor * nA;
    // LDS carve: [Q per wave (TD)][pi (when given)][behaviour row per wave (TD)][tie stream per wave (TD)]
    double *q_lds = (double *)lds_raw + (TD ? (size_t)wave * n : 0);
    double *pi_lds = (double *)lds_raw + (TD ? (size_t)waves * n : 0);
    double *beh_lds = pi_lds + (pi ? (size_t)n : 0) + (TD ? (size_t)wave * nA : 0);
    volatile uint32_t *mt_lds = (volatile uint32_t *)(pi_lds + (pi ? (size_t)n : 0) + (TD ? (size_t)waves * nA : 0)) + (TD ? (size_t)wave * 624 : 0);
    if (pi)
        for (int i = threadIdx.x; i < n; i += blockDim.x) pi_lds[i] = pi[i];
    __syncthreads();
    int r = blockIdx.x * waves + wave;
    if constexpr (POP) {
        const int ord = __builtin_amdgcn_readfirstlane((blockIdx.x - pop_l * pop_nb) * waves + wave);
        if (ord >= ea.S) return;
        r = __builtin_amdgcn_readfirstlane(pop_l * ea.S + ord);
    } else {
        if (r >= ro.R) return;
    }
    uint32_t mt_pos = 624u;
    if (TD) {
        for (int i = lane; i < n; i += WAVE) q_lds[i] = td.q[(int64_t)r * n + i];
        if (td.tie_mt) {
            for (int i = lane; i < 624; i += WAVE) mt_lds[i] = td.tie_mt[(int64_t)r * 625 + i];
            mt_pos = td.tie_mt[(int64_t)r * 625 + 624];
        }
    }
    U128 st = stream_row_base(ro.rng, r);  // the action stream: the state before the next draw's step
    const U128 inc = stream_row_inc(ro.rng, r);
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): Q and the tie stream visible to the whole wave

    PcgSeq exo;  // the episode's exogenous stream (NOISE, COUNTER)
    exo.init(PcgInit{u128(0, 0), u128(0, 1)});
    int64_t ep = 0, n_len = 0, steps = 0;
    uint64_t consumed = 0;
    double sum_g = 0.0;
    int status = OFFSIM_ST_OK;
    bool terminate = false, mt_pending = false;
    uint32_t mt_seed = 0u;
    while (ep < max_episodes && !terminate) {
        if (TD && ea.tie_reseed) {  // np.random.seed(episode), tabular.py:114 / :166 -- before env.reset
            mt_pending = true;
            mt_seed = ea.tie_episode0 + (uint32_t)ep;
        }
        // env.reset(seed=episode)  (gridworld.py:50-53, :138-141, :167-170)
        int x = 0, y = 0, sc = 0;
        int extra = __builtin_amdgcn_readfirstlane(grid_reset_extra(E, exo, ea.episode0 + (uint64_t)ep));
        double G = 0.0;
        int64_t tt = 0;
        bool done = false;
        while (!done) {
            const double gp = discount_at(gamma_pow, (uint64_t)n_gamma_pow, gamma, (uint64_t)tt);  // issued ahead of the step
            const int b = (x + E.num_cells * y + ncc * extra) * nA;  // the row of observation o starts at o * nA
            // p = pi[S] (tabular.py:171, :258) or behavior_policy(Q[[S], :], ...)[0] (:119)
            const double *p = pi_lds + b;
            if (TD && td.behaviour != OFFSIM_BEHAVIOUR_FIXED) {
                if (mt_pending && td.behaviour == OFFSIM_BEHAVIOUR_EPS_GREEDY) {
                    mt_seed_lds(mt_lds, mt_seed, lane);
                    mt_pos = 624u;
                    mt_pending = false;
                }
                td_behaviour(td, q_lds + b, nA, beh_lds, mt_lds, mt_pos, lane, r, ep, steps);
                p = beh_lds;
            }
            // A = rng.choice(env.nA, p=p)  (tabular.py:120, :172, :259)
            st = pcg_step(st, inc);
            consumed++;
            const double u = (double)(pcg_output(st) >> 11) * 0x1.0p-53;
            const int A = queue_draw(p, nA, u, lane);
            if (lane == 0 && out.trace_pop && steps < out.trace_cap) out.trace_pop[(int64_t)r * out.trace_cap + steps] = (uint32_t)A;
            if (A >= nA) {  // no action drawn (p of NaN or zeros): the draw is consumed, the environment has not stepped
                status = OFFSIM_ST_KEYERROR;
                terminate = true;
                break;
            }
            // env.step(A)
            extra = __builtin_amdgcn_readfirstlane(grid_step_extra(E, exo, extra));
            double rew;
            const bool dn = grid_move(E, x, y, sc, A, rew);
            const int b_next = (x + E.num_cells * y + ncc * extra) * nA;
            if (TD) {  // tabular.py:123-126 (Q-learning) / :175-178 (expected SARSA) on Q[o, A] with Q[o']; every lane computes the same update
                const double q_sa = q_lds[b + A];
                const double *qn = q_lds + b_next;
                double nxt;
                if (td.mode == OFFSIM_TD_QLEARN) {
                    nxt = qn[0];
                    for (int k2 = 1; k2 < nA; k2++) nxt = qn[k2] > nxt ? qn[k2] : nxt;
                } else {  // Q[S_] @ pi[S_], left to right
                    const double *pn = pi_lds + b_next;
                    nxt = 0.0;
                    for (int k2 = 0; k2 < nA; k2++) nxt = nxt + qn[k2] * pn[k2];
                }
                const double td_err = rew + gamma * nxt - q_sa;
                if (lane == 0 && td.td_err && steps < td.td_cap) td.td_err[(int64_t)r * td.td_cap + steps] = td_err;
                const double alpha = td.alpha_ep ? td.alpha_ep[ep < td.n_sched ? ep : td.n_sched - 1] : td.alpha;  // alpha(episode)
                __builtin_amdgcn_s_waitcnt(0xc07f);
                q_lds[b + A] = q_sa + alpha * td_err;
                if (td.q_snap && steps % td.snap_stride == 0 && steps / td.snap_stride < td.snap_cap) {  // save_Q (tabular.py:131, :183)
                    __builtin_amdgcn_s_waitcnt(0xc07f);
                    double *dst = td.q_snap + ((int64_t)r * td.snap_cap + steps / td.snap_stride) * n;
                    for (int i = lane; i < n; i += WAVE) dst[i] = q_lds[i];
                }
            }
            G = G + gp * rew;  // tabular.py:129 (no FMA contraction: built with -ffp-contract=off)
            tt++;
            steps++;
            done = dn;
        }
        if (status == OFFSIM_ST_KEYERROR) break;  // the reference raises out of the driver here
        if (lane == 0 && out.ep_len && n_len <= out.ep_cap) out.ep_len[(int64_t)r * (out.ep_cap + 1) + n_len] = (int32_t)tt;
        n_len++;
        if (lane == 0 && out.ep_g && ep < out.ep_cap) out.ep_g[(int64_t)r * out.ep_cap + ep] = G;
        sum_g += G;
        ep++;
    }
    // write back what a later call continues from: the action stream, Q, the tie stream
    if (TD && mt_pending && td.tie_mt) {
        mt_seed_lds(mt_lds, mt_seed, lane);
        mt_pos = 624u;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    if (TD) {
        for (int i = lane; i < n; i += WAVE) td.q[(int64_t)r * n + i] = q_lds[i];
        if (td.tie_mt) {
            for (int i = lane; i < 624; i += WAVE) td.tie_mt[(int64_t)r * 625 + i] = mt_lds[i];
            if (lane == 0) td.tie_mt[(int64_t)r * 625 + 624] = mt_pos;
        }
    }
    if (lane == 0) {
        if (consumed) {  // the state after the last draw
            ro.rng[4 * r + 0] = st.hi;
            ro.rng[4 * r + 1] = st.lo;
        }
        out.sum_g[r] = sum_g;
        out.n_ep[r] = ep;
        out.steps[r] = steps;
        out.cand[r] = steps;  // one action drawn per step
        out.n_len[r] = n_len;
        out.status[r] = status;
    }
}

// evalMC, the rollout is the lane.  pi: [L, n] (n = nS * 5), rollout r reads row r / S.  One flat loop per lane -- reset when the last step
// closed an episode, then one step -- so that lanes whose episodes differ in length do not wait for each other at episode ends.
#define ENV_MC_THREADS 256
template <bool PI_LDS>
__global__ void __launch_bounds__(ENV_MC_THREADS) k_eval_env_mc(offsim_grid_env E, offsim_env_rollouts ro, const double *__restrict__ pi, int32_t L,
                                                                int32_t S, double gamma, const double *__restrict__ gamma_pow, int64_t n_gamma_pow,
                                                                int64_t max_episodes, offsim_evalmc_out out, uint64_t episode0) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    constexpr int nA = ENV_NA;
    const int ncc = E.num_cells * E.num_cells;
    const int n = ncc * E.factor * nA;
    if constexpr (PI_LDS) {
        double *pi_lds = (double *)lds_raw;
        for (int i = threadIdx.x; i < L * n; i += blockDim.x) pi_lds[i] = pi[i];
        __syncthreads();
    }
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= ro.R) return;  // (no barrier below)
    const double *prow = (PI_LDS ? (const double *)lds_raw : pi) + (int64_t)(r / S) * n;
    U128 st = stream_row_base(ro.rng, r);
    const U128 inc = stream_row_inc(ro.rng, r);
    PcgSeq exo;
    exo.init(PcgInit{u128(0, 0), u128(0, 1)});
    int64_t ep = 0, n_len = 0, steps = 0, tt = 0;
    double sum_g = 0.0, G = 0.0;
    int status = OFFSIM_ST_OK;
    int x = 0, y = 0, sc = 0, extra = 0;
    bool fresh = true;
    while (ep < max_episodes) {
        if (fresh) {  // env.reset(seed=episode)
            x = y = sc = 0;
            extra = grid_reset_extra(E, exo, episode0 + (uint64_t)ep);
            G = 0.0;
            tt = 0;
            fresh = false;
        }
        const double gp = discount_at(gamma_pow, (uint64_t)n_gamma_pow, gamma, (uint64_t)tt);
        const double *p = prow + (x + E.num_cells * y + ncc * extra) * nA;
        st = pcg_step(st, inc);
        const double u = (double)(pcg_output(st) >> 11) * 0x1.0p-53;
        // queue_draw's expressions, serially: tot = c_4, c_k = c_{k-1} + p_k from 0, the first k with c_k / tot > u
        double pk[nA];
        double tot = 0.0;
        for (int k = 0; k < nA; k++) {
            pk[k] = p[k];
            tot = tot + pk[k];
        }
        int A = nA;
        double c = 0.0;
        for (int k = 0; k < nA; k++) {
            c = c + pk[k];
            if (A == nA && c / tot > u) A = k;
        }
        if (out.trace_pop && steps < out.trace_cap) out.trace_pop[r * out.trace_cap + steps] = (uint32_t)A;
        if (A >= nA) {
            status = OFFSIM_ST_KEYERROR;
            break;
        }
        extra = grid_step_extra(E, exo, extra);
        double rew;
        const bool done = grid_move(E, x, y, sc, A, rew);
        G = G + gp * rew;
        tt++;
        steps++;
        if (done) {
            if (out.ep_len && n_len <= out.ep_cap) out.ep_len[r * (out.ep_cap + 1) + n_len] = (int32_t)tt;
            n_len++;
            if (out.ep_g && ep < out.ep_cap) out.ep_g[r * out.ep_cap + ep] = G;
            sum_g += G;
            ep++;
            fresh = true;
        }
    }
    if (steps > 0 || status != OFFSIM_ST_OK) {  // the state after the last draw
        ro.rng[4 * r + 0] = st.hi;
        ro.rng[4 * r + 1] = st.lo;
    }
    out.sum_g[r] = sum_g;
    out.n_ep[r] = ep;
    out.steps[r] = steps;
    out.cand[r] = steps;
    out.n_len[r] = n_len;
    out.status[r] = status;
}

static size_t env_lds_bytes(int waves, int64_t n, bool have_pi, bool td) {
    return (td ? (size_t)waves * n * 8 : 0) + (have_pi ? (size_t)n * 8 : 0) + (td ? (size_t)waves * ENV_NA * 8 + (size_t)waves * 624 * 4 : 0);
}

#define ENV_MAX_CELLS2 40960  // num_cells^2 and nS * 5 at most this: the learner's one-rollout carve ends below it (keeps the sums in range)
#define ENV_MC_MAX_N (1 << 24)  // evalMC reads pi from global memory past 64 KiB: nS * 5 up to this (row offsets stay in 32 bits)

// what offsim_eval_env and offsim_eval_env_pop check alike, in this order: the world, the rollout state and its provider, out, the capacities,
// max_episodes, episode0, the learner and the tie mode
static int env_check(const char *who, const offsim_grid_env *env, const offsim_env_rollouts *ro, const double *gamma_pow, int64_t n_gamma_pow,
                     int64_t max_episodes, const offsim_evalmc_out *out, const offsim_td *td, int32_t tie_reseed_episode, int64_t episode0) {
    if (!env) return fail(OFFSIM_EINVAL, "%s: env is NULL", who);
    if (env->kind != OFFSIM_GRID_PLAIN && env->kind != OFFSIM_GRID_NOISE && env->kind != OFFSIM_GRID_COUNTER) return fail(OFFSIM_EINVAL, "%s: bad kind", who);
    if (env->num_cells < 1 || env->num_steps < 1) return fail(OFFSIM_EINVAL, "%s: num_cells and num_steps must be positive", who);
    if (env->goal_x < 0 || env->goal_x >= env->num_cells || env->goal_y < 0 || env->goal_y >= env->num_cells)
        return fail(OFFSIM_EINVAL, "%s: the goal lies off the grid", who);
    if (env->factor < 1 || (env->kind == OFFSIM_GRID_PLAIN && env->factor != 1))
        return fail(OFFSIM_EINVAL, "%s: factor must be positive (1 for OFFSIM_GRID_PLAIN)", who);
    if (!ro || ro->R < 0) return fail(OFFSIM_EINVAL, "%s: ro is NULL or R < 0", who);
    if (ro->R > 0 && !ro->rng) return fail(OFFSIM_EINVAL, "%s: NULL rollout state", who);
    if (ro->rng_kind == OFFSIM_STREAM_PHILOX)
        return fail(OFFSIM_EUNSUPPORTED, "%s: the action stream must be OFFSIM_STREAM_PCG64 (a Philox double lies in (0, 1]: u = 1.0 selects action nA)", who);
    if (ro->rng_kind != OFFSIM_STREAM_PCG64) return fail(OFFSIM_EINVAL, "%s: unknown stream provider", who);
    if (!out) return fail(OFFSIM_EINVAL, "%s: out is NULL", who);
    int rc = check_evalmc_out(who, out, gamma_pow, n_gamma_pow);
    if (rc) return rc;
    if (out->ep_cap < 0 || out->trace_cap < 0) return fail(OFFSIM_EINVAL, "%s: negative ep_cap / trace_cap", who);
    if (max_episodes <= 0) return fail(OFFSIM_EINVAL, "%s: max_episodes must be positive (an environment never runs dry)", who);
    if (episode0 < 0) return fail(OFFSIM_EINVAL, "%s: episode0 is negative", who);
    if (tie_reseed_episode != 0 && tie_reseed_episode != 1) return fail(OFFSIM_EINVAL, "%s: tie_reseed_episode is 0 or 1", who);
    if (td) {
        if ((rc = check_td(who, td, TD_RULES))) return rc;
        if (tie_reseed_episode && !td->tie_mt) return fail(OFFSIM_EINVAL, "%s: tie_reseed_episode needs td->tie_mt (the stream is written back there)", who);
    } else if (tie_reseed_episode) {
        return fail(OFFSIM_EINVAL, "%s: tie_reseed_episode without a learner", who);
    }
    return OFFSIM_OK;
}

// nS * 5, or -1 past `limit`
static int64_t env_table_len(const offsim_grid_env *env, int64_t limit) {
    const int64_t ncc = (int64_t)env->num_cells * env->num_cells;
    if (ncc > limit || ncc * env->factor > limit / ENV_NA) return -1;
    return ncc * env->factor * ENV_NA;
}

// the launch shape of k_eval_env (launch_shape's 4 / 2 / 1 rule on the carve above)
static int env_launch_shape(const char *who, const offsim_grid_env *env, bool have_pi, bool td, int *waves_out, size_t *lds_out) {
    const int64_t n = env_table_len(env, ENV_MAX_CELLS2);
    if (n < 0 || !launch_shape([&](int w) { return env_lds_bytes(w, n, have_pi, td); }, waves_out, lds_out))
        return fail(OFFSIM_EUNSUPPORTED, "%s: policy and Q table (nS * 5 entries) exceed 160 KiB of LDS", who);
    return OFFSIM_OK;
}

template <bool TD, bool POP = false>
static int env_launch(const offsim_grid_env *env, offsim_env_rollouts *ro, const double *pi, double gamma, const double *gamma_pow, int64_t n_gamma_pow,
                      int64_t max_episodes, const offsim_evalmc_out *out, const offsim_td &td, const EnvKernelArgs<POP> &ea, int waves, size_t lds,
                      void *stream) {
    if (lds > 64 * 1024) HIP_TRY(allow_big_lds((k_eval_env<TD, POP>), (int)lds));
    unsigned grid = (unsigned)((ro->R + waves - 1) / waves);
    if constexpr (POP) grid = pop_grid(ro->R, ea.S, waves);
    hipLaunchKernelGGL((k_eval_env<TD, POP>), dim3(grid), dim3(waves * WAVE), lds, (hipStream_t)stream, *env, *ro, pi, gamma, gamma_pow, n_gamma_pow,
                       max_episodes, *out, td, ea);
    LAUNCH_CHECK();
    return OFFSIM_OK;
}

// evalMC of a stack of L policies on S rollouts each (L = 1, S = R: one policy); the stack in LDS when L * nS * 5 * 8 <= 64 KiB
static int env_launch_mc(const char *who, const offsim_grid_env *env, offsim_env_rollouts *ro, const double *pi, int32_t L, int32_t S, double gamma,
                         const double *gamma_pow, int64_t n_gamma_pow, int64_t max_episodes, const offsim_evalmc_out *out, int64_t episode0, void *stream) {
    const int64_t n = env_table_len(env, ENV_MC_MAX_N);
    if (n < 0) return fail(OFFSIM_EUNSUPPORTED, "%s: nS * 5 exceeds 2^24 entries", who);
    if (ro->R == 0) return OFFSIM_OK;
    const size_t bytes = (size_t)L * (size_t)n * 8;
    const unsigned grid = (unsigned)((ro->R + ENV_MC_THREADS - 1) / ENV_MC_THREADS);
    if (bytes <= 64 * 1024)
        hipLaunchKernelGGL((k_eval_env_mc<true>), dim3(grid), dim3(ENV_MC_THREADS), bytes, (hipStream_t)stream, *env, *ro, pi, L, S, gamma, gamma_pow,
                           n_gamma_pow, max_episodes, *out, (uint64_t)episode0);
    else
        hipLaunchKernelGGL((k_eval_env_mc<false>), dim3(grid), dim3(ENV_MC_THREADS), 0, (hipStream_t)stream, *env, *ro, pi, L, S, gamma, gamma_pow,
                           n_gamma_pow, max_episodes, *out, (uint64_t)episode0);
    LAUNCH_CHECK();
    return OFFSIM_OK;
}

extern "C" int offsim_eval_env(const offsim_grid_env *env, offsim_env_rollouts *ro, const double *pi, double gamma, const double *gamma_pow,
                               int64_t n_gamma_pow, int64_t max_episodes, const offsim_evalmc_out *out, const offsim_td *td,
                               int32_t tie_reseed_episode, int64_t episode0, void *stream) {
    static const char *who = "eval_env";
    int rc = env_check(who, env, ro, gamma_pow, n_gamma_pow, max_episodes, out, td, tie_reseed_episode, episode0);
    if (rc) return rc;
    if (!pi && !(td && td->behaviour != OFFSIM_BEHAVIOUR_FIXED && td->mode == OFFSIM_TD_QLEARN))
        return fail(OFFSIM_EINVAL, "%s: pi is NULL (only Q-learning with a behaviour on the learner's own Q runs without one)", who);
    static const bool mc_wave = getenv("OFFSIM_ENV_EVALMC_WAVE") && atoi(getenv("OFFSIM_ENV_EVALMC_WAVE")) != 0;
    if (!td && !mc_wave) return env_launch_mc(who, env, ro, pi, 1, ro->R > 0 ? ro->R : 1, gamma, gamma_pow, n_gamma_pow, max_episodes, out, episode0, stream);
    int waves = 0;
    size_t lds = 0;
    if ((rc = env_launch_shape(who, env, pi != nullptr, td != nullptr, &waves, &lds))) return rc;
    if (ro->R == 0) return OFFSIM_OK;
    offsim_td tdv;
    memset(&tdv, 0, sizeof(tdv));
    if (td) tdv = *td;
    const EnvArgs ea{tie_reseed_episode, (uint32_t)episode0, (uint64_t)episode0};
    if (td) return env_launch<true>(env, ro, pi, gamma, gamma_pow, n_gamma_pow, max_episodes, out, tdv, ea, waves, lds, stream);
    return env_launch<false>(env, ro, pi, gamma, gamma_pow, n_gamma_pow, max_episodes, out, tdv, ea, waves, lds, stream);
}

extern "C" int offsim_eval_env_pop(const offsim_grid_env *env, offsim_env_rollouts *ro, int32_t L, int32_t S, const offsim_td_pop *pop,
                                   const double *pi_stack, double gamma, const double *gamma_pow, int64_t n_gamma_pow, int64_t max_episodes,
                                   const offsim_evalmc_out *out, int32_t tie_reseed_episode, int64_t episode0, void *stream) {
    static const char *who = "eval_env_pop";
    if (!pop) {  // evalMC of the stack pi_stack [L, nS, 5]
        int rc = env_check(who, env, ro, gamma_pow, n_gamma_pow, max_episodes, out, nullptr, tie_reseed_episode, episode0);
        if (rc) return rc;
        if (L < 1 || L > 65535 || S < 1) return fail(OFFSIM_EINVAL, "%s: L must be 1..65535 and S >= 1", who);
        if (ro->R != 0 && ro->R != (int64_t)L * S) return fail(OFFSIM_EINVAL, "%s: ro->R must be L * S", who);
        if (!pi_stack) return fail(OFFSIM_EINVAL, "%s: pi_stack is NULL", who);
        return env_launch_mc(who, env, ro, pi_stack, L, S, gamma, gamma_pow, n_gamma_pow, max_episodes, out, episode0, stream);
    }
    const offsim_td td = td_of_pop(pop);
    int rc = env_check(who, env, ro, pop->gamma_pow, pop->n_gamma_pow, max_episodes, out, &td, tie_reseed_episode, episode0);
    if (rc || (rc = check_td_pop(who, L, S, ro->R, pop, true))) return rc;
    if (!pop->pi) {  // (behaviour_host has been validated)
        bool fixed = false;
        for (int32_t l = 0; l < L; l++) fixed = fixed || pop->behaviour_host[l] == OFFSIM_BEHAVIOUR_FIXED;
        if (fixed || pop->mode != OFFSIM_TD_QLEARN)
            return fail(OFFSIM_EINVAL, "%s: pi is NULL (only Q-learning with a behaviour on every learner's own Q runs without one)", who);
    }
    int waves = 0;
    size_t lds = 0;
    if ((rc = env_launch_shape(who, env, pop->pi != nullptr, true, &waves, &lds))) return rc;
    if (ro->R == 0) return OFFSIM_OK;
    const EnvPopArgs ea{EnvArgs{tie_reseed_episode, (uint32_t)episode0, (uint64_t)episode0}, td_pop_fields(pop, S)};
    return env_launch<true, true>(env, ro, nullptr, 0.0, nullptr, pop->n_gamma_pow, max_episodes, out, td, ea, waves, lds, stream);
}
