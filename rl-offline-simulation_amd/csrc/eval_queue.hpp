// eval_queue.hpp -- whole rollouts on QueueEvaluator (offsim4rl/evaluators/queue_evaluator.py:90-131) under the reference's tabular drivers
// evalMC, qlearn and expSARSA (offsim4rl/agents/tabular.py:247-270, :71-139, :141-191), many rollouts per launch: offsim_eval_queue
// (include/offsim.h).
//
// The queues are keyed by (z, a): the table is grouped by the composite slot z * nA + a, z_next / init_slot hold BASE slots z' * nA
// (evaluators/queue_evaluator.py: BatchedQueueEvaluator), while pi and Q are [nZ, nA] by state -- flat, so the row of the state with base
// slot b starts at b.  The agent draws its own action (tabular.py:57, :120, :172, :259: rng.choice(env.nA, p=p)) and the simulator pops the
// head of queue (z, A) (queue_evaluator.py:121-131): no rejection, one row per step.
//
// The loop is k_eval_mc's (one wavefront per rollout, uniform control flow, the same episode bookkeeping, TD update, outputs, status codes
// and write-back); the step is
//   p      pi[z], or td_behaviour on Q[z] (the block k_eval_mc and k_eval_mc_exo call)
//   A      Generator.choice(nA, p=p): c_k = c_{k-1} + p_k in f64 from 0, cdf_k = c_k / c_{nA-1}, u = (next64 >> 11) * 2^-53 from the
//          rollout's PCG64 stream, A = the first k with cdf_k > u (searchsorted side='right').  One draw per step.  The sums run in every
//          lane (the same values); lane k keeps c_k of its chunk of 64, so the divisions are one per lane.
//   pop    the head of segment b + A through perm and the cursor.  An empty segment: OFFSIM_ST_KEYERROR (queues[z, a] of a never-logged
//          pair); the cursor at its end: OFFSIM_ST_EXHAUSTED (queue_evaluator.py:125-126).  State and cursor stay in both cases.
// The action stream needs no per-lane position and no jump table: one LCG step per step of the rollout, and the state after the last draw
// is what the row holds on exit.
//
// Ties of the epsilon-greedy arg max: td.tie_mt as in k_eval_mc (NULL: first maximum; else the rollout's MT19937 stream), and with
// tie_reseed the stream is re-initialised at the start of episode e as np.random.seed(episode0 + e) does (tabular.py:114, :166):
// init_genrand, position 624.  The 624-word recurrence is serial, so it is run only when the stream is next needed (an epsilon-greedy
// step, or the write-back).
//
// LDS carve of a workgroup of `waves` rollouts (n = n_slots = nZ * nA):
//   [Q per wave (TD): waves * n f64][pi (when given): n f64][behaviour row per wave (TD): waves * nA f64][seg_off: n + 1 u32]
//   [cursors per wave: waves * n u32][tie stream per wave (TD): waves * 624 u32]
//
// Many learners per launch (offsim_eval_queue_pop): the POP instance below, arguments and index rules in csrc/td_pop.hpp.
//
// Included by offsim_hip.hip behind eval_exo.hpp: check_table, check_evalmc_out, check_td_pop, td_of_pop, td_behaviour, discount_at and
// allow_big_lds are that file's.
#pragma once

// init_genrand(seed) of MT19937 into the rollout's LDS copy; every lane runs the recurrence, lane i % 64 stores word i
__device__ __forceinline__ void mt_seed_lds(volatile uint32_t *mt, uint32_t seed, int lane) {
    uint32_t v = seed;
    for (int i = 0; i < 624; i++) {
        if (i) v = 1812433253u * (v ^ (v >> 30)) + (uint32_t)i;
        if ((i & (WAVE - 1)) == lane) mt[i] = v;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
}

// Generator.choice(nA, p=p) for the uniform u: nA when no cdf entry exceeds u (a row of NaN or zeros)
__device__ __forceinline__ int queue_draw(const double *p, int nA, double u, int lane) {
    double tot = 0.0;
    for (int k = 0; k < nA; k++) tot = tot + p[k];
    double c = 0.0;
    for (int base = 0; base < nA; base += WAVE) {
        const int n = nA - base < WAVE ? nA - base : WAVE;
        double mine = 0.0;
        for (int k = 0; k < n; k++) {
            c = c + p[base + k];
            if (k == lane) mine = c;
        }
        const uint64_t m = __ballot(lane < n && mine / tot > u);
        if (m) return base + __ffsll((unsigned long long)m) - 1;
    }
    return nA;
}

struct QueueArgs {
    int32_t tie_reseed;
    uint32_t episode0;
    int32_t *obs_row;
};

// POP = true (with TD): a population of L tabular learners on the same S seeds (offsim_eval_queue_pop; arguments and index rules in
// csrc/td_pop.hpp).  The instance overwrites its per-launch hyper-parameters -- td.alpha / epsilon / behaviour / the schedule rows,
// gamma, gamma_pow, pi -- with its workgroup's learner's before anything reads them; rollout r = l * S + j reads queue orders j.  The LDS
// carve is the learner carve above.  The POP instance takes its own argument struct, so the kernel arguments of the other two are what they were.
struct QueuePopArgs : QueueArgs, TdPopFields {};
static_assert(td_pop_layout<QueuePopArgs>(96, 16, 88), "kernel arguments of k_eval_queue<TD, POP>");
template <bool POP>
using QueueKernelArgs = std::conditional_t<POP, QueuePopArgs, QueueArgs>;

// The learner blocks around the step (POP prologue and index, tie stream, TD update, episode close, outputs) are written out in each of the three
// rollout kernels: called as shared inline functions they changed every instance's code (profiles/td_learner_one_definition/isa_compare.txt).
template <bool TD, bool POP = false>
__global__ void __launch_bounds__(256, 4) k_eval_queue(offsim_table t, offsim_rollouts ro, const double *__restrict__ pi, double gamma,
                                                    const double *__restrict__ gamma_pow, int64_t n_gamma_pow, int64_t max_episodes,
                                                    offsim_evalmc_out out, offsim_td td, QueueKernelArgs<POP> qa) {
    static_assert(!POP || TD, "a population is a population of learners");
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int waves = blockDim.x / WAVE;
    int pop_l = 0, pop_nb = 1;  // POP: this workgroup's learner, workgroups per learner
    if constexpr (POP) {
        pop_nb = (qa.S + waves - 1) / waves;
        pop_l = blockIdx.x / pop_nb;
        td.alpha = qa.alpha[pop_l];
        td.epsilon = qa.epsilon[pop_l];
        td.behaviour = qa.behaviour[pop_l];
        td.alpha_ep = qa.alpha_ep ? qa.alpha_ep + (int64_t)pop_l * td.n_sched : nullptr;
        td.epsilon_ep = qa.epsilon_ep ? qa.epsilon_ep + (int64_t)pop_l * td.n_sched : nullptr;
        gamma = qa.gamma[pop_l];
        gamma_pow = qa.gamma_pow + (int64_t)pop_l * n_gamma_pow;
        pi = qa.pi ? qa.pi + (int64_t)pop_l * qa.pi_stride : nullptr;
    }
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE), lane = threadIdx.x & (WAVE - 1);  // uniform -> SGPR
    const int n = t.n_slots, nA = t.nA;
    double *q_lds = (double *)lds_raw + (TD ? (size_t)wave * n : 0);
    double *pi_lds = (double *)lds_raw + (TD ? (size_t)waves * n : 0);
    double *beh_lds = pi_lds + (pi ? (size_t)n : 0) + (TD ? (size_t)wave * nA : 0);
    uint32_t *seg_lds = (uint32_t *)(pi_lds + (pi ? (size_t)n : 0) + (TD ? (size_t)waves * nA : 0));
    uint32_t *cur_lds = seg_lds + (n + 1) + (size_t)wave * n;
    volatile uint32_t *mt_lds = (volatile uint32_t *)(seg_lds + (n + 1) + (size_t)waves * n) + (TD ? (size_t)wave * 624 : 0);
    if (pi)
        for (int i = threadIdx.x; i < n; i += blockDim.x) pi_lds[i] = pi[i];
    for (int i = threadIdx.x; i <= n; i += blockDim.x) seg_lds[i] = t.seg_off[i];
    __syncthreads();
    int r = blockIdx.x * waves + wave;
    int ord = r;  // POP: the queue orders rollout r walks
    if constexpr (POP) {
        ord = __builtin_amdgcn_readfirstlane((blockIdx.x - pop_l * pop_nb) * waves + wave);
        if (ord >= qa.S) return;
        r = __builtin_amdgcn_readfirstlane(pop_l * qa.S + ord);
    } else {
        if (r >= ro.R) return;
    }
    uint32_t *cur_glb = ro.cursor + (int64_t)r * n;
    for (int s = lane; s < n; s += WAVE) cur_lds[s] = cur_glb[s];
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
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): cursors, Q and the tie stream visible to the whole wave

    const uint32_t *perm_row = ro.perm ? ro.perm + (int64_t)(POP ? ord : r) * ro.perm_stride : nullptr;
    const uint32_t *init_row = ro.init_perm ? ro.init_perm + (int64_t)(POP ? ord : r) * ro.init_stride : nullptr;
    uint32_t ic = ro.init_cursor[r];
    int b = __builtin_amdgcn_readfirstlane(ro.cur_slot[r]);  // base slot z * nA of the current state
    int64_t ep = 0, n_len = 0, steps = 0;
    uint64_t consumed = 0;
    double sum_g = 0.0;
    int status = OFFSIM_ST_OK;
    bool terminate = false, no_init = false, mt_pending = false;
    uint32_t mt_seed = 0u;
    int32_t g_prev = -1;
    uint32_t k_init = 0;
    while (ep < max_episodes && !terminate) {
        if (TD && qa.tie_reseed) {  // np.random.seed(episode), tabular.py:114 / :166 -- before env.reset
            mt_pending = true;
            mt_seed = qa.episode0 + (uint32_t)ep;
        }
        // env.reset()  (queue_evaluator.py:113-119)
        if ((int64_t)ic >= t.N0) {
            status = OFFSIM_ST_NO_INIT;
            b = -1;
            no_init = true;
            break;
        }
        const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane((int)(init_row ? init_row[ic] : ic));
        ic++;
        b = __builtin_amdgcn_readfirstlane(t.init_slot[k]);
        g_prev = -1;
        k_init = k;
        double G = 0.0;
        int64_t tt = 0;
        bool done = false;
        while (!done) {
            const double gp = discount_at(gamma_pow, (uint64_t)n_gamma_pow, gamma, (uint64_t)tt);  // issued ahead of the step
            if (b < 0 || b + nA > n) {  // a state outside the table: queues[z, a] raises KeyError
                status = OFFSIM_ST_KEYERROR;
                terminate = true;
                break;
            }
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
            if (A >= nA) {  // no action drawn (p of NaN or zeros): queues[z, nA] has no queue
                status = OFFSIM_ST_KEYERROR;
                terminate = true;
                break;
            }
            // env.step(A)  (queue_evaluator.py:121-131)
            const int slot = b + A;
            const uint32_t beg = seg_lds[slot], len = seg_lds[slot + 1] - beg;
            if (len == 0) {  // (z, A) never logged: self.queues[z, a] raises KeyError
                status = OFFSIM_ST_KEYERROR;
                terminate = true;
                break;
            }
            const uint32_t cur = (uint32_t)__builtin_amdgcn_readfirstlane((int)cur_lds[slot]);
            if (cur >= len) {  // :125-126 (None): the state stays
                status = OFFSIM_ST_EXHAUSTED;
                terminate = true;
                break;
            }
            uint32_t gl = beg + cur;
            if (perm_row) gl = perm_row[gl];
            const int g = __builtin_amdgcn_readfirstlane((int)gl);
            const double rew = t.r_dtype == OFFSIM_F64 ? ((const double *)t.r)[g] : (double)((const float *)t.r)[g];
            const int b_next = __builtin_amdgcn_readfirstlane(t.z_next[g]);
            const bool dn = t.done[g] != 0;
            if (lane == 0) cur_lds[slot] = cur + 1u;
            g_prev = g;
            if (TD) {  // tabular.py:123-126 (Q-learning) / :175-178 (expected SARSA) on Q[z, A] with Q[z']; every lane computes the same update
                if (b_next < 0 || b_next + nA > n) {  // Q[S'] has no row: the environment has stepped, the learner raises
                    b = b_next;
                    status = OFFSIM_ST_KEYERROR;
                    terminate = true;
                    break;
                }
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
            if (lane == 0 && out.trace_row && steps < out.trace_cap) out.trace_row[(int64_t)r * out.trace_cap + steps] = t.orig_idx[g];
            G = G + gp * rew;  // tabular.py:129 (no FMA contraction: built with -ffp-contract=off)
            tt++;
            steps++;
            b = b_next;
            done = dn;
        }
        if (status == OFFSIM_ST_KEYERROR) break;  // the reference raises out of the driver here
        if (lane == 0 && out.ep_len && n_len <= out.ep_cap) out.ep_len[(int64_t)r * (out.ep_cap + 1) + n_len] = (int32_t)tt;
        n_len++;
        if (done) {
            if (lane == 0 && out.ep_g && ep < out.ep_cap) out.ep_g[(int64_t)r * out.ep_cap + ep] = G;
            sum_g += G;
            ep++;
        } else if (lane == 0 && out.ep_g && ep < out.ep_cap) {
            // return of the episode cut short by exhaustion (the reference's drivers do not survive it; the *_psrs drivers' rule:
            // evalMC drops it, the learner drivers append it): stored past the n_ep completed ones
            out.ep_g[(int64_t)r * out.ep_cap + ep] = G;
        }
    }
    // write back the env state so that a later call continues where this one stopped
    if (TD && mt_pending && td.tie_mt) {
        mt_seed_lds(mt_lds, mt_seed, lane);
        mt_pos = 624u;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    for (int s = lane; s < n; s += WAVE) cur_glb[s] = cur_lds[s];
    if (TD) {
        for (int i = lane; i < n; i += WAVE) td.q[(int64_t)r * n + i] = q_lds[i];
        if (td.tie_mt) {
            for (int i = lane; i < 624; i += WAVE) td.tie_mt[(int64_t)r * 625 + i] = mt_lds[i];
            if (lane == 0) td.tie_mt[(int64_t)r * 625 + 624] = mt_pos;
        }
    }
    if (lane == 0) {
        ro.init_cursor[r] = ic;
        ro.cur_slot[r] = b;
        if (qa.obs_row) {  // env.s: the convention of offsim_eval_mc_rows_policy (left as the caller filled it when the loop ran no reset)
            if (no_init) qa.obs_row[r] = -1;
            else if (n_len > 0 || g_prev >= 0 || status != OFFSIM_ST_OK) qa.obs_row[r] = g_prev >= 0 ? t.orig_idx[g_prev] : -2 - t.init_orig[k_init];
        }
        if (consumed) {  // the state after the last draw
            ro.rng[4 * r + 0] = st.hi;
            ro.rng[4 * r + 1] = st.lo;
        }
        out.sum_g[r] = sum_g;
        out.n_ep[r] = ep;
        out.steps[r] = steps;
        out.cand[r] = steps;  // one row popped per step
        out.n_len[r] = n_len;
        out.status[r] = status;
    }
}

static size_t queue_lds_bytes(int waves, int64_t n, int64_t nA, bool have_pi, bool td) {
    return (td ? (size_t)waves * n * 8 : 0) + (have_pi ? (size_t)n * 8 : 0) + (td ? (size_t)waves * nA * 8 : 0) + (size_t)(n + 1) * 4 +
           (size_t)waves * n * 4 + (td ? (size_t)waves * 624 * 4 : 0);
}

template <bool TD, bool POP = false>
static int queue_launch(const offsim_table *t, offsim_rollouts *ro, const double *pi, double gamma, const double *gamma_pow, int64_t n_gamma_pow,
                        int64_t max_episodes, const offsim_evalmc_out *out, const offsim_td &td, const QueueKernelArgs<POP> &qa, int waves, size_t lds,
                        void *stream) {
    if (lds > 64 * 1024) HIP_TRY(allow_big_lds((k_eval_queue<TD, POP>), (int)lds));
    unsigned grid = (unsigned)((ro->R + waves - 1) / waves);
    if constexpr (POP) grid = pop_grid(ro->R, qa.S, waves);
    hipLaunchKernelGGL((k_eval_queue<TD, POP>), dim3(grid), dim3(waves * WAVE), lds, (hipStream_t)stream, *t, *ro, pi, gamma, gamma_pow, n_gamma_pow,
                       max_episodes, *out, td, qa);
    LAUNCH_CHECK();
    return OFFSIM_OK;
}

// the table rules of every queue entry point (also offsim_queue_collect's, csrc/collect_queue.hpp): the table and its key, ro, the action
// stream's provider
static int queue_check_table(const char *who, const offsim_table *t, const offsim_rollouts *ro, int32_t nA_actions) {
    int rc = check_table(t);
    if (rc) return rc;
    if (t->N0 > 0 && (!t->init_slot || !t->init_orig)) return fail(OFFSIM_EINVAL, "%s: table without its init rows", who);
    if (!ro || ro->R < 0) return fail(OFFSIM_EINVAL, "%s: ro is NULL or R < 0", who);
    if (ro->R > 0 && (!ro->rng || !ro->cursor || !ro->init_cursor || !ro->cur_slot)) return fail(OFFSIM_EINVAL, "%s: NULL rollout state", who);
    if (nA_actions <= 0 || t->nA != nA_actions) return fail(OFFSIM_EINVAL, "%s: nA_actions is not the table's nA", who);
    if (t->n_slots % nA_actions != 0) return fail(OFFSIM_EINVAL, "%s: n_slots is no multiple of nA (the table is not keyed by z * nA + a)", who);
    if (ro->rng_kind == OFFSIM_STREAM_PHILOX)
        return fail(OFFSIM_EUNSUPPORTED, "%s: the action stream must be OFFSIM_STREAM_PCG64 (a Philox double lies in (0, 1]: u = 1.0 selects action nA)", who);
    if (ro->rng_kind != OFFSIM_STREAM_PCG64) return fail(OFFSIM_EINVAL, "%s: unknown stream provider", who);
    return OFFSIM_OK;
}

// what offsim_eval_queue and offsim_eval_queue_pop check alike, in offsim_eval_queue's order: the table rules, out, the capacities, the
// learner (td; NULL: evalMC) and the tie mode ...
static int queue_check(const char *who, const offsim_table *t, const offsim_rollouts *ro, int32_t nA_actions, const double *gamma_pow,
                       int64_t n_gamma_pow, const offsim_evalmc_out *out, const offsim_td *td, int32_t tie_reseed_episode, int64_t episode0) {
    int rc = queue_check_table(who, t, ro, nA_actions);
    if (rc) return rc;
    if (!out) return fail(OFFSIM_EINVAL, "%s: out is NULL", who);
    if ((rc = check_evalmc_out(who, out, gamma_pow, n_gamma_pow))) return rc;
    if (out->ep_cap < 0 || out->trace_cap < 0) return fail(OFFSIM_EINVAL, "%s: negative ep_cap / trace_cap", who);
    if (tie_reseed_episode != 0 && tie_reseed_episode != 1) return fail(OFFSIM_EINVAL, "%s: tie_reseed_episode is 0 or 1", who);
    if (td) {
        if ((rc = check_td(who, td, TD_RULES))) return rc;
        if (tie_reseed_episode && (!td->tie_mt || episode0 < 0))
            return fail(OFFSIM_EINVAL, "%s: tie_reseed_episode needs td->tie_mt (the stream is written back there) and episode0 >= 0", who);
    } else if (tie_reseed_episode) {
        return fail(OFFSIM_EINVAL, "%s: tie_reseed_episode without a learner", who);
    }
    return OFFSIM_OK;
}

// ... and the launch shape (launch_shape) of the carve above; beyond 160 KiB: refused
static int queue_launch_shape(const char *who, const offsim_table *t, bool have_pi, bool td, int *waves_out, size_t *lds_out) {
    if (t->n_slots > 40960) return fail(OFFSIM_EUNSUPPORTED, "%s: cursors, policy and Q table exceed 160 KiB of LDS", who);  // (keeps the sums in range)
    if (!launch_shape([&](int w) { return queue_lds_bytes(w, t->n_slots, t->nA, have_pi, td); }, waves_out, lds_out))
        return fail(OFFSIM_EUNSUPPORTED, "%s: cursors, policy and Q table exceed 160 KiB of LDS", who);
    return OFFSIM_OK;
}

extern "C" int offsim_eval_queue(const offsim_table *t, offsim_rollouts *ro, int32_t nA_actions, const double *pi, double gamma,
                                 const double *gamma_pow, int64_t n_gamma_pow, int64_t max_episodes, const offsim_evalmc_out *out,
                                 const offsim_td *td, int32_t tie_reseed_episode, int64_t episode0, int32_t *out_obs_row, void *stream) {
    static const char *who = "eval_queue";
    int rc = queue_check(who, t, ro, nA_actions, gamma_pow, n_gamma_pow, out, td, tie_reseed_episode, episode0);
    if (rc) return rc;
    if (!pi && !(td && td->behaviour != OFFSIM_BEHAVIOUR_FIXED && td->mode == OFFSIM_TD_QLEARN))
        return fail(OFFSIM_EINVAL, "%s: pi is NULL (only Q-learning with a behaviour on the learner's own Q runs without one)", who);
    int waves = 0;
    size_t lds = 0;
    if ((rc = queue_launch_shape(who, t, pi != nullptr, td != nullptr, &waves, &lds))) return rc;
    if (ro->R == 0) return OFFSIM_OK;
    offsim_td tdv;
    memset(&tdv, 0, sizeof(tdv));
    if (td) tdv = *td;
    const QueueArgs qa{tie_reseed_episode, (uint32_t)episode0, out_obs_row};
    if (td) return queue_launch<true>(t, ro, pi, gamma, gamma_pow, n_gamma_pow, max_episodes, out, tdv, qa, waves, lds, stream);
    return queue_launch<false>(t, ro, pi, gamma, gamma_pow, n_gamma_pow, max_episodes, out, tdv, qa, waves, lds, stream);
}

// ---- offsim_eval_queue's learner drivers for L learners on the same S seeds in one launch (k_eval_queue<TD, POP>, csrc/td_pop.hpp): every
// learner has its own hyper-parameters, behaviour and target policy; the queue orders are the seeds', shared by all learners and only read.
extern "C" int offsim_eval_queue_pop(const offsim_table *t, offsim_rollouts *ro, int32_t nA_actions, int32_t L, int32_t S, const offsim_td_pop *pop,
                                     int64_t max_episodes, const offsim_evalmc_out *out, int32_t tie_reseed_episode, int64_t episode0,
                                     int32_t *out_obs_row, void *stream) {
    static const char *who = "eval_queue_pop";
    if (!pop) return fail(OFFSIM_EINVAL, "%s: pop is NULL", who);
    const offsim_td td = td_of_pop(pop);
    int rc = queue_check(who, t, ro, nA_actions, pop->gamma_pow, pop->n_gamma_pow, out, &td, tie_reseed_episode, episode0);
    if (rc || (rc = check_td_pop(who, L, S, ro->R, pop, true))) return rc;
    if (!pop->pi) {  // (behaviour_host has been validated)
        bool fixed = false;
        for (int32_t l = 0; l < L; l++) fixed = fixed || pop->behaviour_host[l] == OFFSIM_BEHAVIOUR_FIXED;
        if (fixed || pop->mode != OFFSIM_TD_QLEARN)
            return fail(OFFSIM_EINVAL, "%s: pi is NULL (only Q-learning with a behaviour on every learner's own Q runs without one)", who);
    }
    int waves = 0;
    size_t lds = 0;
    if ((rc = queue_launch_shape(who, t, pop->pi != nullptr, true, &waves, &lds))) return rc;
    if (ro->R == 0) return OFFSIM_OK;
    const QueuePopArgs qa{QueueArgs{tie_reseed_episode, (uint32_t)episode0, out_obs_row}, td_pop_fields(pop, S)};
    return queue_launch<true, true>(t, ro, nullptr, 0.0, nullptr, pop->n_gamma_pow, max_episodes, out, td, qa, waves, lds, stream);
}
