// eval_exo.hpp -- whole rollouts on PSRS_Exo (offsim4rl/evaluators/psrs.py:59-117) under the reference's three drivers, evalMC_psrs,
// qlearn_psrs and expSARSA_psrs (psrs.py:119-271), many rollouts per launch: offsim_eval_mc_exo (include/offsim.h).
//
// The loop is k_eval_mc's (one wavefront per rollout, the same episode bookkeeping, TD update, outputs and status codes); the step is
// the two-cursor candidate round of k_step_exo (lane k tests candidate k of s_queues[s] and x_queues[x] with draw c + k); the policy and
// Q are indexed by the OBSERVATION o = o_combine_func(s, x) (psrs.py:255, :158, :214), tabulated by the host as obs_of [ns_slots, nx_slots].
//
// LDS carve of a workgroup of `waves` rollouts:
//   [jump tables: waves * 65 Jump][Q per wave (TD): waves * n_obs * nA f64][pi: n_obs * nA PROB][obs_of: ns * nx i32]
//   [seg_off of s: ns + 1][seg_off of x: nx + 1][cursors of s per wave: waves * ns][cursors of x per wave: waves * nx]
//
// The rejection stream (`reseed`):
//   OFFSIM_EXO_RESEED_EPISODE  PSRS_Exo.reset(seed) restarts the stream (psrs.py:92) and the drivers call env.reset(seed=episode), so
//                              episode e of every rollout draws from default_rng(episode0 + e): pcg_seed at every reset -- BEFORE the
//                              init queue is looked at, as the reference does -- and the per-wave jump table rebuilt for the new increment.
//                              PCG64 only.
//   OFFSIM_EXO_RESEED_NONE     the rollout's own stream (rs.rng, either provider) runs on across episodes.
//
// The epsilon-greedy / soft-greedy behaviour policies of k_eval_mc and their tie stream (the learner acts on its own Q row) are the POP
// instances' (offsim_eval_td_exo_pop, a population of L >= 1 learners; below): offsim_eval_mc_exo keeps returning OFFSIM_EUNSUPPORTED for
// them.  Not here, deliberately: the reject modes other than the default rule.
//
// Included by offsim_hip.hip behind offsim_eval_td: check_table, check_prob_mode, check_evalmc_out, with_plog_prob, rejects_f64 / _f32,
// WaveRng, wave_rng_init and allow_big_lds are that file's.
#pragma once

struct ExoArgs {
    const int32_t *obs_of;
    int32_t n_obs, reseed;
    uint64_t episode0;
    offsim_exo_out xout;
};

// POP = true (with TD): a population of L tabular learners on the same S seeds, every one acting on its own Q (offsim_eval_td_exo_pop;
// arguments and index rule in csrc/td_pop.hpp).  The instance overwrites its per-launch hyper-parameters -- td.alpha / epsilon /
// behaviour / the schedule rows, gamma, gamma_pow, pi -- with its workgroup's learner's before anything reads them, and before every step
// rebuilds the behaviour distribution from the Q row of the current observation (td_behaviour, the block k_eval_mc calls) in beh_lds,
// which the step then rejects against.  LDS: the carve above, then -- behind the x-cursors, so that every offset above stays --
//   [beh_lds per wave: waves * nA f64, 8-byte aligned][tie stream per wave: waves * 624 u32]
// The POP instances take their own argument struct, so the kernel arguments of every other instance are what they were.
struct TdPopExoArgs : ExoArgs, TdPopFields {};
static_assert(td_pop_layout<TdPopExoArgs>(120, 40, 112), "kernel arguments of k_eval_mc_exo<.., TD, POP>");
template <bool POP>
using ExoKernelArgs = std::conditional_t<POP, TdPopExoArgs, ExoArgs>;

// The learner blocks around the step (POP prologue and index, tie stream, TD update, episode close, outputs) are written out in each of the three
// rollout kernels: called as shared inline functions they changed every instance's code (profiles/td_learner_one_definition/isa_compare.txt).
template <typename PL, typename PROB, bool TD, bool POP = false>
__global__ void __launch_bounds__(256, 4) k_eval_mc_exo(offsim_table ts, offsim_table tx, offsim_rollouts rs, offsim_rollouts rx,
                                                     const PROB *__restrict__ pi, ExoKernelArgs<POP> xa, double gamma,
                                                     const double *__restrict__ gamma_pow, int64_t n_gamma_pow, int64_t max_episodes,
                                                     offsim_evalmc_out out, offsim_td td) {
    static_assert(!POP || (TD && sizeof(PROB) == 8), "a population is a population of learners (f64 pi)");
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int waves = blockDim.x / WAVE;
    int pop_l = 0, pop_nb = 1;  // POP: this workgroup's learner, workgroups per learner
    if constexpr (POP) {
        pop_nb = (xa.S + waves - 1) / waves;
        pop_l = blockIdx.x / pop_nb;
        td.alpha = xa.alpha[pop_l];
        td.epsilon = xa.epsilon[pop_l];
        td.behaviour = xa.behaviour[pop_l];
        td.alpha_ep = xa.alpha_ep ? xa.alpha_ep + (int64_t)pop_l * td.n_sched : nullptr;
        td.epsilon_ep = xa.epsilon_ep ? xa.epsilon_ep + (int64_t)pop_l * td.n_sched : nullptr;
        gamma = xa.gamma[pop_l];
        gamma_pow = xa.gamma_pow + (int64_t)pop_l * n_gamma_pow;
        pi = (const PROB *)xa.pi + (int64_t)pop_l * xa.pi_stride;
    }
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE), lane = threadIdx.x & (WAVE - 1);  // uniform -> SGPR
    const int ns = ts.n_slots, nx = tx.n_slots, nA = ts.nA, n_obs = xa.n_obs;
    Jump *tables = (Jump *)lds_raw;
    double *q_lds = (double *)(tables + waves * (WAVE + 1)) + (TD ? (size_t)wave * n_obs * nA : 0);
    PROB *pi_lds = (PROB *)((double *)(tables + waves * (WAVE + 1)) + (TD ? (size_t)waves * n_obs * nA : 0));
    int32_t *obs_lds = (int32_t *)(pi_lds + (size_t)n_obs * nA);
    uint32_t *seg_s = (uint32_t *)(obs_lds + (size_t)ns * nx);
    uint32_t *seg_x = seg_s + (ns + 1);
    uint32_t *cur_s = seg_x + (nx + 1) + (size_t)wave * ns;
    uint32_t *cur_x = seg_x + (nx + 1) + (size_t)waves * ns + (size_t)wave * nx;
    // POP: this rollout's action distribution at its current observation, and its copy of the tie-breaking MT19937 stream (624 words; the
    // position is kept in a register)
    double *beh_all = (double *)(((uintptr_t)(seg_x + (nx + 1) + (size_t)waves * (ns + nx)) + 7) & ~(uintptr_t)7);
    double *beh_lds = beh_all + (size_t)wave * nA;
    volatile uint32_t *mt_lds = (volatile uint32_t *)(beh_all + (size_t)waves * nA) + (size_t)wave * 624;
    for (int i = threadIdx.x; i < n_obs * nA; i += blockDim.x) pi_lds[i] = pi[i];
    for (int i = threadIdx.x; i < ns * nx; i += blockDim.x) obs_lds[i] = xa.obs_of[i];
    for (int i = threadIdx.x; i <= ns; i += blockDim.x) seg_s[i] = ts.seg_off[i];
    for (int i = threadIdx.x; i <= nx; i += blockDim.x) seg_x[i] = tx.seg_off[i];
    __syncthreads();
    int r = blockIdx.x * waves + wave;
    int ord = r;  // POP: the queue orders rollout r walks
    if constexpr (POP) {
        ord = __builtin_amdgcn_readfirstlane((blockIdx.x - pop_l * pop_nb) * waves + wave);
        if (ord >= xa.S) return;
        r = pop_l * xa.S + ord;
    } else {
        if (r >= rs.R) return;
    }
    uint32_t *cur_s_glb = rs.cursor + (int64_t)r * ns, *cur_x_glb = rx.cursor + (int64_t)r * nx;
    for (int i = lane; i < ns; i += WAVE) cur_s[i] = cur_s_glb[i];
    for (int i = lane; i < nx; i += WAVE) cur_x[i] = cur_x_glb[i];
    if (TD)
        for (int i = lane; i < n_obs * nA; i += WAVE) q_lds[i] = td.q[(int64_t)r * n_obs * nA + i];
    uint32_t mt_pos = 624u;
    if constexpr (POP) {
        if (td.tie_mt) {
            for (int i = lane; i < 624; i += WAVE) mt_lds[i] = td.tie_mt[(int64_t)r * 625 + i];
            mt_pos = td.tie_mt[(int64_t)r * 625 + 624];
        }
    }

    const bool per_episode = xa.reseed == OFFSIM_EXO_RESEED_EPISODE;
    const int kind = per_episode ? OFFSIM_STREAM_PCG64 : rs.rng_kind;
    Jump *table = tables + wave * (WAVE + 1);
    WaveRng rng;
    U128 base = stream_row_base(rs.rng, r), inc = stream_row_inc(rs.rng, r);
    rng.lane_state = base;
    wave_rng_init(rng, table, base, inc, kind);  // (per episode: filled again at every reset)
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): table, cursors and Q visible to the whole wave

    const uint32_t *perm_s = rs.perm ? rs.perm + (int64_t)(POP ? ord : r) * rs.perm_stride : nullptr;
    const uint32_t *perm_x = rx.perm ? rx.perm + (int64_t)(POP ? ord : r) * rx.perm_stride : nullptr;
    const uint32_t *init_row = rs.init_perm ? rs.init_perm + (int64_t)(POP ? ord : r) * rs.init_stride : nullptr;
    const PL *plog = (const PL *)ts.p_log;
    uint32_t ic = rs.init_cursor[r];
    int ss = __builtin_amdgcn_readfirstlane(rs.cur_slot[r]), xs = __builtin_amdgcn_readfirstlane(rx.cur_slot[r]);
    int64_t ep = 0, n_len = 0, steps = 0, cand = 0;
    uint64_t consumed = 0;
    double sum_g = 0.0;
    int status = OFFSIM_ST_OK;
    bool terminate = false, reseeded = false, have_last = false;
    int32_t last_s = -1, last_x = -1, last_init = -1;
    while (ep < max_episodes && !terminate) {
        // env.reset(seed=episode)  (psrs.py:91-97, :249-252)
        if (per_episode) {  // :92, before the init queue is looked at
            const PcgInit p = pcg_seed(xa.episode0 + (uint64_t)ep);
            base = p.state;
            inc = p.inc;
            consumed = 0;
            reseeded = true;
            __builtin_amdgcn_s_waitcnt(0xc07f);  // (the last step's table reads are done)
            wave_rng_init(rng, table, base, inc, OFFSIM_STREAM_PCG64);
            __builtin_amdgcn_s_waitcnt(0xc07f);
        }
        if ((int64_t)ic >= ts.N0) {
            status = OFFSIM_ST_NO_INIT;
            ss = xs = -1;
            break;
        }
        const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane((int)(init_row ? init_row[ic] : ic));
        ic++;
        ss = __builtin_amdgcn_readfirstlane(ts.init_slot[k]);
        xs = __builtin_amdgcn_readfirstlane(tx.init_slot[k]);
        have_last = true;
        last_s = last_x = -1;
        last_init = ts.init_orig[k];
        double G = 0.0;
        int64_t tt = 0;
        bool done = false;
        while (!done) {
            const double gp = discount_at(gamma_pow, (uint64_t)n_gamma_pow, gamma, (uint64_t)tt);  // issued ahead of the step
            // p = pi[S] with S = o_combine_func(s, x) (psrs.py:255 / :214), then env.step(p) (:99-117)
            if (ss < 0 || ss >= ns || xs < 0 || xs >= nx) {
                status = OFFSIM_ST_KEYERROR;
                terminate = true;
                break;
            }
            const int o_cur = __builtin_amdgcn_readfirstlane(obs_lds[ss * nx + xs]);
            const uint32_t beg_s = seg_s[ss], len_s = seg_s[ss + 1] - beg_s;
            const uint32_t beg_x = seg_x[xs], len_x = seg_x[xs + 1] - beg_x;
            if ((unsigned)o_cur >= (unsigned)n_obs || (!POP && (len_s == 0 || len_x == 0))) {  // pi has no row (IndexError) / a queue is missing (KeyError)
                status = OFFSIM_ST_KEYERROR;
                terminate = true;
                break;
            }
            const PROB *pn = pi_lds + (size_t)o_cur * nA;
            if constexpr (POP) {
                // p = behavior_policy(Q[[S], :], ...) (psrs.py:158) comes BEFORE env.step: a step that finds a queue missing has drawn its tie
                if (td.behaviour != OFFSIM_BEHAVIOUR_FIXED) {
                    td_behaviour(td, q_lds + (size_t)o_cur * nA, nA, beh_lds, mt_lds, mt_pos, lane, r, ep, steps);
                    pn = (const PROB *)beh_lds;
                }
                if (len_s == 0 || len_x == 0) {
                    status = OFFSIM_ST_KEYERROR;
                    terminate = true;
                    break;
                }
            }
            uint32_t cs = (uint32_t)__builtin_amdgcn_readfirstlane((int)cur_s[ss]), cx = (uint32_t)__builtin_amdgcn_readfirstlane((int)cur_x[xs]);
            uint32_t popped = 0;
            int gsf = -1, gxf = -1;
            for (;;) {
                const uint32_t rem_s = len_s - cs, rem_x = len_x - cx;
                const uint32_t rem = rem_s < rem_x ? rem_s : rem_x;
                if (rem == 0) break;  // psrs.py:104-107
                const uint32_t nv = rem < WAVE ? rem : WAVE;
                const bool valid = (uint32_t)lane < nv;
                uint32_t gs = beg_s + cs + (valid ? lane : 0), gx = beg_x + cx + (valid ? lane : 0);
                if (perm_s) gs = perm_s[gs];
                if (perm_x) gx = perm_x[gx];
                const int a = ts.a[gs];
                const uint64_t k53 = kind == OFFSIM_STREAM_PHILOX ? philox_k53(rng.seed, rng.c + (uint64_t)lane) : pcg_output(rng.lane_state) >> 11;
                bool rej;
                if constexpr (sizeof(PROB) == 4) rej = rejects_f32((const float *)plog, (int64_t)gs, a, (const float *)pn, nA, k53);
                else rej = rejects_f64<PL>(plog, (int64_t)gs, a, (const double *)pn, nA, k53);
                const uint64_t m = __ballot(valid && !rej);
                const int f = m ? __ffsll((unsigned long long)m) - 1 : -1;
                const uint32_t d = f < 0 ? nv : (uint32_t)f + 1;
                cs += d;
                cx += d;
                popped += d;
                consumed += d;
                if (kind == OFFSIM_STREAM_PHILOX) rng.c += d;
                else rng.lane_state = pcg_apply(rng.table[d], rng.lane_state);
                if (f >= 0) {
                    gsf = __builtin_amdgcn_readlane((int)gs, f);
                    gxf = __builtin_amdgcn_readlane((int)gx, f);
                    break;
                }
            }
            if (lane == 0) {
                cur_s[ss] = cs;
                cur_x[xs] = cx;
            }
            cand += popped;
            if (gsf < 0) {  // :104-107 (None): the state stays
                status = OFFSIM_ST_EXHAUSTED;
                terminate = true;
                break;
            }
            // the accepted s-row gives (a, r, s', done), the x-row popped with it gives x' (psrs.py:108-117)
            const int A = ts.a[gsf];
            const double rew = ts.r_dtype == OFFSIM_F64 ? ((const double *)ts.r)[gsf] : (double)((const float *)ts.r)[gsf];
            const int ss_next = __builtin_amdgcn_readfirstlane(ts.z_next[gsf]), xs_next = __builtin_amdgcn_readfirstlane(tx.z_next[gxf]);
            const bool dn = ts.done[gsf] != 0;
            last_s = ts.orig_idx[gsf];
            last_x = tx.orig_idx[gxf];
            last_init = -1;
            if (TD) {  // psrs.py:165-168 (Q-learning) / :223 (expected SARSA) at S = o, S' = o_combine_func(s', x'); every lane computes the same update
                int o_next = -1;
                if (ss_next >= 0 && ss_next < ns && xs_next >= 0 && xs_next < nx) o_next = __builtin_amdgcn_readfirstlane(obs_lds[ss_next * nx + xs_next]);
                if ((unsigned)o_next >= (unsigned)n_obs) {  // Q[S'] has no row: the environment has stepped, the learner raises (IndexError)
                    ss = ss_next;
                    xs = xs_next;
                    status = OFFSIM_ST_KEYERROR;
                    terminate = true;
                    break;
                }
                const double q_sa = q_lds[o_cur * nA + A];
                const double *qn = q_lds + (size_t)o_next * nA;
                double nxt;
                if (td.mode == OFFSIM_TD_QLEARN) {
                    nxt = qn[0];
                    for (int k2 = 1; k2 < nA; k2++) nxt = qn[k2] > nxt ? qn[k2] : nxt;
                } else {  // Q[S_] @ pi[S_], left to right
                    const PROB *pn2 = pi_lds + (size_t)o_next * nA;
                    nxt = 0.0;
                    for (int k2 = 0; k2 < nA; k2++) nxt = nxt + qn[k2] * (double)pn2[k2];
                }
                const double td_err = rew + gamma * nxt - q_sa;
                if (lane == 0 && td.td_err && steps < td.td_cap) td.td_err[(int64_t)r * td.td_cap + steps] = td_err;
                const double alpha = td.alpha_ep ? td.alpha_ep[ep < td.n_sched ? ep : td.n_sched - 1] : td.alpha;  // alpha(episode), psrs.py:168
                __builtin_amdgcn_s_waitcnt(0xc07f);
                q_lds[o_cur * nA + A] = q_sa + alpha * td_err;
                if (td.q_snap && steps % td.snap_stride == 0 && steps / td.snap_stride < td.snap_cap) {  // save_Q (psrs.py:172-173)
                    __builtin_amdgcn_s_waitcnt(0xc07f);
                    double *dst = td.q_snap + ((int64_t)r * td.snap_cap + steps / td.snap_stride) * n_obs * nA;
                    for (int i = lane; i < n_obs * nA; i += WAVE) dst[i] = q_lds[i];
                }
            }
            if (lane == 0 && steps < out.trace_cap) {
                if (out.trace_row) out.trace_row[(int64_t)r * out.trace_cap + steps] = last_s;
                if (xa.xout.trace_row_x) xa.xout.trace_row_x[(int64_t)r * out.trace_cap + steps] = last_x;
                if (out.trace_pop) out.trace_pop[(int64_t)r * out.trace_cap + steps] = popped;
            }
            G = G + gp * rew;  // :262 (no FMA contraction: built with -ffp-contract=off)
            tt++;
            steps++;
            ss = ss_next;
            xs = xs_next;
            done = dn;
        }
        if (status == OFFSIM_ST_KEYERROR) break;  // the reference raises out of the driver here
        if (lane == 0 && out.ep_len && n_len <= out.ep_cap) out.ep_len[(int64_t)r * (out.ep_cap + 1) + n_len] = (int32_t)tt;
        n_len++;  // :265 lengths.append(t) always
        if (done) {  // :266-269
            if (lane == 0 && out.ep_g && ep < out.ep_cap) out.ep_g[(int64_t)r * out.ep_cap + ep] = G;
            sum_g += G;
            ep++;
        } else if (lane == 0 && out.ep_g && ep < out.ep_cap) {
            // return of the episode cut short by exhaustion: evalMC_psrs drops it (:266), the learner drivers append it (:177, :232);
            // stored past the n_ep completed ones
            out.ep_g[(int64_t)r * out.ep_cap + ep] = G;
        }
    }
    // write back the env state so that a later call (or offsim_step_exo) continues where this one stopped
    __builtin_amdgcn_s_waitcnt(0xc07f);
    for (int i = lane; i < ns; i += WAVE) cur_s_glb[i] = cur_s[i];
    for (int i = lane; i < nx; i += WAVE) cur_x_glb[i] = cur_x[i];
    if (TD)
        for (int i = lane; i < n_obs * nA; i += WAVE) td.q[(int64_t)r * n_obs * nA + i] = q_lds[i];
    if constexpr (POP) {
        if (td.tie_mt) {
            for (int i = lane; i < 624; i += WAVE) td.tie_mt[(int64_t)r * 625 + i] = mt_lds[i];
            if (lane == 0) td.tie_mt[(int64_t)r * 625 + 624] = mt_pos;
        }
    }
    if (lane == 0) {
        rs.init_cursor[r] = ic;
        rx.init_cursor[r] = ic;  // (both families pop the same initial row: a later PSRS_Exo.reset finds them in step)
        rs.cur_slot[r] = ss;
        rx.cur_slot[r] = xs;
        if (per_episode) {
            if (reseeded) {  // the state after the last draw of the last episode's stream
                const U128 nb = pcg_apply(pcg_jump(inc, consumed), base);
                rs.rng[4 * r + 0] = nb.hi;
                rs.rng[4 * r + 1] = nb.lo;
                rs.rng[4 * r + 2] = inc.hi;
                rs.rng[4 * r + 3] = inc.lo;
            }
        } else {
            stream_row_commit(rs.rng, r, kind, base, inc, consumed);
        }
        if (xa.xout.last && have_last) {  // where env.o comes from (left as the caller filled it when no reset served a row)
            xa.xout.last[3 * (int64_t)r + 0] = last_s;
            xa.xout.last[3 * (int64_t)r + 1] = last_x;
            xa.xout.last[3 * (int64_t)r + 2] = last_init;
        }
        out.sum_g[r] = sum_g;
        out.n_ep[r] = ep;
        out.steps[r] = steps;
        out.cand[r] = cand;
        out.n_len[r] = n_len;
        out.status[r] = status;
    }
}

// (pop: 8 bytes for the alignment of beh_lds, as evalmc_lds_bytes counts them)
static size_t exo_lds_bytes(int waves, int64_t ns, int64_t nx, int64_t n_obs, int64_t nA, size_t prob_bytes, bool td, bool pop = false) {
    return (size_t)waves * (WAVE + 1) * sizeof(Jump) + (td ? (size_t)waves * n_obs * nA * 8 : 0) + (size_t)(n_obs * nA) * prob_bytes +
           (size_t)(ns * nx) * 4 + (size_t)(ns + 1) * 4 + (size_t)(nx + 1) * 4 + (size_t)waves * (ns + nx) * 4 +
           (pop ? 8 + (size_t)waves * nA * 8 + (size_t)waves * 624 * 4 : 0);
}

// the launch shape (launch_shape) of the carve above
static int exo_launch_shape(const offsim_table *ts, const offsim_table *tx, int32_t n_obs, size_t pb, bool td, int *waves_out, size_t *lds_out,
                            bool pop = false, const char *who = "eval_mc_exo") {
    if ((int64_t)ts->n_slots * tx->n_slots > 40960 || (int64_t)n_obs * ts->nA > 40960)  // (beyond 160 KiB whatever else: also keeps the sums below in range)
        return fail(OFFSIM_EUNSUPPORTED, "%s: obs_of, policy, Q table and cursors exceed 160 KiB of LDS", who);
    if (!launch_shape([&](int w) { return exo_lds_bytes(w, ts->n_slots, tx->n_slots, n_obs, ts->nA, pb, td, pop); }, waves_out, lds_out))
        return fail(OFFSIM_EUNSUPPORTED, "%s: obs_of, policy, Q table and cursors exceed 160 KiB of LDS", who);
    return OFFSIM_OK;
}

template <typename PL, typename PROB, bool TD, bool POP = false>
static int exo_launch(const offsim_table *ts, const offsim_table *tx, offsim_rollouts *rs, offsim_rollouts *rx, const void *pi,
                      const ExoKernelArgs<POP> &xa, double gamma, const double *gamma_pow, int64_t n_gamma_pow, int64_t max_episodes,
                      const offsim_evalmc_out *out, const offsim_td &td, int waves, size_t lds, void *stream) {
    if (lds > 64 * 1024) HIP_TRY(allow_big_lds((k_eval_mc_exo<PL, PROB, TD, POP>), (int)lds));
    unsigned grid = (unsigned)((rs->R + waves - 1) / waves);
    if constexpr (POP) grid = pop_grid(rs->R, xa.S, waves);
    hipLaunchKernelGGL((k_eval_mc_exo<PL, PROB, TD, POP>), dim3(grid), dim3(waves * WAVE), lds, (hipStream_t)stream, *ts, *tx, *rs, *rx,
                       (const PROB *)pi, xa, gamma, gamma_pow, n_gamma_pow, max_episodes, *out, td);
    LAUNCH_CHECK();
    return OFFSIM_OK;
}

// what offsim_eval_mc_exo and offsim_eval_td_exo_pop check alike: the two tables, rs / rx, obs_of / n_obs, the reseed / provider pair, out
static int exo_check_common(const char *who, const offsim_table *ts, const offsim_table *tx, const offsim_rollouts *rs, const offsim_rollouts *rx,
                            const int32_t *obs_of, int32_t n_obs, int32_t reseed, const offsim_evalmc_out *out, const double *gamma_pow,
                            int64_t n_gamma_pow) {
    int rc = check_table(ts);
    if (rc) return rc;
    if ((rc = check_table(tx))) return rc;
    if (ts->N != tx->N || ts->N0 != tx->N0) return fail(OFFSIM_EINVAL, "%s: the s-table and the x-table hold different logs (N / N0 differ)", who);
    if (ts->N0 > 0 && (!ts->init_slot || !tx->init_slot || !ts->init_orig)) return fail(OFFSIM_EINVAL, "%s: table without its init rows", who);
    if (!rs || !rx || rs->R < 0 || rs->R != rx->R) return fail(OFFSIM_EINVAL, "%s: rs / rx NULL or of different R", who);
    if (n_obs <= 0 || !obs_of) return fail(OFFSIM_EINVAL, "%s: bad n_obs, or obs_of / pi is NULL", who);
    if (reseed != OFFSIM_EXO_RESEED_NONE && reseed != OFFSIM_EXO_RESEED_EPISODE) return fail(OFFSIM_EINVAL, "%s: bad reseed mode", who);
    if (rs->rng_kind != OFFSIM_STREAM_PCG64 && rs->rng_kind != OFFSIM_STREAM_PHILOX) return fail(OFFSIM_EINVAL, "%s: unknown stream provider", who);
    if (reseed == OFFSIM_EXO_RESEED_EPISODE && rs->rng_kind == OFFSIM_STREAM_PHILOX)
        return fail(OFFSIM_EUNSUPPORTED, "%s: OFFSIM_EXO_RESEED_EPISODE seeds default_rng(episode): the stream must be OFFSIM_STREAM_PCG64", who);
    if (!out) return fail(OFFSIM_EINVAL, "%s: out is NULL", who);
    if ((rc = check_evalmc_out(who, out, gamma_pow, n_gamma_pow))) return rc;
    if (out->ep_cap < 0 || out->trace_cap < 0) return fail(OFFSIM_EINVAL, "%s: negative ep_cap / trace_cap", who);
    return OFFSIM_OK;
}
static ExoArgs exo_args(const int32_t *obs_of, int32_t n_obs, int32_t reseed, uint64_t episode0, const offsim_exo_out *xout) {
    return ExoArgs{obs_of, n_obs, reseed, episode0, offsim_exo_out{xout ? xout->trace_row_x : nullptr, xout ? xout->last : nullptr}};
}

extern "C" int offsim_eval_mc_exo(const offsim_table *ts, const offsim_table *tx, offsim_rollouts *rs, offsim_rollouts *rx, const void *pi,
                                  const int32_t *obs_of, int32_t n_obs, int32_t prob_mode, int32_t reseed, uint64_t episode0, double gamma,
                                  const double *gamma_pow, int64_t n_gamma_pow, int64_t max_episodes, const offsim_evalmc_out *out,
                                  const offsim_exo_out *xout, const offsim_td *td, void *stream) {
    static const char *who = "eval_mc_exo";
    int rc = exo_check_common(who, ts, tx, rs, rx, obs_of, n_obs, reseed, out, gamma_pow, n_gamma_pow);
    if (rc) return rc;
    if (!pi) return fail(OFFSIM_EINVAL, "%s: bad n_obs, or obs_of / pi is NULL", who);
    if ((rc = check_prob_mode(who, ts, prob_mode))) return rc;
    if (td) {  // check_td around this entry point's own two rules; of the schedules it looks at alpha_ep only
        if ((rc = check_td(who, td, TD_RULE_MODE))) return rc;
        if (prob_mode != OFFSIM_PROB_F64) return fail(OFFSIM_EINVAL, "%s: the learner drivers take an f64 pi (OFFSIM_PROB_F64)", who);
        if ((rc = check_td(who, td, TD_RULE_BEHAVIOUR))) return rc;
        if (td->behaviour != OFFSIM_BEHAVIOUR_FIXED || td->tie_mt)
            return fail(OFFSIM_EUNSUPPORTED, "%s: only OFFSIM_BEHAVIOUR_FIXED (no greedy behaviour on the learner's own Q, no tie stream)", who);
        if ((rc = check_td(who, td, TD_RULE_SCHED_ALPHA | TD_RULE_CAP | TD_RULE_SNAP))) return rc;
    }
    int waves = 0;
    size_t lds = 0;
    if ((rc = exo_launch_shape(ts, tx, n_obs, prob_mode == OFFSIM_PROB_F32 ? 4 : 8, td != nullptr, &waves, &lds))) return rc;
    if (rs->R == 0) return OFFSIM_OK;
    const ExoArgs xa = exo_args(obs_of, n_obs, reseed, episode0, xout);
    offsim_td tdv;
    memset(&tdv, 0, sizeof(tdv));
    if (td) tdv = *td;
    return with_plog_prob(ts, prob_mode, [&](auto pl, auto prob) -> int {
        using PL = decltype(pl);
        using PROB = decltype(prob);
        if constexpr (sizeof(PROB) == 8) {
            if (td) return exo_launch<PL, PROB, true>(ts, tx, rs, rx, pi, xa, gamma, gamma_pow, n_gamma_pow, max_episodes, out, tdv, waves, lds, stream);
        }
        return exo_launch<PL, PROB, false>(ts, tx, rs, rx, pi, xa, gamma, gamma_pow, n_gamma_pow, max_episodes, out, tdv, waves, lds, stream);
    });
}

// ---- offsim_eval_mc_exo's learner drivers for L learners on the same S seeds in one launch, every learner on its own Q with any behaviour
// policy of the reference (k_eval_mc_exo<.., TD, POP>, csrc/td_pop.hpp); L = 1 is the single learner with a greedy behaviour
extern "C" int offsim_eval_td_exo_pop(const offsim_table *ts, const offsim_table *tx, offsim_rollouts *rs, offsim_rollouts *rx, int32_t L, int32_t S,
                                      const offsim_td_pop *pop, const int32_t *obs_of, int32_t n_obs, int32_t reseed, uint64_t episode0,
                                      int64_t max_episodes, const offsim_evalmc_out *out, const offsim_exo_out *xout, void *stream) {
    static const char *who = "eval_td_exo_pop";
    if (!pop) return fail(OFFSIM_EINVAL, "%s: pop is NULL", who);
    int rc = exo_check_common(who, ts, tx, rs, rx, obs_of, n_obs, reseed, out, pop->gamma_pow, pop->n_gamma_pow);
    if (rc || (rc = check_td_pop(who, L, S, rs->R, pop))) return rc;
    if (pop->td_cap < 0) return fail(OFFSIM_EINVAL, "%s: negative td_cap", who);
    int waves = 0;
    size_t lds = 0;
    if ((rc = exo_launch_shape(ts, tx, n_obs, 8, true, &waves, &lds, true, who))) return rc;
    if (rs->R == 0) return OFFSIM_OK;
    const TdPopExoArgs xa{exo_args(obs_of, n_obs, reseed, episode0, xout), td_pop_fields(pop, S)};
    const offsim_td td = td_of_pop(pop);
    return with_plog(ts, [&](auto pl) -> int {
        return exo_launch<decltype(pl), double, true, true>(ts, tx, rs, rx, nullptr, xa, 0.0, nullptr, pop->n_gamma_pow, max_episodes, out, td, waves, lds,
                                                            stream);
    });
}
