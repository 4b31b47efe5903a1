// eval_queue_rows.hpp -- evalMC (offsim4rl/agents/tabular.py:247-270) on QueueEvaluator (offsim4rl/evaluators/queue_evaluator.py:113-131) for
// policies over OBSERVATIONS (the PPO actor of offsim4rl/agents/ppo.py:258-279), many rollouts per launch: offsim_eval_queue_rows_policy and,
// for L policies on the same S seeds, offsim_eval_queue_rows_policy_pop (include/offsim.h).
//
// The loop is k_eval_queue<false>'s (csrc/eval_queue.hpp: one wavefront per rollout, uniform control flow, the same episode bookkeeping,
// outputs, status codes and write-back, the same obs_row convention, trace_pop = the action drawn).  What differs is where p comes from --
// the rule of offsim_eval_mc_rows_policy:
//   right after a reset that popped initial row k   p = p_init[k]   (init_orig order)
//   after a served grouped row g                    p = p_next[g]
// The row (f32 or f64 elements, P) is widened exactly to f64 into the rollout's LDS slot of nA doubles, and the draw is queue_draw of
// eval_queue.hpp on it: Generator.choice(nA, p=p) on the rollout's PCG64 action stream, one LCG step per step; no action drawn (a row of
// NaN or zeros): OFFSIM_ST_KEYERROR.
//
// Loads of a step: p_next[g] hangs on the same address as r / z_next / done of row g, so its loads (lanes 0 .. nA-1, one element each; elements
// beyond 64 follow after the bookkeeping) are issued with those, ahead of the step's bookkeeping, and waited for once before the next
// draw: the dependent chain of a step stays cursor -> perm entry -> row, as in k_eval_queue.
//
// Across calls: every episode begins with env.reset() (tabular.py:255), as in k_eval_queue, so a call never needs the row of a state an
// earlier call left -- a rollout that stands inside an episode (after OFFSIM_ST_EXHAUSTED, or after steps taken by hand) starts the next
// episode like any other.  cur_row [R] (optional) is therefore written on exit only and never read: g >= 0 the last served GROUPED row,
// -2 - k the initial row k (init_orig order) with no step since, -1 none (no initial row left); left as it was when the loop ran no reset.
// It names the table row that holds the policy at the state the rollout stands in.
//
// LDS carve of a workgroup of `waves` rollouts (n = n_slots = nZ * nA):
//   [seg_off: n + 1 u32][cursors per wave: waves * n u32][pad to 8 bytes][p row per wave: waves * nA f64]
// No policy lives in LDS beyond the current row, so a workgroup of the POP instance may hold rollouts of different policies.
//
// POP: ro.R = L * S, policy-major: rollout r evaluates policy r / S on seed index r % S, reads queue orders r % S, and its tables are
// p_next + (r / S) * N * nA, p_init + (r / S) * N0 * nA.  Grid: ceil(L * S / waves).
//
// Included by offsim_hip.hip behind eval_queue.hpp: queue_draw, queue_check_table and launch_shape's users are that file's.
#pragma once

struct QueueRowsArgs {
    const void *p_next;
    const void *p_init;
    int32_t *cur_row;
    int32_t *obs_row;
    int32_t S;  // POP: seeds per policy
};

template <typename P, bool POP>
__global__ void __launch_bounds__(256, 4) k_eval_queue_rows(offsim_table t, offsim_rollouts ro, double gamma, const double *__restrict__ gamma_pow,
                                                         int64_t n_gamma_pow, int64_t max_episodes, offsim_evalmc_out out, QueueRowsArgs qa) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int waves = blockDim.x / WAVE;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE), lane = threadIdx.x & (WAVE - 1);  // uniform -> SGPR
    const int n = t.n_slots, nA = t.nA;
    uint32_t *seg_lds = (uint32_t *)lds_raw;
    uint32_t *cur_lds = seg_lds + (n + 1) + (size_t)wave * n;
    double *p_lds = (double *)(lds_raw + ((((size_t)(n + 1) + (size_t)waves * n) * 4 + 7) & ~(size_t)7)) + (size_t)wave * nA;
    for (int i = threadIdx.x; i <= n; i += blockDim.x) seg_lds[i] = t.seg_off[i];
    __syncthreads();
    const int r = blockIdx.x * waves + wave;
    if (r >= ro.R) return;
    int ord = r, pol = 0;  // POP: the queue orders rollout r walks, its policy
    if constexpr (POP) {
        pol = __builtin_amdgcn_readfirstlane(r / qa.S);
        ord = __builtin_amdgcn_readfirstlane(r - pol * qa.S);
    }
    const P *__restrict__ pn_tab = (const P *)qa.p_next + (int64_t)pol * t.N * nA;
    const P *__restrict__ p0_tab = (const P *)qa.p_init + (int64_t)pol * t.N0 * nA;
    uint32_t *cur_glb = ro.cursor + (int64_t)r * n;
    for (int s = lane; s < n; s += WAVE) cur_lds[s] = cur_glb[s];
    U128 st = stream_row_base(ro.rng, r);  // the action stream: the state before the next draw's step
    const U128 inc = stream_row_inc(ro.rng, r);
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): cursors visible to the whole wave

    const uint32_t *perm_row = ro.perm ? ro.perm + (int64_t)ord * ro.perm_stride : nullptr;
    const uint32_t *init_row = ro.init_perm ? ro.init_perm + (int64_t)ord * ro.init_stride : nullptr;
    uint32_t ic = ro.init_cursor[r];
    int b = __builtin_amdgcn_readfirstlane(ro.cur_slot[r]);  // base slot z * nA of the current state
    int64_t ep = 0, n_len = 0, steps = 0;
    uint64_t consumed = 0;
    double sum_g = 0.0;
    int status = OFFSIM_ST_OK;
    bool terminate = false, no_init = false;
    int32_t g_prev = -1;
    uint32_t k_init = 0;
    while (ep < max_episodes && !terminate) {
        // env.reset()  (queue_evaluator.py:113-119)
        if ((int64_t)ic >= t.N0) {
            status = OFFSIM_ST_NO_INIT;
            b = -1;
            no_init = true;
            break;
        }
        const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane((int)(init_row ? init_row[ic] : ic));
        ic++;
        const int b0 = t.init_slot[k];
        for (int e = lane; e < nA; e += WAVE) p_lds[e] = (double)p0_tab[(int64_t)k * nA + e];  // p = pi(obs of initial row k)
        b = __builtin_amdgcn_readfirstlane(b0);
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
            // A = rng.choice(env.nA, p=p)  (tabular.py:259), p = the row the last reset / step left in p_lds
            st = pcg_step(st, inc);
            consumed++;
            const double u = (double)(pcg_output(st) >> 11) * 0x1.0p-53;
            __builtin_amdgcn_s_waitcnt(0xc07f);  // the row's lanes have written it
            const int A = queue_draw(p_lds, nA, u, lane);
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
            // everything that hangs on g, issued together: the row, and the policy at its next_obs
            const double rew = t.r_dtype == OFFSIM_F64 ? ((const double *)t.r)[g] : (double)((const float *)t.r)[g];
            const int zn = t.z_next[g];
            const uint8_t dn8 = t.done[g];
            P pn = P(0);
            if (lane < nA) pn = pn_tab[(int64_t)g * nA + lane];
            const int b_next = __builtin_amdgcn_readfirstlane(zn);
            const bool dn = dn8 != 0;
            if (lane == 0) cur_lds[slot] = cur + 1u;
            g_prev = g;
            if (lane == 0 && out.trace_row && steps < out.trace_cap) out.trace_row[(int64_t)r * out.trace_cap + steps] = t.orig_idx[g];
            G = G + gp * rew;  // tabular.py:262 (no FMA contraction: built with -ffp-contract=off)
            tt++;
            steps++;
            b = b_next;
            done = dn;
            if (lane < nA) p_lds[lane] = (double)pn;  // p = pi(next_obs of row g)
            for (int e = WAVE + lane; e < nA; e += WAVE) p_lds[e] = (double)pn_tab[(int64_t)g * nA + e];  // (more than 64 actions)
        }
        if (status == OFFSIM_ST_KEYERROR) break;  // the reference raises out of the driver here
        if (lane == 0 && out.ep_len && n_len <= out.ep_cap) out.ep_len[(int64_t)r * (out.ep_cap + 1) + n_len] = (int32_t)tt;
        n_len++;
        if (done) {
            if (lane == 0 && out.ep_g && ep < out.ep_cap) out.ep_g[(int64_t)r * out.ep_cap + ep] = G;
            sum_g += G;
            ep++;
        }
        else if (lane == 0 && out.ep_g && ep < out.ep_cap) {
            // return of the episode cut short by exhaustion: stored past the n_ep completed ones, as k_eval_queue does
            out.ep_g[(int64_t)r * out.ep_cap + ep] = G;
        }
    }
    // write back the env state so that a later call continues where this one stopped
    __builtin_amdgcn_s_waitcnt(0xc07f);
    for (int s = lane; s < n; s += WAVE) cur_glb[s] = cur_lds[s];
    if (lane == 0) {
        ro.init_cursor[r] = ic;
        ro.cur_slot[r] = b;
        if (no_init) {
            if (qa.obs_row) qa.obs_row[r] = -1;
            if (qa.cur_row) qa.cur_row[r] = -1;
        } else if (n_len > 0 || g_prev >= 0 || status != OFFSIM_ST_OK) {  // (left as the caller filled them when the loop ran no reset)
            if (qa.obs_row) qa.obs_row[r] = g_prev >= 0 ? t.orig_idx[g_prev] : -2 - t.init_orig[k_init];
            if (qa.cur_row) qa.cur_row[r] = g_prev >= 0 ? g_prev : -2 - (int32_t)k_init;
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

static size_t queue_rows_lds_bytes(int waves, int64_t n, int64_t nA) {
    return ((((size_t)(n + 1) + (size_t)waves * n) * 4 + 7) & ~(size_t)7) + (size_t)waves * nA * 8;
}

template <typename P, bool POP>
static int queue_rows_launch(const offsim_table *t, offsim_rollouts *ro, double gamma, const double *gamma_pow, int64_t n_gamma_pow, int64_t max_episodes,
                             const offsim_evalmc_out *out, const QueueRowsArgs &qa, int waves, size_t lds, void *stream) {
    if (lds > 64 * 1024) HIP_TRY(allow_big_lds((k_eval_queue_rows<P, POP>), (int)lds));
    const unsigned grid = (unsigned)(((int64_t)ro->R + waves - 1) / waves);
    hipLaunchKernelGGL((k_eval_queue_rows<P, POP>), dim3(grid), dim3(waves * WAVE), lds, (hipStream_t)stream, *t, *ro, gamma, gamma_pow, n_gamma_pow,
                       max_episodes, *out, qa);
    LAUNCH_CHECK();
    return OFFSIM_OK;
}

// what both entry points check, before any HIP call, and the launch (pop: L policies on S seeds)
static int queue_rows_run(const char *who, const offsim_table *t, offsim_rollouts *ro, int32_t nA_actions, const void *p_next, const void *p_init,
                          int32_t p_dtype, bool pop, int32_t L, int32_t S, double gamma, const double *gamma_pow, int64_t n_gamma_pow, int64_t max_episodes,
                          const offsim_evalmc_out *out, int32_t *cur_row, int32_t *out_obs_row, void *stream) {
    int rc = queue_check_table(who, t, ro, nA_actions);
    if (rc) return rc;
    if (!out) return fail(OFFSIM_EINVAL, "%s: out is NULL", who);
    if ((rc = check_evalmc_out(who, out, gamma_pow, n_gamma_pow))) return rc;
    if (out->ep_cap < 0 || out->trace_cap < 0) return fail(OFFSIM_EINVAL, "%s: negative ep_cap / trace_cap", who);
    if ((t->N > 0 && !p_next) || (t->N0 > 0 && !p_init)) return fail(OFFSIM_EINVAL, "%s: p_next / p_init is NULL", who);
    if (p_dtype != OFFSIM_F32 && p_dtype != OFFSIM_F64) return fail(OFFSIM_EINVAL, "%s: p_dtype is OFFSIM_F32 or OFFSIM_F64", who);
    if (pop && (L < 1 || L > 65535 || S < 1 || (int64_t)L * S != ro->R))
        return fail(OFFSIM_EINVAL, "%s: L in 1..65535, S >= 1 and ro->R = L * S expected", who);
    int waves = 0;
    size_t lds = 0;
    if (t->n_slots > 40960 || !launch_shape([&](int w) { return queue_rows_lds_bytes(w, t->n_slots, t->nA); }, &waves, &lds))  // (keeps the sums in range)
        return fail(OFFSIM_EUNSUPPORTED, "%s: cursors and policy rows exceed 160 KiB of LDS", who);
    if (ro->R == 0) return OFFSIM_OK;
    const QueueRowsArgs qa{p_next, p_init, cur_row, out_obs_row, pop ? S : ro->R};
    if (pop)
        return p_dtype == OFFSIM_F32
                   ? queue_rows_launch<float, true>(t, ro, gamma, gamma_pow, n_gamma_pow, max_episodes, out, qa, waves, lds, stream)
                   : queue_rows_launch<double, true>(t, ro, gamma, gamma_pow, n_gamma_pow, max_episodes, out, qa, waves, lds, stream);
    return p_dtype == OFFSIM_F32 ? queue_rows_launch<float, false>(t, ro, gamma, gamma_pow, n_gamma_pow, max_episodes, out, qa, waves, lds, stream)
                                 : queue_rows_launch<double, false>(t, ro, gamma, gamma_pow, n_gamma_pow, max_episodes, out, qa, waves, lds, stream);
}

extern "C" int offsim_eval_queue_rows_policy(const offsim_table *t, offsim_rollouts *ro, int32_t nA_actions, const void *p_next, const void *p_init,
                                             int32_t p_dtype, double gamma, const double *gamma_pow, int64_t n_gamma_pow, int64_t max_episodes,
                                             const offsim_evalmc_out *out, int32_t *cur_row, int32_t *out_obs_row, void *stream) {
    return queue_rows_run("eval_queue_rows_policy", t, ro, nA_actions, p_next, p_init, p_dtype, false, 1, 0, gamma, gamma_pow, n_gamma_pow, max_episodes,
                          out, cur_row, out_obs_row, stream);
}

extern "C" int offsim_eval_queue_rows_policy_pop(const offsim_table *t, offsim_rollouts *ro, int32_t nA_actions, const void *p_next, const void *p_init,
                                                 int32_t p_dtype, int32_t L, int32_t S, double gamma, const double *gamma_pow, int64_t n_gamma_pow,
                                                 int64_t max_episodes, const offsim_evalmc_out *out, int32_t *cur_row, int32_t *out_obs_row,
                                                 void *stream) {
    return queue_rows_run("eval_queue_rows_policy_pop", t, ro, nA_actions, p_next, p_init, p_dtype, true, L, S, gamma, gamma_pow, n_gamma_pow,
                          max_episodes, out, cur_row, out_obs_row, stream);
}
