// A learner's data collection on QueueEvaluator in one launch (include/offsim.h: offsim_queue_collect; VectorQueueEvaluator.collect).
//
// The loop of the reference's PPOAgent on a QueueEvaluator (offsim4rl/agents/ppo.py:258-279 on offsim4rl/evaluators/queue_evaluator.py:77-88):
// the agent draws its own action from its policy at the current observation and the simulator pops the head of queue (z, a) -- k_collect
// (collect.hpp) with k_eval_queue's step (eval_queue.hpp) in the place of psrs_step.  Launch shape and carried state are k_collect's: one
// wavefront per environment, COLLECT_WAVES environments per workgroup, the networks staged once per workgroup, the environment's state in
// registers for the launch and written back once.  The table is keyed by the composite slot z * nA + a and cur_slot / z_next / init_slot
// hold BASE slots b = (z - z_lo) * nA (evaluators/queue_evaluator.py: BatchedQueueEvaluator).  Each step:
//   0. the critic at the current observation (collect_value);
//   1. the policy at the current observation, k_collect's three forms: MLP (collect_forward + pmlp_softmax: offsim_policy_mlp's bits),
//      ROWS (p_next[row] / p_init[row], f32 or f64 tables) and TABULAR (pi [nZ, nA] by state, f64 in LDS, the row at pi_lds + b).  The row
//      stands in f64 -- an f32 value widened exactly -- in the wave's pn slot (TABULAR: in pi_lds itself); probs records the f32 value;
//   2. A = queue_draw on that row with u = (next64 >> 11) * 2^-53 of the environment's PCG64 action stream, one LCG step per asked step;
//   3. the pop: the head of segment b + A through perm and the cursor.  A >= nA (a row of NaN or zeros) or an empty segment:
//      OFFSIM_ST_KEYERROR; the cursor at its end: OFFSIM_ST_EXHAUSTED.  The environment then stops for the rest of the launch, its state,
//      observation and cursor as they were and the draw consumed.  Cursors stay in global memory (lane 0's store, read back by the same
//      wave), so n_slots has no LDS bound and the state mixes with BatchedQueueEvaluator.step / eval_td;
//   4. the record, ep_t, the reset and the PPO records: collect_served_step, k_collect's own; logp is taken at the drawn action, which is
//      t.a[g] of the served row by construction.  action [T, R] gets the action drawn at every asked step, the unserved last one included.
// The action stream needs no jump: the state after the last draw is what the row holds on exit (k_eval_queue's rule).
//
// LDS of one workgroup: k_collect's carve without the jump tables --
//   [actor's W^T / b | pi f64][critic's W^T / b][pn f64 x 16 per wave][probs f32 x 16 per wave][2 activation rows per wave]
//
// Included by offsim_hip.hip behind collect.hpp and eval_queue.hpp.
#pragma once

template <int VF>
struct QueueCollectArgs : CollectKArgs<VF> {
    int32_t *action;  // [T, R]
    int32_t p_f32;    // ROWS / TABULAR: the caller's tables are f32 (else f64)
};

template <int FORM, typename XT, int VF>
__global__ void __launch_bounds__(COLLECT_WAVES * WAVE) k_collect_queue(offsim_table t, offsim_rollouts ro, QueueCollectArgs<VF> A) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int waves = blockDim.x / WAVE;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE), lane = threadIdx.x & (WAVE - 1);
    const int nA = t.nA, n = t.n_slots;
    float *w_lds = (float *)lds_raw;    // MLP: the weights
    double *pi_lds = (double *)lds_raw;  // TABULAR: pi, flat [nZ * nA]: the row of the state with base slot b starts at b
    double *pn_lds = (double *)(lds_raw + A.off_pn) + wave * PMLP_MAX_ACTIONS;
    float *pf_lds = (float *)(lds_raw + A.off_pf) + wave * PMLP_MAX_ACTIONS;
    float *act_lds = (float *)(lds_raw + A.off_act) + (size_t)wave * 2 * A.mlp.w_max;
    if constexpr (FORM == OFFSIM_COLLECT_MLP) {
        if constexpr (VF == COLLECT_VF_NONE) pmlp_stage(w_lds, A.mlp, A.mlp.out, threadIdx.x, blockDim.x);
        else pmlp_stage(w_lds, A.mlp, A.mlp.out, threadIdx.x, blockDim.x, (int)blockIdx.y);
    } else if constexpr (FORM == OFFSIM_COLLECT_TABULAR) {
        for (int i = threadIdx.x; i < n; i += blockDim.x) pi_lds[i] = A.p_f32 ? (double)((const float *)A.pi)[i] : ((const double *)A.pi)[i];
    }
    float *v_lds = nullptr;  // the critic's W^T / b (VF = OFFSIM_VALUE_MLP)
    if constexpr (VF == OFFSIM_VALUE_MLP) {
        v_lds = (float *)(lds_raw + A.V.off_w);
        pmlp_stage(v_lds, A.V.mlp, A.V.mlp.out, threadIdx.x, blockDim.x, (int)blockIdx.y);
    }
    __syncthreads();
    int r = blockIdx.x * waves + wave;
    if constexpr (VF == COLLECT_VF_NONE) {
        if (r >= ro.R) return;
    } else {  // the tail of each learner's environments
        if (r >= A.V.envs) return;
        r += (int)blockIdx.y * A.V.envs;
    }
    r = __builtin_amdgcn_readfirstlane(r);
    const int64_t R = ro.R, ob = A.st.obs_bytes;

    int b = __builtin_amdgcn_readfirstlane(ro.cur_slot[r]);  // base slot of the current state
    uint32_t ic = ro.init_cursor[r];
    int32_t ep_t = A.st.ep_t[r];
    int32_t xrow = A.st.obs_row[r];  // where the observation comes from once it has moved (ROWS: from the start)
    bool alive = A.st.alive[r] != 0, moved = false, none = false;
    int status = b < 0 ? OFFSIM_ST_INACTIVE : OFFSIM_ST_OK;
    if (FORM == OFFSIM_COLLECT_ROWS && status == OFFSIM_ST_OK && !collect_row_ok(xrow, t.N)) status = OFFSIM_ST_INACTIVE;  // (no tables row)
    if (VF == OFFSIM_VALUE_ROWS && status == OFFSIM_ST_OK && !collect_row_ok(xrow, t.N)) status = OFFSIM_ST_INACTIVE;
    const bool had_state = status == OFFSIM_ST_OK;
    bool live = status == OFFSIM_ST_OK;

    U128 st = stream_row_base(ro.rng, r);  // the action stream: the state before the next draw's step
    const U128 inc = stream_row_inc(ro.rng, r);
    uint64_t consumed = 0;
    const uint32_t *perm_row = ro.perm ? ro.perm + (int64_t)r * ro.perm_stride : nullptr;
    const uint32_t *init_row = ro.init_perm ? ro.init_perm + (int64_t)r * ro.init_stride : nullptr;
    uint32_t *cursor = ro.cursor + (int64_t)r * n;
    unsigned char *obs_cur = (unsigned char *)A.st.obs + r * ob;

    for (int64_t i = 0; i < A.T; i++) {
        const int64_t o = i * R + r;
        if (live && (b < 0 || b + nA > n)) {  // a state outside the table: queues[z, a] raises KeyError, before pi[z] is read
            status = OFFSIM_ST_KEYERROR;
            live = false;
            alive = false;
        }
        if (!live) {  // no state, or stopped earlier in this launch: nothing asked, nothing served
            collect_dead_step<VF>(A, o, nA, ob, lane);
            if (lane == 0) A.action[o] = -1;
            continue;
        }
        if (A.out.obs) wave_copy_row((unsigned char *)A.out.obs + o * ob, collect_obs_row(obs_cur, A.st.obs_next, A.st.obs_init, ob, moved, xrow), ob, lane);
        // 0. the critic at the current observation (the actor's forward reuses the activation rows after it)
        float v = 0.0f;
        if constexpr (VF != COLLECT_VF_NONE) v = collect_value<VF, XT>(A.V, v_lds, act_lds, A.mlp.w_max, moved, r, xrow, lane);
        // 1. the policy at the current observation: an f64 row at pn
        const double *pn = pn_lds;
        const float *logits = nullptr;  // MLP: the last layer's outputs, in the activation rows until the next forward
        if constexpr (FORM == OFFSIM_COLLECT_MLP) {
            const XT *x = collect_obs_row((const XT *)A.mlp.x_start + (int64_t)r * A.mlp.dO, A.mlp.x_next, A.mlp.x_init, A.mlp.dO, moved, xrow);
            logits = collect_forward<XT>(A.mlp, w_lds, x, act_lds, act_lds + A.mlp.w_max, lane);
            if (lane == 0) pmlp_softmax(logits, nA, pf_lds);
            wave_lds_sync();
            if (lane < nA) {
                const float p = pf_lds[lane];
                pn_lds[lane] = (double)p;
                if (A.out.probs) A.out.probs[o * nA + lane] = p;
            }
            wave_lds_sync();
        } else if constexpr (FORM == OFFSIM_COLLECT_ROWS) {
            const int64_t at = xrow >= 0 ? (int64_t)xrow * nA : (-2 - (int64_t)xrow) * nA;
            const void *tab = xrow >= 0 ? A.p_next : A.p_init;
            if (lane < nA) {
                const double p = A.p_f32 ? (double)((const float *)tab)[at + lane] : ((const double *)tab)[at + lane];
                pn_lds[lane] = p;
                if (A.out.probs) A.out.probs[o * nA + lane] = (float)p;
            }
            wave_lds_sync();
        } else {
            pn = pi_lds + b;
            if (A.out.probs && lane < nA) A.out.probs[o * nA + lane] = (float)pn[lane];
        }
        // 2. A = choice(nA, p) on the environment's action stream
        st = pcg_step(st, inc);
        consumed++;
        const double u = (double)(pcg_output(st) >> 11) * 0x1.0p-53;
        const int a = __builtin_amdgcn_readfirstlane(queue_draw(pn, nA, u, lane));
        if (lane == 0) A.action[o] = a;
        // 3. env.step(A): the head of queue (z, A)
        int g = -1;
        int why = OFFSIM_ST_OK;
        if (a >= nA) {  // no action drawn (p of NaN or zeros): queues[z, nA] has no queue
            why = OFFSIM_ST_KEYERROR;
        } else {
            const int slot = b + a;
            const uint32_t beg = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.seg_off[slot]);
            const uint32_t len = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.seg_off[slot + 1]) - beg;
            if (len == 0) {  // (z, A) never logged: self.queues[z, a] raises KeyError
                why = OFFSIM_ST_KEYERROR;
            } else {
                const uint32_t cur = (uint32_t)__builtin_amdgcn_readfirstlane((int)cursor[slot]);
                if (cur >= len) {  // None: the state stays
                    why = OFFSIM_ST_EXHAUSTED;
                } else {
                    uint32_t gl = beg + cur;
                    if (perm_row) gl = perm_row[gl];
                    g = __builtin_amdgcn_readfirstlane((int)gl);
                    if (lane == 0) cursor[slot] = cur + 1u;
                }
            }
        }
        if (why != OFFSIM_ST_OK) {  // the loop's `break`, for this environment (state left as it is)
            status = why;
            live = false;
            alive = false;
            collect_unserved_step<VF>(A, o, lane);
            continue;
        }
        const bool done = t.done[g] != 0;
        const int32_t b_next = __builtin_amdgcn_readfirstlane(t.z_next[g]);
        collect_served_step<FORM, XT, VF, true>(t, A, v_lds, act_lds, init_row, o, r, lane, nA, g, done, b_next, a, v, logits, pn, b, ic, ep_t, xrow, alive,
                                                live, moved, none, status);
        b = __builtin_amdgcn_readfirstlane(b);
    }
    collect_write_back<XT, VF>(ro, A, v_lds, act_lds, obs_cur, ob, r, lane, had_state, b, ic, ep_t, xrow, alive, moved, none, status, [&] {
        if (consumed) {  // the state after the last draw
            ro.rng[4 * r + 0] = st.hi;
            ro.rng[4 * r + 1] = st.lo;
        }
    });
}

// One launch of k_collect_queue<FORM, XT, VF>: k_collect's instances without the p_log / prob axes.
template <int VF>
static int queue_collect_launch(const offsim_table *t, offsim_rollouts *ro, int32_t form, int32_t x_dtype, size_t lds, const QueueCollectArgs<VF> &A,
                                void *stream, int L, int E) {
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)((E + COLLECT_WAVES - 1) / COLLECT_WAVES), (unsigned)L), block(COLLECT_WAVES * WAVE);
#define LAUNCH_QCOLLECT(FORM, XT)                                                                  \
    do {                                                                                           \
        if (lds > 64 * 1024) HIP_TRY(allow_big_lds((k_collect_queue<FORM, XT, VF>), (int)lds));    \
        hipLaunchKernelGGL((k_collect_queue<FORM, XT, VF>), grid, block, lds, s, *t, *ro, A);      \
    } while (0)
#define LAUNCH_QFORM_XT(FORM)                                  \
    do {                                                       \
        if (x_dtype == OFFSIM_F32) LAUNCH_QCOLLECT(FORM, float); \
        else LAUNCH_QCOLLECT(FORM, __half);                    \
    } while (0)
    if (form == OFFSIM_COLLECT_MLP) LAUNCH_QFORM_XT(OFFSIM_COLLECT_MLP);
    else if constexpr (VF == OFFSIM_VALUE_MLP) {
        if (form == OFFSIM_COLLECT_ROWS) LAUNCH_QFORM_XT(OFFSIM_COLLECT_ROWS);
        else LAUNCH_QFORM_XT(OFFSIM_COLLECT_TABULAR);
    } else if (form == OFFSIM_COLLECT_ROWS) LAUNCH_QCOLLECT(OFFSIM_COLLECT_ROWS, float);
    else LAUNCH_QCOLLECT(OFFSIM_COLLECT_TABULAR, float);
    LAUNCH_CHECK();
    return OFFSIM_OK;
#undef LAUNCH_QFORM_XT
#undef LAUNCH_QCOLLECT
}

// The checks of the three entry points and the actor's part of A: queue_check's table rules (the key, the PCG64 action stream),
// collect_prepare's (state, records, the network), and the queue form's own (nA <= 16, the tables' element type, out_action).
static int queue_collect_prepare(const char *who, const offsim_table *t, offsim_rollouts *ro, int32_t nA_actions, const offsim_collect_policy *pol,
                                 int64_t T, int32_t max_episode_steps, const offsim_collect_state *st, const offsim_collect_out *out,
                                 int32_t *out_action, CollectArgs &A, size_t &shared, int32_t &p_f32) {
    int rc = queue_check_table(who, t, ro, nA_actions);
    if (rc) return rc;
    if (nA_actions > PMLP_MAX_ACTIONS) return fail(OFFSIM_EUNSUPPORTED, "%s: more than 16 actions", who);
    if ((rc = collect_prepare(who, t, ro, pol, OFFSIM_PROB_F64, OFFSIM_REJECT_NEVER, T, max_episode_steps, st, out, A, shared))) return rc;
    if (T > 0 && !out_action) return fail(OFFSIM_EINVAL, "%s: out_action is NULL", who);
    p_f32 = 0;
    if (pol->form != OFFSIM_COLLECT_MLP) {
        if (pol->x_dtype != OFFSIM_F32 && pol->x_dtype != OFFSIM_F64)
            return fail(OFFSIM_EINVAL, "%s: x_dtype names the tables' element type, OFFSIM_F32 or OFFSIM_F64", who);
        p_f32 = pol->x_dtype == OFFSIM_F32;
    }
    if (pol->form == OFFSIM_COLLECT_TABULAR) shared = (size_t)t->n_slots * sizeof(double);  // pi [nZ, nA] = n_slots values, f64 in LDS
    return OFFSIM_OK;
}

// k_collect's carve (collect_lds_layout) moved to the front of the workgroup's LDS: this kernel has no jump tables
static size_t queue_collect_lds(size_t shared, CollectArgs &A) {
    const size_t head = (size_t)COLLECT_WAVES * (WAVE + 1) * sizeof(Jump);
    const size_t lds = collect_lds_layout(COLLECT_WAVES, shared, A.mlp.w_max, A);
    A.off_pn -= (uint32_t)head;
    A.off_pf -= (uint32_t)head;
    A.off_act -= (uint32_t)head;
    return lds - head;
}

extern "C" int offsim_queue_collect(const offsim_table *t, offsim_rollouts *ro, int32_t nA_actions, const offsim_collect_policy *pol, int64_t T,
                                    int32_t max_episode_steps, const offsim_collect_state *st, const offsim_collect_out *out, int32_t *out_action,
                                    void *stream) {
    static const char *who = "queue_collect";
    QueueCollectArgs<COLLECT_VF_NONE> A;
    size_t shared;
    int rc = queue_collect_prepare(who, t, ro, nA_actions, pol, T, max_episode_steps, st, out, out_action, A, shared, A.p_f32);
    if (rc) return rc;
    A.action = out_action;
    const size_t lds = queue_collect_lds(shared, A);
    if (lds > 160 * 1024) return fail(OFFSIM_EUNSUPPORTED, "%s: the policy table and per-wave scratch exceed 160 KiB of LDS", who);
    if (ro->R == 0 || T == 0) return OFFSIM_OK;
    return queue_collect_launch<COLLECT_VF_NONE>(t, ro, pol->form, pol->form == OFFSIM_COLLECT_MLP ? pol->x_dtype : OFFSIM_F32, lds, A, stream, 1, ro->R);
}

// offsim_queue_collect_ppo (L = 1, E = ro->R) and offsim_queue_collect_ppo_pop
static int queue_collect_ppo_run(const char *who, const char *who_critic, const offsim_table *t, offsim_rollouts *ro, int32_t nA_actions,
                                 const offsim_collect_policy *pol, const offsim_collect_value *val, int L, int E, int64_t T, int32_t max_episode_steps,
                                 const offsim_collect_state *st, const offsim_collect_out *out, int32_t *out_action, const offsim_collect_ppo_out *ppo,
                                 void *stream) {
    int rc;
    size_t shared;
    int32_t p_f32;
    CollectPpoArgs P;
    if ((rc = queue_collect_prepare(who, t, ro, nA_actions, pol, T, max_episode_steps, st, out, out_action, P, shared, p_f32))) return rc;
    int x_dtype = pol->form == OFFSIM_COLLECT_MLP ? pol->x_dtype : OFFSIM_F32;
    if ((rc = collect_prepare_value(who, who_critic, t, pol, val, ppo, T, E, 0, P, shared, x_dtype))) return rc;
    const size_t lds = queue_collect_lds(shared, P);
    if (lds > 160 * 1024) return fail(OFFSIM_EUNSUPPORTED, "%s: the policy table, the critic and per-wave scratch exceed 160 KiB of LDS", who);
    if (ro->R == 0 || T == 0) return OFFSIM_OK;
    auto launch = [&](auto vf) -> int {
        QueueCollectArgs<decltype(vf)::value> A;
        static_cast<CollectPpoArgs &>(A) = P;
        A.action = out_action;
        A.p_f32 = p_f32;
        return queue_collect_launch<decltype(vf)::value>(t, ro, pol->form, x_dtype, lds, A, stream, L, E);
    };
    if (val->form == OFFSIM_VALUE_MLP) return launch(std::integral_constant<int, OFFSIM_VALUE_MLP>{});
    return launch(std::integral_constant<int, OFFSIM_VALUE_ROWS>{});
}

extern "C" int offsim_queue_collect_ppo(const offsim_table *t, offsim_rollouts *ro, int32_t nA_actions, const offsim_collect_policy *pol,
                                        const offsim_collect_value *val, int64_t T, int32_t max_episode_steps, const offsim_collect_state *st,
                                        const offsim_collect_out *out, int32_t *out_action, const offsim_collect_ppo_out *ppo, void *stream) {
    return queue_collect_ppo_run("queue_collect_ppo", "queue_collect_ppo critic", t, ro, nA_actions, pol, val, 1, ro ? ro->R : 0, T, max_episode_steps, st,
                                 out, out_action, ppo, stream);
}

extern "C" int offsim_queue_collect_ppo_pop(const offsim_table *t, offsim_rollouts *ro, int32_t nA_actions, const offsim_collect_policy *pol,
                                            const offsim_collect_value *val, int32_t L, int32_t E, int64_t T, int32_t max_episode_steps,
                                            const offsim_collect_state *st, const offsim_collect_out *out, int32_t *out_action,
                                            const offsim_collect_ppo_out *ppo, void *stream) {
    static const char *who = "queue_collect_ppo_pop";
    if (L <= 0 || E <= 0 || L > 65535) return fail(OFFSIM_EINVAL, "%s: L must be in 1..65535 and E >= 1", who);
    if (!ro || !pol || !val) return fail(OFFSIM_EINVAL, "%s: ro / pol / val is NULL", who);
    if ((int64_t)L * E != (int64_t)ro->R) return fail(OFFSIM_EINVAL, "%s: ro->R must be L * E", who);
    if (pol->form != OFFSIM_COLLECT_MLP || val->form != OFFSIM_VALUE_MLP)
        return fail(OFFSIM_EUNSUPPORTED, "%s: only OFFSIM_COLLECT_MLP actors and OFFSIM_VALUE_MLP critics", who);
    return queue_collect_ppo_run(who, "queue_collect_ppo_pop critic", t, ro, nA_actions, pol, val, L, E, T, max_episode_steps, st, out, out_action, ppo,
                                 stream);
}
