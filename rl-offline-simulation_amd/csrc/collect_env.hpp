// The logged environments themselves in one launch (include/offsim.h: offsim_env_collect; VectorGridNavi / VectorCartPole.collect).
//
// k_collect_queue (collect_queue.hpp) with the environment's dynamics in the place of the queue pop: the learner's loop on the environment
// that produced the log -- the reference's MyGridNavi / MyGridNaviCoords (offsim4rl/envs/gridworld.py:14-124, 187-211) and CartPole-v1, the
// Euler equations of synth.cartpole_log -- so that a learner's curve inside a simulator and its curve in the real environment come from the
// same launch shape, the same networks' bits and the same action rule.  Launch shape and carve are k_collect_queue's: one wavefront per
// environment, COLLECT_WAVES environments per workgroup, grid.y the learner of a population, the networks staged once per workgroup, the
// environment's state in registers for the launch and written back once.  Each step:
//   0. the critic at the current observation (collect_forward on the critic's network);
//   1. the policy at the current observation: MLP (collect_forward + pmlp_softmax: offsim_policy_mlp's bits) or, on the grids, TABULAR
//      (pi [num_cells^2, nA] by cell id, f64 in LDS);
//   2. A = queue_draw on that row with u = (next64 >> 11) * 2^-53 of the environment's PCG64 ACTION stream, as k_collect_queue;
//   3. the dynamics, the same f64 arithmetic in every lane (wave-uniform); noise and resets draw from the environment's own PCG64 ENV stream;
//   4. the records, ep_t, and the reset at terminated / at max_episode_steps.
// There is no table: nothing is popped, so an environment never runs dry.  The one way to stop is a row from which no action can be drawn
// (NaN or zeros: A >= nA), which ends the environment for the launch with OFFSIM_ST_KEYERROR as in k_collect_queue, the draw consumed.
//
// The observation the networks read is the wave's own f32 row in LDS (x_lds: the current observation; x_lds + ENV_MAX_OBS: the next one,
// for v_trunc), so collect_forward runs as it is, on XT = float.
//
// LDS of one workgroup: k_collect_queue's carve and the observation rows behind it --
//   [actor's W^T / b | pi f64][critic's W^T / b][pn f64 x 16 per wave][probs f32 x 16 per wave][2 activation rows per wave][2 x 4 f32 per wave]
//
// Included by offsim_hip.hip behind collect.hpp and collect_queue.hpp.
#pragma once

#define ENV_MAX_OBS 4  // the widest observation (CartPole)

template <int VF>
struct EnvCollectArgs : CollectKArgs<VF> {
    offsim_env env;
    offsim_env_out rec;
    uint32_t off_x;  // byte offset of the per-wave observation rows
    int32_t p_f32;   // TABULAR: the caller's pi is f32 (else f64)
};

__host__ __device__ constexpr int env_nA(int kind) { return kind == OFFSIM_ENV_CARTPOLE ? 2 : 5; }
__host__ __device__ constexpr int env_dO(int kind) { return kind == OFFSIM_ENV_CARTPOLE ? 4 : kind == OFFSIM_ENV_GRID_COORDS ? 2 : 1; }

// the next double of a PCG64 stream: Generator.random's (next64 >> 11) * 2^-53
__device__ __forceinline__ double env_next_double(U128 &st, U128 inc) {
    st = pcg_step(st, inc);
    return (double)(pcg_output(st) >> 11) * 0x1.0p-53;
}

// Generator.uniform(lo, hi): lo + (hi - lo) * next_double
__device__ __forceinline__ double env_uniform(U128 &st, U128 inc, double lo, double range) { return lo + range * env_next_double(st, inc); }

// An environment's state, the same in every lane.  s: CartPole (x, x_dot, theta, theta_dot); the grids (x, y, obs_0, obs_1) with x, y whole
// numbers and obs the f64 observation of MyGridNaviCoords.external_state (zeros for GRID).
struct EnvState {
    double s[4];
    int32_t step_count;  // MyGridNavi.step_count (CartPole: unused)
};

// reset(): MyGridNavi.reset / MyGridNaviCoords.reset without a seed (two draws of the env stream) / CartPole's uniform(-0.05, 0.05, 4)
template <int ENV>
__device__ __forceinline__ void env_reset(EnvState &e, U128 &st, U128 inc) {
    e.step_count = 0;
    if constexpr (ENV == OFFSIM_ENV_CARTPOLE) {
        for (int k = 0; k < 4; k++) e.s[k] = env_uniform(st, inc, -0.05, 0.1);
    } else {
        e.s[0] = e.s[1] = e.s[2] = e.s[3] = 0.0;
        if constexpr (ENV == OFFSIM_ENV_GRID_COORDS) {
            const double d0 = env_uniform(st, inc, -0.1, 0.2), d1 = env_uniform(st, inc, -0.1, 0.2);
            e.s[2] = 0.0 / 5 + 0.1 + d0;
            e.s[3] = 0.0 / 5 + 0.1 + d1;
        }
    }
}

// the f32 observation, element k < env_dO (GRID: the cell id as the network reads it)
template <int ENV>
__device__ __forceinline__ float env_obs(const EnvState &e, int num_cells, int k) {
    if constexpr (ENV == OFFSIM_ENV_CARTPOLE) return (float)(k == 0 ? e.s[0] : k == 1 ? e.s[1] : k == 2 ? e.s[2] : e.s[3]);
    else if constexpr (ENV == OFFSIM_ENV_GRID_COORDS) return (float)(k == 0 ? e.s[2] : e.s[3]);
    else return (float)((int)e.s[0] + num_cells * (int)e.s[1]);
}

template <int ENV>
__device__ __forceinline__ int env_cell(const EnvState &e, int num_cells) {
    return ENV == OFFSIM_ENV_CARTPOLE ? 0 : (int)e.s[0] + num_cells * (int)e.s[1];
}

// step(a): the new state in e; returns done (the old API's, recorded as terminated) and the reward
template <int ENV>
__device__ __forceinline__ bool env_step(const offsim_env &E, EnvState &e, int a, U128 &st, U128 inc, float &reward) {
    if constexpr (ENV == OFFSIM_ENV_CARTPOLE) {
        const double G = 9.8, MC = 1.0, MP = 0.1, LEN = 0.5, F = 10.0, TAU = 0.02;
        const double pm = MP * LEN, tm = MC + MP;
        const double TH_LIM = 12 * 2 * 3.141592653589793 / 360, X_LIM = 2.4;
        const double x = e.s[0], xd = e.s[1], th = e.s[2], thd = e.s[3];
        const double f = a == 1 ? F : -F;
        const double ct = cos(th), sn = sin(th);
        const double tmp = (f + pm * thd * thd * sn) / tm;
        const double tha = (G * sn - ct * tmp) / (LEN * (4.0 / 3.0 - MP * ct * ct / tm));
        const double xa = tmp - pm * tha * ct / tm;
        e.s[0] = x + TAU * xd;
        e.s[1] = xd + TAU * xa;
        e.s[2] = th + TAU * thd;
        e.s[3] = thd + TAU * tha;
        reward = 1.0f;
        return e.s[0] < -X_LIM || e.s[0] > X_LIM || e.s[2] < -TH_LIM || e.s[2] > TH_LIM;
    } else {
        int x = (int)e.s[0], y = (int)e.s[1];
        if constexpr (ENV == OFFSIM_ENV_GRID_COORDS) {  // MyGridNaviCoords.step: the deltas first
            const double d0 = env_uniform(st, inc, -0.1, 0.2), d1 = env_uniform(st, inc, -0.1, 0.2);
            e.s[2] = d0;
            e.s[3] = d1;
        }
        bool done = x == E.goal_x && y == E.goal_y;
        if (a == 1) y = y + 1 < E.num_cells - 1 ? y + 1 : E.num_cells - 1;
        else if (a == 2) x = x + 1 < E.num_cells - 1 ? x + 1 : E.num_cells - 1;
        else if (a == 3) y = y - 1 > 0 ? y - 1 : 0;
        else if (a == 4) x = x - 1 > 0 ? x - 1 : 0;
        e.step_count++;
        if (e.step_count >= E.num_steps) done = true;
        if (done) reward = 0.0f;
        else if (x == E.goal_x && y == E.goal_y) {
            reward = 1.0f;
            done = true;
        } else reward = -0.1f;
        e.s[0] = (double)x;
        e.s[1] = (double)y;
        if constexpr (ENV == OFFSIM_ENV_GRID_COORDS) {
            e.s[2] = (double)x / 5 + 0.1 + e.s[2];
            e.s[3] = (double)y / 5 + 0.1 + e.s[3];
        }
        return done;
    }
}

// the records of one observation / state at record index o: obs rows of env_dO elements (GRID: the i32 cell id), state rows (CartPole: the
// four f64; the grids: the i32 cell id); either buffer may be NULL
template <int ENV>
__device__ __forceinline__ void env_record(const EnvState &e, int num_cells, void *obs, void *state, int64_t o, int lane) {
    constexpr int dO = env_dO(ENV);
    if constexpr (ENV == OFFSIM_ENV_GRID) {
        if (obs && lane == 0) ((int32_t *)obs)[o] = env_cell<ENV>(e, num_cells);
    } else {
        if (obs && lane < dO) ((float *)obs)[o * dO + lane] = env_obs<ENV>(e, num_cells, lane);
    }
    if constexpr (ENV == OFFSIM_ENV_CARTPOLE) {
        if (state && lane < 4) ((double *)state)[o * 4 + lane] = lane == 0 ? e.s[0] : lane == 1 ? e.s[1] : lane == 2 ? e.s[2] : e.s[3];
    } else {
        if (state && lane == 0) ((int32_t *)state)[o] = env_cell<ENV>(e, num_cells);
    }
}

template <int ENV, int FORM, typename XT, int VF>
__global__ void __launch_bounds__(COLLECT_WAVES * WAVE) k_collect_env(EnvCollectArgs<VF> A) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    constexpr int nA = env_nA(ENV), dO = env_dO(ENV);
    const int waves = blockDim.x / WAVE;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE), lane = threadIdx.x & (WAVE - 1);
    const offsim_env &E = A.env;
    float *w_lds = (float *)lds_raw;    // MLP: the weights
    double *pi_lds = (double *)lds_raw;  // TABULAR: pi, flat [nS * nA]
    double *pn_lds = (double *)(lds_raw + A.off_pn) + wave * PMLP_MAX_ACTIONS;
    float *pf_lds = (float *)(lds_raw + A.off_pf) + wave * PMLP_MAX_ACTIONS;
    float *act_lds = (float *)(lds_raw + A.off_act) + (size_t)wave * 2 * A.mlp.w_max;
    float *x_lds = (float *)(lds_raw + A.off_x) + wave * 2 * ENV_MAX_OBS;
    if constexpr (FORM == OFFSIM_COLLECT_MLP) {
        if constexpr (VF == COLLECT_VF_NONE) pmlp_stage(w_lds, A.mlp, A.mlp.out, threadIdx.x, blockDim.x);
        else pmlp_stage(w_lds, A.mlp, A.mlp.out, threadIdx.x, blockDim.x, (int)blockIdx.y);
    } else {
        const int n = E.num_cells * E.num_cells * nA;
        for (int i = threadIdx.x; i < n; i += blockDim.x) pi_lds[i] = A.p_f32 ? (double)((const float *)A.pi)[i] : ((const double *)A.pi)[i];
    }
    float *v_lds = nullptr;  // the critic's W^T / b
    if constexpr (VF == OFFSIM_VALUE_MLP) {
        v_lds = (float *)(lds_raw + A.V.off_w);
        pmlp_stage(v_lds, A.V.mlp, A.V.mlp.out, threadIdx.x, blockDim.x, (int)blockIdx.y);
    }
    __syncthreads();
    int r = blockIdx.x * waves + wave;
    if constexpr (VF == COLLECT_VF_NONE) {
        if (r >= E.R) return;
    } else {  // the tail of each learner's environments
        if (r >= A.V.envs) return;
        r += (int)blockIdx.y * A.V.envs;
    }
    r = __builtin_amdgcn_readfirstlane(r);
    const int64_t R = E.R;

    EnvState e;
    for (int k = 0; k < 4; k++) e.s[k] = E.state[4 * (int64_t)r + k];
    e.step_count = E.step_count[r];
    int32_t ep_t = E.ep_t[r];
    U128 act_st = stream_row_base(E.rng_act, r), env_st = stream_row_base(E.rng_env, r);
    const U128 act_inc = stream_row_inc(E.rng_act, r), env_inc = stream_row_inc(E.rng_env, r);
    bool live = true;
    int status = OFFSIM_ST_OK;
    auto put_obs = [&](float *x) {  // the networks' input row of the state in e
        if (lane < dO) x[lane] = env_obs<ENV>(e, E.num_cells, lane);
        wave_lds_sync();
    };
    put_obs(x_lds);

    for (int64_t i = 0; i < A.T; i++) {
        const int64_t o = i * R + r;
        if (!live) {  // stopped earlier in this launch: nothing asked, nothing served
            if (lane == 0) {
                A.rec.flags[o] = 0;
                A.rec.action[o] = -1;
                A.rec.reward[o] = 0.0f;
                A.rec.ep_step[o] = 0;
                if constexpr (VF != COLLECT_VF_NONE) A.V.rec.value[o] = A.V.rec.logp[o] = 0.0f;
            }
            if (A.rec.probs && lane < nA) A.rec.probs[o * nA + lane] = 0.0f;
            EnvState z{};
            env_record<ENV>(z, E.num_cells, A.rec.obs, A.rec.state, o, lane);
            env_record<ENV>(z, E.num_cells, A.rec.next_obs, A.rec.next_state, o, lane);
            continue;
        }
        env_record<ENV>(e, E.num_cells, A.rec.obs, A.rec.state, o, lane);
        // 0. the critic at the current observation (the actor's forward reuses the activation rows after it)
        float v = 0.0f;
        if constexpr (VF != COLLECT_VF_NONE) v = collect_forward<XT>(A.V.mlp, v_lds, x_lds, act_lds, act_lds + A.mlp.w_max, lane)[0];
        // 1. the policy at the current observation: an f64 row at pn
        const double *pn = pn_lds;
        const float *logits = nullptr;  // MLP: the last layer's outputs, in the activation rows until the next forward
        if constexpr (FORM == OFFSIM_COLLECT_MLP) {
            logits = collect_forward<XT>(A.mlp, w_lds, x_lds, act_lds, act_lds + A.mlp.w_max, lane);
            if (lane == 0) pmlp_softmax(logits, nA, pf_lds);
            wave_lds_sync();
            if (lane < nA) {
                const float p = pf_lds[lane];
                pn_lds[lane] = (double)p;
                if (A.rec.probs) A.rec.probs[o * nA + lane] = p;
            }
            wave_lds_sync();
        } else {
            pn = pi_lds + (size_t)env_cell<ENV>(e, E.num_cells) * nA;
            if (A.rec.probs && lane < nA) A.rec.probs[o * nA + lane] = (float)pn[lane];
        }
        // 2. A = choice(nA, p) on the environment's action stream
        const double u = env_next_double(act_st, act_inc);
        const int a = __builtin_amdgcn_readfirstlane(queue_draw(pn, nA, u, lane));
        if (a >= nA) {  // no action drawn (p of NaN or zeros): the environment stops, state as it is, the draw consumed
            status = OFFSIM_ST_KEYERROR;
            live = false;
            if (lane == 0) {
                A.rec.flags[o] = 0;
                A.rec.action[o] = a;
                A.rec.reward[o] = 0.0f;
                A.rec.ep_step[o] = ep_t;
                if constexpr (VF != COLLECT_VF_NONE) A.V.rec.value[o] = A.V.rec.logp[o] = 0.0f;
            }
            EnvState z{};
            env_record<ENV>(z, E.num_cells, A.rec.next_obs, A.rec.next_state, o, lane);
            continue;
        }
        if constexpr (VF != COLLECT_VF_NONE) {  // the PPO records: v(obs), logp of the drawn action (before another forward takes the rows)
            if (lane == 0) {
                A.V.rec.value[o] = v;
                if constexpr (FORM == OFFSIM_COLLECT_MLP) A.V.rec.logp[o] = pmlp_logp(logits, nA, a);
                else A.V.rec.logp[o] = logf((float)pn[a]);
            }
        }
        // 3. env.step(A)
        float reward;
        const bool term = env_step<ENV>(E, e, a, env_st, env_inc, reward);
        // 4. the record, ep_t, the reset at terminated / truncated
        env_record<ENV>(e, E.num_cells, A.rec.next_obs, A.rec.next_state, o, lane);
        const int32_t t_ep = ep_t;
        ep_t++;
        const bool trunc = A.max_ep > 0 && ep_t >= A.max_ep;
        uint32_t fl = OFFSIM_COLLECT_SERVED | OFFSIM_COLLECT_ALIVE | (term ? OFFSIM_COLLECT_TERMINATED : 0u) | (trunc ? OFFSIM_COLLECT_TRUNCATED : 0u);
        if constexpr (VF != COLLECT_VF_NONE) {  // v(next_obs), before the reset replaces the observation (spinup's bootstrap)
            if (trunc && !term && A.V.rec.v_trunc) {
                put_obs(x_lds + ENV_MAX_OBS);
                const float vt = collect_forward<XT>(A.V.mlp, v_lds, x_lds + ENV_MAX_OBS, act_lds, act_lds + A.mlp.w_max, lane)[0];
                if (lane == 0) A.V.rec.v_trunc[o] = vt;
            }
        }
        if (term || trunc) {
            ep_t = 0;
            env_reset<ENV>(e, env_st, env_inc);
            fl |= OFFSIM_COLLECT_RESET;
        }
        if (lane == 0) {
            A.rec.flags[o] = (uint8_t)fl;
            A.rec.action[o] = a;
            A.rec.reward[o] = reward;
            A.rec.ep_step[o] = t_ep;
        }
        put_obs(x_lds);
    }
    if constexpr (VF != COLLECT_VF_NONE) {  // the bootstrap of the open path: v at the observation the environment holds
        const float vf = collect_forward<XT>(A.V.mlp, v_lds, x_lds, act_lds, act_lds + A.mlp.w_max, lane)[0];
        if (lane == 0) A.V.rec.final_value[r] = vf;
    }
    // the state, for the next call
    if (lane < 4) E.state[4 * (int64_t)r + lane] = lane == 0 ? e.s[0] : lane == 1 ? e.s[1] : lane == 2 ? e.s[2] : e.s[3];
    if (lane == 0) {
        E.rng_act[4 * r + 0] = act_st.hi;
        E.rng_act[4 * r + 1] = act_st.lo;
        E.rng_env[4 * r + 0] = env_st.hi;
        E.rng_env[4 * r + 1] = env_st.lo;
        E.step_count[r] = e.step_count;
        E.ep_t[r] = ep_t;
        if (A.rec.status) A.rec.status[r] = status;
    }
}

// reset() of the environments in mask (NULL: all): one thread per environment
template <int ENV>
__global__ void __launch_bounds__(256) k_env_true_reset(offsim_env E, const uint8_t *mask) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= E.R || (mask && !mask[r])) return;
    U128 st = stream_row_base(E.rng_env, r);
    const U128 inc = stream_row_inc(E.rng_env, r);
    EnvState e;
    env_reset<ENV>(e, st, inc);
    for (int k = 0; k < 4; k++) E.state[4 * (int64_t)r + k] = e.s[k];
    E.step_count[r] = 0;
    E.ep_t[r] = 0;
    E.rng_env[4 * r + 0] = st.hi;
    E.rng_env[4 * r + 1] = st.lo;
}

static int env_check(const char *who, const offsim_env *env) {
    if (!env) return fail(OFFSIM_EINVAL, "%s: env is NULL", who);
    if (env->kind != OFFSIM_ENV_GRID && env->kind != OFFSIM_ENV_GRID_COORDS && env->kind != OFFSIM_ENV_CARTPOLE)
        return fail(OFFSIM_EINVAL, "%s: unknown environment kind", who);
    if (env->R < 0) return fail(OFFSIM_EINVAL, "%s: R < 0", who);
    if (!env->rng_env || !env->rng_act || !env->state || !env->step_count || !env->ep_t)
        return fail(OFFSIM_EINVAL, "%s: env->rng_env / rng_act / state / step_count / ep_t is NULL", who);
    if (env->kind != OFFSIM_ENV_CARTPOLE && (env->num_cells < 1 || env->num_cells > 1024 || env->num_steps < 1))
        return fail(OFFSIM_EINVAL, "%s: num_cells must be in 1..1024 and num_steps >= 1", who);
    return OFFSIM_OK;
}

extern "C" int offsim_env_collect_reset(const offsim_env *env, const uint8_t *mask, void *stream) {
    int rc = env_check("env_collect_reset", env);
    if (rc) return rc;
    if (env->R == 0) return OFFSIM_OK;
    const dim3 grid((unsigned)((env->R + 255) / 256)), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (env->kind == OFFSIM_ENV_GRID) hipLaunchKernelGGL(k_env_true_reset<OFFSIM_ENV_GRID>, grid, block, 0, s, *env, mask);
    else if (env->kind == OFFSIM_ENV_GRID_COORDS) hipLaunchKernelGGL(k_env_true_reset<OFFSIM_ENV_GRID_COORDS>, grid, block, 0, s, *env, mask);
    else hipLaunchKernelGGL(k_env_true_reset<OFFSIM_ENV_CARTPOLE>, grid, block, 0, s, *env, mask);
    LAUNCH_CHECK();
    return OFFSIM_OK;
}

// The checks of the three entry points and the actor's part of A (`shared`: the bytes of the actor's LDS region, weights or pi).
static int env_collect_prepare(const char *who, const offsim_env *env, const offsim_collect_policy *pol, int64_t T, int32_t max_episode_steps,
                               const offsim_env_out *out, CollectArgs &A, size_t &shared, int32_t &p_f32) {
    int rc = env_check(who, env);
    if (rc) return rc;
    if (!pol || !out || T < 0 || max_episode_steps < 0) return fail(OFFSIM_EINVAL, "%s: bad argument", who);
    if (T > 0 && (!out->flags || !out->action || !out->reward || !out->ep_step))
        return fail(OFFSIM_EINVAL, "%s: out->flags / action / reward / ep_step is NULL", who);
    memset(&A, 0, sizeof(A));
    shared = 0;
    p_f32 = 0;
    static const offsim_table no_table{};  // collect_mlp reads t->N alone: no logged rows, so no x_next / x_init
    if (pol->form == OFFSIM_COLLECT_MLP) {
        offsim_collect_policy p = *pol;
        p.x_start = env->state;  // the observations are the environment's own: x_start / x_next / x_init are not read
        if (p.x_dtype != OFFSIM_F32) return fail(OFFSIM_EINVAL, "%s: the environment's observations are f32 (x_dtype must be OFFSIM_F32)", who);
        if (p.dO != env_dO(env->kind)) return fail(OFFSIM_EINVAL, "%s: the network's input width differs from the environment's observation", who);
        if ((rc = collect_mlp(who, &no_table, p, env_nA(env->kind), A.mlp))) return rc;
        if (A.mlp.floats > OFFSIM_COLLECT_MLP_MAX_FLOATS)
            return fail(OFFSIM_EUNSUPPORTED, "%s: the network's weights exceed OFFSIM_COLLECT_MLP_MAX_FLOATS (64 KiB of LDS)", who);
        shared = (size_t)A.mlp.floats * sizeof(float);
    } else if (pol->form == OFFSIM_COLLECT_TABULAR) {
        if (env->kind == OFFSIM_ENV_CARTPOLE) return fail(OFFSIM_EUNSUPPORTED, "%s: a tabular policy needs a grid environment", who);
        if (!pol->pi) return fail(OFFSIM_EINVAL, "%s: pi is NULL", who);
        if (pol->x_dtype != OFFSIM_F32 && pol->x_dtype != OFFSIM_F64)
            return fail(OFFSIM_EINVAL, "%s: x_dtype names pi's element type, OFFSIM_F32 or OFFSIM_F64", who);
        p_f32 = pol->x_dtype == OFFSIM_F32;
        A.pi = pol->pi;
        A.mlp.w_max = 1;
        shared = (size_t)env->num_cells * env->num_cells * env_nA(env->kind) * sizeof(double);
    } else {
        return fail(OFFSIM_EUNSUPPORTED, "%s: the policy form must be OFFSIM_COLLECT_MLP or OFFSIM_COLLECT_TABULAR (there are no logged rows)", who);
    }
    A.max_ep = max_episode_steps;
    A.T = T;
    return OFFSIM_OK;
}

// queue_collect_lds's carve and the per-wave observation rows behind it
static size_t env_collect_lds(size_t shared, CollectArgs &A, uint32_t &off_x) {
    size_t lds = queue_collect_lds(shared, A);
    lds = (lds + 15) & ~(size_t)15;
    off_x = (uint32_t)lds;
    return lds + (size_t)COLLECT_WAVES * 2 * ENV_MAX_OBS * sizeof(float);
}

template <int VF>
static int env_collect_launch(int32_t form, size_t lds, const EnvCollectArgs<VF> &A, void *stream, int L, int E) {
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)((E + COLLECT_WAVES - 1) / COLLECT_WAVES), (unsigned)L), block(COLLECT_WAVES * WAVE);
#define LAUNCH_ENV(ENV, FORM)                                                                    \
    do {                                                                                         \
        if (lds > 64 * 1024) HIP_TRY(allow_big_lds((k_collect_env<ENV, FORM, float, VF>), (int)lds)); \
        hipLaunchKernelGGL((k_collect_env<ENV, FORM, float, VF>), grid, block, lds, s, A);       \
    } while (0)
    const int kind = A.env.kind;
    if (form == OFFSIM_COLLECT_MLP) {
        if (kind == OFFSIM_ENV_GRID) LAUNCH_ENV(OFFSIM_ENV_GRID, OFFSIM_COLLECT_MLP);
        else if (kind == OFFSIM_ENV_GRID_COORDS) LAUNCH_ENV(OFFSIM_ENV_GRID_COORDS, OFFSIM_COLLECT_MLP);
        else LAUNCH_ENV(OFFSIM_ENV_CARTPOLE, OFFSIM_COLLECT_MLP);
    } else if (kind == OFFSIM_ENV_GRID) LAUNCH_ENV(OFFSIM_ENV_GRID, OFFSIM_COLLECT_TABULAR);
    else LAUNCH_ENV(OFFSIM_ENV_GRID_COORDS, OFFSIM_COLLECT_TABULAR);
    LAUNCH_CHECK();
    return OFFSIM_OK;
#undef LAUNCH_ENV
}

extern "C" int offsim_env_collect(const offsim_env *env, const offsim_collect_policy *pol, int64_t T, int32_t max_episode_steps,
                                  const offsim_env_out *out, void *stream) {
    static const char *who = "env_collect";
    EnvCollectArgs<COLLECT_VF_NONE> A;
    size_t shared;
    int rc = env_collect_prepare(who, env, pol, T, max_episode_steps, out, A, shared, A.p_f32);
    if (rc) return rc;
    const size_t lds = env_collect_lds(shared, A, A.off_x);
    if (lds > 160 * 1024) return fail(OFFSIM_EUNSUPPORTED, "%s: the policy table and per-wave scratch exceed 160 KiB of LDS", who);
    if (env->R == 0 || T == 0) return OFFSIM_OK;
    A.env = *env;
    A.rec = *out;
    return env_collect_launch<COLLECT_VF_NONE>(pol->form, lds, A, stream, 1, env->R);
}

// offsim_env_collect_ppo (L = 1, E = env->R) and offsim_env_collect_ppo_pop
static int env_collect_ppo_run(const char *who, const char *who_critic, const offsim_env *env, const offsim_collect_policy *pol,
                               const offsim_collect_value *val, int L, int E, int64_t T, int32_t max_episode_steps, const offsim_env_out *out,
                               const offsim_collect_ppo_out *ppo, void *stream) {
    EnvCollectArgs<OFFSIM_VALUE_MLP> A;
    size_t shared;
    int rc = env_collect_prepare(who, env, pol, T, max_episode_steps, out, A, shared, A.p_f32);
    if (rc) return rc;
    if (!val) return fail(OFFSIM_EINVAL, "%s: val / ppo is NULL", who);
    if (val->form != OFFSIM_VALUE_MLP) return fail(OFFSIM_EUNSUPPORTED, "%s: the critic must be OFFSIM_VALUE_MLP (there are no logged rows)", who);
    offsim_collect_value v = *val;
    v.x_start = env->state;
    if (v.x_dtype != OFFSIM_F32) return fail(OFFSIM_EINVAL, "%s: the environment's observations are f32 (x_dtype must be OFFSIM_F32)", who_critic);
    if (v.dO != env_dO(env->kind)) return fail(OFFSIM_EINVAL, "%s: the network's input width differs from the environment's observation", who_critic);
    static const offsim_table no_table{};
    offsim_collect_policy p = *pol;
    if (p.form != OFFSIM_COLLECT_MLP) p.x_dtype = OFFSIM_F32;
    int x_dtype = OFFSIM_F32;
    if ((rc = collect_prepare_value(who, who_critic, &no_table, &p, &v, ppo, T, E, 0, A, shared, x_dtype))) return rc;
    const size_t lds = env_collect_lds(shared, A, A.off_x);
    if (lds > 160 * 1024) return fail(OFFSIM_EUNSUPPORTED, "%s: the policy table, the critic and per-wave scratch exceed 160 KiB of LDS", who);
    if (env->R == 0 || T == 0) return OFFSIM_OK;
    A.env = *env;
    A.rec = *out;
    return env_collect_launch<OFFSIM_VALUE_MLP>(pol->form, lds, A, stream, L, E);
}

extern "C" int offsim_env_collect_ppo(const offsim_env *env, const offsim_collect_policy *pol, const offsim_collect_value *val, int64_t T,
                                      int32_t max_episode_steps, const offsim_env_out *out, const offsim_collect_ppo_out *ppo, void *stream) {
    return env_collect_ppo_run("env_collect_ppo", "env_collect_ppo critic", env, pol, val, 1, env ? env->R : 0, T, max_episode_steps, out, ppo, stream);
}

extern "C" int offsim_env_collect_ppo_pop(const offsim_env *env, const offsim_collect_policy *pol, const offsim_collect_value *val, int32_t L,
                                          int32_t E, int64_t T, int32_t max_episode_steps, const offsim_env_out *out,
                                          const offsim_collect_ppo_out *ppo, void *stream) {
    static const char *who = "env_collect_ppo_pop";
    if (L <= 0 || E <= 0 || L > 65535) return fail(OFFSIM_EINVAL, "%s: L must be in 1..65535 and E >= 1", who);
    if (!env || !pol || !val) return fail(OFFSIM_EINVAL, "%s: env / pol / val is NULL", who);
    if ((int64_t)L * E != (int64_t)env->R) return fail(OFFSIM_EINVAL, "%s: env->R must be L * E", who);
    if (pol->form != OFFSIM_COLLECT_MLP || val->form != OFFSIM_VALUE_MLP)
        return fail(OFFSIM_EUNSUPPORTED, "%s: only OFFSIM_COLLECT_MLP actors and OFFSIM_VALUE_MLP critics", who);
    return env_collect_ppo_run(who, "env_collect_ppo_pop critic", env, pol, val, L, E, T, max_episode_steps, out, ppo, stream);
}
