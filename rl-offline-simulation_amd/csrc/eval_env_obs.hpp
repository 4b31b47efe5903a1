// evalMC of policies over OBSERVATIONS in the environments that produced the logs, whole rollouts per launch (include/offsim.h:
// offsim_eval_env_obs; evaluators/true_env_population.py: evalmc_rollouts_true_env, PPOPopulation.evaluate_env).
//
// The third number beside evalmc_rollouts_population (PSRS) and evalmc_rollouts_queue_population (the (z, a) queues): the value of the same
// MLP actors in the true dynamics, on paired seeds.  k_collect_env (collect_env.hpp) with the records taken out and the episode bookkeeping
// of the evalMC kernels put in: n_episodes episodes per rollout instead of T steps per environment, a discounted return per episode instead
// of a [T, E] record, and no carried state -- a query.  Launch shape and carve are k_collect_env's: one wavefront per rollout, COLLECT_WAVES
// rollouts per workgroup, grid.y the policy of a stacked population, that policy's W^T / b staged once per workgroup (pmlp_stage), wave-uniform
// control flow.  Rollout (l, j) runs policy l on seed j: its two PCG64 streams are row j of rng_env / rng_act, read only, so every policy of a
// seed sees the same resets, the same noise and the same action uniforms.  Per episode: env_reset; per step the observation row, collect_forward
// + pmlp_softmax (offsim_policy_mlp's bits), the row widened to f64, u = one next_double of the action stream, A = queue_draw, env_step,
// G = G + gamma_pow[t] * reward in f64 in step order; the episode ends at terminated or at max_episode_steps.  Every device function called is
// collect.hpp's, collect_env.hpp's, policy_mlp.hpp's or eval_queue.hpp's as it stands, so a rollout equals what k_collect_env records for the
// same streams, bit for bit.
//
// Loops: a grid episode ends by num_steps (>= 1), a CartPole episode by the cap (> 0, checked on the host), so a rollout takes at most
// n_episodes * bound steps and t stays below the bound the host sized gamma_pow for.
//
// LDS of one workgroup: env_collect_lds's carve without a critic --
//   [W^T / b][pn f64 x 16 per wave][probs f32 x 16 per wave][2 activation rows per wave][2 x 4 f32 per wave (the first is the observation row)]
//
// Included by offsim_hip.hip behind collect_env.hpp.
#pragma once

struct EnvEvalObsArgs {
    CollectMlp mlp;
    offsim_env env;  // kind, R = S seeds, the grid's parameters and the two stream tables (read only); no carried state
    offsim_env_eval_out out;
    const double *gamma_pow;
    int64_t n_episodes;
    int32_t cap;  // max_episode_steps (0: the grid's own num_steps alone)
    uint32_t off_pn, off_pf, off_act, off_x;
};

template <int ENV, bool POP>
__global__ void __launch_bounds__(COLLECT_WAVES * WAVE) k_eval_env_obs(EnvEvalObsArgs A) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    constexpr int nA = env_nA(ENV), dO = env_dO(ENV);
    const int waves = blockDim.x / WAVE;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE), lane = threadIdx.x & (WAVE - 1);
    const offsim_env &E = A.env;
    const offsim_env_eval_out &O = A.out;
    float *w_lds = (float *)lds_raw;
    double *pn_lds = (double *)(lds_raw + A.off_pn) + wave * PMLP_MAX_ACTIONS;
    float *pf_lds = (float *)(lds_raw + A.off_pf) + wave * PMLP_MAX_ACTIONS;
    float *act_lds = (float *)(lds_raw + A.off_act) + (size_t)wave * 2 * A.mlp.w_max;
    float *x_lds = (float *)(lds_raw + A.off_x) + wave * 2 * ENV_MAX_OBS;
    const int l = POP ? (int)blockIdx.y : 0;  // the policy of this workgroup
    if constexpr (POP) pmlp_stage(w_lds, A.mlp, A.mlp.out, threadIdx.x, blockDim.x, l);
    else pmlp_stage(w_lds, A.mlp, A.mlp.out, threadIdx.x, blockDim.x);
    __syncthreads();
    const int j = __builtin_amdgcn_readfirstlane(blockIdx.x * waves + wave);  // the seed
    if (j >= E.R) return;  // (no barrier below)
    const int64_t r = (int64_t)l * E.R + j;

    U128 act_st = stream_row_base(E.rng_act, j), env_st = stream_row_base(E.rng_env, j);
    const U128 act_inc = stream_row_inc(E.rng_act, j), env_inc = stream_row_inc(E.rng_env, j);
    EnvState e;
    int64_t ep = 0, steps = 0;
    double sum_g = 0.0;
    int status = OFFSIM_ST_OK;
    auto trace_state = [&](double *tr) {  // the four f64 of the state in e at the rollout's step `steps`
        if (tr && steps < O.trace_cap && lane < 4)
            tr[(r * O.trace_cap + steps) * 4 + lane] = lane == 0 ? e.s[0] : lane == 1 ? e.s[1] : lane == 2 ? e.s[2] : e.s[3];
    };
    while (ep < A.n_episodes && status == OFFSIM_ST_OK) {
        env_reset<ENV>(e, env_st, env_inc);
        double G = 0.0;
        int32_t t = 0;
        uint32_t end = 0u;
        while (!end) {
            const double gp = A.gamma_pow[t];  // issued ahead of the step (t < the bound the table covers)
            // the policy at the current observation: an f64 row at pn
            if (lane < dO) x_lds[lane] = env_obs<ENV>(e, E.num_cells, lane);
            wave_lds_sync();
            const float *logits = collect_forward<float>(A.mlp, w_lds, x_lds, act_lds, act_lds + A.mlp.w_max, lane);
            if (lane == 0) pmlp_softmax(logits, nA, pf_lds);
            wave_lds_sync();
            if (lane < nA) pn_lds[lane] = (double)pf_lds[lane];
            wave_lds_sync();
            // A = choice(nA, p) on the seed's action stream
            const double u = env_next_double(act_st, act_inc);
            const int a = __builtin_amdgcn_readfirstlane(queue_draw(pn_lds, nA, u, lane));
            if (lane == 0 && O.trace_action && steps < O.trace_cap) O.trace_action[r * O.trace_cap + steps] = a;
            if (a >= nA) {  // no action drawn (p of NaN or zeros): the rollout stops, the draw consumed, the open episode dropped
                status = OFFSIM_ST_KEYERROR;
                break;
            }
            trace_state(O.trace_state);
            float reward;
            const bool term = env_step<ENV>(E, e, a, env_st, env_inc, reward);
            trace_state(O.trace_next_state);
            G = G + gp * (double)reward;  // (no FMA contraction: built with -ffp-contract=off)
            t++;
            steps++;
            const bool trunc = A.cap > 0 && t >= A.cap;
            end = (term ? OFFSIM_COLLECT_TERMINATED : 0u) | (trunc ? OFFSIM_COLLECT_TRUNCATED : 0u);
        }
        if (status != OFFSIM_ST_OK) break;
        if (lane == 0) {
            O.Gs[r * A.n_episodes + ep] = G;
            O.lengths[r * A.n_episodes + ep] = t;
            O.ended[r * A.n_episodes + ep] = (uint8_t)end;
        }
        sum_g = sum_g + G;
        ep++;
    }
    for (int64_t i = ep + lane; i < A.n_episodes; i += WAVE) {  // the episodes a stopped rollout did not complete
        O.Gs[r * A.n_episodes + i] = 0.0;
        O.lengths[r * A.n_episodes + i] = 0;
        O.ended[r * A.n_episodes + i] = 0;
    }
    if (lane == 0) {
        O.n_ep[r] = ep;
        O.steps[r] = steps;
        O.status[r] = status;
        O.value[r] = sum_g / (double)ep;  // (NaN where no episode was completed)
    }
}

// the longest episode: the cap, and on the grids num_steps
static int64_t env_eval_obs_bound(const offsim_env_eval *env, int32_t max_episode_steps) {
    if (env->kind == OFFSIM_ENV_CARTPOLE) return max_episode_steps;
    return max_episode_steps > 0 && max_episode_steps < env->num_steps ? max_episode_steps : env->num_steps;
}

template <bool POP>
static int env_eval_obs_launch(size_t lds, const EnvEvalObsArgs &A, int L, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)((A.env.R + COLLECT_WAVES - 1) / COLLECT_WAVES), (unsigned)L), block(COLLECT_WAVES * WAVE);
#define LAUNCH_ENV_OBS(ENV)                                                              \
    do {                                                                                 \
        if (lds > 64 * 1024) HIP_TRY(allow_big_lds((k_eval_env_obs<ENV, POP>), (int)lds)); \
        hipLaunchKernelGGL((k_eval_env_obs<ENV, POP>), grid, block, lds, s, A);          \
    } while (0)
    if (A.env.kind == OFFSIM_ENV_GRID) LAUNCH_ENV_OBS(OFFSIM_ENV_GRID);
    else if (A.env.kind == OFFSIM_ENV_GRID_COORDS) LAUNCH_ENV_OBS(OFFSIM_ENV_GRID_COORDS);
    else LAUNCH_ENV_OBS(OFFSIM_ENV_CARTPOLE);
    LAUNCH_CHECK();
    return OFFSIM_OK;
#undef LAUNCH_ENV_OBS
}

extern "C" int offsim_eval_env_obs(const offsim_env_eval *env, const offsim_collect_policy *pol, int32_t L, int64_t n_episodes,
                                   int32_t max_episode_steps, const double *gamma_pow, int64_t n_gamma_pow, const offsim_env_eval_out *out,
                                   void *stream) {
    static const char *who = "eval_env_obs";
    if (!env) return fail(OFFSIM_EINVAL, "%s: env is NULL", who);
    if (env->kind != OFFSIM_ENV_GRID && env->kind != OFFSIM_ENV_GRID_COORDS && env->kind != OFFSIM_ENV_CARTPOLE)
        return fail(OFFSIM_EINVAL, "%s: unknown environment kind", who);
    if (env->S < 0) return fail(OFFSIM_EINVAL, "%s: S < 0", who);
    if (env->S > 0 && (!env->rng_env || !env->rng_act)) return fail(OFFSIM_EINVAL, "%s: env->rng_env / rng_act is NULL", who);
    if (env->kind != OFFSIM_ENV_CARTPOLE && (env->num_cells < 1 || env->num_cells > 1024 || env->num_steps < 1))
        return fail(OFFSIM_EINVAL, "%s: num_cells must be in 1..1024 and num_steps >= 1", who);
    if (!pol || !out || n_episodes < 0 || max_episode_steps < 0) return fail(OFFSIM_EINVAL, "%s: bad argument", who);
    if (pol->form != OFFSIM_COLLECT_MLP)
        return fail(OFFSIM_EUNSUPPORTED, "%s: the policy form must be OFFSIM_COLLECT_MLP (no logged rows; tabular policies on the grids: offsim_eval_env)", who);
    if (L < 1 || L > 65535) return fail(OFFSIM_EINVAL, "%s: L must be in 1..65535", who);
    EnvEvalObsArgs A;
    memset(&A, 0, sizeof(A));
    static const offsim_table no_table{};  // collect_mlp reads t->N alone: no logged rows, so no x_next / x_init
    offsim_collect_policy p = *pol;
    p.x_start = env;  // the observations are the environment's own: x_start / x_next / x_init are not read
    if (p.x_dtype != OFFSIM_F32) return fail(OFFSIM_EINVAL, "%s: the environment's observations are f32 (x_dtype must be OFFSIM_F32)", who);
    if (p.dO != env_dO(env->kind)) return fail(OFFSIM_EINVAL, "%s: the network's input width differs from the environment's observation", who);
    int rc = collect_mlp(who, &no_table, p, env_nA(env->kind), A.mlp);
    if (rc) return rc;
    if (env->kind == OFFSIM_ENV_CARTPOLE && max_episode_steps < 1)
        return fail(OFFSIM_EINVAL, "%s: CartPole needs max_episode_steps > 0 (nothing else bounds an episode)", who);
    const int64_t bound = env_eval_obs_bound(env, max_episode_steps);
    if (!gamma_pow || n_gamma_pow < bound) return fail(OFFSIM_EINVAL, "%s: gamma_pow is NULL or shorter than the longest episode", who);
    if (out->trace_cap < 0) return fail(OFFSIM_EINVAL, "%s: negative trace_cap", who);
    // the carve: the weights' size is bounded by it alone (no critic shares the workgroup's LDS)
    CollectArgs carve;
    memset(&carve, 0, sizeof(carve));
    carve.mlp.w_max = A.mlp.w_max;
    const size_t lds = env_collect_lds((size_t)A.mlp.floats * sizeof(float), carve, A.off_x);
    if (lds > 160 * 1024) return fail(OFFSIM_EUNSUPPORTED, "%s: the network's weights and per-wave scratch exceed 160 KiB of LDS", who);
    if (env->S == 0 || n_episodes == 0) return OFFSIM_OK;
    if (!out->Gs || !out->lengths || !out->ended || !out->n_ep || !out->steps || !out->status || !out->value)
        return fail(OFFSIM_EINVAL, "%s: out->Gs / lengths / ended / n_ep / steps / status / value is NULL", who);
    A.off_pn = carve.off_pn;
    A.off_pf = carve.off_pf;
    A.off_act = carve.off_act;
    A.env.kind = env->kind;
    A.env.R = env->S;
    A.env.num_cells = env->num_cells;
    A.env.num_steps = env->num_steps;
    A.env.goal_x = env->goal_x;
    A.env.goal_y = env->goal_y;
    A.env.rng_env = const_cast<uint64_t *>(env->rng_env);  // (read only here)
    A.env.rng_act = const_cast<uint64_t *>(env->rng_act);
    A.out = *out;
    A.gamma_pow = gamma_pow;
    A.n_episodes = n_episodes;
    A.cap = max_episode_steps;
    return L == 1 ? env_eval_obs_launch<false>(lds, A, 1, stream) : env_eval_obs_launch<true>(lds, A, L, stream);
}
