// eval_env_latent.hpp -- tabular policies and TD learners on the LATENT STATES of the environments with continuous observations: the
// reference's evalMC, qlearn, expSARSA (offsim4rl/agents/tabular.py:247-270, :71-139, :141-191) and z_expSARSA (:193-245) on CartPole-v1 and
// MyGridNaviCoords (offsim4rl/envs/gridworld.py:187-211) behind an encoder, many rollouts per launch: offsim_eval_env_latent /
// offsim_eval_env_latent_pop (include/offsim.h).  The ground truth of the *_psrs and *_queue drivers on a log encoded by the same encoder.
//
// k_eval_env (eval_env.hpp) with collect_env.hpp's dynamics in the place of the discrete grid's and an encoder between the observation and
// the table row: one wavefront per rollout, wave-uniform control flow, Q, the behaviour row and the tie stream per rollout in LDS, shared
// pi in LDS.  Per step
//   obs    the f32 observation (env_obs)
//   z      enc(obs); the row is z for 0 <= z < nS and z + nS for -nS <= z < 0 (NumPy's index wrap: the reference's Q[-1] is the last row)
//   p      pi[row], or td_behaviour on Q[row]
//   A      queue_draw on one next_double of the rollout's PCG64 action stream
//   step   env_step (collect_env.hpp), its draws from the rollout's environment stream
//   z'     enc(obs'), computed once: it is the z of the next step
//   TD     the update of k_eval_env on Q[row, A] with Q[row'], the same expressions in the same order; with rec_max the RECORDED error is
//          R + gamma * max Q[row'] - Q[row, A] while the update stays expected SARSA (z_expSARSA, tabular.py:229 / :232)
//   G      G + gamma_pow[t] * (double)reward
// The reward of the grid is the reference's Python float: env_step returns 0, 1 or -0.1f, and -0.1f is widened to the f64 literal -0.1
// (the other two are exact), so that Q, the TD errors and G are the reference's bits.
//
// Encoders (ENC), run in the kernel at every observation the loop visits:
//   BOX  CartpoleBoxEncoder.get_box on the f32 observation with k_encode_box's f32 literals and comparisons; CartPole only; -1 out of bounds.
//   MLP  the HOMER obs_encoder Linear(dO, H) -> LeakyReLU(0.01) -> Linear(H, nZ) -> the first arg max (a row without a logit above -inf --
//        all NaN -- gives 0), k_encode_mlp's arithmetic: per unit one k-ordered fmaf chain from 0, then the bias.  The weights are staged
//        once per workgroup in LDS, transposed ([dO][H] and [H][nZ]) so that the lanes -- which run over the units -- read consecutive words.
//
// Episodes.  reseed = 1 (the reference): episode e restarts the environment stream as default_rng(episode0 + e) (pcg_seed on the device, as
// eval_env.hpp) and draws the reset from it; reseed = 0: the rollout's own environment stream runs on across episodes.  An episode ends at
// done or at max_episode_steps (> 0 required for CartPole); done is not masked in the update, as in the reference.
//
// Loops: a grid episode ends by num_steps (>= 1), a CartPole episode by the cap, so a rollout takes at most n_episodes * bound steps.
//
// LDS of one workgroup: k_eval_env's carve and the encoder behind it --
//   [Q per wave (TD)][pi (when given)][behaviour row per wave (TD)][tie stream per wave (TD)][W1^T b1 W2^T b2 (MLP)][x 4, h H, logits nZ per wave (MLP)]
//
// Included by offsim_hip.hip behind eval_env.hpp and collect_env.hpp: env_reset / env_step / env_obs / env_nA / env_dO, wave_lds_sync,
// mt_seed_lds, queue_draw, td_behaviour, check_evalmc_out, check_td, check_td_pop, td_of_pop, td_pop_fields, pop_grid, launch_shape,
// discount_at, allow_big_lds and ENV_MAX_CELLS2 are those files' and their includes'.
#pragma once

#define LATENT_MAX_UNITS 4096  // H and nZ at most this each (the sums of the carve stay in range; the carve itself bounds their product)

struct LatentArgs {
    offsim_env env;  // kind, R rollouts, the grid's parameters, the two stream tables [R, 4] (read only here)
    offsim_latent_encoder enc;
    offsim_latent_run run;
    const double *pi;
    double gamma;
    const double *gamma_pow;
    int64_t n_gamma_pow;
    int64_t n_episodes;
};

// CartpoleBoxEncoder.get_box (heuristic.py:19-60) on the f32 observation: k_encode_box's literals and comparisons
__device__ __forceinline__ int latent_box(float x, float xd, float th, float thd) {
    const float ONE = 0.0174532f, SIX = 0.1047192f, TWELVE = 0.2094384f, FIFTY = 0.87266f;
    if (x < -2.4f || x > 2.4f || th < -TWELVE || th > TWELVE) return -1;
    int box = x < -0.8f ? 0 : (x < 0.8f ? 1 : 2);
    box += xd < -0.5f ? 0 : (xd < 0.5f ? 3 : 6);
    box += th < -SIX ? 0 : (th < -ONE ? 9 : (th < 0.f ? 18 : (th < ONE ? 27 : (th < SIX ? 36 : 45))));
    box += thd < -FIFTY ? 0 : (thd < FIFTY ? 54 : 108);
    return box;
}

// the f64 reward of the reference: CartPole's 1.0; the grid's Python floats 0.0, 1.0 and -0.1 (env_step returns the last as -0.1f)
template <int ENV>
__device__ __forceinline__ double latent_reward(float reward) {
    if constexpr (ENV == OFFSIM_ENV_CARTPOLE) return (double)reward;
    else return reward == -0.1f ? -0.1 : (double)reward;
}

// The encoder's LDS: the staged weights (shared) and the wave's scratch
struct LatentEncLds {
    const float *w1t, *b1, *w2t, *b2;  // [dO][H], [H], [H][nZ], [nZ]
    float *x, *h, *logits;             // this wave's
};

// z of the state in e, the same value in every lane
template <int ENV, int ENC>
__device__ __forceinline__ int latent_encode(const EnvState &e, const offsim_env &E, const offsim_latent_encoder &enc, const LatentEncLds &m, int lane) {
    if constexpr (ENC == OFFSIM_LATENT_BOX) {
        return latent_box(env_obs<ENV>(e, E.num_cells, 0), env_obs<ENV>(e, E.num_cells, 1), env_obs<ENV>(e, E.num_cells, 2), env_obs<ENV>(e, E.num_cells, 3));
    } else {
        constexpr int dO = env_dO(ENV);
        const int H = enc.H, nZ = enc.nZ;
        if (lane < dO) m.x[lane] = env_obs<ENV>(e, E.num_cells, lane);
        wave_lds_sync();
        for (int j = lane; j < H; j += WAVE) {
            float acc = 0.f;
            for (int k = 0; k < dO; k++) acc = fmaf(m.x[k], m.w1t[k * H + j], acc);
            acc += m.b1[j];
            m.h[j] = acc > 0.f ? acc : 0.01f * acc;  // LeakyReLU(0.01)
        }
        wave_lds_sync();
        for (int c = lane; c < nZ; c += WAVE) {
            float acc = 0.f;
            for (int k = 0; k < H; k++) acc = fmaf(m.h[k], m.w2t[k * nZ + c], acc);
            acc += m.b2[c];
            m.logits[c] = acc;
        }
        wave_lds_sync();
        // the first maximal index, as torch.max(dim=1): each lane keeps the first maximum of its own logits (c = lane, lane + 64, ..:
        // ascending), then a butterfly keeps the larger value and, between equal values, the smaller index.  A lane without a logit
        // above -inf holds (-inf, nZ); a row without one at all -- all NaN -- ends as nZ and gives 0.
        int best = nZ;
        float bv = -__builtin_inff();
        for (int c = lane; c < nZ; c += WAVE) {
            const float v = m.logits[c];
            if (v > bv) {
                bv = v;
                best = c;
            }
        }
        for (int off = WAVE / 2; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off, WAVE);
            const int ob = __shfl_xor(best, off, WAVE);
            if (ov > bv || (ov == bv && ob < best)) {
                bv = ov;
                best = ob;
            }
        }
        return __builtin_amdgcn_readfirstlane(best < nZ ? best : 0);
    }
}

// The learner blocks around the step (POP prologue and index, tie stream, TD update, episode close, outputs) are written out here as in each of
// the rollout kernels (see the note above k_eval_queue).
template <int ENV, int ENC, bool TD, bool POP>
__global__ void __launch_bounds__(256) k_eval_env_latent(LatentArgs A, offsim_evalmc_out out, offsim_td td, TdPopFields pf) {
    static_assert(ENC == OFFSIM_LATENT_MLP || ENV == OFFSIM_ENV_CARTPOLE, "the box encoder reads CartPole's observation");
    extern __shared__ __align__(16) unsigned char lds_raw[];
    constexpr int nA = env_nA(ENV), dO = env_dO(ENV);
    const offsim_env &E = A.env;
    const offsim_latent_run &run = A.run;
    const int waves = blockDim.x / WAVE;
    const double *pi = A.pi;
    double gamma = A.gamma;
    const double *gamma_pow = A.gamma_pow;
    const int64_t n_gamma_pow = A.n_gamma_pow;
    int pop_l = 0, pop_nb = 1;  // POP: this workgroup's member, workgroups per member
    if constexpr (POP) {
        pop_nb = (pf.S + waves - 1) / waves;
        pop_l = blockIdx.x / pop_nb;
        pi = pf.pi ? pf.pi + (int64_t)pop_l * pf.pi_stride : nullptr;
        if constexpr (TD) {
            td.alpha = pf.alpha[pop_l];
            td.epsilon = pf.epsilon[pop_l];
            td.behaviour = pf.behaviour[pop_l];
            td.alpha_ep = pf.alpha_ep ? pf.alpha_ep + (int64_t)pop_l * td.n_sched : nullptr;
            td.epsilon_ep = pf.epsilon_ep ? pf.epsilon_ep + (int64_t)pop_l * td.n_sched : nullptr;
            gamma = pf.gamma[pop_l];
            gamma_pow = pf.gamma_pow + (int64_t)pop_l * n_gamma_pow;
        }
    }
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE), lane = threadIdx.x & (WAVE - 1);  // uniform -> SGPR
    const int nS = A.enc.nS;
    const int n = nS * nA;
    // LDS carve: [Q per wave (TD)][pi (when given)][behaviour row per wave (TD)][tie stream per wave (TD)][encoder][encoder scratch per wave]
    double *q_lds = (double *)lds_raw + (TD ? (size_t)wave * n : 0);
    double *pi_lds = (double *)lds_raw + (TD ? (size_t)waves * n : 0);
    double *beh_lds = pi_lds + (pi ? (size_t)n : 0) + (TD ? (size_t)wave * nA : 0);
    uint32_t *mt_all = (uint32_t *)(pi_lds + (pi ? (size_t)n : 0) + (TD ? (size_t)waves * nA : 0));
    volatile uint32_t *mt_lds = mt_all + (TD ? (size_t)wave * 624 : 0);
    LatentEncLds m{};
    if constexpr (ENC == OFFSIM_LATENT_MLP) {
        const int H = A.enc.H, nZ = A.enc.nZ;
        float *w = (float *)(mt_all + (TD ? (size_t)waves * 624 : 0));
        float *w1t = w, *b1 = w1t + H * dO, *w2t = b1 + H, *b2 = w2t + (size_t)nZ * H;
        float *scr = b2 + nZ + (size_t)wave * (4 + H + nZ);
        for (int i = threadIdx.x; i < H * dO; i += blockDim.x) w1t[(i % dO) * H + i / dO] = A.enc.W1[i];  // W1 [H][dO] -> [dO][H]
        for (int i = threadIdx.x; i < H; i += blockDim.x) b1[i] = A.enc.b1[i];
        for (int i = threadIdx.x; i < nZ * H; i += blockDim.x) w2t[(size_t)(i % H) * nZ + i / H] = A.enc.W2[i];  // W2 [nZ][H] -> [H][nZ]
        for (int i = threadIdx.x; i < nZ; i += blockDim.x) b2[i] = A.enc.b2[i];
        m = LatentEncLds{w1t, b1, w2t, b2, scr, scr + 4, scr + 4 + H};
    }
    if (pi)
        for (int i = threadIdx.x; i < n; i += blockDim.x) pi_lds[i] = pi[i];
    __syncthreads();
    int r = blockIdx.x * waves + wave;
    if constexpr (POP) {
        const int ord = __builtin_amdgcn_readfirstlane((blockIdx.x - pop_l * pop_nb) * waves + wave);
        if (ord >= pf.S) return;
        r = __builtin_amdgcn_readfirstlane(pop_l * pf.S + ord);
    } else {
        if (r >= E.R) return;
    }
    uint32_t mt_pos = 624u;
    if (TD) {
        for (int i = lane; i < n; i += WAVE) q_lds[i] = td.q[(int64_t)r * n + i];
        if (td.tie_mt) {
            for (int i = lane; i < 624; i += WAVE) mt_lds[i] = td.tie_mt[(int64_t)r * 625 + i];
            mt_pos = td.tie_mt[(int64_t)r * 625 + 624];
        }
    }
    U128 act_st = stream_row_base(E.rng_act, r);  // the action stream: the state before the next draw's step
    const U128 act_inc = stream_row_inc(E.rng_act, r);
    U128 env_st = u128(0, 0), env_inc = u128(0, 1);  // the environment stream: the rollout's own, or the episode's
    if (!run.reseed) {
        env_st = stream_row_base(E.rng_env, r);
        env_inc = stream_row_inc(E.rng_env, r);
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): Q and the tie stream visible to the whole wave

    auto row_of = [&](int z) { return z < 0 ? z + nS : z; };  // NumPy's index wrap (the host has checked that every z the encoder gives has a row)
    auto trace_state = [&](double *tr, const EnvState &e, int64_t at) {
        if (tr && at < run.trace_cap && lane < 4) tr[((int64_t)r * run.trace_cap + at) * 4 + lane] = lane == 0 ? e.s[0] : lane == 1 ? e.s[1] : lane == 2 ? e.s[2] : e.s[3];
    };
    EnvState e;
    int64_t ep = 0, n_len = 0, steps = 0;
    double sum_g = 0.0;
    int status = OFFSIM_ST_OK;
    bool terminate = false, mt_pending = false;
    uint32_t mt_seed = 0u;
    while (ep < A.n_episodes && !terminate) {
        if (TD && run.tie_reseed_episode) {  // np.random.seed(episode), tabular.py:114 / :166 / :218 -- before env.reset
            mt_pending = true;
            mt_seed = (uint32_t)run.episode0 + (uint32_t)ep;
        }
        // env.reset(seed=episode)
        if (run.reseed) {
            const PcgInit p = pcg_seed((uint64_t)run.episode0 + (uint64_t)ep);
            env_st = p.state;
            env_inc = p.inc;
        }
        env_reset<ENV>(e, env_st, env_inc);
        int z = latent_encode<ENV, ENC>(e, E, A.enc, m, lane);
        double G = 0.0;
        int64_t tt = 0;
        bool done = false;
        while (!done) {
            const double gp = discount_at(gamma_pow, (uint64_t)n_gamma_pow, gamma, (uint64_t)tt);  // issued ahead of the step
            const int b = row_of(z) * nA;
            // p = pi[z] (tabular.py:224, :258) or behavior_policy(Q[[z], :], ...)[0] (:119)
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
            // A = rng.choice(env.nA, p=p)
            const double u = env_next_double(act_st, act_inc);
            const int a = queue_draw(p, nA, u, lane);
            if (lane == 0 && out.trace_pop && steps < out.trace_cap) out.trace_pop[(int64_t)r * out.trace_cap + steps] = (uint32_t)a;
            if (a >= nA) {  // no action drawn (p of NaN or zeros): the draw is consumed, the environment has not stepped
                status = OFFSIM_ST_KEYERROR;
                terminate = true;
                break;
            }
            trace_state(run.trace_state, e, steps);
            // env.step(A), then z' = enc(obs')
            float reward;
            const bool term = env_step<ENV>(E, e, a, env_st, env_inc, reward);
            const double rew = latent_reward<ENV>(reward);
            const int z_next = latent_encode<ENV, ENC>(e, E, A.enc, m, lane);
            const int b_next = row_of(z_next) * nA;
            const bool dn = term || (run.max_episode_steps > 0 && tt + 1 >= run.max_episode_steps);
            trace_state(run.trace_next_state, e, steps);
            if (lane == 0 && steps < run.trace_cap) {
                const int64_t at = (int64_t)r * run.trace_cap + steps;
                if (run.trace_z) run.trace_z[at] = z;
                if (run.trace_z_next) run.trace_z_next[at] = z_next;
                if (run.trace_reward) run.trace_reward[at] = rew;
                if (run.trace_done) run.trace_done[at] = dn ? 1 : 0;
            }
            if (TD) {  // tabular.py:123-126 (Q-learning) / :175-178, :229-232 (expected SARSA) on Q[z, A] with Q[z']; every lane computes the same update
                const double q_sa = q_lds[b + a];
                const double *qn = q_lds + b_next;
                double nxt;
                if (td.mode == OFFSIM_TD_QLEARN) {
                    nxt = qn[0];
                    for (int k2 = 1; k2 < nA; k2++) nxt = qn[k2] > nxt ? qn[k2] : nxt;
                } else {  // Q[z_] @ pi[z_], left to right
                    const double *pn = pi_lds + b_next;
                    nxt = 0.0;
                    for (int k2 = 0; k2 < nA; k2++) nxt = nxt + qn[k2] * pn[k2];
                }
                const double td_err = rew + gamma * nxt - q_sa;
                double rec = td_err;
                if (run.rec_max) {  // z_expSARSA records R + gamma * Q[z_].max() - Q[z, A] (tabular.py:229)
                    double mx = qn[0];
                    for (int k2 = 1; k2 < nA; k2++) mx = qn[k2] > mx ? qn[k2] : mx;
                    rec = rew + gamma * mx - q_sa;
                }
                if (lane == 0 && td.td_err && steps < td.td_cap) td.td_err[(int64_t)r * td.td_cap + steps] = rec;
                const double alpha = td.alpha_ep ? td.alpha_ep[ep < td.n_sched ? ep : td.n_sched - 1] : td.alpha;  // alpha(episode)
                __builtin_amdgcn_s_waitcnt(0xc07f);
                q_lds[b + a] = q_sa + alpha * td_err;
                if (td.q_snap && steps % td.snap_stride == 0 && steps / td.snap_stride < td.snap_cap) {  // save_Q
                    __builtin_amdgcn_s_waitcnt(0xc07f);
                    double *dst = td.q_snap + ((int64_t)r * td.snap_cap + steps / td.snap_stride) * n;
                    for (int i = lane; i < n; i += WAVE) dst[i] = q_lds[i];
                }
            }
            G = G + gp * rew;  // (no FMA contraction: built with -ffp-contract=off)
            tt++;
            steps++;
            z = z_next;
            done = dn;
        }
        if (status == OFFSIM_ST_KEYERROR) break;  // the reference raises out of the driver here
        if (lane == 0 && out.ep_len && n_len <= out.ep_cap) out.ep_len[(int64_t)r * (out.ep_cap + 1) + n_len] = (int32_t)tt;
        n_len++;
        if (lane == 0 && out.ep_g && ep < out.ep_cap) out.ep_g[(int64_t)r * out.ep_cap + ep] = G;
        sum_g += G;
        ep++;
    }
    // what a later call continues from: Q, the tie stream, and where the two streams stand
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
        if (run.rng_act_end) {
            uint64_t *d = run.rng_act_end + 4 * (int64_t)r;
            d[0] = act_st.hi, d[1] = act_st.lo, d[2] = act_inc.hi, d[3] = act_inc.lo;
        }
        if (run.rng_env_end) {
            uint64_t *d = run.rng_env_end + 4 * (int64_t)r;
            d[0] = env_st.hi, d[1] = env_st.lo, d[2] = env_inc.hi, d[3] = env_inc.lo;
        }
        out.sum_g[r] = sum_g;
        out.n_ep[r] = ep;
        out.steps[r] = steps;
        out.cand[r] = steps;  // one action drawn per step
        out.n_len[r] = n_len;
        out.status[r] = status;
    }
}

// floats of the staged encoder and of one wave's scratch (BOX: none)
static int64_t latent_enc_floats(const offsim_latent_encoder *enc) {
    return enc->kind == OFFSIM_LATENT_MLP ? (int64_t)enc->H * enc->dO + enc->H + (int64_t)enc->nZ * enc->H + enc->nZ : 0;
}
static int64_t latent_wave_floats(const offsim_latent_encoder *enc) { return enc->kind == OFFSIM_LATENT_MLP ? 4 + (int64_t)enc->H + enc->nZ : 0; }

static size_t latent_lds_bytes(int waves, int64_t n, int nA, bool have_pi, bool td, int64_t enc_floats, int64_t wave_floats) {
    return (td ? (size_t)waves * n * 8 : 0) + (have_pi ? (size_t)n * 8 : 0) + (td ? (size_t)waves * nA * 8 + (size_t)waves * 624 * 4 : 0) +
           (size_t)enc_floats * 4 + (size_t)waves * wave_floats * 4;
}

// what offsim_eval_env_latent and offsim_eval_env_latent_pop check alike, in this order: the world, the encoder and its pairing with the world,
// the run, the streams, out, the capacities, n_episodes, the learner, the tie mode and the recorded-error flag
static int latent_check(const char *who, const offsim_env_eval *env, const offsim_latent_encoder *enc, const offsim_latent_run *run,
                        const double *gamma_pow, int64_t n_gamma_pow, int64_t n_episodes, const offsim_evalmc_out *out, const offsim_td *td) {
    if (!env) return fail(OFFSIM_EINVAL, "%s: env is NULL", who);
    if (env->kind == OFFSIM_ENV_GRID)
        return fail(OFFSIM_EUNSUPPORTED, "%s: the discrete grid has no encoder (offsim_eval_env runs the tabular drivers on it)", who);
    if (env->kind != OFFSIM_ENV_GRID_COORDS && env->kind != OFFSIM_ENV_CARTPOLE) return fail(OFFSIM_EINVAL, "%s: unknown environment kind", who);
    if (env->S < 0) return fail(OFFSIM_EINVAL, "%s: env->S < 0", who);
    if (env->kind == OFFSIM_ENV_GRID_COORDS) {
        if (env->num_cells < 1 || env->num_cells > 1024 || env->num_steps < 1)
            return fail(OFFSIM_EINVAL, "%s: num_cells must be in 1..1024 and num_steps >= 1", who);
        if (env->goal_x < 0 || env->goal_x >= env->num_cells || env->goal_y < 0 || env->goal_y >= env->num_cells)
            return fail(OFFSIM_EINVAL, "%s: the goal lies off the grid", who);
    }
    if (!enc) return fail(OFFSIM_EINVAL, "%s: enc is NULL", who);
    if (enc->kind != OFFSIM_LATENT_BOX && enc->kind != OFFSIM_LATENT_MLP) return fail(OFFSIM_EINVAL, "%s: unknown encoder kind", who);
    if (enc->kind == OFFSIM_LATENT_BOX && env->kind != OFFSIM_ENV_CARTPOLE)
        return fail(OFFSIM_EUNSUPPORTED, "%s: OFFSIM_LATENT_BOX reads CartPole's observation (pair it with OFFSIM_ENV_CARTPOLE)", who);
    if (enc->nS < 1) return fail(OFFSIM_EINVAL, "%s: enc->nS must be positive", who);
    if ((int64_t)enc->nS * env_nA(env->kind) > ENV_MAX_CELLS2)
        return fail(OFFSIM_EUNSUPPORTED, "%s: policy and Q table (nS * nA entries) exceed 160 KiB of LDS", who);
    if (enc->kind == OFFSIM_LATENT_BOX) {
        if (enc->nS < 162) return fail(OFFSIM_EINVAL, "%s: the box encoder gives -1 .. 161: nS must be at least 162", who);
    } else {
        if (!enc->W1 || !enc->b1 || !enc->W2 || !enc->b2) return fail(OFFSIM_EINVAL, "%s: enc->W1 / b1 / W2 / b2 is NULL", who);
        if (enc->dO != env_dO(env->kind)) return fail(OFFSIM_EINVAL, "%s: the encoder's input width differs from the environment's observation", who);
        if (enc->H < 1 || enc->nZ < 1) return fail(OFFSIM_EINVAL, "%s: enc->H and enc->nZ must be positive", who);
        if (enc->H > LATENT_MAX_UNITS || enc->nZ > LATENT_MAX_UNITS)
            return fail(OFFSIM_EUNSUPPORTED, "%s: enc->H and enc->nZ are at most 4096 each (and the staged weights must fit the 160 KiB LDS carve)", who);
        if (enc->nZ > enc->nS) return fail(OFFSIM_EINVAL, "%s: the encoder gives nZ latent states but pi and Q have only nS rows", who);
    }
    if (!run) return fail(OFFSIM_EINVAL, "%s: run is NULL", who);
    if (run->reseed != 0 && run->reseed != 1) return fail(OFFSIM_EINVAL, "%s: reseed is 0 or 1", who);
    if (run->max_episode_steps < 0) return fail(OFFSIM_EINVAL, "%s: negative max_episode_steps", who);
    if (env->kind == OFFSIM_ENV_CARTPOLE && run->max_episode_steps < 1)
        return fail(OFFSIM_EINVAL, "%s: CartPole needs max_episode_steps > 0 (nothing else bounds an episode)", who);
    if (run->episode0 < 0) return fail(OFFSIM_EINVAL, "%s: episode0 is negative", who);
    if (run->rec_max != 0 && run->rec_max != 1) return fail(OFFSIM_EINVAL, "%s: rec_max is 0 or 1", who);
    if (run->trace_cap < 0) return fail(OFFSIM_EINVAL, "%s: negative trace_cap", who);
    if (env->S > 0 && (!env->rng_act || (!run->reseed && !env->rng_env)))
        return fail(OFFSIM_EINVAL, "%s: env->rng_act is NULL, or env->rng_env is NULL with reseed = 0", who);
    if (!out) return fail(OFFSIM_EINVAL, "%s: out is NULL", who);
    int rc = check_evalmc_out(who, out, gamma_pow, n_gamma_pow);
    if (rc) return rc;
    if (out->ep_cap < 0 || out->trace_cap < 0) return fail(OFFSIM_EINVAL, "%s: negative ep_cap / trace_cap", who);
    if (n_episodes <= 0) return fail(OFFSIM_EINVAL, "%s: n_episodes must be positive (an environment never runs dry)", who);
    if (run->tie_reseed_episode != 0 && run->tie_reseed_episode != 1) return fail(OFFSIM_EINVAL, "%s: tie_reseed_episode is 0 or 1", who);
    if (td) {
        if ((rc = check_td(who, td, TD_RULES))) return rc;
        if (run->tie_reseed_episode && !td->tie_mt) return fail(OFFSIM_EINVAL, "%s: tie_reseed_episode needs tie_mt (the stream is written back there)", who);
        if (run->rec_max && td->mode != OFFSIM_TD_EXPSARSA) return fail(OFFSIM_EINVAL, "%s: rec_max is z_expSARSA's: the mode must be OFFSIM_TD_EXPSARSA", who);
    } else if (run->tie_reseed_episode || run->rec_max) {
        return fail(OFFSIM_EINVAL, "%s: tie_reseed_episode / rec_max without a learner", who);
    }
    return OFFSIM_OK;
}

// the launch shape (launch_shape's 4 / 2 / 1 rule on the carve above)
static int latent_launch_shape(const char *who, const offsim_env_eval *env, const offsim_latent_encoder *enc, bool have_pi, bool td, int *waves_out,
                               size_t *lds_out) {
    const int nA = env_nA(env->kind);
    const int64_t n = (int64_t)enc->nS * nA, ef = latent_enc_floats(enc), wf = latent_wave_floats(enc);
    if (!launch_shape([&](int w) { return latent_lds_bytes(w, n, nA, have_pi, td, ef, wf); }, waves_out, lds_out))
        return fail(OFFSIM_EUNSUPPORTED, "%s: policy, Q table and the encoder's weights exceed 160 KiB of LDS", who);
    return OFFSIM_OK;
}

template <bool TD, bool POP>
static int latent_launch(const LatentArgs &A, const offsim_evalmc_out *out, const offsim_td &td, const TdPopFields &pf, int waves, size_t lds, void *stream) {
    unsigned grid = (unsigned)((A.env.R + waves - 1) / waves);
    if constexpr (POP) grid = pop_grid(A.env.R, pf.S, waves);
#define LAUNCH_LATENT(ENV, ENC)                                                                        \
    do {                                                                                               \
        if (lds > 64 * 1024) HIP_TRY(allow_big_lds((k_eval_env_latent<ENV, ENC, TD, POP>), (int)lds)); \
        hipLaunchKernelGGL((k_eval_env_latent<ENV, ENC, TD, POP>), dim3(grid), dim3(waves * WAVE), lds, (hipStream_t)stream, A, *out, td, pf); \
    } while (0)
    if (A.env.kind == OFFSIM_ENV_GRID_COORDS) LAUNCH_LATENT(OFFSIM_ENV_GRID_COORDS, OFFSIM_LATENT_MLP);
    else if (A.enc.kind == OFFSIM_LATENT_MLP) LAUNCH_LATENT(OFFSIM_ENV_CARTPOLE, OFFSIM_LATENT_MLP);
    else LAUNCH_LATENT(OFFSIM_ENV_CARTPOLE, OFFSIM_LATENT_BOX);
    LAUNCH_CHECK();
    return OFFSIM_OK;
#undef LAUNCH_LATENT
}

static LatentArgs latent_args(const offsim_env_eval *env, const offsim_latent_encoder *enc, const offsim_latent_run *run, const double *pi, double gamma,
                              const double *gamma_pow, int64_t n_gamma_pow, int64_t n_episodes) {
    LatentArgs A;
    memset(&A, 0, sizeof(A));
    A.env.kind = env->kind;
    A.env.R = env->S;
    A.env.num_cells = env->num_cells;
    A.env.num_steps = env->num_steps;
    A.env.goal_x = env->goal_x;
    A.env.goal_y = env->goal_y;
    A.env.rng_env = const_cast<uint64_t *>(env->rng_env);  // (read only here)
    A.env.rng_act = const_cast<uint64_t *>(env->rng_act);
    A.enc = *enc;
    A.run = *run;
    A.pi = pi;
    A.gamma = gamma;
    A.gamma_pow = gamma_pow;
    A.n_gamma_pow = n_gamma_pow;
    A.n_episodes = n_episodes;
    return A;
}

extern "C" int offsim_eval_env_latent(const offsim_env_eval *env, const offsim_latent_encoder *enc, const double *pi, double gamma,
                                      const double *gamma_pow, int64_t n_gamma_pow, int64_t n_episodes, const offsim_evalmc_out *out,
                                      const offsim_td *td, const offsim_latent_run *run, void *stream) {
    static const char *who = "eval_env_latent";
    int rc = latent_check(who, env, enc, run, gamma_pow, n_gamma_pow, n_episodes, out, td);
    if (rc) return rc;
    if (!pi && !(td && td->behaviour != OFFSIM_BEHAVIOUR_FIXED && td->mode == OFFSIM_TD_QLEARN))
        return fail(OFFSIM_EINVAL, "%s: pi is NULL (only Q-learning with a behaviour on the learner's own Q runs without one)", who);
    int waves = 0;
    size_t lds = 0;
    if ((rc = latent_launch_shape(who, env, enc, pi != nullptr, td != nullptr, &waves, &lds))) return rc;
    if (env->S == 0) return OFFSIM_OK;
    offsim_td tdv;
    memset(&tdv, 0, sizeof(tdv));
    if (td) tdv = *td;
    const LatentArgs A = latent_args(env, enc, run, pi, gamma, gamma_pow, n_gamma_pow, n_episodes);
    const TdPopFields pf{};
    if (td) return latent_launch<true, false>(A, out, tdv, pf, waves, lds, stream);
    return latent_launch<false, false>(A, out, tdv, pf, waves, lds, stream);
}

extern "C" int offsim_eval_env_latent_pop(const offsim_env_eval *env, const offsim_latent_encoder *enc, int32_t L, int32_t S, const offsim_td_pop *pop,
                                          const double *pi_stack, double gamma, const double *gamma_pow, int64_t n_gamma_pow, int64_t n_episodes,
                                          const offsim_evalmc_out *out, const offsim_latent_run *run, void *stream) {
    static const char *who = "eval_env_latent_pop";
    int waves = 0;
    size_t lds = 0;
    if (!pop) {  // evalMC of the stack pi_stack [L, nS, nA]
        int rc = latent_check(who, env, enc, run, gamma_pow, n_gamma_pow, n_episodes, out, nullptr);
        if (rc) return rc;
        if (L < 1 || L > 65535 || S < 1) return fail(OFFSIM_EINVAL, "%s: L must be 1..65535 and S >= 1", who);
        if (env->S != 0 && env->S != (int64_t)L * S) return fail(OFFSIM_EINVAL, "%s: env->S must be L * S", who);
        if (!pi_stack) return fail(OFFSIM_EINVAL, "%s: pi_stack is NULL", who);
        if ((rc = latent_launch_shape(who, env, enc, true, false, &waves, &lds))) return rc;
        if (env->S == 0) return OFFSIM_OK;
        const LatentArgs A = latent_args(env, enc, run, nullptr, gamma, gamma_pow, n_gamma_pow, n_episodes);
        TdPopFields pf{};
        pf.S = S;
        pf.pi = pi_stack;
        pf.pi_stride = (int64_t)enc->nS * env_nA(env->kind);
        offsim_td tdv;
        memset(&tdv, 0, sizeof(tdv));
        return latent_launch<false, true>(A, out, tdv, pf, waves, lds, stream);
    }
    const offsim_td td = td_of_pop(pop);
    int rc = latent_check(who, env, enc, run, pop->gamma_pow, pop->n_gamma_pow, n_episodes, out, &td);
    if (rc || (rc = check_td_pop(who, L, S, env->S, pop, true))) return rc;
    if (!pop->pi) {  // (behaviour_host has been validated)
        bool fixed = false;
        for (int32_t l = 0; l < L; l++) fixed = fixed || pop->behaviour_host[l] == OFFSIM_BEHAVIOUR_FIXED;
        if (fixed || pop->mode != OFFSIM_TD_QLEARN)
            return fail(OFFSIM_EINVAL, "%s: pi is NULL (only Q-learning with a behaviour on every learner's own Q runs without one)", who);
    }
    if ((rc = latent_launch_shape(who, env, enc, pop->pi != nullptr, true, &waves, &lds))) return rc;
    if (env->S == 0) return OFFSIM_OK;
    const LatentArgs A = latent_args(env, enc, run, nullptr, 0.0, nullptr, pop->n_gamma_pow, n_episodes);
    return latent_launch<true, true>(A, out, td, td_pop_fields(pop, S), waves, lds, stream);
}
