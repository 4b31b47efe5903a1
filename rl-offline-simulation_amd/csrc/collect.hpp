// A learner's data collection in one launch (include/offsim.h: offsim_vector_collect; VectorPSRS.collect).
//
// The loop of examples/cartpole/psrs_from_expert_heuristic.py:59-80 -- policy at the current observation, PSRS.step, reset at terminated
// or at the episode's step cap -- for T steps, one wavefront per environment, as k_vector_step and the generic k_eval_mc.  Each step:
//   1. p_new at the current observation, in one of three forms (template parameter FORM):
//        MLP      the network in-wave: the workgroup stages every layer's W^T [in][out] and b into LDS once; the wave reads its
//                 observation row, lanes run over output units (pmlp_unit: the fmaf chain of k_policy_mlp, so the same bits), lane 0
//                 runs the softmax (pmlp_softmax);
//        ROWS     p_next[row] / p_init[row] of the caller's per-row tables (row = the observation's source row);
//        TABULAR  pi[slot], staged into LDS once per workgroup;
//   2. psrs_step, unchanged (cursors in global memory, as k_step_batch / k_vector_step keep them);
//   3. the step's record ([T, R], step-major: a step's stores from all environments are adjacent);
//   4. reset on done or at max_episode_steps (k_env_reset's logic, as k_vector_step's).
// The environment's state lives in registers for the launch and is written back once at the end.
//
// VF (offsim_vector_collect_ppo) adds the critic of the PPO buffer, in either form whatever the actor's: at every live step v(obs) at the
// observation the actor is asked at (VF = OFFSIM_VALUE_MLP: a second network in LDS behind the actor's; VF = OFFSIM_VALUE_ROWS:
// v_next[row] / v_init[row]), logp of the served action, v(next_obs) of a step that truncates without terminating, and after the last
// step v(obs) of the observation the environment holds.  VF = COLLECT_VF_NONE is offsim_vector_collect: none of it.
//
// An in-LDS network, the actor's or the critic's, is ONE descriptor (CollectMlp, filled by collect_mlp from policy_mlp.hpp's PmlpNet),
// staged by pmlp_stage and evaluated by collect_forward; where an environment's observation row is, is collect_obs_row.
//
// A population (offsim_vector_collect_ppo_pop) is the VF = OFFSIM_VALUE_MLP instance of the MLP form on a grid (ceil(E / 8), L): the
// workgroups of row l stage learner l's actor and critic out of the stacked weights and serve environments l * E + [0, E), so no
// workgroup holds two learners' environments.  One learner is the row l = 0 with E = R: the launch and the code of before.
#pragma once

#include <type_traits>

#define COLLECT_WAVES 8  // environments per workgroup: one copy of the weights in LDS serves eight wavefronts
// candidates a step looks at per round (psrs_step's `width`; the served row and the draws consumed do not depend on it).  Every lane
// that looks at a candidate gathers its columns from a random line of the log, and a step is usually served by the first or second
// candidate, so 64 lanes per round made the kernel bound by that traffic.
#define COLLECT_WIDTH 16
#define COLLECT_VF_NONE -1  // VF of offsim_vector_collect: no critic

// a network in LDS and the observations it reads.  The actor's w_max is the stride of the wave's activation rows: the widest activation
// of the actor and, where there is one, the critic.
struct CollectMlp {
    const float *W[PMLP_MAX_LAYERS];
    const float *b[PMLP_MAX_LAYERS];
    int in[PMLP_MAX_LAYERS], out[PMLP_MAX_LAYERS];
    int woff[PMLP_MAX_LAYERS], boff[PMLP_MAX_LAYERS];  // LDS float offsets of W^T [in][out] and b [out] (boff -1: no bias)
    int n, w_max, floats, act, dO;
    float slope;
    const void *x_start, *x_next, *x_init;
};

// the critic of offsim_vector_collect_ppo (offsim_collect_value): a network in LDS from the byte offset off_w, or ROWS tables; and the PPO
// records (offsim_collect_ppo_out)
struct CollectValue {
    CollectMlp mlp;
    uint32_t off_w;
    int envs;  // environments per learner: workgroups (x, l) serve l * envs + [0, envs), with learner l's networks (one learner: ro->R)
    const float *v_next, *v_init;
    offsim_collect_ppo_out rec;
};

struct CollectArgs {
    CollectMlp mlp;
    const void *p_next, *p_init, *pi;
    int reject_mode, max_ep;
    int64_t T;
    offsim_collect_state st;
    offsim_collect_out out;
    uint32_t off_pn, off_pf, off_act;  // byte offsets of the per-wave p_new (f64 slots), probs (f32) and activation buffers
};

// the kernel's arguments: offsim_vector_collect's instances (VF = COLLECT_VF_NONE) take CollectArgs alone, so their code and argument
// layout are those of the kernel before the critic existed
struct CollectPpoArgs : CollectArgs {
    CollectValue V;
};
template <int VF>
using CollectKArgs = std::conditional_t<VF == COLLECT_VF_NONE, CollectArgs, CollectPpoArgs>;

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's LDS writes are done
    __builtin_amdgcn_wave_barrier();
}

// nb bytes from s to d (d NULL-free), the lanes of one wave striding; s NULL: zeros
__device__ __forceinline__ void wave_copy_row(unsigned char *d, const unsigned char *s, int64_t nb, int lane) {
    if (((nb | (int64_t)(uintptr_t)d | (int64_t)(uintptr_t)s) & 3) == 0) {
        for (int64_t b = 4 * lane; b < nb; b += 4 * WAVE) *(uint32_t *)(d + b) = s ? *(const uint32_t *)(s + b) : 0u;
    } else {
        for (int64_t b = lane; b < nb; b += WAVE) d[b] = s ? s[b] : (unsigned char)0;
    }
}

// obs_row encoding (offsim_eval_mc_rows_policy's out_obs_row): i >= 0 next_obs of caller row i, -2 - i obs of caller row i
__device__ __forceinline__ bool collect_row_ok(int32_t v, int64_t N) { return (v >= 0 && v < N) || (v <= -2 && -2 - (int64_t)v < N); }

// Where an environment's observation row is, in rows of w elements T: its own row `own` of the start rows until the observation has
// moved, then obs_row encoding xrow into next / init.
template <typename T>
__device__ __forceinline__ const T *collect_obs_row(const T *own, const void *next, const void *init, int64_t w, bool moved, int32_t xrow) {
    return !moved ? own : xrow >= 0 ? (const T *)next + (int64_t)xrow * w : (const T *)init + (-2 - (int64_t)xrow) * w;
}

// One wave's forward of the network M, its W^T / b at w (pmlp_stage, stride out), from the observation row x: lanes run over output
// units, every unit pmlp_unit's chain (so offsim_policy_mlp's / offsim_value_mlp's bits).  cur / nxt: the wave's two activation rows.
// Returns the last layer's outputs, which stay in one of the rows until the wave's next forward.
template <typename XT>
__device__ __forceinline__ const float *collect_forward(const CollectMlp &M, const float *w, const XT *x, float *cur, float *nxt, int lane) {
    for (int k = lane; k < M.dO; k += WAVE) cur[k] = pmlp_in<XT>(x, k);
    wave_lds_sync();
    for (int l = 0; l < M.n; l++) {
        const int in = M.in[l], out = M.out[l];
        const float *wt = w + M.woff[l];
        const float *bl = M.boff[l] >= 0 ? w + M.boff[l] : nullptr;
        const bool last = l == M.n - 1;
        for (int j = lane; j < out; j += WAVE) nxt[j] = pmlp_unit(cur, wt + j, out, in, bl ? bl + j : nullptr, last, M.act, M.slope);
        wave_lds_sync();
        float *sw = cur;
        cur = nxt;
        nxt = sw;
    }
    return cur;
}

// The critic at an observation (moved false: the environment's x_start row; else obs_row encoding xrow), the same value in every lane.
// MLP: the last layer's one unit.  It uses the wave's activation rows, which the actor's forward overwrites afterwards.  ROWS: the
// caller's tables.
template <int VF, typename XT>
__device__ __forceinline__ float collect_value(const CollectValue &V, const float *v_lds, float *act, int w_max, bool moved, int64_t r,
                                               int32_t xrow, int lane) {
    if constexpr (VF == OFFSIM_VALUE_ROWS) {
        return xrow >= 0 ? V.v_next[xrow] : V.v_init[-2 - (int64_t)xrow];
    } else {
        const XT *x = collect_obs_row((const XT *)V.mlp.x_start + r * V.mlp.dO, V.mlp.x_next, V.mlp.x_init, V.mlp.dO, moved, xrow);
        return collect_forward<XT>(V.mlp, v_lds, x, act, act + w_max, lane)[0];
    }
}

// ---- k_collect's blocks as functions, for k_collect_queue (collect_queue.hpp): what a step records, the reset, the state written back ----
// (KA: the kernel's arguments, CollectKArgs<VF> or a struct derived from it; k_collect itself: see the note above it)

// The records of a step at which nothing is asked (no state, or stopped earlier in this launch): nothing served, zeros.
template <int VF, typename KA>
__device__ __forceinline__ void collect_dead_step(const KA &A, int64_t o, int nA, int64_t ob, int lane) {
    if (lane == 0) {
        A.out.row[o] = -1;
        A.out.flags[o] = 0;
    }
    if (A.out.probs)
        for (int a = lane; a < nA; a += WAVE) A.out.probs[o * nA + a] = 0.0f;
    if (A.out.obs) wave_copy_row((unsigned char *)A.out.obs + o * ob, nullptr, ob, lane);
    if constexpr (VF != COLLECT_VF_NONE)
        if (lane == 0) A.V.rec.value[o] = A.V.rec.logp[o] = 0.0f;
}

// The records of a step that was asked and not served (None or KeyError): obs and probs stay as recorded.
template <int VF, typename KA>
__device__ __forceinline__ void collect_unserved_step(const KA &A, int64_t o, int lane) {
    if (lane == 0) {
        A.out.row[o] = -1;
        A.out.flags[o] = 0;
        if constexpr (VF != COLLECT_VF_NONE) A.V.rec.value[o] = A.V.rec.logp[o] = 0.0f;
    }
}

// A served step, row g of the grouped table (done / z_next: its columns): the PPO records (v: the critic at the observation asked at;
// logp of action `act`, or with act < 0 of the row's logged action t.a[g], from the logits or from pn), the step's record, ep_t, and
// the reset at terminated / truncated (k_env_reset's logic).  The environment's state is the caller's registers.
template <int FORM, typename XT, int VF, bool DRAWN, typename PROB, typename KA>
__device__ __forceinline__ void collect_served_step(const offsim_table &t, const KA &A, const float *v_lds, float *act_lds, const uint32_t *init_row,
                                                    int64_t o, int64_t r, int lane, int nA, int g, bool done, int32_t z_next, int act, float v,
                                                    const float *logits, const PROB *pn, int &slot, uint32_t &ic, int32_t &ep_t, int32_t &xrow,
                                                    bool &alive, bool &live, bool &moved, bool &none, int &status) {
    if constexpr (VF != COLLECT_VF_NONE) {  // the PPO records of a served step: v(obs), logp of the served action (lane 0)
        if (lane == 0) {
            int a;
            if constexpr (DRAWN) a = act;
            else a = t.a[g];
            A.V.rec.value[o] = v;
            if constexpr (FORM == OFFSIM_COLLECT_MLP) A.V.rec.logp[o] = pmlp_logp(logits, nA, a);
            else A.V.rec.logp[o] = logf((float)pn[a]);
        }
    }
    // 3. the record, 4. the reset at terminated / truncated
    const int32_t row = t.orig_idx[g];
    ep_t++;
    const bool term = done, trunc = A.max_ep > 0 && ep_t >= A.max_ep;
    uint32_t fl = OFFSIM_COLLECT_SERVED | (term ? OFFSIM_COLLECT_TERMINATED : 0u) | (trunc ? OFFSIM_COLLECT_TRUNCATED : 0u);
    if constexpr (VF != COLLECT_VF_NONE) {  // v(next_obs) of the served row, before a reset replaces the observation (spinup's bootstrap)
        if (trunc && !term && A.V.rec.v_trunc) {
            const float vt = collect_value<VF, XT>(A.V, v_lds, act_lds, A.mlp.w_max, true, r, row, lane);
            if (lane == 0) A.V.rec.v_trunc[o] = vt;
        }
    }
    slot = z_next;
    xrow = row;
    moved = true;
    if (term || trunc) {
        ep_t = 0;
        if ((int64_t)ic >= t.N0) {  // psrs.py:33-35: reset() returned None; the observation stays next_obs of the row
            slot = -1;
            alive = false;
            live = false;
            none = true;
            status = OFFSIM_ST_NO_INIT;
        } else {
            const uint32_t k = init_row ? init_row[ic] : ic;
            ic++;
            slot = t.init_slot[k];
            xrow = -2 - t.init_orig[k];
            fl |= OFFSIM_COLLECT_RESET;
        }
    }
    if (alive) fl |= OFFSIM_COLLECT_ALIVE;
    if (lane == 0) {
        A.out.row[o] = row;
        A.out.flags[o] = (uint8_t)fl;
    }
}

// The end of the launch: the bootstrap of a path still open, the observation buffer, and (lane 0) the draw-stream row through `commit`
// and the environment's state, for the next call.
template <typename XT, int VF, typename KA, typename COMMIT>
__device__ __forceinline__ void collect_write_back(const offsim_rollouts &ro, const KA &A, const float *v_lds, float *act_lds, unsigned char *obs_cur,
                                                   int64_t ob, int64_t r, int lane, bool had_state, int slot, uint32_t ic, int32_t ep_t, int32_t xrow,
                                                   bool alive, bool moved, bool none, int status, COMMIT &&commit) {
    if constexpr (VF != COLLECT_VF_NONE) {  // the bootstrap of a path still open: v at the observation the environment holds (0: no state)
        const float vf = had_state ? collect_value<VF, XT>(A.V, v_lds, act_lds, A.mlp.w_max, moved, r, xrow, lane) : 0.0f;
        if (lane == 0) A.V.rec.final_value[r] = vf;
    }
    // the state, for the next call
    if (moved) wave_copy_row(obs_cur, collect_obs_row(obs_cur, A.st.obs_next, A.st.obs_init, ob, moved, xrow), ob, lane);
    if (lane == 0) {
        commit();
        ro.cur_slot[r] = slot;
        ro.init_cursor[r] = ic;
        A.st.ep_t[r] = ep_t;
        if (moved) A.st.obs_row[r] = none ? -1 : xrow;
        A.st.alive[r] = (uint8_t)alive;
        if (A.out.status) A.out.status[r] = status;
    }
}

// k_collect writes the four blocks above out itself: with any one of them called from here -- collect_dead_step and collect_unserved_step alone
// were enough -- the register allocation and schedule of all 56 instances changed (profiles/queue_collect/isa_compare.txt), so the kernel's
// text, and with it every instance's instructions, stays what it was and the helpers serve k_collect_queue.  A change to a block below
// belongs in its helper too.
template <typename PL, typename PROB, int FORM, typename XT, int VF>
__global__ void __launch_bounds__(COLLECT_WAVES * WAVE) k_collect(offsim_table t, offsim_rollouts ro, CollectKArgs<VF> A) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int waves = blockDim.x / WAVE;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE), lane = threadIdx.x & (WAVE - 1);
    const int nA = t.nA;
    Jump *tables = (Jump *)lds_raw;
    float *w_lds = (float *)(tables + waves * (WAVE + 1));  // MLP: the weights; TABULAR: pi
    PROB *pi_lds = (PROB *)w_lds;
    PROB *pn_lds = (PROB *)(lds_raw + A.off_pn) + wave * PMLP_MAX_ACTIONS;
    float *pf_lds = (float *)(lds_raw + A.off_pf) + wave * PMLP_MAX_ACTIONS;
    float *act_lds = (float *)(lds_raw + A.off_act) + (size_t)wave * 2 * A.mlp.w_max;
    if constexpr (FORM == OFFSIM_COLLECT_MLP) {
        if constexpr (VF == COLLECT_VF_NONE) pmlp_stage(w_lds, A.mlp, A.mlp.out, threadIdx.x, blockDim.x);
        else pmlp_stage(w_lds, A.mlp, A.mlp.out, threadIdx.x, blockDim.x, (int)blockIdx.y);
    } else if constexpr (FORM == OFFSIM_COLLECT_TABULAR) {
        for (int i = threadIdx.x; i < t.n_slots * nA; i += blockDim.x) pi_lds[i] = ((const PROB *)A.pi)[i];
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
    const int64_t R = ro.R, ob = A.st.obs_bytes;

    int slot = ro.cur_slot[r];
    uint32_t ic = ro.init_cursor[r];
    int32_t ep_t = A.st.ep_t[r];
    int32_t xrow = A.st.obs_row[r];  // where the observation comes from once it has moved (ROWS: from the start)
    bool alive = A.st.alive[r] != 0, moved = false, none = false;
    int status = slot < 0 ? OFFSIM_ST_INACTIVE : OFFSIM_ST_OK;
    if (FORM == OFFSIM_COLLECT_ROWS && status == OFFSIM_ST_OK && !collect_row_ok(xrow, t.N)) status = OFFSIM_ST_INACTIVE;  // (no tables row)
    if (VF == OFFSIM_VALUE_ROWS && status == OFFSIM_ST_OK && !collect_row_ok(xrow, t.N)) status = OFFSIM_ST_INACTIVE;
    const bool had_state = status == OFFSIM_ST_OK;
    bool live = status == OFFSIM_ST_OK;

    WaveRng rng;
    const U128 base = u128(ro.rng[4 * r + 0], ro.rng[4 * r + 1]), inc = u128(ro.rng[4 * r + 2], ro.rng[4 * r + 3]);
    rng.kind = ro.rng_kind;
    if (A.reject_mode != OFFSIM_REJECT_NEVER) wave_rng_init(rng, tables + wave * (WAVE + 1), base, inc, ro.rng_kind);
    wave_lds_sync();
    uint64_t consumed = 0;
    const uint32_t *perm_row = ro.perm ? ro.perm + (int64_t)r * ro.perm_stride : nullptr;
    const uint32_t *init_row = ro.init_perm ? ro.init_perm + (int64_t)r * ro.init_stride : nullptr;
    uint32_t *cursor = ro.cursor + (int64_t)r * t.n_slots;
    unsigned char *obs_cur = (unsigned char *)A.st.obs + r * ob;

    for (int64_t i = 0; i < A.T; i++) {
        const int64_t o = i * R + r;
        if (live && (unsigned)slot >= (unsigned)t.n_slots) {  // (a slot outside the table: psrs_step's KeyError, before pi[slot] is read)
            status = OFFSIM_ST_KEYERROR;
            live = false;
            alive = false;
        }
        if (!live) {  // no state, or stopped earlier in this launch: nothing asked, nothing served
            if (lane == 0) {
                A.out.row[o] = -1;
                A.out.flags[o] = 0;
            }
            if (A.out.probs)
                for (int a = lane; a < nA; a += WAVE) A.out.probs[o * nA + a] = 0.0f;
            if (A.out.obs) wave_copy_row((unsigned char *)A.out.obs + o * ob, nullptr, ob, lane);
            if constexpr (VF != COLLECT_VF_NONE)
                if (lane == 0) A.V.rec.value[o] = A.V.rec.logp[o] = 0.0f;
            continue;
        }
        if (A.out.obs) wave_copy_row((unsigned char *)A.out.obs + o * ob, collect_obs_row(obs_cur, A.st.obs_next, A.st.obs_init, ob, moved, xrow), ob, lane);
        // 0. the critic at the current observation (the actor's forward reuses the activation rows after it)
        float v = 0.0f;
        if constexpr (VF != COLLECT_VF_NONE) v = collect_value<VF, XT>(A.V, v_lds, act_lds, A.mlp.w_max, moved, r, xrow, lane);
        // 1. the policy at the current observation
        const PROB *pn;
        const float *logits = nullptr;  // MLP: the last layer's outputs, in the activation rows until the next forward
        if constexpr (FORM == OFFSIM_COLLECT_MLP) {
            const XT *x = collect_obs_row((const XT *)A.mlp.x_start + (int64_t)r * A.mlp.dO, A.mlp.x_next, A.mlp.x_init, A.mlp.dO, moved, xrow);
            logits = collect_forward<XT>(A.mlp, w_lds, x, act_lds, act_lds + A.mlp.w_max, lane);
            if (lane == 0) pmlp_softmax(logits, nA, pf_lds);
            wave_lds_sync();
            if (lane < nA) {
                const float p = pf_lds[lane];
                pn_lds[lane] = (PROB)p;
                if (A.out.probs) A.out.probs[o * nA + lane] = p;
            }
            wave_lds_sync();
            pn = pn_lds;
        } else {
            if constexpr (FORM == OFFSIM_COLLECT_ROWS)
                pn = xrow >= 0 ? (const PROB *)A.p_next + (int64_t)xrow * nA : (const PROB *)A.p_init + (-2 - (int64_t)xrow) * nA;
            else
                pn = pi_lds + (size_t)slot * nA;
            if (A.out.probs)
                for (int a = lane; a < nA; a += WAVE) A.out.probs[o * nA + a] = (float)pn[a];
        }
        // 2. PSRS.step
        const StepResult s = psrs_step<PL, PROB>(t, t.seg_off, perm_row, slot, cursor, pn, A.reject_mode, 0u, rng, consumed, COLLECT_WIDTH);
        if (s.status != OFFSIM_ST_OK) {  // None or KeyError: the example's `break`, for this environment (state left as it is)
            status = s.status;
            live = false;
            alive = false;
            if (lane == 0) {
                A.out.row[o] = -1;
                A.out.flags[o] = 0;
                if constexpr (VF != COLLECT_VF_NONE) A.V.rec.value[o] = A.V.rec.logp[o] = 0.0f;
            }
            continue;
        }
        if constexpr (VF != COLLECT_VF_NONE) {  // the PPO records of a served step: v(obs), logp of the served action (lane 0)
            if (lane == 0) {
                const int a = t.a[s.g];
                A.V.rec.value[o] = v;
                if constexpr (FORM == OFFSIM_COLLECT_MLP) A.V.rec.logp[o] = pmlp_logp(logits, nA, a);
                else A.V.rec.logp[o] = logf((float)pn[a]);
            }
        }
        // 3. the record, 4. the reset at terminated / truncated
        const int32_t row = t.orig_idx[s.g];
        ep_t++;
        const bool term = s.done, trunc = A.max_ep > 0 && ep_t >= A.max_ep;
        uint32_t fl = OFFSIM_COLLECT_SERVED | (term ? OFFSIM_COLLECT_TERMINATED : 0u) | (trunc ? OFFSIM_COLLECT_TRUNCATED : 0u);
        if constexpr (VF != COLLECT_VF_NONE) {  // v(next_obs) of the served row, before a reset replaces the observation (spinup's bootstrap)
            if (trunc && !term && A.V.rec.v_trunc) {
                const float vt = collect_value<VF, XT>(A.V, v_lds, act_lds, A.mlp.w_max, true, r, row, lane);
                if (lane == 0) A.V.rec.v_trunc[o] = vt;
            }
        }
        slot = s.z_next;
        xrow = row;
        moved = true;
        if (term || trunc) {
            ep_t = 0;
            if ((int64_t)ic >= t.N0) {  // psrs.py:33-35: reset() returned None; the observation stays next_obs of the row
                slot = -1;
                alive = false;
                live = false;
                none = true;
                status = OFFSIM_ST_NO_INIT;
            } else {
                const uint32_t k = init_row ? init_row[ic] : ic;
                ic++;
                slot = t.init_slot[k];
                xrow = -2 - t.init_orig[k];
                fl |= OFFSIM_COLLECT_RESET;
            }
        }
        if (alive) fl |= OFFSIM_COLLECT_ALIVE;
        if (lane == 0) {
            A.out.row[o] = row;
            A.out.flags[o] = (uint8_t)fl;
        }
    }
    if constexpr (VF != COLLECT_VF_NONE) {  // the bootstrap of a path still open: v at the observation the environment holds (0: no state)
        const float vf = had_state ? collect_value<VF, XT>(A.V, v_lds, act_lds, A.mlp.w_max, moved, r, xrow, lane) : 0.0f;
        if (lane == 0) A.V.rec.final_value[r] = vf;
    }
    // the state, for the next call
    if (moved) wave_copy_row(obs_cur, collect_obs_row(obs_cur, A.st.obs_next, A.st.obs_init, ob, moved, xrow), ob, lane);
    if (lane == 0) {
        if (consumed && ro.rng_kind == OFFSIM_STREAM_PHILOX) {
            ro.rng[4 * r + 1] = base.lo + consumed;
        } else if (consumed) {
            const U128 nb = pcg_apply(pcg_jump(inc, consumed), base);
            ro.rng[4 * r + 0] = nb.hi;
            ro.rng[4 * r + 1] = nb.lo;
        }
        ro.cur_slot[r] = slot;
        ro.init_cursor[r] = ic;
        A.st.ep_t[r] = ep_t;
        if (moved) A.st.obs_row[r] = none ? -1 : xrow;
        A.st.alive[r] = (uint8_t)alive;
        if (A.out.status) A.out.status[r] = status;
    }
}

// LDS of one workgroup: [jump tables][weights | pi][p_new f64 x 16 per wave][probs f32 x 16 per wave][2 activation rows per wave]
static size_t collect_lds_layout(int waves, size_t shared_bytes, int w_max, CollectArgs &A) {
    size_t off = (size_t)waves * (WAVE + 1) * sizeof(Jump) + ((shared_bytes + 15) & ~(size_t)15);
    A.off_pn = (uint32_t)off;
    off += (size_t)waves * PMLP_MAX_ACTIONS * sizeof(double);
    A.off_pf = (uint32_t)off;
    off += (size_t)waves * PMLP_MAX_ACTIONS * sizeof(float);
    A.off_act = (uint32_t)off;
    off += (size_t)waves * 2 * w_max * sizeof(float);
    return off;
}

// The MLP form of an offsim_collect_policy (n_out = the table's nA) or an offsim_collect_value (n_out = 1): pmlp_describe's checks, the
// observations, and the kernel's descriptor with W^T [in][out] and b packed from LDS float 0.  The float cap is the caller's.
template <typename SPEC>
static int collect_mlp(const char *who, const offsim_table *t, const SPEC &p, int n_out, CollectMlp &M) {
    PmlpNet N;
    int rc = pmlp_describe(who, p.layers_host, p.n_layers, p.dO, p.activation, p.slope, p.x_dtype, n_out, N);
    if (rc) return rc;
    M.floats = 0;
    if (!p.x_start || (t->N > 0 && (!p.x_next || !p.x_init))) return fail(OFFSIM_EINVAL, "%s: x_start / x_next / x_init is NULL", who);
    for (int l = 0; l < N.n; l++) {
        M.W[l] = N.W[l];
        M.b[l] = N.b[l];
        M.in[l] = N.in[l];
        M.out[l] = N.out[l];
        M.woff[l] = M.floats;
        M.floats += N.in[l] * N.out[l];
        M.boff[l] = N.b[l] ? M.floats : -1;
        M.floats += N.b[l] ? N.out[l] : 0;
    }
    M.n = N.n;
    M.w_max = N.w_max;
    M.act = N.act;
    M.slope = N.slope;
    M.dO = N.dO;
    M.x_start = p.x_start;
    M.x_next = p.x_next;
    M.x_init = p.x_init;
    return OFFSIM_OK;
}

// Validation of offsim_vector_collect's arguments and the actor's part of A (`who`: the entry point, in the network's error text); `shared`
// gets the bytes of the actor's LDS region (weights or pi).
static int collect_prepare(const char *who, const offsim_table *t, offsim_rollouts *ro, const offsim_collect_policy *pol, int32_t prob_mode, int32_t reject_mode,
                           int64_t T, int32_t max_episode_steps, const offsim_collect_state *st, const offsim_collect_out *out, CollectArgs &A,
                           size_t &shared) {
    int rc = check_table(t);
    if (rc) return rc;
    if (!ro || ro->R < 0 || !pol || !st || !out || T < 0 || max_episode_steps < 0) return fail(OFFSIM_EINVAL, "vector_collect: bad argument%s");
    if ((rc = check_prob_mode("vector_collect", t, prob_mode))) return rc;
    if (reject_mode != OFFSIM_REJECT_DEFAULT && reject_mode != OFFSIM_REJECT_NEVER) return fail(OFFSIM_EINVAL, "vector_collect: bad reject_mode%s");
    if (!st->ep_t || !st->obs_row || !st->alive || !st->obs || st->obs_bytes <= 0 || (t->N > 0 && (!st->obs_next || !st->obs_init)))
        return fail(OFFSIM_EINVAL, "vector_collect: bad state (ep_t, obs_row, alive, obs, obs_next, obs_init, obs_bytes)%s");
    if (T > 0 && (!out->row || !out->flags)) return fail(OFFSIM_EINVAL, "vector_collect: out->row / out->flags is NULL%s");
    if (t->N0 > 0 && (!t->init_slot || !t->init_orig)) return fail(OFFSIM_EINVAL, "vector_collect: table has no init rows%s");
    memset(&A, 0, sizeof(A));
    shared = 0;
    const size_t pb = prob_mode == OFFSIM_PROB_F32 ? 4 : 8;
    if (pol->form == OFFSIM_COLLECT_MLP) {
        rc = collect_mlp(who, t, *pol, t->nA, A.mlp);
        if (rc) return rc;
        if (A.mlp.floats > OFFSIM_COLLECT_MLP_MAX_FLOATS)
            return fail(OFFSIM_EUNSUPPORTED, "%s: the network's weights exceed OFFSIM_COLLECT_MLP_MAX_FLOATS (64 KiB of LDS)", who);
        shared = (size_t)A.mlp.floats * sizeof(float);
    } else if (pol->form == OFFSIM_COLLECT_ROWS) {
        if (t->N > 0 && (!pol->p_next || !pol->p_init)) return fail(OFFSIM_EINVAL, "vector_collect: p_next / p_init is NULL%s");
        A.p_next = pol->p_next;
        A.p_init = pol->p_init;
    } else if (pol->form == OFFSIM_COLLECT_TABULAR) {
        if (!pol->pi) return fail(OFFSIM_EINVAL, "vector_collect: pi is NULL%s");
        A.pi = pol->pi;
        shared = (size_t)t->n_slots * t->nA * pb;
    } else {
        return fail(OFFSIM_EINVAL, "vector_collect: unknown policy form%s");
    }
    A.reject_mode = reject_mode;
    A.max_ep = max_episode_steps;
    A.T = T;
    A.st = *st;
    A.out = *out;
    return OFFSIM_OK;
}

// One launch of k_collect<..., VF> for the actor's form and the observations' type (XT: the in-kernel networks' input; float where none is).
// L learners of E environments each (one learner: L = 1, E = ro->R).
template <int VF>
static int collect_launch(const offsim_table *t, offsim_rollouts *ro, int32_t form, int32_t x_dtype, int32_t prob_mode, size_t lds,
                          const CollectKArgs<VF> &A, void *stream, int L, int E) {
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)((E + COLLECT_WAVES - 1) / COLLECT_WAVES), (unsigned)L), block(COLLECT_WAVES * WAVE);
#define LAUNCH_COLLECT(PL, PROB, FORM, XT)                                                               \
    do {                                                                                                  \
        if (lds > 64 * 1024) HIP_TRY(allow_big_lds((k_collect<PL, PROB, FORM, XT, VF>), (int)lds));      \
        hipLaunchKernelGGL((k_collect<PL, PROB, FORM, XT, VF>), grid, block, lds, s, *t, *ro, A);         \
    } while (0)
#define LAUNCH_FORM_XT(PL, PROB, FORM)                                                                            \
    do {                                                                                                          \
        if (x_dtype == OFFSIM_F32) LAUNCH_COLLECT(PL, PROB, FORM, float);                                         \
        else LAUNCH_COLLECT(PL, PROB, FORM, __half);                                                              \
    } while (0)
    return with_plog_prob(t, prob_mode, [&](auto pl, auto prob) -> int {
        using PL = decltype(pl);
        using PROB = decltype(prob);
        if (form == OFFSIM_COLLECT_MLP) LAUNCH_FORM_XT(PL, PROB, OFFSIM_COLLECT_MLP);
        else if constexpr (VF == OFFSIM_VALUE_MLP) {
            if (form == OFFSIM_COLLECT_ROWS) LAUNCH_FORM_XT(PL, PROB, OFFSIM_COLLECT_ROWS);
            else LAUNCH_FORM_XT(PL, PROB, OFFSIM_COLLECT_TABULAR);
        } else if (form == OFFSIM_COLLECT_ROWS) LAUNCH_COLLECT(PL, PROB, OFFSIM_COLLECT_ROWS, float);
        else LAUNCH_COLLECT(PL, PROB, OFFSIM_COLLECT_TABULAR, float);
        LAUNCH_CHECK();
        return OFFSIM_OK;
    });
#undef LAUNCH_FORM_XT
#undef LAUNCH_COLLECT
}

extern "C" int offsim_vector_collect(const offsim_table *t, offsim_rollouts *ro, const offsim_collect_policy *pol, int32_t prob_mode,
                                     int32_t reject_mode, int64_t T, int32_t max_episode_steps, const offsim_collect_state *st,
                                     const offsim_collect_out *out, void *stream) {
    CollectArgs A;
    size_t shared;
    int rc = collect_prepare("vector_collect", t, ro, pol, prob_mode, reject_mode, T, max_episode_steps, st, out, A, shared);
    if (rc) return rc;
    const size_t lds = collect_lds_layout(COLLECT_WAVES, shared, A.mlp.w_max, A);
    if (lds > 160 * 1024) return fail(OFFSIM_EUNSUPPORTED, "vector_collect: the policy table and per-wave scratch exceed 160 KiB of LDS%s");
    if (ro->R == 0 || T == 0) return OFFSIM_OK;
    return collect_launch<COLLECT_VF_NONE>(t, ro, pol->form, pol->form == OFFSIM_COLLECT_MLP ? pol->x_dtype : OFFSIM_F32, prob_mode, lds, A, stream,
                                           1, ro->R);
}

// The critic's part of the arguments of a collect with the PPO records (k_collect's and k_collect_queue's): val and ppo checked, A.V filled,
// the critic's network placed behind the actor's region, which starts `head` bytes into the workgroup's LDS (`shared`: in, the actor's bytes;
// out, both networks').  x_dtype: in, the actor's observations' type; out, the type the in-kernel networks read.
static int collect_prepare_value(const char *who, const char *who_critic, const offsim_table *t, const offsim_collect_policy *pol,
                                 const offsim_collect_value *val, const offsim_collect_ppo_out *ppo, int64_t T, int E, size_t head, CollectPpoArgs &A,
                                 size_t &shared, int &x_dtype) {
    memset(&A.V, 0, sizeof(A.V));
    if (!val || !ppo) return fail(OFFSIM_EINVAL, "%s: val / ppo is NULL", who);
    if (T > 0 && (!ppo->value || !ppo->logp || !ppo->final_value)) return fail(OFFSIM_EINVAL, "%s: ppo->value / logp / final_value is NULL", who);
    CollectValue &V = A.V;
    if (val->form == OFFSIM_VALUE_MLP) {
        int rc = collect_mlp(who_critic, t, *val, 1, V.mlp);
        if (rc) return rc;
        if (pol->form == OFFSIM_COLLECT_MLP && val->x_dtype != pol->x_dtype)
            return fail(OFFSIM_EINVAL, "%s: the actor and the critic read observations of different types", who);
        if (A.mlp.floats + V.mlp.floats > OFFSIM_COLLECT_MLP_MAX_FLOATS)
            return fail(OFFSIM_EUNSUPPORTED, "%s: the actor's and the critic's weights exceed OFFSIM_COLLECT_MLP_MAX_FLOATS (64 KiB of LDS)", who);
        x_dtype = val->x_dtype;
        if (V.mlp.w_max > A.mlp.w_max) A.mlp.w_max = V.mlp.w_max;
        const size_t actor = (shared + 15) & ~(size_t)15;
        V.off_w = (uint32_t)(head + actor);
        shared = actor + (size_t)V.mlp.floats * sizeof(float);
    } else if (val->form == OFFSIM_VALUE_ROWS) {
        if (t->N > 0 && (!val->v_next || !val->v_init)) return fail(OFFSIM_EINVAL, "%s: v_next / v_init is NULL", who);
        V.v_next = val->v_next;
        V.v_init = val->v_init;
    } else {
        return fail(OFFSIM_EINVAL, "%s: unknown critic form", who);
    }
    V.rec = *ppo;
    V.envs = E;
    return OFFSIM_OK;
}

// offsim_vector_collect_ppo (L = 1, E = ro->R) and offsim_vector_collect_ppo_pop: L learners' stacked networks, E environments each.
// `who` / `who_critic` name the entry point in the error text.
static int collect_ppo_run(const char *who, const char *who_critic, const offsim_table *t, offsim_rollouts *ro, const offsim_collect_policy *pol,
                           const offsim_collect_value *val, int L, int E, int32_t prob_mode, int32_t reject_mode, int64_t T,
                           int32_t max_episode_steps, const offsim_collect_state *st, const offsim_collect_out *out,
                           const offsim_collect_ppo_out *ppo, void *stream) {
    CollectPpoArgs A;
    size_t shared;
    int rc = collect_prepare(who, t, ro, pol, prob_mode, reject_mode, T, max_episode_steps, st, out, A, shared);
    if (rc) return rc;
    int x_dtype = pol->form == OFFSIM_COLLECT_MLP ? pol->x_dtype : OFFSIM_F32;
    if ((rc = collect_prepare_value(who, who_critic, t, pol, val, ppo, T, E, (size_t)COLLECT_WAVES * (WAVE + 1) * sizeof(Jump), A, shared, x_dtype))) return rc;
    const size_t lds = collect_lds_layout(COLLECT_WAVES, shared, A.mlp.w_max, A);
    if (lds > 160 * 1024) return fail(OFFSIM_EUNSUPPORTED, "%s: the policy table, the critic and per-wave scratch exceed 160 KiB of LDS", who);
    if (ro->R == 0 || T == 0) return OFFSIM_OK;
    if (val->form == OFFSIM_VALUE_MLP) return collect_launch<OFFSIM_VALUE_MLP>(t, ro, pol->form, x_dtype, prob_mode, lds, A, stream, L, E);
    return collect_launch<OFFSIM_VALUE_ROWS>(t, ro, pol->form, x_dtype, prob_mode, lds, A, stream, L, E);
}

extern "C" int offsim_vector_collect_ppo(const offsim_table *t, offsim_rollouts *ro, const offsim_collect_policy *pol, const offsim_collect_value *val,
                                         int32_t prob_mode, int32_t reject_mode, int64_t T, int32_t max_episode_steps, const offsim_collect_state *st,
                                         const offsim_collect_out *out, const offsim_collect_ppo_out *ppo, void *stream) {
    return collect_ppo_run("vector_collect_ppo", "vector_collect_ppo critic", t, ro, pol, val, 1, ro ? ro->R : 0, prob_mode, reject_mode, T,
                           max_episode_steps, st, out, ppo, stream);
}

extern "C" int offsim_vector_collect_ppo_pop(const offsim_table *t, offsim_rollouts *ro, const offsim_collect_policy *pol,
                                             const offsim_collect_value *val, int32_t L, int32_t E, int32_t prob_mode, int32_t reject_mode, int64_t T,
                                             int32_t max_episode_steps, const offsim_collect_state *st, const offsim_collect_out *out,
                                             const offsim_collect_ppo_out *ppo, void *stream) {
    if (L <= 0 || E <= 0 || L > 65535) return fail(OFFSIM_EINVAL, "vector_collect_ppo_pop: L must be in 1..65535 and E >= 1%s");
    if (!ro || !pol || !val) return fail(OFFSIM_EINVAL, "vector_collect_ppo_pop: ro / pol / val is NULL%s");
    if ((int64_t)L * E != (int64_t)ro->R) return fail(OFFSIM_EINVAL, "vector_collect_ppo_pop: ro->R must be L * E%s");
    if (pol->form != OFFSIM_COLLECT_MLP || val->form != OFFSIM_VALUE_MLP)
        return fail(OFFSIM_EUNSUPPORTED, "vector_collect_ppo_pop: only OFFSIM_COLLECT_MLP actors and OFFSIM_VALUE_MLP critics%s");
    return collect_ppo_run("vector_collect_ppo_pop", "vector_collect_ppo_pop critic", t, ro, pol, val, L, E, prob_mode, reject_mode, T,
                           max_episode_steps, st, out, ppo, stream);
}
