// The PPO buffer over step-major [T, E] records (include/offsim.h: offsim_ppo_advantages; VectorPSRS.collect_ppo, ppo_advantages):
// spinup's PPOBuffer.finish_path (GAE-lambda advantages, rewards-to-go) under the path rules of the reference's agent
// (offsim4rl/agents/ppo.py:106-158), then PPOBuffer.get's normalisation with mpi_statistics_scalar over all environments.
//
//   k_ppo_gae    one thread per environment scans t = T-1 .. 0 (thread e reads [t*E + e]: every t is one coalesced line per wave),
//                f64 accumulators, f32 stores; the block's sum of the stored advantages and its count of valid entries -> work
//   k_ppo_sqdev  the mean from the partials (thread 0 of every block, in block order), the block's sum of (adv - mean)^2 -> work
//   k_ppo_norm   mean and std from the partials, adv_norm = (adv - mean) / std; block 0 writes stats
// No float atomics: every sum runs in a fixed order, so two runs give the same bits.
//
// A population (offsim_ppo_advantages_pop) runs the same three kernels on a grid (ceil(E / 256), L) over [T, L * E] records: row l of the
// grid takes the columns l * E + [0, E) (ld: the records' row stride), its own 3 * gridDim.x partials and its own stats pair, so learner l's
// sums run in the order the single call has on a contiguous [T, E] input.  One learner is the row l = 0 with ld = E.
#pragma once

#define PPO_BLOCK 256

// the block's sum of one double per thread, in a fixed tree order; the result in thread 0
__device__ __forceinline__ double ppo_block_sum(double x, double *sh) {
    sh[threadIdx.x] = x;
    __syncthreads();
    for (int w = PPO_BLOCK / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(PPO_BLOCK) k_ppo_gae(const float *__restrict__ rew, const float *__restrict__ val, const uint8_t *__restrict__ flags,
                                                       const float *__restrict__ final_value, const float *__restrict__ v_trunc, int64_t T, int64_t E,
                                                       int64_t ld, double gamma, double lam, int boot_mode, float *__restrict__ adv, float *__restrict__ ret,
                                                       double *__restrict__ work) {
    __shared__ double sh[PPO_BLOCK];
    const int64_t e = (int64_t)blockIdx.x * PPO_BLOCK + threadIdx.x;
    const int64_t c = (int64_t)blockIdx.y * E + e;  // the environment's column of the records
    double sum = 0.0, n = 0.0;
    if (e < E) {
        bool open = true;  // no valid step seen yet (scanning backwards): the first one closes an open path unless it ends one itself
        double v_next = 0.0, A = 0.0, G = 0.0;
        for (int64_t t = T - 1; t >= 0; t--) {
            const int64_t o = t * ld + c;
            const uint32_t fl = flags[o];
            if (!(fl & OFFSIM_COLLECT_SERVED)) {
                adv[o] = 0.0f;
                ret[o] = 0.0f;
                continue;
            }
            const double v = val[o], r = rew[o];
            const bool term = fl & OFFSIM_COLLECT_TERMINATED, trunc = fl & OFFSIM_COLLECT_TRUNCATED;
            if (term || trunc) {  // end_episode: finish_path(bootstrap)
                double b;
                if (boot_mode == OFFSIM_PPO_BOOT_REFERENCE) b = (trunc || t == T - 1) ? v : 0.0;
                else b = term ? 0.0 : (double)v_trunc[o];
                v_next = b;
                A = 0.0;
                G = b;
            } else if (open) {  // the path the call leaves open: step's epoch cut, or the environment stopped
                v_next = final_value[c];
                A = 0.0;
                G = v_next;
            }
            open = false;
            const double delta = r + gamma * v_next - v;
            A = delta + gamma * lam * A;
            G = r + gamma * G;
            const float a32 = (float)A;
            adv[o] = a32;
            ret[o] = (float)G;
            v_next = v;
            sum += (double)a32;
            n += 1.0;
        }
    }
    sum = ppo_block_sum(sum, sh);
    n = ppo_block_sum(n, sh);
    if (work && threadIdx.x == 0) {
        work += (size_t)blockIdx.y * 3 * gridDim.x;
        work[blockIdx.x] = sum;
        work[gridDim.x + blockIdx.x] = n;
    }
}

// mean over the partials of k_ppo_gae, in block order (thread 0), broadcast through LDS; n in *n_out
__device__ __forceinline__ double ppo_mean(const double *work, int nb, double *sh, double *n_out) {
    if (threadIdx.x == 0) {
        double s = 0.0, n = 0.0;
        for (int b = 0; b < nb; b++) {
            s += work[b];
            n += work[nb + b];
        }
        sh[0] = n > 0.0 ? s / n : 0.0;
        sh[1] = n;
    }
    __syncthreads();
    const double m = sh[0];
    *n_out = sh[1];
    __syncthreads();
    return m;
}

__global__ void __launch_bounds__(PPO_BLOCK) k_ppo_sqdev(const float *__restrict__ adv, const uint8_t *__restrict__ flags, int64_t T, int64_t E,
                                                         int64_t ld, double *__restrict__ work) {
    __shared__ double sh[PPO_BLOCK];
    double n;
    work += (size_t)blockIdx.y * 3 * gridDim.x;
    const double mean = ppo_mean(work, gridDim.x, sh, &n);
    const int64_t e = (int64_t)blockIdx.x * PPO_BLOCK + threadIdx.x;
    double q = 0.0;
    if (e < E)
        for (int64_t t = 0; t < T; t++) {
            const int64_t o = t * ld + (int64_t)blockIdx.y * E + e;
            if (flags[o] & OFFSIM_COLLECT_SERVED) {
                const double d = (double)adv[o] - mean;
                q += d * d;
            }
        }
    q = ppo_block_sum(q, sh);
    if (threadIdx.x == 0) work[2 * gridDim.x + blockIdx.x] = q;
}

__global__ void __launch_bounds__(PPO_BLOCK) k_ppo_norm(const float *__restrict__ adv, const uint8_t *__restrict__ flags, int64_t T, int64_t E,
                                                        int64_t ld, const double *__restrict__ work, float *__restrict__ adv_norm,
                                                        double *__restrict__ stats) {
    __shared__ double sh[PPO_BLOCK];
    const int nb = gridDim.x;
    work += (size_t)blockIdx.y * 3 * nb;
    stats += 2 * blockIdx.y;
    double n;
    const double mean = ppo_mean(work, nb, sh, &n);
    if (threadIdx.x == 0) {
        double q = 0.0;
        for (int b = 0; b < nb; b++) q += work[2 * nb + b];
        sh[0] = n > 0.0 ? sqrt(q / n) : 0.0;
    }
    __syncthreads();
    const double std_ = sh[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        stats[0] = mean;
        stats[1] = std_;
    }
    const int64_t e = (int64_t)blockIdx.x * PPO_BLOCK + threadIdx.x;
    if (e >= E) return;
    for (int64_t t = 0; t < T; t++) {
        const int64_t o = t * ld + (int64_t)blockIdx.y * E + e;
        const float a = adv[o];
        adv_norm[o] = n > 0.0 && (flags[o] & OFFSIM_COLLECT_SERVED) ? (float)(((double)a - mean) / std_) : a;
    }
}

// offsim_ppo_advantages (L = 1) and offsim_ppo_advantages_pop over [T, L * E] records
static int ppo_advantages_run(const char *who, const float *rew, const float *value, const uint8_t *flags, const float *final_value, const float *v_trunc,
                              int64_t T, int64_t L, int64_t E, double gamma, double lam, int32_t bootstrap, float *adv, float *ret, float *adv_norm,
                              double *stats, double *work, void *stream) {
    if (T < 0 || E < 0) return fail(OFFSIM_EINVAL, "%s: T and E must be >= 0", who);
    if (bootstrap != OFFSIM_PPO_BOOT_REFERENCE && bootstrap != OFFSIM_PPO_BOOT_SPINUP) return fail(OFFSIM_EINVAL, "%s: bad bootstrap mode", who);
    if (!(gamma >= 0.0 && gamma <= 1.0) || !(lam >= 0.0 && lam <= 1.0)) return fail(OFFSIM_EINVAL, "%s: gamma and lam must be in [0, 1]", who);
    if (E > 0 && (int64_t)((E + PPO_BLOCK - 1) / PPO_BLOCK) > 0x7fffffffll) return fail(OFFSIM_EINVAL, "%s: too many environments", who);
    const bool any = T > 0 && E > 0;
    if (any && (!rew || !value || !flags || !final_value || !adv || !ret))
        return fail(OFFSIM_EINVAL, "%s: rew / value / flags / final_value / adv / ret is NULL", who);
    if (any && bootstrap == OFFSIM_PPO_BOOT_SPINUP && !v_trunc) return fail(OFFSIM_EINVAL, "%s: OFFSIM_PPO_BOOT_SPINUP needs v_trunc", who);
    if (adv_norm && (!stats || !work)) return fail(OFFSIM_EINVAL, "%s: adv_norm needs stats and work", who);
    hipStream_t s = (hipStream_t)stream;
    if (!any) {  // nothing valid: mean = std = 0
        if (adv_norm) HIP_TRY(hipMemsetAsync(stats, 0, (size_t)L * 2 * sizeof(double), s));
        return OFFSIM_OK;
    }
    const dim3 grid((unsigned)((E + PPO_BLOCK - 1) / PPO_BLOCK), (unsigned)L);
    const int64_t ld = L * E;
    hipLaunchKernelGGL(k_ppo_gae, grid, dim3(PPO_BLOCK), 0, s, rew, value, flags, final_value, v_trunc, T, E, ld, gamma, lam, (int)bootstrap, adv, ret,
                       adv_norm ? work : nullptr);
    LAUNCH_CHECK();
    if (!adv_norm) return OFFSIM_OK;
    hipLaunchKernelGGL(k_ppo_sqdev, grid, dim3(PPO_BLOCK), 0, s, (const float *)adv, flags, T, E, ld, work);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ppo_norm, grid, dim3(PPO_BLOCK), 0, s, (const float *)adv, flags, T, E, ld, (const double *)work, adv_norm, stats);
    LAUNCH_CHECK();
    return OFFSIM_OK;
}

extern "C" int offsim_ppo_advantages(const float *rew, const float *value, const uint8_t *flags, const float *final_value, const float *v_trunc,
                                     int64_t T, int64_t E, double gamma, double lam, int32_t bootstrap, float *adv, float *ret, float *adv_norm,
                                     double *stats, double *work, void *stream) {
    return ppo_advantages_run("ppo_advantages", rew, value, flags, final_value, v_trunc, T, 1, E, gamma, lam, bootstrap, adv, ret, adv_norm, stats, work,
                              stream);
}

extern "C" int offsim_ppo_advantages_pop(const float *rew, const float *value, const uint8_t *flags, const float *final_value, const float *v_trunc,
                                         int64_t T, int32_t L, int64_t E, double gamma, double lam, int32_t bootstrap, float *adv, float *ret,
                                         float *adv_norm, double *stats, double *work, void *stream) {
    if (L <= 0 || E <= 0 || L > 65535) return fail(OFFSIM_EINVAL, "ppo_advantages_pop: L must be in 1..65535 and E >= 1%s");
    return ppo_advantages_run("ppo_advantages_pop", rew, value, flags, final_value, v_trunc, T, L, E, gamma, lam, bootstrap, adv, ret, adv_norm, stats,
                              work, stream);
}
