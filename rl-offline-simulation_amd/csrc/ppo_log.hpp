// The epoch log of the reference's PPO agent over step-major [T, L * E] records (include/offsim.h: offsim_ppo_epoch_log;
// evaluators/ppo_log.py): what PPOAgentRevealed hands to its EpochLogger during an epoch (offsim4rl/agents/ppo.py:103-160, :225-227) --
// EpRet / EpLen of every episode that ended, the open episode of an environment in which none ended, VVals of every step -- and
// spinup's mpi_statistics_scalar of them, per learner, E environments standing for E MPI processes.
//
//   k_ppo_epoch_log   one workgroup per learner, a lane per environment striding over E (lane i reads column l * E + i of a step-major
//                     row: adjacent lanes, adjacent addresses).  First walk over t = 0 .. T-1 from the carried (open_ret, open_len):
//                     the sums, extremes and counts of the entries and of the values, the raw lists; an LDS tree of fixed shape gives
//                     the means.  Second walk from the same carried state: the squared deviations from those means, a second tree, and
//                     the carry of the next epoch, written only now (so the second walk starts where the first did).
// Everything is f64 and every sum runs in a fixed order (a lane's environments in order, each in step order, then the tree): no atomics,
// the same bits every run, and learner l's bits those of the L = 1 call on its columns (the block sees only l * E + [0, E) and ld).
#pragma once

#define PPL_BLOCK 256
#define PPL_CHUNK 8  // steps loaded ahead of the serial walk (the loads do not depend on the carry)

enum { PPL_SUM = 0, PPL_MIN = 1, PPL_MAX = 2 };

// K values per thread reduced over the block in a fixed tree, each with its own operation; the results to every thread
template <int K>
__device__ __forceinline__ void ppl_reduce(double (&x)[K], const int (&kind)[K], double *sh) {
#pragma unroll
    for (int k = 0; k < K; k++) sh[k * PPL_BLOCK + threadIdx.x] = x[k];
    __syncthreads();
    for (int w = PPL_BLOCK / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
#pragma unroll
            for (int k = 0; k < K; k++) {
                const double a = sh[k * PPL_BLOCK + threadIdx.x], b = sh[k * PPL_BLOCK + threadIdx.x + w];
                sh[k * PPL_BLOCK + threadIdx.x] = kind[k] == PPL_SUM ? a + b : kind[k] == PPL_MIN ? (b < a ? b : a) : (b > a ? b : a);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < K; k++) x[k] = sh[k * PPL_BLOCK];
    __syncthreads();
}

// One environment's valid steps in order, from the carried (ret, len): step(v) at every valid step, episode(ret, len) at every end.
// Leaves the carry of the next epoch in (ret, len); returns the number of valid steps.
template <typename STEP, typename EPISODE>
__device__ __forceinline__ int64_t ppl_walk(const float *__restrict__ rew, const float *__restrict__ val, const uint8_t *__restrict__ valid,
                                            const uint8_t *__restrict__ term, const uint8_t *__restrict__ trunc, int64_t T, int64_t ld, int64_t c,
                                            int mode, double &ret, int32_t &len, STEP &&step, EPISODE &&episode) {
    int64_t served = 0;
    for (int64_t t0 = 0; t0 < T; t0 += PPL_CHUNK) {
        uint32_t f[PPL_CHUNK];
        float r[PPL_CHUNK], v[PPL_CHUNK];
#pragma unroll
        for (int k = 0; k < PPL_CHUNK; k++) {
            const int64_t t = t0 + k;
            f[k] = 0;
            r[k] = v[k] = 0.0f;
            if (t < T) {
                const int64_t o = t * ld + c;
                f[k] = valid[o] ? 1u | ((term[o] | trunc[o]) ? 2u : 0u) : 0u;
                r[k] = rew[o];
                if (val) v[k] = val[o];
            }
        }
#pragma unroll
        for (int k = 0; k < PPL_CHUNK; k++) {
            if (!(f[k] & 1u)) continue;
            served++;
            ret += (double)r[k];
            len++;
            step((double)v[k]);
            if (f[k] & 2u) {  // end_episode: it does not count its own transition (ppo.py:116-133; step does, :138-140)
                episode(ret, mode == OFFSIM_EPLEN_STEPS ? len : len - 1);
                ret = 0.0;
                len = 0;
            }
        }
    }
    return served;
}

__global__ void __launch_bounds__(PPL_BLOCK) k_ppo_epoch_log(const float *__restrict__ rew, const float *__restrict__ val,
                                                             const uint8_t *__restrict__ valid, const uint8_t *__restrict__ term,
                                                             const uint8_t *__restrict__ trunc, int64_t T, int64_t E, int64_t ld, int mode,
                                                             double *__restrict__ open_ret, int32_t *__restrict__ open_len,
                                                             double *__restrict__ stats, int64_t *__restrict__ counts,
                                                             double *__restrict__ ep_ret, int32_t *__restrict__ ep_len, int32_t *__restrict__ n_ep,
                                                             int64_t ep_cap) {
    __shared__ double sh[10 * PPL_BLOCK];
    const int64_t c0 = (int64_t)blockIdx.x * E;
    const double inf = __builtin_inf();
    // ---- first walk: entries (ended episodes, or the open one) and values
    double a[10] = {0.0, 0.0, 0.0, 0.0, inf, -inf, 0.0, 0.0, inf, -inf};  // sum ret, sum len, entries, ended | min, max ret | sum v, steps | min, max v
    for (int64_t e = threadIdx.x; e < E; e += PPL_BLOCK) {
        const int64_t c = c0 + e;
        double ret = open_ret[c];
        int32_t len = open_len[c];
        int64_t ended = 0;
        auto entry = [&](double g, int32_t n) {
            a[0] += g;
            a[1] += (double)n;
            a[2] += 1.0;
            a[4] = g < a[4] ? g : a[4];
            a[5] = g > a[5] ? g : a[5];
        };
        const int64_t served = ppl_walk(
            rew, val, valid, term, trunc, T, ld, c, mode, ret, len,
            [&](double v) {
                a[6] += v;
                a[8] = v < a[8] ? v : a[8];
                a[9] = v > a[9] ? v : a[9];
            },
            [&](double g, int32_t n) {
                entry(g, n);
                if (ended < ep_cap) {
                    if (ep_ret) ep_ret[c * ep_cap + ended] = g;
                    if (ep_len) ep_len[c * ep_cap + ended] = n;
                }
                ended++;
            });
        a[3] += (double)ended;
        a[7] += (double)served;
        if (served > 0 && ended == 0) entry(ret, len);  // _log_epoch_metrics (ppo.py:226-227): the open episode, its transitions so far
        if (n_ep) n_ep[c] = (int32_t)ended;
    }
    const int kind[10] = {PPL_SUM, PPL_SUM, PPL_SUM, PPL_SUM, PPL_MIN, PPL_MAX, PPL_SUM, PPL_SUM, PPL_MIN, PPL_MAX};
    ppl_reduce<10>(a, kind, sh);
    const double nan = __builtin_nan("");
    const double n = a[2], nv = a[7];
    const double mean = n > 0.0 ? a[0] / n : nan, vmean = nv > 0.0 ? a[6] / nv : nan;
    // ---- second walk: squared deviations, from the same carried state; the carry moves on here
    double q[2] = {0.0, 0.0};
    for (int64_t e = threadIdx.x; e < E; e += PPL_BLOCK) {
        const int64_t c = c0 + e;
        double ret = open_ret[c];
        int32_t len = open_len[c];
        int64_t ended = 0;
        const int64_t served = ppl_walk(
            rew, val, valid, term, trunc, T, ld, c, mode, ret, len,
            [&](double v) { q[1] += (v - vmean) * (v - vmean); },
            [&](double g, int32_t) {
                q[0] += (g - mean) * (g - mean);
                ended++;
            });
        if (served > 0 && ended == 0) q[0] += (ret - mean) * (ret - mean);
        open_ret[c] = ret;
        open_len[c] = len;
    }
    const int kind2[2] = {PPL_SUM, PPL_SUM};
    ppl_reduce<2>(q, kind2, sh);
    if (threadIdx.x == 0) {
        double *s = stats + (size_t)blockIdx.x * OFFSIM_PPO_LOG_STATS;
        s[0] = mean;
        s[1] = n > 0.0 ? sqrt(q[0] / n) : nan;
        s[2] = n > 0.0 ? a[4] : nan;
        s[3] = n > 0.0 ? a[5] : nan;
        s[4] = n > 0.0 ? a[1] / n : nan;
        s[5] = vmean;
        s[6] = nv > 0.0 ? sqrt(q[1] / nv) : nan;
        s[7] = nv > 0.0 ? a[8] : nan;
        s[8] = nv > 0.0 ? a[9] : nan;
        s[9] = n;
        counts[2 * blockIdx.x] = (int64_t)a[3];
        counts[2 * blockIdx.x + 1] = (int64_t)nv;
    }
}

// offsim_ppo_epoch_log (L = 1) and offsim_ppo_epoch_log_pop
static int ppo_epoch_log_run(const char *who, const float *rew, const float *value, const uint8_t *valid, const uint8_t *terminated,
                             const uint8_t *truncated, int64_t T, int64_t L, int64_t E, int32_t eplen_mode, double *open_ret, int32_t *open_len,
                             double *stats, int64_t *counts, double *ep_ret, int32_t *ep_len, int32_t *n_ep, int64_t ep_cap, void *stream) {
    if (T < 1 || E < 1) return fail(OFFSIM_EINVAL, "%s: T and E must be >= 1", who);
    if (L < 1 || L > 65535) return fail(OFFSIM_EINVAL, "%s: L must be in 1..65535", who);
    if (eplen_mode != OFFSIM_EPLEN_REFERENCE && eplen_mode != OFFSIM_EPLEN_STEPS) return fail(OFFSIM_EINVAL, "%s: bad EpLen mode", who);
    if (!rew || !value || !valid || !terminated || !truncated) return fail(OFFSIM_EINVAL, "%s: rew / value / valid / terminated / truncated is NULL", who);
    if (!open_ret || !open_len) return fail(OFFSIM_EINVAL, "%s: the carried state open_ret / open_len is NULL", who);
    if (!stats || !counts) return fail(OFFSIM_EINVAL, "%s: stats / counts is NULL", who);
    if (ep_cap < 0) return fail(OFFSIM_EINVAL, "%s: ep_cap must be >= 0", who);
    if (E > 0x7fffffffffffffffll / L || T > 0x7fffffffffffffffll / (L * E)) return fail(OFFSIM_EINVAL, "%s: T * L * E overflows", who);
    hipLaunchKernelGGL(k_ppo_epoch_log, dim3((unsigned)L), dim3(PPL_BLOCK), 0, (hipStream_t)stream, rew, value, valid, terminated, truncated, T, E,
                       L * E, (int)eplen_mode, open_ret, open_len, stats, counts, ep_ret, ep_len, n_ep, ep_cap);
    LAUNCH_CHECK();
    return OFFSIM_OK;
}

extern "C" int offsim_ppo_epoch_log(const float *rew, const float *value, const uint8_t *valid, const uint8_t *terminated, const uint8_t *truncated,
                                    int64_t T, int64_t E, int32_t eplen_mode, double *open_ret, int32_t *open_len, double *stats, int64_t *counts,
                                    double *ep_ret, int32_t *ep_len, int32_t *n_ep, int64_t ep_cap, void *stream) {
    return ppo_epoch_log_run("ppo_epoch_log", rew, value, valid, terminated, truncated, T, 1, E, eplen_mode, open_ret, open_len, stats, counts, ep_ret,
                             ep_len, n_ep, ep_cap, stream);
}

extern "C" int offsim_ppo_epoch_log_pop(const float *rew, const float *value, const uint8_t *valid, const uint8_t *terminated,
                                        const uint8_t *truncated, int64_t T, int32_t L, int64_t E, int32_t eplen_mode, double *open_ret,
                                        int32_t *open_len, double *stats, int64_t *counts, double *ep_ret, int32_t *ep_len, int32_t *n_ep,
                                        int64_t ep_cap, void *stream) {
    return ppo_epoch_log_run("ppo_epoch_log_pop", rew, value, valid, terminated, truncated, T, L, E, eplen_mode, open_ret, open_len, stats, counts,
                             ep_ret, ep_len, n_ep, ep_cap, stream);
}
