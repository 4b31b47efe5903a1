// td_pop.hpp -- a population of tabular TD learners in one launch (offsim_eval_td_pop) and their learning curves (offsim_td_curves).
//
// The learner loop itself is k_eval_mc<PL, double, TD = true, ROWP = false, POP = true> (offsim_hip.hip): the one definition of the step,
// the behaviour block, the TD update, the episode bookkeeping and the write-back.  What the population adds is here: the kernel arguments
// of that instance, from which the kernel overwrites its per-launch hyper-parameters with learner l's before the loop starts, and the
// reduction of the per-seed returns to one curve per learner.
//
//   ro.R = L * S, learner-major: rollout r = l * S + j is learner l on seed j and walks queue order j (ro.perm / ro.init_perm hold S orders,
//   only read).  A workgroup holds rollouts of ONE learner -- grid = L * ceil(S / waves), workgroup b serves learner b / ceil(S / waves) and
//   seeds (b % ceil(S / waves)) * waves + wave, the waves past S idle -- so the learner's pi is staged in LDS once per workgroup and its
//   scalars (alpha, epsilon, gamma, behaviour, the schedule rows, the discount table row) are workgroup-uniform scalar loads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The index rule is the same for the three learner kernels (k_eval_mc, k_eval_mc_exo, k_eval_queue; each applies it in its own text, see the
// note above each kernel): the waves past S leave after the staging barrier, and rollout (l, j) walks queue orders j of every queue family
// while its streams, cursors, current state and outputs are row r's own.
//
// The per-learner kernel arguments: what offsim_td_pop holds per learner, filled by td_pop_fields.  Every POP instance carries them behind
// its kernel's own argument struct, so the arguments of the other instances are what they were.
struct TdPopFields {
    int32_t S;
    const double *alpha, *epsilon, *gamma;  // [L]
    const double *gamma_pow;                // [L, n_gamma_pow]
    const int32_t *behaviour;               // [L]
    const double *alpha_ep, *epsilon_ep;    // [L, n_sched] or NULL
    const double *pi;                       // [L, rows, nA], or one table when pi_stride == 0 (k_eval_queue: NULL when no learner reads one)
    int64_t pi_stride;
};
static TdPopFields td_pop_fields(const offsim_td_pop *pop, int32_t S) {
    return TdPopFields{S, pop->alpha, pop->epsilon, pop->gamma, pop->gamma_pow, pop->behaviour, pop->alpha_ep, pop->epsilon_ep, pop->pi, pop->pi_stride};
}
// the grid of a POP launch of R = L * S rollouts: a workgroup holds rollouts of one learner
static unsigned pop_grid(int64_t R, int32_t S, int waves) { return (unsigned)(R / S) * (unsigned)((S + waves - 1) / waves); }
// the kernel-argument layout of a POP instance must not move: pinned next to each struct
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"  // (two bases: not standard-layout; laid out base after base)
template <typename ARGS>
constexpr bool td_pop_layout(size_t size, size_t s_at, size_t pi_stride_at) {
    return sizeof(ARGS) == size && offsetof(ARGS, S) == s_at && offsetof(ARGS, pi_stride) == pi_stride_at;
}
#pragma clang diagnostic pop

struct TdPopArgs : RowPolicyArgs, TdPopFields {};  // (the row-policy members stay NULL: the learner drivers index their tables by state)
static_assert(td_pop_layout<TdPopArgs>(104, 24, 96), "kernel arguments of k_eval_mc<.., TD, false, POP>");

// curve of learner l at episode e over the seeds that completed it: one thread per (l, e), the seeds in order j = 0 .. S - 1, two passes,
// no atomics -- the sums are a plain left-to-right f64 loop, so two calls give the same bits and a host loop in that order gives them too
__global__ void __launch_bounds__(256) k_td_curves(const double *__restrict__ ep_g, const int64_t *__restrict__ n_ep, int32_t L, int32_t S,
                                                   int64_t ep_cap, int64_t *__restrict__ n_out, double *__restrict__ mean_out,
                                                   double *__restrict__ var_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)L * ep_cap) return;
    const int64_t l = i / ep_cap, e = i - l * ep_cap;
    int64_t n = 0;
    double sum = 0.0;
    for (int32_t j = 0; j < S; j++) {
        const int64_t r = l * S + j;
        if (e < n_ep[r]) {
            sum = sum + ep_g[r * ep_cap + e];
            n++;
        }
    }
    double mean = __longlong_as_double(0x7ff8000000000000ll), var = mean;  // no seed got this far: NaN
    if (n > 0) {
        mean = sum / (double)n;
        double ss = 0.0;
        for (int32_t j = 0; j < S; j++) {
            const int64_t r = l * S + j;
            if (e < n_ep[r]) {
                const double d = ep_g[r * ep_cap + e] - mean;
                ss = ss + d * d;
            }
        }
        var = ss / (double)n;
    }
    n_out[i] = n;
    mean_out[i] = mean;
    var_out[i] = var;
}
