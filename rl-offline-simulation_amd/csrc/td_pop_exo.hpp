// td_pop_exo.hpp -- a population of tabular TD learners on PSRS_Exo in one launch (offsim_eval_td_exo_pop): the kernel arguments of
// k_eval_mc_exo<PL, double, TD = true, POP = true> (csrc/eval_exo.hpp).
//
// The loop is k_eval_mc_exo's TD loop, the behaviour block is td_behaviour (offsim_hip.hip) on the Q row of the current observation, and
// the population index is csrc/td_pop.hpp's, rule for rule:
//
//   rs.R = rx.R = L * S, learner-major: rollout r = l * S + j is learner l on seed j and walks queue orders j of both families (rs.perm /
//   rs.init_perm and rx.perm hold S orders, only read).  A workgroup holds rollouts of ONE learner -- grid = L * ceil(S / waves), workgroup b
//   serves learner b / ceil(S / waves) and seeds (b % ceil(S / waves)) * waves + wave, the waves past S leave after the staging barrier -- so
//   the learner's pi is staged in LDS once per workgroup and its scalars (alpha, epsilon, gamma, behaviour, the schedule rows, the discount
//   table row) are workgroup-uniform scalar loads that overwrite the per-launch values before anything reads them.
//
// Included by eval_exo.hpp behind ExoArgs.
#pragma once

struct TdPopExoArgs : ExoArgs {
    int32_t S;
    const double *alpha, *epsilon, *gamma;  // [L]
    const double *gamma_pow;                // [L, n_gamma_pow]
    const int32_t *behaviour;               // [L]
    const double *alpha_ep, *epsilon_ep;    // [L, n_sched] or NULL
    const double *pi;                       // [L, n_obs, nA], or one table when pi_stride == 0
    int64_t pi_stride;
};
