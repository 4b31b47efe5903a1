// td_pop_queue.hpp -- a population of tabular TD learners on QueueEvaluator in one launch (offsim_eval_queue_pop): the kernel arguments of
// k_eval_queue<TD = true, POP = true> (csrc/eval_queue.hpp).
//
// The loop is k_eval_queue's learner loop -- td_behaviour on the Q row of the current state, queue_draw, the lazy mt_seed_lds under
// tie_reseed, the pop, the update, the snapshots, the episode bookkeeping and the write-back, none of it restated -- and the population
// index is csrc/td_pop.hpp's, rule for rule:
//
//   ro.R = L * S, learner-major: rollout r = l * S + j is learner l on seed j and walks queue orders j (ro.perm / ro.init_perm hold S orders,
//   only read), while its action stream, cursors, init cursor and current slot are row r's own.  A workgroup holds rollouts of ONE learner --
//   grid = L * ceil(S / waves), workgroup b serves learner b / ceil(S / waves) and seeds (b % ceil(S / waves)) * waves + wave, the waves past
//   S leave after the staging barrier -- so the learner's pi is staged in LDS once per workgroup and its scalars (alpha, epsilon, gamma,
//   behaviour, the schedule rows, the discount table row) are workgroup-uniform scalar loads that overwrite the per-launch values before
//   anything reads them.
//
// Included by eval_queue.hpp behind QueueArgs.
#pragma once

struct QueuePopArgs : QueueArgs {
    int32_t S;
    const double *alpha, *epsilon, *gamma;  // [L]
    const double *gamma_pow;                // [L, n_gamma_pow]
    const int32_t *behaviour;               // [L]
    const double *alpha_ep, *epsilon_ep;    // [L, n_sched] or NULL
    const double *pi;                       // [L, nZ, nA], or one table when pi_stride == 0; NULL: no learner reads one
    int64_t pi_stride;
};
