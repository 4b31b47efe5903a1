/*
 * offsim.h -- C ABI of the MI355X-native Per-State Rejection Sampling (PSRS) engine.
 *
 * Drop-in boundary for the replay-loop hot path of microsoft/rl-offline-simulation (offsim4rl).
 * The reference has no FFI of its own (it is pure Python); each entry point below names the
 * reference function it replaces (paths relative to the reference checkout).  A maintainer binds
 * these with ctypes -- see INTEGRATION.md for the stub that goes into
 * offsim4rl/evaluators/per_state_rejection.py.
 *
 * Conventions
 *   - Every pointer is a DEVICE pointer (hipMalloc / torch.Tensor.data_ptr() of a contiguous
 *     ROCm tensor) unless the name ends in _host.  The library never frees caller memory and never
 *     allocates what it returns; scratch is passed in.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream).  All
 *     calls are asynchronous with respect to the host and safe to capture in a hipGraph.
 *   - Return value: 0 = OFFSIM_OK, negative = error; offsim_last_error() gives the message for the
 *     calling thread.  Nothing throws across the boundary.  No Python state; call with the GIL released.
 *   - "slot" = z - z_base: latent states are stored as non-negative slots so that z = -1
 *     (CartpoleBoxEncoder failure code, offsim4rl/encoders/heuristic.py:23-24) is a legal queue key.
 */
#ifndef OFFSIM_H
#define OFFSIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OFFSIM_OK 0
#define OFFSIM_EINVAL (-1)   /* bad argument */
#define OFFSIM_EHIP (-2)     /* HIP runtime error (launch, no device, ...) */
#define OFFSIM_EUNSUPPORTED (-3)

/* dtype tags */
#define OFFSIM_F32 0
#define OFFSIM_F64 1
#define OFFSIM_F16 2

/* accept/reject rule (offsim4rl/evaluators/per_state_rejection.py:97 `_reject` hook) */
#define OFFSIM_REJECT_DEFAULT 0 /* psrs.py:53-57  u > p_new[a]/p_log[a]/max(p_new/p_log)          */
#define OFFSIM_REJECT_NEVER 1   /* trivial_baselines.py:8-10,22-24  accept head, no RNG draw       */

/* arithmetic of the default rule, following NumPy promotion */
#define OFFSIM_PROB_F64 0 /* p_new f64 (p_log widened exactly): divisions and compare in f64      */
#define OFFSIM_PROB_F32 1 /* p_new f32 and p_log f32: divisions in f32, u rounded to f32          */

/* per-rollout status written by offsim_eval_mc / offsim_step_batch */
#define OFFSIM_ST_OK 0          /* step accepted / episode cap reached                              */
#define OFFSIM_ST_EXHAUSTED 1   /* PSRS.step returned (None,)*4: queue of current state empty       */
#define OFFSIM_ST_NO_INIT 2     /* PSRS.reset returned None: init queue empty                       */
#define OFFSIM_ST_KEYERROR 3    /* current state never occurs as a from-state (psrs.py:44)          */
#define OFFSIM_ST_INACTIVE 4    /* rollout had no current state (s is None); nothing done           */
#define OFFSIM_ST_PROTOCOL 5    /* internal: a bounded wait between the two wavefronts of offsim_eval_mc_streams expired
                                   (never expected; the rollout stops instead of hanging the stream) */

/* The logged-transition table, SoA, rows physically grouped by from-state (CSR).  Built by
 * offsim_group_by_state + offsim_table_gather from the OfflineDataset.experience arrays
 * (offsim4rl/data.py:46-58) and the encoder output (per_state_rejection.py:29-35).
 * Replaces PSRS._calculate_latent_state + the sorted/groupby of reset_sampler (psrs.py:16-17,26). */
typedef struct offsim_table {
    int64_t N;              /* logged transitions                                               */
    int32_t n_slots;        /* states are slots 0..n_slots-1                                    */
    int32_t nA;             /* actions                                                          */
    int32_t plog_dtype;     /* OFFSIM_F32 | OFFSIM_F64 | OFFSIM_F16                             */
    int32_t r_dtype;        /* OFFSIM_F32 | OFFSIM_F64                                          */
    const uint32_t *seg_off;  /* [n_slots+1] first grouped row of each state                    */
    const void *p_log;        /* [N,nA] logging-policy probabilities (hot candidate stream)     */
    const int32_t *a;         /* [N]    logged action            (hot candidate stream)         */
    const void *r;            /* [N]    reward                   (accept-only stream)           */
    const int32_t *z_next;    /* [N]    slot of the next state   (accept-only stream)           */
    const uint8_t *done;      /* [N]    terminal flag            (accept-only stream)           */
    const int32_t *orig_idx;  /* [N]    row in the caller's buffer (for accepted-index reports) */
    int64_t N0;               /* rows with step == 0 (all rows if `steps` is absent, data.py:72) */
    const int32_t *init_slot; /* [N0]   slot of the k-th initial row, buffer order (psrs.py:22) */
    const int32_t *init_orig; /* [N0]   its row in the caller's buffer                          */
    int64_t max_seg;          /* longest state segment (max of seg_off[s+1]-seg_off[s]); 0 = unknown:
                                 the shuffle then sizes its LDS for the worst case (65536 rows)      */
    int64_t min_seg;          /* shortest non-empty state segment; 0 = unknown (the shuffle then launches
                                 every size class)                                                  */
} offsim_table;

/* State of R independent simulated rollouts (one PSRS env each).  Owned by the caller. */
typedef struct offsim_rollouts {
    int32_t R;
    uint64_t *rng;          /* [R,4] rejection stream: PCG64 state hi, lo, inc hi, lo (psrs.py:20) */
    uint32_t *cursor;       /* [R,n_slots] candidates popped so far from each state's queue       */
    uint32_t *init_cursor;  /* [R] initial states popped so far (psrs.py:36)                      */
    int32_t *cur_slot;      /* [R] current state slot, -1 = none (self.s is None)                 */
    const uint32_t *perm;   /* queue order: perm[r*perm_stride + seg_off[s] + k] = grouped row of
                               the k-th element of state s's queue.  perm_stride = N for per-rollout
                               shuffles, 0 for one order shared by all rollouts; NULL = table order */
    int64_t perm_stride;
    const uint32_t *init_perm; /* init_perm[r*init_stride + k] = index into init_slot/init_orig   */
    int64_t init_stride;
    int32_t rng_kind;       /* OFFSIM_STREAM_*: what `rng` holds and which generator draws u (psrs.py:56)  */
} offsim_rollouts;
/* Provider of the rejection stream u ~ U (one draw per candidate examined, psrs.py:56):
 *   OFFSIM_STREAM_PCG64   NumPy's default_rng(seed).random(): u in [0,1).  The parity default: accepted-index sequences equal the
 *                         reference's bit for bit.  rng row = PCG64 state hi, lo, increment hi, lo (offsim_seed_streams).
 *   OFFSIM_STREAM_PHILOX  rocRAND's Philox4x32-10 through its device API (rocrand_init(seed, 0, 2 i) / rocrand): draw i of a rollout is
 *                         rocrand_uniform_double of the engine seeded with the rollout's seed, u in (0,1] -- a different, equally valid
 *                         sample path, NOT the reference's numbers; its oracle is the reference's own PSRS.step with
 *                         env.rejection_sampling_rng replaced by an object that replays this stream (tests/golden/make_golden.py).
 *                         rng row = seed, draws consumed so far, 0, 0.  Taken by offsim_step_batch, offsim_eval_mc, offsim_eval_td and
 *                         (round 6) by both compiled-policy scans, offsim_eval_mc_streams and offsim_eval_mc_keys, which fill their
 *                         draw rings from the same engine (rocrand_device::philox4x32_10_engine::ten_rounds, csrc/philox_dev.hpp).
 *                         In the compiled-policy
 *                         scans a draw is compared as the integer k = u * 2^53 in [1, 2^53] against the 53-bit key; k = 2^53 (u = 1.0
 *                         exactly, probability 2^-53 per draw) is looked at as 2^53 - 1, which differs from the reference's rule only
 *                         against an importance ratio of exactly 1 - 2^-53. */
#define OFFSIM_STREAM_PCG64 0
#define OFFSIM_STREAM_PHILOX 1

const char *offsim_last_error(void);
int offsim_version(void);
/* number of HIP devices visible, or a negative error; never initialises a context */
int offsim_device_count(void);

/* ---- table construction (a1, a6, a12) -------------------------------------------------------- */

/* Stable group-by of rows by slot: order[g] = original row of grouped row g, seg_off = CSR offsets.
 * == sorted(buffer, key=z) + groupby of psrs.py:26 (buffer order inside a state).
 * scratch: at least offsim_group_scratch_bytes(N, n_slots) bytes. */
int64_t offsim_group_scratch_bytes(int64_t N, int32_t n_slots);
int offsim_group_by_state(const int32_t *slot, int64_t N, int32_t n_slots, uint32_t *seg_off /*[n_slots+1]*/,
                          int32_t *order /*[N]*/, void *scratch, void *stream);

/* Gathers the caller's row-major arrays into the grouped SoA layout: dst[g] = src[order[g]].
 * elem_bytes in {1,2,4,8,...}; row_elems = elements per row (nA for p_log). */
int offsim_gather_rows(const void *src, const int32_t *order, int64_t N, int32_t row_bytes, void *dst, void *stream);

/* ---- sampler (a2, a3) ------------------------------------------------------------------------ */

/* np.random.default_rng(seed) for R seeds: SeedSequence -> PCG64 (psrs.py:20).  seeds, out on device. */
int offsim_seed_streams(const uint64_t *seeds, int32_t R, uint64_t *rng_out /*[R,4]*/, void *stream);

/* Debug view of where a chain of the sampler reset starts its draw stream (csrc/shuffle_wave.hpp; the jump tables of
 * csrc/pcg64_jump_tab.hpp).  For every {seed, count, g in {0, 1}}, in that order, OFFSIM_PCG_PROBE_WORDS uint64: the PCG64 states
 * (hi, lo) of the 64 lanes of G wavefront g -- lane l: the state q + 64 g + l + 1 steps behind default_rng(seed)'s, q = count (halve = 0)
 * or count >> 1 (halve != 0: count is a number of 32-bit draws) -- then the jump by 128 steps as {mult hi, lo, plus hi, lo}.
 * out_tab: from the tables, as the chains compute it; out_ref: from the squaring loop.  All pointers on the device. */
#define OFFSIM_PCG_PROBE_WORDS 132
int offsim_pcg_jump_probe(const uint64_t *seeds, int32_t n_seeds, const uint32_t *counts, int32_t n_counts, int32_t halve,
                          uint64_t *out_tab /*[n_seeds,n_counts,2,132]*/, uint64_t *out_ref, void *stream);

/* PSRS.reset_sampler(seed) queue shuffles (psrs.py:22-23,29-30) for n_perm seeds at once:
 * every state's queue and the init queue get a backward Fisher-Yates driven by a FRESH
 * default_rng(seed).  perm_out [n_perm,N] holds grouped rows, init_perm_out [n_perm,N0] indices. */
int offsim_shuffle_queues(const offsim_table *t, const uint64_t *seeds, int32_t n_perm, uint32_t *perm_out,
                          uint32_t *init_perm_out, void *stream);

/* PSRS.reset() (psrs.py:32-37) for every rollout with mask[r] != 0 (mask NULL = all): pops the
 * init queue, sets cur_slot; out_init_row[r] = caller-buffer row of the initial state or -1 (None). */
int offsim_env_reset(const offsim_table *t, offsim_rollouts *ro, const uint8_t *mask, int32_t *out_init_row,
                     void *stream);

/* ---- the replay loop (a4, a5, a7, a8, a9) ---------------------------------------------------- */

/* One PSRS.step(p_new) (psrs.py:39-51) per rollout with a current state.
 * p_new [R,nA] f64 (prob_mode F64) or f32 (prob_mode F32).
 * out_row[r]   caller-buffer row of the accepted transition, or -1
 * out_status[r] OFFSIM_ST_*;  out_popped[r] candidates consumed by this call.
 * max_pop > 0 caps the candidates popped (max_pop = 1 with OFFSIM_REJECT_NEVER is the "pop one
 * candidate for a Python-side _reject override" primitive); advance = 0 leaves cur_slot unchanged. */
int offsim_step_batch(const offsim_table *t, offsim_rollouts *ro, const void *p_new, int32_t prob_mode,
                      int32_t reject_mode, int32_t advance, int32_t *out_row, int32_t *out_status,
                      uint32_t *out_popped, void *stream);

/* ---- step server: PSRS.step for one environment without a launch per call (a4, a7) ----------------------------------
 * The reference's evaluator is driven by one Python call per simulated step (per_state_rejection.py:85-95); a kernel launch plus a
 * stream synchronise per call costs ~27 us against ~9 us for the reference's own Python step.  offsim_step_server_start leaves ONE
 * wavefront resident that serves offsim_step_batch's step (R = 1, same arithmetic, same state rows) for requests posted through a
 * mailbox in host-coherent pinned memory:
 *   host:   write p_new (p_head / p_tail) and cmd / reject_mode, then seq_in2 = previous seq_in + 1, THEN seq_in = the same
 *           wait until seq_out == seq_in, read row / status / popped
 *   device: ends on OFFSIM_SERVER_CMD_EXIT, or by itself after `idle_polls` polls (~1-2 us each) without a request: `state` says so,
 *           and the host starts it again.  While it runs, nothing else may touch the rollout's state rows (cursor, rng, cur_slot).
 * offsim_host_alloc / offsim_host_free: the mailbox's memory (hipHostMalloc, coherent + mapped: host and device see each other's
 * stores while the kernel runs).  `stream` must not be a stream the caller synchronises while the server is meant to stay up. */
#define OFFSIM_MAILBOX_MAX_ACTIONS 24
#define OFFSIM_SERVER_CMD_STEP 1     /* PSRS.step(p_new) */
#define OFFSIM_SERVER_CMD_POP_ONE 2  /* pop one candidate, accept it, leave the state (the Python-side _reject hook's primitive) */
#define OFFSIM_SERVER_CMD_EXIT 3
#define OFFSIM_SERVER_CMD_RESET 4    /* PSRS.reset (psrs.py:32-37): row = caller-buffer row of the initial state, or -1 */
#define OFFSIM_SERVER_STARTING 1
#define OFFSIM_SERVER_RUNNING 2
#define OFFSIM_SERVER_EXITED 3
typedef struct offsim_step_mailbox {
    /* the first 64 bytes are what ONE poll of the server reads */
    uint32_t seq_in;      /* host -> device: request number, written LAST */
    uint32_t cmd;         /* OFFSIM_SERVER_CMD_* */
    int32_t reject_mode;  /* OFFSIM_REJECT_* */
    uint32_t reserved0;
    double p_head[5];     /* p_new[0..4] (f64), or p_new[0..9] as packed f32 (OFFSIM_PROB_F32) */
    uint32_t reserved1;
    uint32_t seq_in2;     /* the request number once more, written BEFORE seq_in and behind everything else: a snapshot of the 64 bytes
                           * that shows the new number in both places holds the new payload, whatever order its parts were read in */
    double p_tail[OFFSIM_MAILBOX_MAX_ACTIONS - 5]; /* p_new[5..] (f64), or p_new[10..] as packed f32 */
    uint32_t reserved2[2];
    /* the answer: one 16-byte store of the device */
    uint32_t seq_out;     /* device -> host: the request served */
    int32_t row;          /* caller-buffer row of the accepted transition (RESET: of the initial state), or -1 */
    int32_t status;       /* OFFSIM_ST_* */
    uint32_t popped;      /* candidates consumed */
    uint32_t state;       /* OFFSIM_SERVER_* (0: never started) */
    uint32_t reserved3[3];
} offsim_step_mailbox;
int offsim_host_alloc(int64_t bytes, void **host_ptr);
int offsim_host_free(void *host_ptr);
int offsim_step_server_start(const offsim_table *t, offsim_rollouts *ro, offsim_step_mailbox *mailbox, int32_t prob_mode,
                             uint32_t idle_polls, void *stream);
/* The host side of ONE request, in C (no device call: stores to the mailbox, then a spin on seq_out): p_new = n_actions probabilities
 * (f64 / f32 by prob_mode; NULL for RESET), out3 = {row, status, popped}.  Returns OFFSIM_OK, or OFFSIM_SERVER_GONE (> 0) when the
 * server ended by itself before it saw the request -- the request stays posted: synchronise the server's stream, start it again (it
 * serves the posted request) and wait for seq_out == seq_in -- or OFFSIM_EHIP after max_spins polls (0: no bound) or, whatever
 * max_spins says, after OFFSIM_SERVER_ANSWER_SECONDS of wall-clock time spent with the server in state RUNNING (a dead server is
 * reported in seconds, not minutes; a launch still queued on a shared device is not timed; the environment variable
 * OFFSIM_SERVER_ANSWER_SECONDS overrides the bound, 0 = none).  After OFFSIM_EHIP the request is still posted (seq_in has moved): do
 * not call again on this mailbox -- end the server (synchronise its stream or reset the device), clear the mailbox, start afresh. */
#define OFFSIM_SERVER_GONE 1
#define OFFSIM_SERVER_ANSWER_SECONDS 10.0
int offsim_step_server_call(offsim_step_mailbox *mailbox, const void *p_new, int32_t n_actions, int32_t prob_mode, uint32_t cmd,
                            int32_t reject_mode, uint64_t max_spins, int32_t *out3);

/* Sets the current state of masked rollouts (used after a Python-side accept): cur_slot[r] = slot[r]. */
int offsim_env_set_state(offsim_rollouts *ro, const int32_t *slot, const uint8_t *mask, void *stream);

/* Payload of a batched step / reset for many environments at once (the vectorised form of per_state_rejection.py:85-95: the
 * reference returns action, next observation, reward, done of the served row -- `experience[...][row]`).  One launch:
 *   status != NULL (after offsim_step_batch):  ok[k] = status[k] == OFFSIM_ST_OK;  alive[k] &= ok[k]
 *   status == NULL (after offsim_env_reset):   m = mask ? mask[k] : 1;  ok[k] = m && row[k] >= 0;  if (m) alive[k] = row[k] >= 0
 * and for every column c < n_cols: where ok[k], dst_c[k] = src_c[row[k]] (row_bytes bytes); where not, dst_c[k] is left as it
 * is, or zero-filled if zero_if_not_ok (e.g. `done`).  row are rows of the caller's buffer.  n_cols <= 8. */
typedef struct {
    const void *src; /* [n_rows] items of row_bytes bytes, caller's row order */
    void *dst;       /* [R] items */
    int64_t row_bytes;
    int32_t zero_if_not_ok;
    int32_t reserved;
} offsim_column;
int offsim_vector_gather(const int32_t *row, const int32_t *status, const uint8_t *mask, int32_t R, const offsim_column *cols,
                         int32_t n_cols, uint8_t *alive, void *stream);

/* One driver iteration of a batched evaluator in one launch (VectorPSRS.step_and_reset; the loop of
 * examples/cartpole/psrs_from_expert_heuristic.py:59-80 vectorised over environments): PSRS.step(p_new[r]) as offsim_step_batch
 * (advance = 1), then step_cols gathered from the served caller-buffer row into row r of their destinations (zero_if_not_ok columns
 * are cleared where nothing was served), then -- where the served transition ended its episode -- PSRS.reset (offsim_env_reset) and
 * reset_cols gathered from the initial row (typically the observation, written over the next observation).  alive[r] (optional, in/out)
 * is cleared where the step returned None or the reset found the init queue empty.  out_row / out_status (optional) as offsim_step_batch. */
int offsim_vector_step(const offsim_table *t, offsim_rollouts *ro, const void *p_new, int32_t prob_mode, int32_t reject_mode,
                       const offsim_column *step_cols, int32_t n_step_cols, const offsim_column *reset_cols, int32_t n_reset_cols,
                       uint8_t *alive, int32_t *out_row, int32_t *out_status, void *stream);

/* evalMC_psrs(env, n_episodes, pi, gamma) (psrs.py:241-271) for all rollouts in one launch.
 * pi [n_slots,nA] (row s = policy in state slot s), same dtype rule as p_new.
 * gamma_pow [n_gamma_pow] f64 holds gamma**t as the host computes it (Python float ** int == libm pow); Gs are bit-exact
 *   only for t inside the table.  Beyond it: if the table ends stationary (last two entries equal and 0, +-inf or 1 -- for
 *   |gamma| < 1 the factor is exactly 0 from t ~ 7.4e4 on at gamma = 0.99) the last entry is used, which is again exact;
 *   otherwise the device's own pow().  A table of N+1 entries always suffices (an episode has at most N steps).
 * out_sum_g[r] sum of completed episodes' returns (episode order), out_n_ep[r] their number,
 * out_steps[r] accepted steps, out_cand[r] candidates examined, out_n_len[r] entries of `lengths`
 * (n_ep or n_ep+1, psrs.py:265), out_status[r] why the rollout stopped.
 * Optional (NULL to skip): ep_g [R,ep_cap] f64, ep_len [R,ep_cap+1] i32 per-episode values;
 * trace_row [R,trace_cap] i32 accepted caller-buffer rows, trace_pop [R,trace_cap] u32 candidates per step. */
typedef struct offsim_evalmc_out {
    double *sum_g;
    int64_t *n_ep;
    int64_t *steps;
    int64_t *cand;
    int64_t *n_len;
    int32_t *status;
    double *ep_g;
    int32_t *ep_len;
    int64_t ep_cap;
    int32_t *trace_row;
    uint32_t *trace_pop;
    int64_t trace_cap;
    int64_t *dbg; /* optional [R,4] counters of offsim_eval_mc_keys: window-dry events, digest ties, refill phases,
                     64-draw blocks generated; NULL to skip */
} offsim_evalmc_out;

int offsim_eval_mc(const offsim_table *t, offsim_rollouts *ro, const void *pi, int32_t prob_mode, int32_t reject_mode,
                   double gamma, const double *gamma_pow, int64_t n_gamma_pow, int64_t max_episodes,
                   const offsim_evalmc_out *out, void *stream);

/* evalMC_psrs for a policy over OBSERVATIONS (offsim4rl/evaluators/psrs.py:241-271, where p = pi[S] with S the observation, :255;
 * the policy people evaluate is the PPO actor of offsim4rl/agents/ppo.py:18-27).  Such a policy is asked at two kinds of observation only:
 * next_obs of the row just accepted (psrs.py:49-51) and obs of the initial row just popped (psrs.py:32-37), so it is two per-row tables:
 *   p_next [N,nA]  the policy at next_obs of GROUPED row g (table order: caller row orig_idx[g]),
 *   p_init [N0,nA] the policy at obs of initial row k (caller row init_orig[k]).
 * The loop is offsim_eval_mc's (same queues, streams, reject rule, prob modes, outputs and status codes) with p_new = p_next[g] of the
 * previous accepted row, or p_init[k] right after a reset.  Element type: f32 for OFFSIM_PROB_F32 (f32 p_log), f64 otherwise.
 * out_obs_row [R] (optional): where env.s comes from when the loop stops -- i >= 0: next_obs of caller row i; -2 - i: obs of caller
 * row i (an initial row, no step accepted since); -1: None (no initial row left).  Left unwritten when the loop ran no reset. */
int offsim_eval_mc_rows_policy(const offsim_table *t, offsim_rollouts *ro, const void *p_next, const void *p_init, int32_t prob_mode,
                               int32_t reject_mode, double gamma, const double *gamma_pow, int64_t n_gamma_pow, int64_t max_episodes,
                               const offsim_evalmc_out *out, int32_t *out_obs_row, void *stream);

/* offsim_eval_mc_rows_policy_pop: offsim_eval_mc_rows_policy for a population of L policies on the same S seeds in ONE launch (ranking
 * learners on a log: every policy sees the same queues and the same draws, so differences between policies are paired).
 *   p_next [L,N,nA], p_init [L,N0,nA]   the per-row tables of offsim_eval_mc_rows_policy, stacked, contiguous.
 *   ro->R = L * S, policy-major: rollout r evaluates policy r / S on seed index r % S.  ro->rng, cursor, init_cursor and cur_slot are
 *   [R] rows as always (the caller's S rows replicated L times) and are advanced per rollout.
 *   ro->perm / ro->init_perm hold S orders, not R: rollout r reads row r % S (perm_stride = 0: one shared order; NULL: table order, as
 *   always).  The kernel only reads the orders, so all policies of a seed share one copy.
 * Everything else -- both stream providers, the f64 and f32 modes, the reject modes, the outputs [R] with ep_* / trace_* and out_obs_row,
 * the status codes -- is offsim_eval_mc_rows_policy's, and rollout l * S + j equals, in every output and in the state it leaves, that
 * entry point run alone with policy l from seed j's state and order.  L in 1..65535, S >= 1, ro->R = L * S, tables not NULL where N > 0 /
 * N0 > 0 (otherwise OFFSIM_EINVAL).  Argument validation happens before any HIP call; ro->R = 0 launches nothing. */
int offsim_eval_mc_rows_policy_pop(const offsim_table *t, offsim_rollouts *ro, const void *p_next, const void *p_init, int32_t L, int32_t S,
                                   int32_t prob_mode, int32_t reject_mode, double gamma, const double *gamma_pow, int64_t n_gamma_pow,
                                   int64_t max_episodes, const offsim_evalmc_out *out, int32_t *out_obs_row, void *stream);

/* PSRS_Exo.step (offsim4rl/evaluators/psrs.py:99-117): endogenous state s and exogenous state x have their own queue
 * families; every candidate pops the head of both, the accept/reject test reads the s-row, the accepted s-row gives
 * (r, s', done) and the accepted x-row gives x'.  ts / rs: table grouped by s and its rollout state (rng, cursors,
 * permutations, cur_slot = s); tx / rx: table grouped by x (only z_next and orig_idx are read) and its cursors,
 * permutations and cur_slot = x.  Build, shuffle and reset each with the ordinary entry points (same seeds).
 * out_row_s / out_row_x: caller-buffer rows of the accepted s- and x-elements (-1 on None / KeyError).
 * The draws are rs's stream, PCG64 only: rs->rng_kind = OFFSIM_STREAM_PHILOX is refused with OFFSIM_EUNSUPPORTED, nothing is stepped. */
int offsim_step_exo(const offsim_table *ts, const offsim_table *tx, offsim_rollouts *rs, offsim_rollouts *rx,
                    const void *p_new, int32_t prob_mode, int32_t *out_row_s, int32_t *out_row_x, int32_t *out_status,
                    uint32_t *out_popped, void *stream);

/* Learner-in-the-loop drivers qlearn_psrs / expSARSA_psrs (offsim4rl/evaluators/psrs.py:119-239): evalMC's loop plus,
 * after every accepted step (S, A, R, S'):
 *   OFFSIM_TD_QLEARN   Q[S,A] += alpha * (R + gamma * max_a Q[S',a]            - Q[S,A])    (psrs.py:165-168)
 *   OFFSIM_TD_EXPSARSA Q[S,A] += alpha * (R + gamma * sum_a Q[S',a] pi[S',a]   - Q[S,A])    (psrs.py:223)
 * q [R,n_slots,nA] f64 is read as Q_init and written back; td_err [R,td_cap] (optional) gets the TD errors in step
 * order.  pi [n_slots,nA] f64.  Outputs as offsim_eval_mc. */
#define OFFSIM_TD_NONE 0
#define OFFSIM_TD_QLEARN 1
#define OFFSIM_TD_EXPSARSA 2
/* Behaviour policy of the learner drivers (what reveals p_new before every step, psrs.py:158 / :215):
 *   OFFSIM_BEHAVIOUR_FIXED        the tabular `pi` (expSARSA_psrs; qlearn_psrs with a Q-independent policy such as
 *                                 uniformly_random_policy, agents/tabular.py:7-9);
 *   OFFSIM_BEHAVIOUR_EPS_GREEDY   epsilon_greedy_policy on the rollout's own Q row (agents/tabular.py:24-32): epsilon / nA
 *                                 everywhere, 1 - epsilon + epsilon / nA at the arg max; epsilon = 0 is greedy_policy (:11-16);
 *   OFFSIM_BEHAVIOUR_SOFT_GREEDY  soft_greedy_policy (agents/tabular.py:18-22): uniform over the actions whose Q value is
 *                                 np.isclose (rtol 1e-5, atol 1e-8) to the row's maximum.
 * Ties between maxima (EPS_GREEDY): the reference draws np.random.choice among them (agents/tabular.py:4-5), i.e. one masked-
 * rejection bounded integer from NumPy's GLOBAL MT19937 stream per tie and none without a tie.  tie_mt [R,625] u32 is that
 * stream per rollout -- the 624 state words and the position, as np.random.get_state() returns them -- read, advanced and
 * written back; with tie_mt = NULL the FIRST maximum is taken. */
#define OFFSIM_BEHAVIOUR_FIXED 0
#define OFFSIM_BEHAVIOUR_EPS_GREEDY 1
#define OFFSIM_BEHAVIOUR_SOFT_GREEDY 2
typedef struct offsim_td {
    int32_t mode;
    double alpha;
    double *q;
    double *td_err;
    int64_t td_cap;
    int32_t behaviour; /* OFFSIM_BEHAVIOUR_* */
    double epsilon;    /* OFFSIM_BEHAVIOUR_EPS_GREEDY */
    /* schedules (psrs.py:128-135): alpha(episode) / epsilon(episode) tabulated by the caller for episodes 0 .. n_sched-1 (the
     * last entry serves every later episode); NULL: the constants above */
    const double *alpha_ep;
    const double *epsilon_ep;
    int64_t n_sched;
    /* save_Q (psrs.py:172-173, :227-228): Q [n_slots,nA] after every snap_stride-th step (steps 0, stride, 2 stride, ...),
     * q_snap [R,snap_cap,n_slots,nA] f64; NULL: none */
    double *q_snap;
    int64_t snap_cap;
    int64_t snap_stride;
    uint32_t *tie_mt;  /* see above; NULL: first maximum */
    int32_t *beh_arg;  /* [R,td_cap] optional: the action the behaviour policy put its greedy mass on at every step (EPS_GREEDY) */
} offsim_td;
int offsim_eval_td(const offsim_table *t, offsim_rollouts *ro, const double *pi, int32_t reject_mode, double gamma,
                   const double *gamma_pow, int64_t n_gamma_pow, int64_t max_episodes, const offsim_evalmc_out *out,
                   const offsim_td *td, void *stream);

/* offsim_eval_td_pop: offsim_eval_td for a population of L learners on the same S seeds in ONE launch (comparing the learning curves of a
 * grid of step sizes, exploration rates and discounts over many sampler seeds: every learner of a seed sees the same queues and the same
 * draws, so differences between learners are paired).
 *   ro->R = L * S, learner-major: rollout r = l * S + j is learner l on seed j.  ro->rng, cursor, init_cursor and cur_slot are [R] rows as
 *   always (the caller's S rows replicated L times) and are advanced and written back per rollout.
 *   ro->perm / ro->init_perm hold S orders, not R: rollout r reads row j (perm_stride = 0: one shared order; NULL: table order) -- the
 *   stride rule of offsim_eval_mc_rows_policy_pop.  The kernel only reads the orders.
 * Per learner (device arrays, one entry per learner unless said otherwise):
 *   alpha, epsilon, gamma [L] f64; gamma_pow [L, n_gamma_pow] f64, row l the discount table of gamma[l] (the rule of offsim_eval_mc's
 *   gamma_pow, per learner: a row that is stationary before n_gamma_pow is padded with its last entry, which is exact);
 *   behaviour [L] i32 OFFSIM_BEHAVIOUR_*, and behaviour_host, the same L values in HOST memory, which is what is validated;
 *   alpha_ep / epsilon_ep [L, n_sched] f64 or NULL (the constants); pi [L, n_slots, nA] f64 with pi_stride = n_slots * nA, or one table
 *   [n_slots, nA] shared by all learners with pi_stride = 0.
 *   mode is one value per launch (OFFSIM_TD_QLEARN or OFFSIM_TD_EXPSARSA).
 * Per rollout, [L * S, ...] in the layouts of offsim_td: q, td_err / td_cap, q_snap / snap_cap / snap_stride, tie_mt [L * S, 625] or NULL,
 * beh_arg.  out: offsim_evalmc_out as it is, [L * S] rows.
 * Rollout l * S + j equals, in every output bit and in the state it leaves, offsim_eval_td run alone with learner l's setting from seed j's
 * state and order (the loop is the same code: k_eval_mc's TD instance under a population index, csrc/td_pop.hpp).  A workgroup holds
 * rollouts of one learner (grid = L * ceil(S / waves)); the LDS carve, the 4 / 2 / 1 rollouts per workgroup and the refusal past 160 KiB
 * (OFFSIM_EUNSUPPORTED) are offsim_eval_td's.  L in 1..65535, S >= 1, ro->R = L * S, a behaviour outside OFFSIM_BEHAVIOUR_*, NULL
 * per-learner arrays, schedules without n_sched, a bad snapshot stride: OFFSIM_EINVAL.  Argument validation happens before any HIP call;
 * ro->R = 0 launches nothing. */
typedef struct offsim_td_pop {
    int32_t mode;
    const double *alpha;
    const double *epsilon;
    const double *gamma;
    const double *gamma_pow;
    int64_t n_gamma_pow;
    const int32_t *behaviour;
    const int32_t *behaviour_host;
    const double *alpha_ep;
    const double *epsilon_ep;
    int64_t n_sched;
    const double *pi;
    int64_t pi_stride;
    double *q;
    double *td_err;
    int64_t td_cap;
    double *q_snap;
    int64_t snap_cap;
    int64_t snap_stride;
    uint32_t *tie_mt;
    int32_t *beh_arg;
} offsim_td_pop;
int offsim_eval_td_pop(const offsim_table *t, offsim_rollouts *ro, int32_t L, int32_t S, const offsim_td_pop *pop, int32_t reject_mode,
                       int64_t max_episodes, const offsim_evalmc_out *out, void *stream);

/* offsim_td_curves: the learning curves of a population on the device.  ep_g [L * S, ep_cap] f64 and n_ep [L * S] i64 are
 * offsim_eval_td_pop's outputs (learner-major).  For learner l and episode e < ep_cap, over the seeds j with e < n_ep[l * S + j] (completed
 * episodes only): n_out[l, e] their number (i64), mean_out[l, e] the mean return, var_out[l, e] the population variance (two passes: the
 * mean first, then the mean squared deviation).  One thread per (l, e) sums in seed order j = 0 .. S - 1 in f64 without atomics, so the
 * numbers equal a plain float loop in that order bit for bit and two calls give the same bits.  n = 0: NaN (0x7ff8000000000000) for both. */
int offsim_td_curves(const double *ep_g, const int64_t *n_ep, int32_t L, int32_t S, int64_t ep_cap, int64_t *n_out, double *mean_out,
                     double *var_out, void *stream);

/* offsim_eval_mc_exo: whole rollouts on PSRS_Exo (offsim4rl/evaluators/psrs.py:59-117) under the reference's three drivers -- evalMC_psrs
 * (td = NULL), qlearn_psrs and expSARSA_psrs (td->mode; psrs.py:119-271) -- for all rollouts in ONE launch (csrc/eval_exo.hpp).
 * ts / rs, tx / rx: the two queue families of offsim_step_exo (same log: ts->N == tx->N, ts->N0 == tx->N0; rs->R == rx->R).  Rollout r
 * reads its own orders (rs->perm, rx->perm, rs->init_perm with their strides; NULL: table order) and owns its cursors of both families,
 * rs->init_cursor[r] and rs / rx->cur_slot[r]; all of it is written back (rx->init_cursor[r] follows rs's), so a later call or a later
 * offsim_step_exo continues where this one stopped.
 *   reset   the next entry of the s-table's init order; s and x are that row's (psrs.py:91-97)
 *   step    pops s_queues[s] and x_queues[x] together until a candidate is accepted (default reject rule, offsim_step_exo's p_log / prob
 *           dispatch); either queue empty: OFFSIM_ST_EXHAUSTED, the state stays; a slot without rows or out of range in either family:
 *           OFFSIM_ST_KEYERROR.  Reward, done and s' are the accepted s-row's, x' the x-row's popped with it; G += gamma_pow[t] * r.
 * The policy and Q are indexed by the OBSERVATION o = o_combine_func(s, x) (psrs.py:255, :158, :214):
 *   obs_of [ts->n_slots, tx->n_slots] i32   the row of pi / Q for that pair of slots, 0 .. n_obs-1 (several pairs may share a row); -1 (or
 *                                           anything outside the range) where pi has no row: reaching such a pair stops the rollout
 *                                           with OFFSIM_ST_KEYERROR (the reference raises IndexError at pi[S] / Q[S'])
 *   pi [n_obs, nA]                          f32 for OFFSIM_PROB_F32 (f32 p_log), f64 otherwise
 * reseed, the rejection stream:
 *   OFFSIM_EXO_RESEED_EPISODE  the reference's protocol: PSRS_Exo.reset(seed) restarts the stream (psrs.py:92) and the drivers call
 *                              env.reset(seed=episode), so episode e of this call draws from default_rng(episode0 + e) -- seeded at
 *                              the reset, before the init queue is looked at.  PCG64 only: rs->rng_kind = OFFSIM_STREAM_PHILOX is
 *                              refused with OFFSIM_EUNSUPPORTED.  On exit rs->rng[r] holds the state after the last draw.
 *   OFFSIM_EXO_RESEED_NONE     the rollout's own stream rs->rng[r] (either provider) runs on across episodes and is advanced.
 * out: offsim_eval_mc's, trace_row holding the accepted s-rows.  xout (optional, members optional):
 *   trace_row_x [R, out->trace_cap] i32  caller rows of the x-rows popped with the accepted s-rows
 *   last [R,3] i32                       where env.o comes from when the loop stops: caller row of the last accepted s-row, caller row of
 *                                        the x-row popped with it, caller row of the initial row when no step was accepted since the
 *                                        last reset; -1 where a field does not apply.  Left unwritten when no reset served a row.
 * td (NULL: evalMC): OFFSIM_TD_QLEARN / OFFSIM_TD_EXPSARSA on td->q [R, n_obs, nA] f64 -- the update, td_err, alpha_ep, q_snap /
 *   snap_stride / snap_cap and the left-to-right sum of Q[S'] @ pi[S'] are offsim_eval_td's with the slot replaced by obs_of[s, x];
 *   OFFSIM_PROB_F64 only.  An accepted step whose next pair has no row stops the rollout with OFFSIM_ST_KEYERROR: the environment has
 *   stepped (cursors, state, last), the step is not counted.  Behaviour policy: OFFSIM_BEHAVIOUR_FIXED only -- the epsilon-greedy and
 *   soft-greedy behaviours on the learner's own Q and the tie stream (td->tie_mt) return OFFSIM_EUNSUPPORTED here: they are offsim_eval_td_exo_pop's (below).
 * LDS per workgroup: jump tables, pi, obs_of, both seg_off arrays, per-rollout cursors of both families and per-rollout Q; 4 rollouts per
 *   workgroup, then 2, then 1 while the carve exceeds 64 KiB, one rollout up to 160 KiB, beyond that OFFSIM_EUNSUPPORTED.
 * Argument validation happens before any HIP call -- the two tables, rs / rx, n_obs / obs_of / pi, the prob mode, the reseed / provider
 * pair, the TD mode and behaviour, the capacities, the LDS size --; rs->R = 0 launches nothing. */
#define OFFSIM_EXO_RESEED_NONE 0
#define OFFSIM_EXO_RESEED_EPISODE 1
typedef struct offsim_exo_out {
    int32_t *trace_row_x;
    int32_t *last;
} offsim_exo_out;
int offsim_eval_mc_exo(const offsim_table *ts, const offsim_table *tx, offsim_rollouts *rs, offsim_rollouts *rx, const void *pi,
                       const int32_t *obs_of, int32_t n_obs, int32_t prob_mode, int32_t reseed, uint64_t episode0, double gamma,
                       const double *gamma_pow, int64_t n_gamma_pow, int64_t max_episodes, const offsim_evalmc_out *out,
                       const offsim_exo_out *xout, const offsim_td *td /* NULL: evalMC */, void *stream);

/* offsim_eval_td_exo_pop: the learner drivers of offsim_eval_mc_exo for a population of L learners on the same S seeds in ONE launch, every
 * learner with any behaviour policy of the reference on its OWN Q (agents/tabular.py:7-32): what offsim_eval_td_pop is to offsim_eval_td,
 * on PSRS_Exo.  L = 1 is the single learner with an epsilon-greedy / greedy / soft-greedy behaviour, which offsim_eval_mc_exo refuses.
 *   ts / tx, obs_of [ts->n_slots, tx->n_slots], n_obs, xout: offsim_eval_mc_exo's.
 *   rs->R = rx->R = L * S, learner-major: rollout r = l * S + j is learner l on seed j.  rs->rng, both cursor arrays, both init_cursor and
 *   both cur_slot are [R] rows (the caller's S rows replicated L times), advanced and written back per rollout.  rs->perm / rs->init_perm
 *   and rx->perm hold S orders, not R: rollout r reads row j (stride 0: one shared order; NULL: table order).  The kernel only reads them.
 *   pop: struct offsim_td_pop as offsim_eval_td_pop takes it, with n_obs in the place of n_slots: q [L * S, n_obs, nA],
 *   pi [L, n_obs, nA] with pi_stride = n_obs * nA or one table with pi_stride = 0, q_snap [L * S, snap_cap, n_obs, nA]; alpha, epsilon,
 *   gamma, behaviour (+ behaviour_host), gamma_pow [L, n_gamma_pow], alpha_ep / epsilon_ep [L, n_sched], td_err / beh_arg [L * S, td_cap],
 *   tie_mt [L * S, 625] or NULL (first maximum) unchanged.
 * Behaviour (per learner): OFFSIM_BEHAVIOUR_FIXED rejects against pi[o]; OFFSIM_BEHAVIOUR_EPS_GREEDY / _SOFT_GREEDY rebuild the
 *   distribution from the learner's Q row of the current OBSERVATION o = obs_of[s, x] before every step (psrs.py:158) -- the rules, the
 *   schedules and the tie stream are offsim_eval_td's, word for word (one definition on the device).  The distribution is formed before
 *   the step: a step that then finds a queue missing or empty has drawn its tie.
 * reseed: OFFSIM_EXO_RESEED_EPISODE (episode e of every rollout draws from default_rng(episode0 + e), the reference's protocol; PCG64 only,
 *   OFFSIM_STREAM_PHILOX is refused with OFFSIM_EUNSUPPORTED) or OFFSIM_EXO_RESEED_NONE (each seed's own stream rs->rng, either provider;
 *   the L learners of seed j start from the same stream state, so comparisons between learners are paired).
 * Identity: with OFFSIM_BEHAVIOUR_FIXED, rollout l * S + j equals, in every output bit and in the state it leaves, offsim_eval_mc_exo's
 *   learner driver run alone with learner l's setting from seed j's state and orders (the loop is the same code: k_eval_mc_exo's TD
 *   instance under a population index, csrc/td_pop_exo.hpp).
 * LDS per workgroup: offsim_eval_mc_exo's learner carve plus, per rollout, nA f64 for the behaviour distribution and 624 u32 for the tie
 *   stream; 4 / 2 / 1 rollouts per workgroup against 64 KiB, one rollout up to 160 KiB, beyond that OFFSIM_EUNSUPPORTED.  A workgroup holds
 *   rollouts of one learner: grid = L * ceil(S / rollouts per workgroup).
 * Argument validation happens before any HIP call -- everything offsim_eval_mc_exo checks about the two tables, rs / rx, obs_of / n_obs, the
 * reseed / provider pair and the outputs; everything offsim_eval_td_pop checks about L (1..65535), S >= 1, R = L * S, the per-learner arrays,
 * behaviour_host, the schedules and the snapshot stride; negative capacities; the LDS size --; rs->R = 0 launches nothing. */
int offsim_eval_td_exo_pop(const offsim_table *ts, const offsim_table *tx, offsim_rollouts *rs, offsim_rollouts *rx, int32_t L, int32_t S,
                           const offsim_td_pop *pop, const int32_t *obs_of, int32_t n_obs, int32_t reseed, uint64_t episode0,
                           int64_t max_episodes, const offsim_evalmc_out *out, const offsim_exo_out *xout, void *stream);

/* offsim_eval_queue: whole rollouts on QueueEvaluator (offsim4rl/evaluators/queue_evaluator.py:90-131) under the reference's tabular drivers
 * -- evalMC (td = NULL; offsim4rl/agents/tabular.py:247-270), qlearn (:71-139) and expSARSA (:141-191) by td->mode -- for all rollouts in ONE
 * launch (csrc/eval_queue.hpp).  The queues are keyed by (z, a), the agent draws its own action and the simulator pops the head of queue
 * (z, A): no rejection, one row per step.
 *   t    the table grouped by the COMPOSITE slot z * nA + a (z counted from the smallest state), so t->n_slots = nZ * nA_actions; z_next and
 *        init_slot hold BASE slots z' * nA (what evaluators/queue_evaluator.py: BatchedQueueEvaluator builds).  ro->cursor [R, n_slots],
 *        ro->cur_slot [R] the base slot of the current state (-1: none), ro->perm / init_perm as everywhere.
 *   pi   [nZ, nA] f64 by state (the row of base slot b starts at b), or NULL for Q-learning with a behaviour on the learner's own Q.
 *   ro->rng   the ACTION stream of each rollout: PCG64 rows as offsim_seed_streams writes them (tabular.py:75: default_rng(seed)).
 *        OFFSIM_STREAM_PHILOX is refused with OFFSIM_EUNSUPPORTED and nothing is stepped: its double lies in (0, 1], and u = 1.0 would
 *        select action nA.
 * Per step: p = pi[z], or the behaviour policy on Q[z] (td->behaviour, td->epsilon / epsilon_ep: offsim_eval_td's rules, one definition on
 *   the device); A = Generator.choice(nA, p=p) (tabular.py:120, :172, :259) -- c_k = c_{k-1} + p_k sequentially in f64 from 0,
 *   cdf_k = c_k / c_{nA-1}, u = (next64 >> 11) * 2^-53, A the first k with cdf_k > u: exactly one draw per step; then the head of queue
 *   (z, A) is popped (queue_evaluator.py:121-131).  A pair (z, A) that was never logged: OFFSIM_ST_KEYERROR (self.queues[z, a] raises); the
 *   queue at its end: OFFSIM_ST_EXHAUSTED (:125-126); state and cursors stay in both cases, the draw is consumed.  A row p without a cdf
 *   entry above u (NaN, all zeros) draws A = nA: OFFSIM_ST_KEYERROR.
 * td: the update of offsim_eval_td on Q[z, A] with Q[z'] (tabular.py:123-126 / :175-178, the same arithmetic and order), q [R, nZ, nA],
 *   td_err, alpha_ep, q_snap [R, snap_cap, nZ, nA] / snap_stride / snap_cap, beh_arg as there.  The reference's tabular drivers do not
 *   survive exhaustion (None flows on into Q[None]); the rule here is the *_psrs drivers': the rollout stops with the status, evalMC drops
 *   the partial episode and appends its length (n_len = n_ep + 1), the learner drivers store the partial return past the completed ones.
 * Ties of the epsilon-greedy arg max: td->tie_mt = NULL the first maximum; td->tie_mt [R,625] the rollout's MT19937 stream, read, advanced
 *   and written back (offsim_eval_td); tie_reseed_episode = 1 (needs td->tie_mt, episode0 >= 0): at the start of episode e of this call the
 *   stream is re-initialised as np.random.seed(episode0 + e) does (tabular.py:114, :166; mt[0] = seed, mt[i] = 1812433253 * (mt[i-1] ^
 *   (mt[i-1] >> 30)) + i, position 624, the seed taken modulo 2^32) -- for every behaviour, so td->tie_mt comes back as the global stream
 *   the reference leaves.
 * out: offsim_eval_mc's; cand = steps; trace_pop [R, trace_cap] holds the ACTION drawn at every step, the last, unserved one of a rollout
 *   that stopped with OFFSIM_ST_KEYERROR / OFFSIM_ST_EXHAUSTED included (at index steps).  out_obs_row [R] (optional): where env.s comes
 *   from when the loop stops, the convention of offsim_eval_mc_rows_policy.
 * On exit cursors, init_cursor, cur_slot, the action stream (the state after the last draw), q and tie_mt are written back: a second call
 *   continues the first.
 * LDS per workgroup: per rollout the cursors (n_slots * 4), Q (n_slots * 8), the behaviour row (nA * 8) and the tie stream (2496 bytes)
 *   (the last three with td), shared pi (n_slots * 8, when given) and seg_off; 4 rollouts per workgroup, then 2, then 1 while the carve
 *   exceeds 64 KiB, one rollout up to 160 KiB, beyond that OFFSIM_EUNSUPPORTED.
 * OFFSIM_EINVAL: t->nA != nA_actions, t->n_slots % nA_actions != 0, NULL ro / rollout state / out / required outputs / q, pi = NULL where a
 *   policy is read, a bad mode / behaviour / snapshot stride / tie_reseed_episode, schedules without n_sched, negative capacities.
 * Argument validation happens before any HIP call; ro->R = 0 launches nothing. */
int offsim_eval_queue(const offsim_table *t, offsim_rollouts *ro, int32_t nA_actions,
                      const double *pi /* [nZ,nA] or NULL with a Q-dependent behaviour */, double gamma, const double *gamma_pow,
                      int64_t n_gamma_pow, int64_t max_episodes, const offsim_evalmc_out *out, const offsim_td *td /* NULL: evalMC */,
                      int32_t tie_reseed_episode, int64_t episode0, int32_t *out_obs_row, void *stream);

/* offsim_eval_queue_pop: the learner drivers of offsim_eval_queue (qlearn, expSARSA; tabular.py:71-191) for a population of L learners on the
 * same S seeds in ONE launch: what offsim_eval_td_pop is to offsim_eval_td, on QueueEvaluator (queue_evaluator.py:90-131).  Every learner of
 * a seed sees the same queues and starts from the same action stream, so differences between learners are paired.
 *   t, nA_actions, max_episodes, out, tie_reseed_episode, episode0, out_obs_row [L * S]: offsim_eval_queue's.
 *   ro->R = L * S, learner-major: rollout r = l * S + j is learner l on seed j.  ro->rng (the ACTION streams, OFFSIM_STREAM_PCG64;
 *   OFFSIM_STREAM_PHILOX is refused with OFFSIM_EUNSUPPORTED: its double lies in (0, 1]), cursor [R, n_slots], init_cursor and cur_slot are
 *   [R] rows (the caller's S rows replicated L times), advanced and written back per rollout.  ro->perm / ro->init_perm hold S orders, not
 *   R: rollout r reads row j (stride 0: one shared order; NULL: table order).  The kernel only reads them.
 *   pop: struct offsim_td_pop as offsim_eval_td_pop takes it, with nZ * nA in the place of n_slots * nA: q [L * S, nZ, nA], pi [L, nZ, nA]
 *   with pi_stride = nZ * nA or one table with pi_stride = 0, q_snap [L * S, snap_cap, nZ, nA]; alpha, epsilon, gamma, behaviour
 *   (+ behaviour_host), gamma_pow [L, n_gamma_pow], alpha_ep / epsilon_ep [L, n_sched], td_err / beh_arg [L * S, td_cap], tie_mt [L * S, 625]
 *   or NULL (first maximum) unchanged.  pop->pi may be NULL only for OFFSIM_TD_QLEARN with no OFFSIM_BEHAVIOUR_FIXED learner in behaviour_host.
 * Per step and per learner: p, the draw cdf_k = c_k / c_{nA-1} against u, the pop, the update, the tie stream and tie_reseed_episode are
 *   offsim_eval_queue's, word for word (one definition on the device).
 * Identity: rollout l * S + j equals, in every output bit and in the state it leaves, offsim_eval_queue's learner driver run alone with
 *   learner l's setting from seed j's state, order and action stream -- for EVERY behaviour (unlike on PSRS_Exo, the single form has them
 *   all).  The loop is the same code: k_eval_queue's learner instance under a population index (csrc/td_pop_queue.hpp).
 * LDS per workgroup: offsim_eval_queue's learner carve; 4 / 2 / 1 rollouts per workgroup against 64 KiB, one rollout up to 160 KiB, beyond
 *   that OFFSIM_EUNSUPPORTED.  A workgroup holds rollouts of one learner: grid = L * ceil(S / rollouts per workgroup).
 * Argument validation happens before any HIP call -- everything offsim_eval_queue checks about the table, n_slots % nA, the rollout state,
 * the provider, the outputs, the capacities, tie_reseed_episode in {0, 1} (needs pop->tie_mt and episode0 >= 0) and the LDS size; everything
 * offsim_eval_td_pop checks about L (1..65535), S >= 1, R = L * S, the per-learner arrays, behaviour_host, the schedules and the snapshot
 * stride: OFFSIM_EINVAL unless said otherwise --; ro->R = 0 launches nothing. */
int offsim_eval_queue_pop(const offsim_table *t, offsim_rollouts *ro, int32_t nA_actions, int32_t L, int32_t S, const offsim_td_pop *pop,
                          int64_t max_episodes, const offsim_evalmc_out *out, int32_t tie_reseed_episode, int64_t episode0,
                          int32_t *out_obs_row, void *stream);

/* offsim_eval_queue_rows_policy: offsim_eval_queue's evalMC (tabular.py:247-270 on queue_evaluator.py:113-131) for a policy over OBSERVATIONS
 * (the PPO actor of offsim4rl/agents/ppo.py:258-279), all rollouts in ONE launch (csrc/eval_queue_rows.hpp).  What offsim_eval_mc_rows_policy is
 * to offsim_eval_mc, on QueueEvaluator: the policy is two per-row tables,
 *   p_next [N,nA]  the policy at next_obs of GROUPED row g (table order: caller row orig_idx[g]),
 *   p_init [N0,nA] the policy at obs of initial row k (caller row init_orig[k]),
 *   p_dtype        their element type, OFFSIM_F32 or OFFSIM_F64; a row is widened exactly to f64 before the draw.
 * t, ro, nA_actions, gamma, gamma_pow, max_episodes, out, out_obs_row and the status codes are offsim_eval_queue's (the action stream is
 * OFFSIM_STREAM_PCG64; OFFSIM_STREAM_PHILOX is refused with OFFSIM_EUNSUPPORTED).  Per step p = p_init[k] right after a reset that popped
 * initial row k, p_next[g] after a served row g; A = Generator.choice(nA, p=p) exactly as offsim_eval_queue draws it (one definition on the
 * device), one draw per step; a row without a cdf entry above u (NaN, all zeros): OFFSIM_ST_KEYERROR; trace_pop holds the action drawn.
 *   cur_row [R] (optional, written on exit): the table row that holds the policy at the state the rollout stands in -- g >= 0 the last
 *   served GROUPED row, -2 - k initial row k with no step since, -1 none (no initial row left); left as it was when the loop ran no reset.
 *   It is never read: every episode of every call begins with env.reset() (tabular.py:255), exactly as in offsim_eval_queue, so no rollout
 *   ever continues an episode of an earlier call and none needs the row an earlier call stood at.  A rollout that stands inside an episode
 *   on entry (after OFFSIM_ST_EXHAUSTED, or after steps taken through offsim_step_batch) starts its next episode like any other, with
 *   cur_row NULL or not; there is no refusal.
 * Identity: with p_next[g] = pi[z_next[g]] and p_init[k] = pi[z of initial row k] the call equals offsim_eval_queue's evalMC with that pi,
 * bit for bit, in every output and in the state it leaves.
 * LDS per workgroup: seg_off (n_slots + 1 words), per rollout the cursors (n_slots * 4) and the current row (nA * 8); 4 / 2 / 1 rollouts per
 * workgroup against 64 KiB, one rollout up to 160 KiB, beyond that OFFSIM_EUNSUPPORTED.
 * OFFSIM_EINVAL: everything offsim_eval_queue checks about the table, n_slots % nA, ro, out and the capacities; p_next NULL with N > 0 or
 * p_init NULL with N0 > 0; a p_dtype other than the two.  Argument validation happens before any HIP call; ro->R = 0 launches nothing. */
int offsim_eval_queue_rows_policy(const offsim_table *t, offsim_rollouts *ro, int32_t nA_actions, const void *p_next, const void *p_init,
                                  int32_t p_dtype /* OFFSIM_F32 | OFFSIM_F64 */, double gamma, const double *gamma_pow, int64_t n_gamma_pow,
                                  int64_t max_episodes, const offsim_evalmc_out *out, int32_t *cur_row, int32_t *out_obs_row, void *stream);

/* offsim_eval_queue_rows_policy_pop: offsim_eval_queue_rows_policy for L policies on the same S seeds in ONE launch: every policy of a seed
 * sees the same queues and starts from the same action stream, so differences between policies are paired.
 *   p_next [L,N,nA], p_init [L,N0,nA]   the tables, stacked, contiguous.
 *   ro->R = L * S, policy-major: rollout r evaluates policy r / S on seed index r % S.  ro->rng, cursor, init_cursor, cur_slot, the outputs,
 *   cur_row and out_obs_row are [R] rows (the caller's S rows replicated L times), advanced and written per rollout.  ro->perm /
 *   ro->init_perm hold S orders, not R: rollout r reads row r % S (stride 0: one shared order; NULL: table order).  They are only read.
 * Identity: rollout l * S + j equals, in every output bit and in the state it leaves, offsim_eval_queue_rows_policy with policy l from seed
 * j's state, order and action stream.  No per-policy data lives in LDS, so a workgroup may hold rollouts of different policies:
 * grid = ceil(L * S / rollouts per workgroup).
 * OFFSIM_EINVAL as offsim_eval_queue_rows_policy, and L outside 1..65535, S < 1 or ro->R != L * S. */
int offsim_eval_queue_rows_policy_pop(const offsim_table *t, offsim_rollouts *ro, int32_t nA_actions, const void *p_next, const void *p_init,
                                      int32_t p_dtype, int32_t L, int32_t S, double gamma, const double *gamma_pow, int64_t n_gamma_pow,
                                      int64_t max_episodes, const offsim_evalmc_out *out, int32_t *cur_row, int32_t *out_obs_row, void *stream);

/* offsim_eval_env: the reference's tabular drivers -- evalMC (td = NULL; offsim4rl/agents/tabular.py:247-270), qlearn (:71-139) and expSARSA
 * (:141-191) by td->mode -- on its own GRID WORLDS, all rollouts in ONE launch (csrc/eval_env.hpp): the ground truth that offsim_eval_mc /
 * offsim_eval_mc_exo (PSRS, PSRS_Exo) and offsim_eval_queue (the (z, a) queue baseline) are judged against.  There is no table: nothing is
 * popped, an environment never runs dry, and every episode begins with env.reset(seed=episode).
 *   env  the world (struct offsim_grid_env), nA = 5 (noop, up, right, down, left), start (0, 0), the goal an argument:
 *          OFFSIM_GRID_PLAIN    MyGridNavi with discrete observations (offsim4rl/envs/gridworld.py:14-124); factor = 1.
 *          OFFSIM_GRID_NOISE    MyGridNaviNoise (:127-155) with factor = int(augmented_state) >= 1: extra = Generator.integers(factor) at the
 *                               reset and before the move of every step.
 *          OFFSIM_GRID_COUNTER  MyGridNaviModuloCounter (:158-184) with factor = counter_limit >= 1: extra = Generator.integers(factor) at
 *                               the reset, then (extra + 1) % factor before the move of every step.
 *        The observation is o = x + num_cells * y + num_cells^2 * extra, nS = num_cells^2 * factor; pi and Q are [nS, 5] f64 by observation.
 *        The exogenous stream is np.random.default_rng(episode0 + e), created again on the device at the reset of episode e of this call.
 *        integers(n) is NumPy's scalar path: nothing is drawn for n = 1, otherwise Lemire's bounded draw on 32-bit words, which are the low
 *        and then the high half of each 64-bit output (PCG64's buffered next_uint32): m = word * n, and while the low half of m is below
 *        (2^32 - n) % n another word is drawn; the result is m >> 32.
 *   ro   struct offsim_env_rollouts: R rollouts and their ACTION streams, PCG64 rows [R, 4] as offsim_seed_streams writes them (tabular.py:75:
 *        one default_rng(seed) per rollout that runs on across episodes).  OFFSIM_STREAM_PHILOX is refused with OFFSIM_EUNSUPPORTED (its
 *        double lies in (0, 1]: u = 1.0 would select action 5).
 * Per step: p = pi[o], or the behaviour policy on Q[o] (offsim_eval_td's rules, one definition on the device); A = Generator.choice(5, p=p)
 *   as offsim_eval_queue draws it (c_k = c_{k-1} + p_k in f64 from 0, cdf_k = c_k / c_4, u = (next64 >> 11) * 2^-53, the first k with
 *   cdf_k > u), one draw per step; extra is updated; then MyGridNavi.step: done if the agent already stands on the goal, the move clamped to
 *   the grid, step_count += 1 and done at num_steps, reward 0 if done, else 1 and done on reaching the goal, else -0.1 (f64).  A row p without
 *   a cdf entry above u (NaN, all zeros): OFFSIM_ST_KEYERROR, the draw consumed, the environment not stepped.
 * td: the update of offsim_eval_td on Q[o, A] with Q[o'] (tabular.py:123-126 / :175-178, the same arithmetic and order); q [R, nS, 5], td_err,
 *   alpha_ep / epsilon_ep, q_snap [R, snap_cap, nS, 5] / snap_stride / snap_cap, beh_arg, tie_mt, tie_reseed_episode (needs td->tie_mt): all
 *   offsim_eval_queue's, word for word.  The tie stream of episode e restarts as np.random.seed((episode0 + e) mod 2^32).
 * out: offsim_eval_mc's (sum_g, n_ep, steps, cand = steps, n_len, status; ep_g, ep_len); trace_pop [R, trace_cap] holds the ACTION drawn at
 *   every step, the undrawable one (5) of a rollout that stopped with OFFSIM_ST_KEYERROR included (at index steps); trace_row is not written.
 * On exit the action stream (the state after the last draw), q and tie_mt are written back; every episode begins with a reset, so a second
 *   call with episode0 moved on by the episodes of the first continues it.
 * Launch shapes.  Learners: one wavefront per rollout; LDS per workgroup: per rollout Q (nS * 40 bytes), the behaviour row (40) and the tie
 *   stream (2496), and the shared pi (nS * 40, when given); 4 rollouts per workgroup, then 2, then 1 while the carve exceeds 64 KiB, one rollout
 *   up to 160 KiB, beyond that -- or num_cells^2 > 40960 -- OFFSIM_EUNSUPPORTED.  evalMC: one LANE per rollout, 256 rollouts per workgroup, pi in
 *   LDS when its nS * 40 bytes (for a stack: L * nS * 40) are at most 64 KiB and read from global memory otherwise; nS * 5 > 2^24:
 *   OFFSIM_EUNSUPPORTED.
 * OFFSIM_EINVAL: NULL env / ro / out / required outputs / q / ro->rng with R > 0, a kind outside OFFSIM_GRID_*, num_cells < 1, num_steps < 1,
 *   a goal off the grid, factor < 1 (or != 1 for PLAIN), max_episodes <= 0, episode0 < 0, pi = NULL where a policy is read, a bad mode /
 *   behaviour / snapshot stride / tie_reseed_episode, schedules without n_sched, negative capacities.
 * Argument validation happens before any HIP call; ro->R = 0 launches nothing. */
#define OFFSIM_GRID_PLAIN 0
#define OFFSIM_GRID_NOISE 1
#define OFFSIM_GRID_COUNTER 2
typedef struct offsim_grid_env {
    int32_t kind;      /* OFFSIM_GRID_* */
    int32_t num_cells; /* the grid is num_cells x num_cells */
    int32_t num_steps; /* _max_episode_steps */
    int32_t goal_x;
    int32_t goal_y;
    int32_t factor;    /* NOISE: int(augmented_state); COUNTER: counter_limit; PLAIN: 1 */
} offsim_grid_env;
typedef struct offsim_env_rollouts {
    int32_t R;
    int32_t rng_kind; /* OFFSIM_STREAM_PCG64 */
    uint64_t *rng;    /* [R, 4] action streams */
} offsim_env_rollouts;
int offsim_eval_env(const offsim_grid_env *env, offsim_env_rollouts *ro, const double *pi /* [nS,5] or NULL with a Q-dependent behaviour */,
                    double gamma, const double *gamma_pow, int64_t n_gamma_pow, int64_t max_episodes, const offsim_evalmc_out *out,
                    const offsim_td *td /* NULL: evalMC */, int32_t tie_reseed_episode, int64_t episode0, void *stream);

/* offsim_eval_env_pop: offsim_eval_env for L policies or L learners on the same S action-stream seeds in ONE launch.  ro->R = L * S,
 * member-major: rollout r = l * S + j is member l on seed j; ro->rng holds [L * S, 4] rows (the caller's S rows replicated L times), advanced
 * per rollout.  All members of a seed start from the same action stream and see the same exogenous draws (default_rng(episode0 + e) depends
 * on the episode alone), so differences between members are paired.
 *   pop != NULL  a population of learners: struct offsim_td_pop as offsim_eval_queue_pop takes it with nS * 5 in the place of nZ * nA;
 *                pi_stack, gamma, gamma_pow and n_gamma_pow are ignored (pop's are read).  A workgroup holds rollouts of one learner
 *                (grid = L * ceil(S / rollouts per workgroup)); the carve and its 4 / 2 / 1 rule are offsim_eval_env's learner shape.
 *                Rollout l * S + j equals, in every output bit and in the state it leaves, offsim_eval_env's learner driver run alone with
 *                learner l's setting from seed j's stream, for every behaviour.
 *   pop == NULL  evalMC of the stack pi_stack [L, nS, 5] f64 with one gamma / gamma_pow: the lane-per-rollout shape, rollout r reads stack
 *                row r / S; tie_reseed_episode must be 0.  Rollout l * S + j equals offsim_eval_env's evalMC of pi_stack[l] from seed j.
 * OFFSIM_EINVAL as offsim_eval_env, and L outside 1..65535, S < 1, ro->R != L * S, pi_stack = NULL without pop, and everything
 * offsim_eval_td_pop checks about the per-learner arrays, behaviour_host, the schedules and the snapshot stride; OFFSIM_EUNSUPPORTED as
 * offsim_eval_env.  Argument validation happens before any HIP call; ro->R = 0 launches nothing. */
int offsim_eval_env_pop(const offsim_grid_env *env, offsim_env_rollouts *ro, int32_t L, int32_t S, const offsim_td_pop *pop,
                        const double *pi_stack, double gamma, const double *gamma_pow, int64_t n_gamma_pow, int64_t max_episodes,
                        const offsim_evalmc_out *out, int32_t tie_reseed_episode, int64_t episode0, void *stream);

/* Fast path of evalMC_psrs for a fixed tabular policy (the headline scan).
 * offsim_compile_policy folds psrs.py:53-57 for policy pi [n_slots,nA] f64 into one 64-bit key per grouped row:
 *   key = T << 11 | done << 10 | z_next_slot,  T = floor(2^53 * pi[z][a]/p_log[a]/max_a'(pi[z][a']/p_log[a'])),
 * so that  reject <=> u > threshold <=> (53-bit draw) > T, exactly (NaN or >= 1 thresholds give T = 2^53-1).
 * Needs n_slots <= 1024.  keys_out: [N] uint64, caller-owned.
 * offsim_eval_mc_keys runs the same loop as offsim_eval_mc (OFFSIM_PROB_F64, OFFSIM_REJECT_DEFAULT) from those keys,
 * with per-state candidate windows in LDS; n_slots <= 256, otherwise OFFSIM_EUNSUPPORTED (use offsim_eval_mc). */
int offsim_compile_policy(const offsim_table *t, const double *pi, uint64_t *keys_out, void *stream);
/* Name of the kernel offsim_eval_mc_keys launches for this state count and R rollouts ("" if it would refuse): measurement
 * code labels its roofline with it. */
const char *offsim_eval_mc_keys_kernel(int32_t n_slots, int32_t R);
int offsim_eval_mc_keys(const offsim_table *t, offsim_rollouts *ro, const uint64_t *keys, double gamma,
                        const double *gamma_pow, int64_t n_gamma_pow, int64_t max_episodes, const offsim_evalmc_out *out,
                        void *stream);

/* Faults of asynchronous kernels.  Every wait of one wavefront for another (the shuffle's ring protocol, the scan's chain / helper
 * hand-off) is bounded; a wait that gives up ends its workgroup instead of hanging the stream and raises a bit here:
 *   OFFSIM_FAULT_SHUFFLE  offsim_shuffle_queues[_keys]: the orders that call wrote are invalid
 *   OFFSIM_FAULT_SCAN     offsim_eval_mc_streams: the rollouts concerned also report OFFSIM_ST_PROTOCOL
 * offsim_async_faults() returns the bits raised on the current device since its last call and clears them (>= 0; negative: OFFSIM_E*).
 * The entry points themselves return before their kernels run: synchronise the stream first.  No fault has ever been observed in a
 * product build; tests/test_gpu_round3.py raises one with a -DSHUF_FAULT_INJECT build. */
#define OFFSIM_FAULT_SHUFFLE 1
#define OFFSIM_FAULT_SCAN 2
int offsim_async_faults(void);

/* Self-test of the hardware property the headline scan relies on beyond the ISA manual: the LDS applies the lanes of one
 * ds_add_rtn_u32 that hit the same address in ascending lane order (csrc/scan_rows.hpp takes the queue positions of a tick's
 * accepted candidates that way).  *mismatches (device, int64) receives the number of lane operations that returned anything
 * else over ~6e7 randomised ones: 0 on gfx950.  Asynchronous on `stream` like every other entry point. */
int offsim_selftest_lds_atomic_order(int64_t *mismatches, void *stream);
/* The same property as a runtime guard: 1 when the current device has it, 0 when not (or when OFFSIM_FORCE_LDS_ORDER_MISMATCH=1 is in
 * the environment: tests), negative OFFSIM_E* when the test could not run.  The first call on a device runs a short self-test (~1e6
 * lane operations on a stream of its own, synchronised: < 1 ms) and caches the verdict.  offsim_eval_mc_streams and the chunked shuffle
 * (offsim_shuffle_queues[_keys]_ws with a workspace, format C) call it themselves and return OFFSIM_EUNSUPPORTED on 0 -- never wrong
 * numbers; callers that want to route around it (to offsim_eval_mc_keys on permutations and a reset without workspace, as the Python
 * host mirror does) ask first.  The first call on a device allocates and synchronises: those entry points therefore return OFFSIM_EINVAL,
 * with nothing launched, when their stream is being captured and the verdict is not cached yet -- call this once outside the capture
 * (the Python host mirror does, in _lib.require_device()). */
int offsim_lds_order_ok(void);

/* ---- headline scan on per-rollout candidate streams ------------------------------------------------------------
 * For a fixed tabular policy the scan needs, per candidate, only a 32-bit digest of its compiled key (the top bits of the
 * threshold T, done, z_next) -- and per ACCEPTED candidate the row (for its reward).  Gathering digests through a
 * per-rollout permutation moves a 64-byte sector per 4-byte digest, so the sampler reset can instead lay the queue
 * orders out as two streams per rollout, both indexed like `perm` (seg_off[s] + k = k-th element of state s's queue):
 *   dig [n, N] u32   digest of the candidate at that queue position      -> read sequentially by the scan
 *   loc [n, N] u16   its row inside the state's segment (grouped row - seg_off[s]), low 16 bits (format C: u8, low 8 bits)
 * 4 + 2 bytes per queue position and rollout (format C: 4 + 1) in one of three layouts of the digest (offsim_streams.format):
 *   OFFSIM_STREAMS_A   [T >> 32 : 21 | done : 1 | z_next : 10] = the high dword of the compiled key; loc is the whole local row:
 *                      every state has at most 65536 rows;
 *   OFFSIM_STREAMS_B   [T >> 37 : 16 | hi[6:2] : 5 | done : 1 | hi[1:0] : 2 | z_next : 8], hi = bits 16..22 of the local row:
 *                      states of up to 2^23 rows, at most 255 states (a payload of all ones is not a digest).  (The coarser threshold only widens the band of draws that
 *                      are decided by the exact 53-bit look; results are the same bit for bit.)
 *   OFFSIM_STREAMS_C   [T >> 39 : 14 | hi[8:2] : 7 | done : 1 | hi[1:0] : 2 | z_next : 8], hi = bits 8..16 of the local row, loc = its
 *                      low byte: 5 bytes per queue position for states of up to 2^17 rows, at most 255 states -- a sixth less to keep
 *                      resident and to write per sampler reset (a 12.5 M-row shard x 4096 rollouts: 256 GB instead of 307 GB, one
 *                      resident tile instead of two).  Written by offsim_shuffle_queues_keys_ws only (every chain chunk by chunk).
 * offsim_compile_digests: dig32[g] = the digest of grouped row g in `format`, local-row bits zero (from offsim_compile_policy's keys).
 * offsim_shuffle_queues_keys: PSRS.reset_sampler's shuffles (psrs.py:22-23,29-30; same orders as offsim_shuffle_queues,
 *   bit for bit) written as those streams; init_perm_out as in offsim_shuffle_queues.  States of more than 65536 rows need
 *   format B (OFFSIM_EUNSUPPORTED otherwise): their chains are shuffled in place in dig_out and converted afterwards (or see
 *   offsim_shuffle_queues_keys_ws).
 * offsim_eval_mc_streams: evalMC_psrs (psrs.py:241-271) from the streams; same outputs, bit for bit, as offsim_eval_mc /
 *   offsim_eval_mc_keys on the same orders.  `keys` (offsim_compile_policy) is read only to decide digest ties
 *   exactly.  Strides are in elements; stride 0 = one order shared by all rollouts; loc == NULL = queues in table order
 *   (dig = dig32 itself, stride 0; format A).  ro->perm / perm_stride are ignored; ro->init_perm is used as everywhere else.
 *   n_slots <= 256 (255 for formats B and C); offsim_table.max_seg must be set: <= 65536 for format A, <= 2^23 for format B (OFFSIM_EUNSUPPORTED otherwise). */
#define OFFSIM_STREAMS_A 0
#define OFFSIM_STREAMS_B 1
#define OFFSIM_STREAMS_C 2
typedef struct offsim_streams {
    const uint32_t *dig;
    int64_t dig_stride;
    const void *loc;    /* u16 elements (formats A, B) or u8 (format C) */
    int64_t loc_stride; /* in elements */
    int32_t format; /* OFFSIM_STREAMS_* */
} offsim_streams;
int offsim_compile_digests(const offsim_table *t, const uint64_t *keys, int32_t format, uint32_t *dig32_out, void *stream);
int offsim_shuffle_queues_keys(const offsim_table *t, const uint64_t *seeds, int32_t n_perm, const uint32_t *dig32, int32_t format,
                               uint32_t *dig_out, void *loc_out, uint32_t *init_perm_out, void *stream);
/* The same with a workspace lent by the caller (device memory, 8-byte aligned, contents irrelevant before and after): the states of
 * more than 65536 rows are then shuffled chunk by chunk in LDS with sequential global traffic only (csrc/shuffle_chunk.hpp) instead
 * of in place with a random line per swap.  offsim_shuffle_workspace_bytes(t, n) = the bytes n persistent workgroups use (one per
 * compute unit is the most the call starts; 0 = the table has no such state); a smaller workspace runs fewer workgroups, one that
 * holds none (or NULL) gives offsim_shuffle_queues_keys.  Orders are the same bit for bit.  A message list of the chunked kernel
 * that overflowed (probability ~1e-15 per list) raises OFFSIM_FAULT_SHUFFLE (offsim_async_faults): the call's orders are void. */
int64_t offsim_shuffle_workspace_bytes(const offsim_table *t, int32_t n_workgroups);
/* offsim_shuffle_queues with such a workspace: the same permutations, the chains of more than 65536 rows chunk by chunk on chip. */
int offsim_shuffle_queues_ws(const offsim_table *t, const uint64_t *seeds, int32_t n_perm, uint32_t *perm_out, uint32_t *init_perm_out,
                             void *workspace, int64_t workspace_bytes, void *stream);
int offsim_shuffle_queues_keys_ws(const offsim_table *t, const uint64_t *seeds, int32_t n_perm, const uint32_t *dig32, int32_t format,
                                  uint32_t *dig_out, void *loc_out, uint32_t *init_perm_out, void *workspace, int64_t workspace_bytes,
                                  void *stream);
int offsim_eval_mc_streams(const offsim_table *t, offsim_rollouts *ro, const offsim_streams *sm, const uint64_t *keys,
                           double gamma, const double *gamma_pow, int64_t n_gamma_pow, int64_t max_episodes,
                           const offsim_evalmc_out *out, void *stream);

/* ---- encoders (a10, a11) --------------------------------------------------------------------- */

/* CartpoleBoxEncoder.encode (offsim4rl/encoders/heuristic.py:19-71): obs [N,4] f32 -> z [N] i32 in -1..161 */
int offsim_encode_box(const float *obs, int64_t N, int32_t *out_z, void *stream);

/* HOMEREncoder.encode (offsim4rl/encoders/homer.py:159-168) over EncoderModel.obs_encoder
 * (offsim4rl/encoders/models.py:15-19): z = argmax(W2 leaky_relu(W1 x + b1, 0.01) + b2).
 * x [N,dO] f32 (x_dtype OFFSIM_F32) or f16; W1 [H,dO], b1 [H], W2 [nZ,H], b2 [nZ] f32 (state_dict layout).
 * out_logits may be NULL. */
int offsim_encode_mlp(const void *x, int32_t x_dtype, int64_t N, int32_t dO, const float *W1, const float *b1,
                      int32_t H, const float *W2, const float *b2, int32_t nZ, int32_t *out_z, float *out_logits,
                      void *stream);

/* offsim_encode_mlp_pop: offsim_encode_mlp for L stacked encoders of one architecture in ONE launch (HOMERPopulation.encode).  Stacking as
 * offsim_policy_mlp_pop's, which is how HOMERPopulation holds its weights: W1 [L, H, dO], b1 [L, H], W2 [L, nZ, H], b2 [L, nZ], contiguous;
 * learner l's tensors are at W1 + l * H * dO and so on.  x [N, dO] is shared by all learners; out_z is [L, N] i32, out_logits [L, N, nZ]
 * f32 or NULL (64-bit offsets throughout).  The learner is the grid's y of offsim_encode_mlp's four kernels, chosen by the same rule
 * (the shape, 16-byte alignment of x, OFFSIM_ENCODER_F32): a workgroup serves one learner, loads that learner's weights into its
 * registers or LDS and walks the rows as the single call's does, so learner l's out_z[l] and out_logits[l] equal offsim_encode_mlp with
 * its tensors on the same x bit for bit (the order of a row's k summation does not depend on which wavefront takes the row).
 * Grid: (g, L) with g = max(min(single, ceil(N / rows_per_wg)), ceil(single / L)), where `single` is the workgroup count
 * offsim_encode_mlp starts for this N and rows_per_wg the rows a workgroup takes in one pass (4 wavefronts x 32 rows, x 2 on the
 * register kernels at dO = 2 and 4; 256 on the VALU kernel): the single call's count, capped by what the learner's rows fill, but
 * the L learners together never start fewer workgroups than the single call does.  L = 1 is the single call's grid.
 * Limits as offsim_encode_mlp's (H <= 128, the LDS limit: OFFSIM_EUNSUPPORTED; f32 / f16 observations); L in 1..65535 (otherwise
 * OFFSIM_EINVAL).  Argument validation happens before any HIP call; N = 0 launches nothing. */
int offsim_encode_mlp_pop(const void *x, int32_t x_dtype, int64_t N, int32_t dO, const float *W1, const float *b1, int32_t H,
                          const float *W2, const float *b2, int32_t nZ, int32_t L, int32_t *out_z, float *out_logits, void *stream);

/* offsim_latent_counts: what L encoders make of a log (HOMERPopulation.latent_report).  z [L, N] i32 (offsim_encode_mlp_pop's out_z);
 * labels [N] i32 or NULL, shared by all learners (the true state, for instance).  out_counts [L, nZ] i64: rows per latent state;
 * out_joint [L, nZ, nY] i64 or NULL (it must be NULL when labels is): rows per (latent state, label); out_skipped [L] i64: the rows
 * that are in neither, because their z is outside [0, nZ) or, with labels, their label is outside [0, nY).  The call zeroes its outputs
 * itself (on `stream`).  Grid (min(ceil(N / 4096), 1024), L): a workgroup serves one learner with one LDS histogram of
 * nZ * max(nY, 1) * 8 bytes (nY counts only with out_joint), flushed with one integer atomic add per non-empty bin, so the result is
 * exact and the same on every call.  More than 64 KiB of histogram is OFFSIM_EUNSUPPORTED; L in 1..65535, nZ >= 1, nY >= 1 with
 * labels (otherwise OFFSIM_EINVAL).  Argument validation happens before any HIP call; N = 0 zeroes the outputs and launches nothing. */
int offsim_latent_counts(const int32_t *z, int32_t L, int64_t N, int32_t nZ, const int32_t *labels, int32_t nY, int64_t *out_counts,
                         int64_t *out_joint, int64_t *out_skipped, void *stream);

/* The policy network of a row-policy evaluation (offsim4rl/agents/ppo.py:18-27, spinup's MLPCategoricalActor: logits_net =
 * Linear -> act -> ... -> Linear, probs = Categorical(logits=...).probs, a max-subtracted softmax):
 *   out_probs[m] = softmax(L_n(act(... act(L_1(x[rows[m]])))))   m < M, f32 [M, nA] with nA = the last layer's `out`.
 * x [n_x, dO] f32 or f16 (x_dtype); rows [M] i32 gather index into x (NULL: row m), an index outside [0, n_x) gives NaN;
 * layers_host: a HOST array of n_layers (1..4) layers, W [out,in] f32 and b [out] f32 (may be NULL) device pointers in state_dict
 * layout; the activation sits between layers, not after the last.  f32 arithmetic throughout (fmaf in k order per output).
 * Supported: dO <= 128, hidden widths <= 256, nA <= 16; anything else is OFFSIM_EINVAL. */
#define OFFSIM_ACT_IDENTITY 0
#define OFFSIM_ACT_TANH 1
#define OFFSIM_ACT_RELU 2
#define OFFSIM_ACT_LEAKY_RELU 3 /* slope: the negative slope */
typedef struct offsim_mlp_layer {
    const float *W; /* [out, in] */
    const float *b; /* [out] or NULL */
    int32_t in;
    int32_t out;
} offsim_mlp_layer;
int offsim_policy_mlp(const void *x, int32_t x_dtype, int64_t n_x, int32_t dO, const int32_t *rows, int64_t M,
                      const offsim_mlp_layer *layers_host, int32_t n_layers, int32_t activation, float slope, float *out_probs,
                      void *stream);

/* offsim_policy_mlp_pop: offsim_policy_mlp for L stacked networks of one architecture in ONE launch.  Stacking as
 * offsim_vector_collect_ppo_pop's: every layer's W is [L, out, in] and b is [L, out] (or NULL), contiguous; layers_host describes learner
 * 0, learner l's tensors are at W + l * out * in and b + l * out.  x, rows and M are shared by all learners; out_probs is [L, M, nA].
 * The grid is (ceil(M / 32), L): a workgroup serves one learner, and learner l's [M, nA] equals offsim_policy_mlp with its tensors bit
 * for bit (NaN rows included).  Limits as offsim_policy_mlp's; L in 1..65535 (otherwise OFFSIM_EINVAL).
 * Argument validation happens before any HIP call; M = 0 launches nothing. */
int offsim_policy_mlp_pop(const void *x, int32_t x_dtype, int64_t n_x, int32_t dO, const int32_t *rows, int64_t M,
                          const offsim_mlp_layer *layers_host, int32_t n_layers, int32_t activation, float slope, int32_t L,
                          float *out_probs, void *stream);

/* ---- a learner's data collection (VectorPSRS.collect) ------------------------------------------------------------------------
 * The loop a neural learner runs against the log (examples/cartpole/psrs_from_expert_heuristic.py:59-80, with the network fixed for
 * an epoch of steps_per_epoch steps, offsim4rl/agents/ppo.py:122-160): at every step the policy is asked at the current observation,
 * PSRS.step_dist serves a logged transition, and the environment is reset when the transition terminates the episode or when the
 * episode reaches max_episode_steps (:76-78).  offsim_vector_collect advances every environment of `ro` by T such steps in ONE launch
 * (one wavefront per environment) and records each step.  Per step, for an environment with a current state (cur_slot >= 0):
 *   1. p_new = the policy at the current observation (pol->form, below);
 *   2. PSRS.step(p_new) as offsim_step_batch (advance = 1): same queues, streams, reject and prob modes;
 *   3. served:  ep_t += 1; terminated = done of the served row; truncated = max_episode_steps > 0 && ep_t >= max_episode_steps
 *      (as the example, both may be set); on either, PSRS.reset (offsim_env_reset) and ep_t = 0;
 *      not served (None or KeyError): the environment stops for the rest of the launch, state and observation as they were.
 *   A reset that finds the init queue empty leaves cur_slot = -1 (and the observation at next_obs of the served row).
 * alive[r] (in/out) is cleared where a step is not served or a reset finds no initial row, as offsim_vector_step does.
 * Policy forms (pol->form):
 *   OFFSIM_COLLECT_MLP   the network of offsim_policy_mlp (same layers, activations and limits), evaluated by the environment's
 *                        wavefront: every output is the same fmaf chain and softmax as offsim_policy_mlp's, so p_new equals its output
 *                        bit for bit; widened to f64 for OFFSIM_PROB_F64.  The weights are staged into LDS once per workgroup: all
 *                        layers' W and b together at most OFFSIM_COLLECT_MLP_MAX_FLOATS floats (64 KiB, which leaves room for two
 *                        further workgroups of the C2 network per CU), otherwise OFFSIM_EUNSUPPORTED -- there is no L2 path.
 *                        Observations: x_start [R,dO] (the environments' current ones at the call), x_next / x_init [N,dO] (caller
 *                        rows' next_obs / obs), f32 or f16 (x_dtype).
 *   OFFSIM_COLLECT_ROWS  per-row probability tables in CALLER row order, p_next[i] = the policy at next_obs of row i and p_init[i] = the
 *                        policy at obs of row i (only initial rows are read), element type as offsim_eval_mc_rows_policy's; the
 *                        current observation is st->obs_row (below), which must be valid for every environment with a state.
 *   OFFSIM_COLLECT_TABULAR  pi [n_slots,nA] indexed by the state slot (observations are states), element type as offsim_eval_mc's;
 *                        in LDS, at most 160 KiB with the per-wavefront scratch, otherwise OFFSIM_EUNSUPPORTED.
 * State carried between calls (besides ro): ep_t [R] i32 steps of the current episode; obs_row [R] i32 where the observation comes
 * from, encoded as out_obs_row of offsim_eval_mc_rows_policy (i >= 0: next_obs of caller row i; -2 - i: obs of caller row i; -1: None
 * or unknown), rewritten where the observation changed; obs [R] rows of obs_bytes bytes, the environments' observation buffer (gets
 * next_obs / obs rows of obs_next / obs_init as the observation changes).
 * Records [T,R] (step-major): row = served caller row or -1; flags = OFFSIM_COLLECT_* bits; optional obs [T,R] rows of obs_bytes (the
 * observation the policy was asked at) and probs [T,R,nA] f32 (p_new).  Steps of an environment without a state are -1 / 0 / zeros.
 * status [R] (optional): OFFSIM_ST_OK, or why the environment stopped (EXHAUSTED, KEYERROR, NO_INIT, INACTIVE).
 * Argument validation happens before any HIP call; T = 0 launches nothing (row / flags may then be NULL). */
#define OFFSIM_COLLECT_MLP 0
#define OFFSIM_COLLECT_ROWS 1
#define OFFSIM_COLLECT_TABULAR 2
#define OFFSIM_COLLECT_MLP_MAX_FLOATS 16384
#define OFFSIM_COLLECT_SERVED 1     /* a transition was served                                     */
#define OFFSIM_COLLECT_TERMINATED 2 /* its done flag                                                */
#define OFFSIM_COLLECT_TRUNCATED 4  /* the episode reached max_episode_steps with it                 */
#define OFFSIM_COLLECT_RESET 8      /* reset after the step: the next observation is an initial one  */
#define OFFSIM_COLLECT_ALIVE 16     /* alive after the step                                         */
typedef struct offsim_collect_policy {
    int32_t form;                      /* OFFSIM_COLLECT_*                                          */
    int32_t n_layers;                  /* MLP: layers_host[n_layers] as offsim_policy_mlp           */
    const offsim_mlp_layer *layers_host;
    int32_t activation;
    float slope;
    int32_t x_dtype;                   /* MLP: OFFSIM_F32 | OFFSIM_F16                              */
    int32_t dO;
    const void *x_start;               /* MLP: [R,dO]                                               */
    const void *x_next;                /* MLP: [N,dO]                                               */
    const void *x_init;                /* MLP: [N,dO]                                               */
    const void *p_next;                /* ROWS: [N,nA]                                              */
    const void *p_init;                /* ROWS: [N,nA]                                              */
    const void *pi;                    /* TABULAR: [n_slots,nA]                                     */
} offsim_collect_policy;
typedef struct offsim_collect_state {
    int32_t *ep_t;                     /* [R] in/out                                                */
    int32_t *obs_row;                  /* [R] in/out                                                */
    uint8_t *alive;                    /* [R] in/out                                                */
    void *obs;                         /* [R] rows of obs_bytes, in/out                             */
    const void *obs_next;              /* [N] rows: next_observations, caller order                 */
    const void *obs_init;              /* [N] rows: observations, caller order                      */
    int64_t obs_bytes;
} offsim_collect_state;
typedef struct offsim_collect_out {
    int32_t *row;                      /* [T,R]                                                     */
    uint8_t *flags;                    /* [T,R]                                                     */
    void *obs;                         /* [T,R] rows of obs_bytes, or NULL                          */
    float *probs;                      /* [T,R,nA], or NULL                                         */
    int32_t *status;                   /* [R], or NULL                                              */
} offsim_collect_out;
int offsim_vector_collect(const offsim_table *t, offsim_rollouts *ro, const offsim_collect_policy *pol, int32_t prob_mode,
                          int32_t reject_mode, int64_t T, int32_t max_episode_steps, const offsim_collect_state *st,
                          const offsim_collect_out *out, void *stream);

/* ---- the PPO buffer of a collect (VectorPSRS.collect_ppo, ppo_advantages) ----------------------------------------------------
 * The critic spinup's PPO trains beside the actor (offsim4rl/agents/ppo.py:18-27, MLPActorCriticRevealed.step: pi and v(obs)), as
 * offsim_policy_mlp's network with one output unit and no softmax (spinup's MLPCritic: v = squeeze(v_net(obs), -1)):
 *   out_v[m] = L_n(act(... act(L_1(x[rows[m]]))))   m < M, f32 [M]; the last layer must have out = 1.
 * Arguments, limits and arithmetic as offsim_policy_mlp's. */
int offsim_value_mlp(const void *x, int32_t x_dtype, int64_t n_x, int32_t dO, const int32_t *rows, int64_t M,
                     const offsim_mlp_layer *layers_host, int32_t n_layers, int32_t activation, float slope, float *out_v, void *stream);

/* offsim_vector_collect_ppo: offsim_vector_collect (same arguments, same trajectory: rows, flags, probabilities and the sampler state are
 * those of offsim_vector_collect from the same state) plus the per-step records PPOAgentRevealed stores in its buffer
 * (offsim4rl/agents/ppo.py:106-158: begin_episode / step take v(obs) with pi, commit_action takes logp of the action, end_episode / step
 * hand a bootstrap value to PPOBuffer.finish_path):
 *   value [T,R]        v(obs) at the observation the actor is asked at (0 where nothing was served);
 *   logp [T,R]         log p_new[a] of the served action a: for OFFSIM_COLLECT_MLP from the logits as torch's Categorical.log_prob,
 *                      z[a] - (max + log(sum(exp(z - max)))); otherwise logf((float)p_new[a]) (0 where nothing was served);
 *   final_value [R]    v at the observation the environment holds after its last step -- for an environment that stopped (None, KeyError,
 *                      no initial row), the observation it stopped at; 0 for an environment without a state at the call.  Written
 *                      only when T > 0;
 *   v_trunc [T,R]      (optional) at a step that truncates without terminating, v(next_obs) of the served row, before the reset; nothing
 *                      is written at other steps.
 * The critic (val->form), whatever the actor's form:
 *   OFFSIM_VALUE_MLP   layers_host / activation / slope as offsim_value_mlp's, evaluated by the environment's wavefront through the same
 *                      fmaf chains, so value / final_value / v_trunc equal offsim_value_mlp's output bit for bit.  Its weights are staged
 *                      into LDS after the actor's: the actor's and the critic's floats together at most OFFSIM_COLLECT_MLP_MAX_FLOATS,
 *                      otherwise OFFSIM_EUNSUPPORTED.  Observations x_start [R,dO] / x_next / x_init [N,dO] as offsim_collect_policy's
 *                      (x_dtype must equal the actor's when the actor is OFFSIM_COLLECT_MLP).
 *   OFFSIM_VALUE_ROWS  per-row f32 tables in caller row order, v_next[i] = v(next_obs of row i), v_init[i] = v(obs of row i), read through
 *                      st->obs_row (which must be valid for every environment with a state, as for OFFSIM_COLLECT_ROWS). */
#define OFFSIM_VALUE_MLP 0
#define OFFSIM_VALUE_ROWS 1
typedef struct offsim_collect_value {
    int32_t form;                      /* OFFSIM_VALUE_*                                            */
    int32_t n_layers;                  /* MLP: layers_host[n_layers] as offsim_value_mlp            */
    const offsim_mlp_layer *layers_host;
    int32_t activation;
    float slope;
    int32_t x_dtype;                   /* MLP: OFFSIM_F32 | OFFSIM_F16                              */
    int32_t dO;
    const void *x_start;               /* MLP: [R,dO]                                               */
    const void *x_next;                /* MLP: [N,dO]                                               */
    const void *x_init;                /* MLP: [N,dO]                                               */
    const float *v_next;               /* ROWS: [N]                                                 */
    const float *v_init;               /* ROWS: [N]                                                 */
} offsim_collect_value;
typedef struct offsim_collect_ppo_out {
    float *value;                      /* [T,R]                                                     */
    float *logp;                       /* [T,R]                                                     */
    float *final_value;                /* [R]                                                       */
    float *v_trunc;                    /* [T,R], or NULL                                            */
} offsim_collect_ppo_out;
int offsim_vector_collect_ppo(const offsim_table *t, offsim_rollouts *ro, const offsim_collect_policy *pol, const offsim_collect_value *val,
                              int32_t prob_mode, int32_t reject_mode, int64_t T, int32_t max_episode_steps, const offsim_collect_state *st,
                              const offsim_collect_out *out, const offsim_collect_ppo_out *ppo, void *stream);

/* offsim_vector_collect_ppo_pop: offsim_vector_collect_ppo for a population of L independent learners in the same ONE launch.  `ro` holds
 * R = L * E environments, learner-major: environment r belongs to learner r / E and is run with that learner's actor and critic.  The
 * networks are stacked: every layer's W is [L, out, in] and b is [L, out], contiguous; pol->layers_host and val->layers_host describe
 * learner 0, and learner l's tensors are at W + l * out * in and b + l * out.  All learners share the architecture, the activation and
 * the observations' type.  Only pol->form = OFFSIM_COLLECT_MLP with val->form = OFFSIM_VALUE_MLP is supported (anything else:
 * OFFSIM_EUNSUPPORTED); the actor's and the critic's floats of ONE learner together are at most OFFSIM_COLLECT_MLP_MAX_FLOATS.
 * The grid is (ceil(E / 8), L): a workgroup stages one learner's two networks into LDS for up to eight of that learner's environments,
 * so E need not be a multiple of 8 and no workgroup serves two learners.  Everything else -- the step, the reset, the records [T, R]
 * (step-major: learner l's buffer is the columns l * E .. (l + 1) * E - 1), the carried state, x_start [R, dO] -- is
 * offsim_vector_collect_ppo's, and every environment's records and state equal, bit for bit, what offsim_vector_collect_ppo gives for
 * that environment with its learner's networks.  L in 1..65535, E >= 1, ro->R = L * E (otherwise OFFSIM_EINVAL).
 * Argument validation happens before any HIP call; T = 0 launches nothing. */
int offsim_vector_collect_ppo_pop(const offsim_table *t, offsim_rollouts *ro, const offsim_collect_policy *pol, const offsim_collect_value *val,
                                  int32_t L, int32_t E, int32_t prob_mode, int32_t reject_mode, int64_t T, int32_t max_episode_steps,
                                  const offsim_collect_state *st, const offsim_collect_out *out, const offsim_collect_ppo_out *ppo, void *stream);

/* ---- the same collection on QueueEvaluator (VectorQueueEvaluator.collect / collect_ppo / collect_ppo_population) -------------------
 * The loop of the reference's PPOAgent on a QueueEvaluator (offsim4rl/agents/ppo.py:258-279 on offsim4rl/evaluators/queue_evaluator.py:
 * 77-88): the agent draws its own action from its policy at the current observation, and the simulator pops the head of queue (z, a).
 * offsim_queue_collect is offsim_vector_collect with that step in the place of PSRS.step; offsim_queue_collect_ppo and
 * offsim_queue_collect_ppo_pop add what offsim_vector_collect_ppo and offsim_vector_collect_ppo_pop add.  The structs are theirs; the table
 * and `ro` are offsim_eval_queue's: grouped by the composite slot (z - z_lo) * nA + a, cur_slot / z_next / init_slot hold BASE slots
 * b = (z - z_lo) * nA, n_slots % nA == 0, nA_actions = t->nA, and ro->rng holds every environment's ACTION stream, OFFSIM_STREAM_PCG64
 * only (a Philox row: OFFSIM_EUNSUPPORTED, as offsim_eval_queue).  There is no prob_mode and no reject_mode.
 * Per step, for an environment with a state (0 <= b, b + nA <= n_slots; a state outside the table: OFFSIM_ST_KEYERROR):
 *   1. the critic, then the policy p at the current observation, in offsim_vector_collect's forms.  OFFSIM_COLLECT_MLP: offsim_policy_mlp's
 *      bits.  OFFSIM_COLLECT_ROWS: p_next / p_init [N,nA] in caller order.  OFFSIM_COLLECT_TABULAR: pi [n_slots / nA, nA] indexed by the
 *      STATE (row b / nA), as offsim_eval_queue's.  For ROWS and TABULAR pol->x_dtype names the tables' element type, OFFSIM_F32 or
 *      OFFSIM_F64.  The row is widened exactly to f64; probs [T,R,nA] records the f32 value;
 *   2. A = Generator.choice(nA, p=p) as offsim_eval_queue draws it: c_k = c_{k-1} + p_k in f64 from 0, cdf_k = c_k / c_{nA-1},
 *      u = (next64 >> 11) * 2^-53 from the environment's stream (one draw per asked step), A = the first k with cdf_k > u;
 *   3. the pop: the head of segment b + A through perm and the cursor.  No k with cdf_k > u (a row of NaN or zeros) or an empty segment:
 *      OFFSIM_ST_KEYERROR; the cursor at its end: OFFSIM_ST_EXHAUSTED.  Either way the environment stops for the rest of the launch with
 *      state, observation and cursor as they were; the draw stays consumed;
 *   4. records, ep_t, terminated / truncated and the reset: offsim_vector_collect's.  logp is taken at the drawn action, which is the served
 *      row's logged action by construction.
 * out_action [T,R] i32: the action drawn at every asked step, the unserved last one included (nA: none drawn); -1 where nothing was asked.
 * On exit the stream row is the state after the last draw; cursors, cur_slot, init_cursor and st are written back as offsim_vector_collect
 * does, so the call mixes with offsim_step_batch on the composite slot and with offsim_eval_queue.
 * Limits: nA <= 16 for every form (beyond: OFFSIM_EUNSUPPORTED); the networks' floats as offsim_vector_collect[_ppo]'s; the workgroup's LDS
 * -- [actor | pi as f64][critic][16 f64 + 16 f32 + 2 activation rows per environment], 8 environments -- at most 160 KiB.  There is no LDS
 * bound on n_slots outside the TABULAR form: cursors stay in global memory.
 * offsim_queue_collect_ppo_pop: L learners of E environments each, learner-major, grid (ceil(E / 8), L), stacked networks, MLP actors with
 * MLP critics only -- offsim_vector_collect_ppo_pop's rules, and every environment equals offsim_queue_collect_ppo with its learner's
 * networks bit for bit.
 * Argument validation happens before any HIP call; T = 0 or R = 0 launches nothing (row / flags / out_action may then be NULL). */
int offsim_queue_collect(const offsim_table *t, offsim_rollouts *ro, int32_t nA_actions, const offsim_collect_policy *pol, int64_t T,
                         int32_t max_episode_steps, const offsim_collect_state *st, const offsim_collect_out *out, int32_t *out_action,
                         void *stream);
int offsim_queue_collect_ppo(const offsim_table *t, offsim_rollouts *ro, int32_t nA_actions, const offsim_collect_policy *pol,
                             const offsim_collect_value *val, int64_t T, int32_t max_episode_steps, const offsim_collect_state *st,
                             const offsim_collect_out *out, int32_t *out_action, const offsim_collect_ppo_out *ppo, void *stream);
int offsim_queue_collect_ppo_pop(const offsim_table *t, offsim_rollouts *ro, int32_t nA_actions, const offsim_collect_policy *pol,
                                 const offsim_collect_value *val, int32_t L, int32_t E, int64_t T, int32_t max_episode_steps,
                                 const offsim_collect_state *st, const offsim_collect_out *out, int32_t *out_action,
                                 const offsim_collect_ppo_out *ppo, void *stream);

/* ---- the same collection in the environments that produced the logs (VectorGridNavi / VectorCartPole) ---------------------------------
 * The other half of the reference's experiments: the learner's loop in the real environment, to set beside its loop inside a simulator
 * built from a log.  offsim_env_collect is offsim_queue_collect with the environment's dynamics in the place of the queue pop -- there is
 * no table, nothing is popped, and an environment never runs dry; offsim_env_collect_ppo and offsim_env_collect_ppo_pop add what
 * offsim_vector_collect_ppo and offsim_vector_collect_ppo_pop add.  The policy, critic and PPO record structs are theirs.
 * Environments (env->kind), R of them, every one with two PCG64 streams ([R,4] words as offsim_seed_streams writes them): rng_act, from
 * which its actions are drawn, and rng_env, from which the environment draws its own noise and resets:
 *   OFFSIM_ENV_GRID         the reference's MyGridNavi (offsim4rl/envs/gridworld.py:14-124) with discrete observations: nA = 5 (noop, up,
 *                           right, down, left), the observation is the cell id x + num_cells * y (i32; a network reads it as one f32);
 *   OFFSIM_ENV_GRID_COORDS  MyGridNaviCoords (:187-211): observation (x / 5 + 0.1 + d0, y / 5 + 0.1 + d1) computed in f64 and rounded once
 *                           to f32, d = -0.1 + 0.2 * next_double drawn twice at every step and twice at every reset -- default_rng(seed)
 *                           .uniform(-0.1, 0.1, 2), continuing across resets as reset() without a seed does.  The divisor is the literal 5;
 *   OFFSIM_ENV_CARTPOLE     CartPole-v1: nA = 2, Euler steps of tau = 0.02 in f64 with the operation order of the package's host generator
 *                           (synth.cartpole_log), terminated at |x| > 2.4 or |theta| > 12 degrees, reward 1, a reset draws
 *                           uniform(-0.05, 0.05, 4) = -0.05 + 0.1 * next_double; the f32 observation is the f64 state rounded once.
 * Grid step, MyGridNavi.step to the letter: done if the agent stands on the goal before it moves; the move, clamped at the walls;
 * step_count += 1 and done at step_count >= num_steps; reward 0 if done, else 1 (and done) on reaching the goal, else -0.1.  The old
 * API's `done` is recorded as terminated.  goal_x / goal_y, num_cells (1..1024) and num_steps (>= 1) are parameters.
 * State carried between calls, all in/out: state [R,4] f64 -- CartPole (x, x_dot, theta, theta_dot); the grids (x, y, obs_0, obs_1) with
 * the f64 observation of GRID_COORDS (zeros for GRID) -- step_count [R] (the grids'), ep_t [R] (steps of the open episode), and the
 * two streams' positions.  offsim_env_collect_reset is reset() for the environments in mask (NULL: all): the start state, step_count =
 * ep_t = 0, the reset's draws taken from rng_env.  It does not touch rng_act.
 * Per step: the critic, then the policy at the current observation -- OFFSIM_COLLECT_MLP (offsim_policy_mlp's bits; x_dtype must be
 * OFFSIM_F32 and dO the observation's width 1 / 2 / 4; x_start / x_next / x_init are not read) or, on the grids, OFFSIM_COLLECT_TABULAR
 * (pi [num_cells^2, 5] by cell id, x_dtype its element type OFFSIM_F32 | OFFSIM_F64, widened exactly to f64); there are no logged rows and
 * so no ROWS form (OFFSIM_EUNSUPPORTED, as TABULAR on CartPole) -- then A drawn as offsim_queue_collect draws it, one draw of rng_act per
 * asked step; the dynamics; ep_t += 1, truncated = max_episode_steps > 0 && ep_t >= max_episode_steps; on terminated or truncated the
 * reset and ep_t = 0.  No A (a row of NaN or zeros): the environment stops for the rest of the launch with OFFSIM_ST_KEYERROR, state as
 * it was, the draw consumed; otherwise every asked step is served and status stays OFFSIM_ST_OK.
 * Records, step-major [T,R]; obs / next_obs / state / next_state / probs / status may be NULL:
 *   obs, next_obs      rows of the observation's width, f32 (GRID: one i32, the cell id); next_obs is the true next observation, not the
 *                      one a reset puts in its place;
 *   state, next_state  CartPole: [T,R,4] f64; the grids: [T,R] i32 cell ids z / z_next;
 *   probs [T,R,nA] f32, action [T,R] i32 (nA where none could be drawn, -1 where nothing was asked), reward [T,R] f32, flags [T,R]
 *   OFFSIM_COLLECT_* bits (SERVED and ALIVE at every served step), ep_step [T,R] i32 (the step's index in its episode);
 *   value / logp / final_value / v_trunc as offsim_vector_collect_ppo's, the critic OFFSIM_VALUE_MLP only.
 * Limits: the networks' floats as offsim_vector_collect[_ppo]'s; the workgroup's LDS -- [actor | pi as f64][critic][16 f64 + 16 f32 + 2
 * activation rows + 8 f32 per environment], 8 environments -- at most 160 KiB (OFFSIM_EUNSUPPORTED beyond).
 * offsim_env_collect_ppo_pop: L learners of E environments each, learner-major, grid (ceil(E / 8), L), stacked networks, MLP actors with
 * MLP critics only, L in 1..65535, env->R = L * E -- offsim_vector_collect_ppo_pop's rules, and every environment equals
 * offsim_env_collect_ppo with its learner's networks bit for bit.
 * Argument validation happens before any HIP call; T = 0 or R = 0 launches nothing (the record pointers may then be NULL). */
#define OFFSIM_ENV_GRID 0
#define OFFSIM_ENV_GRID_COORDS 1
#define OFFSIM_ENV_CARTPOLE 2
typedef struct offsim_env {
    int32_t kind;                      /* OFFSIM_ENV_*                                              */
    int32_t R;                         /* environments                                              */
    int32_t num_cells;                 /* grids                                                     */
    int32_t num_steps;                 /* grids: MyGridNavi._max_episode_steps                      */
    int32_t goal_x;
    int32_t goal_y;
    uint64_t *rng_env;                 /* [R,4] in/out                                              */
    uint64_t *rng_act;                 /* [R,4] in/out                                              */
    double *state;                     /* [R,4] in/out                                              */
    int32_t *step_count;               /* [R] in/out                                                */
    int32_t *ep_t;                     /* [R] in/out                                                */
} offsim_env;
typedef struct offsim_env_out {
    void *obs;                         /* [T,R] rows, or NULL                                       */
    void *next_obs;                    /* [T,R] rows, or NULL                                       */
    void *state;                       /* [T,R,4] f64 | [T,R] i32, or NULL                          */
    void *next_state;                  /* likewise                                                  */
    float *probs;                      /* [T,R,nA], or NULL                                         */
    int32_t *action;                   /* [T,R]                                                     */
    float *reward;                     /* [T,R]                                                     */
    uint8_t *flags;                    /* [T,R]                                                     */
    int32_t *ep_step;                  /* [T,R]                                                     */
    int32_t *status;                   /* [R], or NULL                                              */
} offsim_env_out;
int offsim_env_collect_reset(const offsim_env *env, const uint8_t *mask, void *stream);
int offsim_env_collect(const offsim_env *env, const offsim_collect_policy *pol, int64_t T, int32_t max_episode_steps,
                       const offsim_env_out *out, void *stream);
int offsim_env_collect_ppo(const offsim_env *env, const offsim_collect_policy *pol, const offsim_collect_value *val, int64_t T,
                           int32_t max_episode_steps, const offsim_env_out *out, const offsim_collect_ppo_out *ppo, void *stream);
int offsim_env_collect_ppo_pop(const offsim_env *env, const offsim_collect_policy *pol, const offsim_collect_value *val, int32_t L, int32_t E,
                               int64_t T, int32_t max_episode_steps, const offsim_env_out *out, const offsim_collect_ppo_out *ppo,
                               void *stream);

/* ---- evalMC of policies over observations in those environments: L actors on S paired seeds per launch ------------------------------------
 * The value of MLP actors in the true dynamics, beside their value inside PSRS (offsim_eval_mc_rows_policy_pop) and inside the (z, a)
 * queues (offsim_eval_queue_rows_policy_pop).  offsim_eval_env_obs runs L * S rollouts in ONE launch, one wavefront each, grid (ceil(S / 8),
 * L): rollout (l, j) runs policy l for n_episodes episodes on seed j.  It is a query: there is no carried state, and the streams are read
 * only -- rollout (l, j) starts from row j of rng_env / rng_act ([S,4] words as offsim_seed_streams writes them), whatever l, so every policy
 * of a seed sees the same resets, the same noise and the same action uniforms, and differences between policies are paired.
 * The environments (env->kind) and their rules are offsim_env_collect's.  Per episode: reset() (its draws from the env stream); per step the
 * policy at the current observation (offsim_policy_mlp's bits, widened to f64), A drawn as offsim_env_collect draws it with one draw of the
 * action stream, the dynamics, G = G + gamma_pow[t] * (double)reward in f64 in step order, t += 1; the episode ends at terminated, or
 * truncated at max_episode_steps > 0 && t >= max_episode_steps (both bits may be set).  max_episode_steps is required for CartPole (> 0;
 * CartPole-v1's is 500) and optional on the grids, whose num_steps already bounds an episode.  gamma_pow [n_gamma_pow]: gamma**t as the
 * host computes it, at least as long as the longest episode (the cap; on the grids min(cap, num_steps) or num_steps).  A rollout equals,
 * bit for bit, what offsim_env_collect records for one environment on the same streams, cut into its first n_episodes episodes.
 * No A (a row of NaN or zeros): the rollout stops with OFFSIM_ST_KEYERROR, the draw consumed, the open episode dropped.
 * pol: OFFSIM_COLLECT_MLP only -- one network (L = 1) or stacked ones (W [L][out][in], b [L][out], the descriptor learner 0's, as
 * offsim_policy_mlp_pop); x_dtype OFFSIM_F32, dO the observation's width 1 / 2 / 4, the last layer nA = 5 / 5 / 2 units; x_start / x_next /
 * x_init are not read.  The ROWS and TABULAR forms are refused with OFFSIM_EUNSUPPORTED (there are no logged rows; tabular policies on the
 * grids are offsim_eval_env's).  L in 1..65535.
 * Outputs, all written by the kernel, policy-major:
 *   Gs [L,S,n_episodes] f64, lengths [L,S,n_episodes] i32, ended [L,S,n_episodes] u8 (OFFSIM_COLLECT_TERMINATED | OFFSIM_COLLECT_TRUNCATED)
 *   per completed episode, zeros for the episodes a stopped rollout did not complete;
 *   n_ep [L,S] episodes completed, steps [L,S] steps taken, status [L,S] OFFSIM_ST_OK | OFFSIM_ST_KEYERROR;
 *   value [L,S] f64: the sum of the completed episodes' G in episode order, divided by n_ep (NaN for n_ep = 0).
 * Trace (optional, for tests; any pointer may be NULL) of a rollout's first trace_cap steps, across episode boundaries: trace_action
 *   [L,S,trace_cap] i32 (nA at the undrawable step); trace_state / trace_next_state [L,S,trace_cap,4] f64: offsim_env's state row before
 *   the step, and after it before any reset.  The caller fills them; steps not taken are left as they were.
 * Limits: the workgroup's LDS -- [W^T / b][16 f64 + 16 f32 + 2 activation rows + 8 f32 per rollout], 8 rollouts -- at most 160 KiB
 * (OFFSIM_EUNSUPPORTED beyond); no other cap on the weights.
 * Argument validation happens before any HIP call; S = 0 or n_episodes = 0 launches nothing (the output pointers may then be NULL). */
typedef struct offsim_env_eval {
    int32_t kind;                      /* OFFSIM_ENV_*                                              */
    int32_t S;                         /* seeds                                                     */
    int32_t num_cells;                 /* grids                                                     */
    int32_t num_steps;                 /* grids: MyGridNavi._max_episode_steps                      */
    int32_t goal_x;
    int32_t goal_y;
    const uint64_t *rng_env;           /* [S,4] read only                                           */
    const uint64_t *rng_act;           /* [S,4] read only                                           */
} offsim_env_eval;
typedef struct offsim_env_eval_out {
    double *Gs;                        /* [L,S,n_episodes]                                          */
    int32_t *lengths;                  /* [L,S,n_episodes]                                          */
    uint8_t *ended;                    /* [L,S,n_episodes]                                          */
    int64_t *n_ep;                     /* [L,S]                                                     */
    int64_t *steps;                    /* [L,S]                                                     */
    int32_t *status;                   /* [L,S]                                                     */
    double *value;                     /* [L,S]                                                     */
    int64_t trace_cap;
    int32_t *trace_action;             /* [L,S,trace_cap], or NULL                                  */
    double *trace_state;               /* [L,S,trace_cap,4], or NULL                                */
    double *trace_next_state;          /* likewise                                                  */
} offsim_env_eval_out;
int offsim_eval_env_obs(const offsim_env_eval *env, const offsim_collect_policy *pol, int32_t L, int64_t n_episodes, int32_t max_episode_steps,
                        const double *gamma_pow, int64_t n_gamma_pow, const offsim_env_eval_out *out, void *stream);

/* ---- tabular policies and TD learners on the LATENT STATES of those environments: the tabular drivers behind an encoder ---------------------
 * offsim_eval_env_latent: the reference's tabular drivers -- evalMC (td = NULL; offsim4rl/agents/tabular.py:247-270), qlearn (:71-139),
 * expSARSA (:141-191) and z_expSARSA (:193-245, run->rec_max) by td->mode -- on CartPole-v1 (OFFSIM_ENV_CARTPOLE) and MyGridNaviCoords
 * (OFFSIM_ENV_GRID_COORDS, offsim4rl/envs/gridworld.py:187-211), whose observations are continuous, with pi and Q [nS, nA] indexed by
 * z = enc(observation): all rollouts in ONE launch (csrc/eval_env_latent.hpp), one wavefront each.  The ground truth that offsim_eval_td /
 * offsim_eval_mc (PSRS) and offsim_eval_queue (the (z, a) queues) on a log encoded by the same encoder are judged against.
 *   env  struct offsim_env_eval: the world and its rules as offsim_env_collect's (nA = 2 / 5); S is the number of ROLLOUTS R, and rng_act /
 *        rng_env hold [R, 4] PCG64 rows as offsim_seed_streams writes them, READ ONLY: the call is a query, and where the streams stand
 *        afterwards comes back in run->rng_act_end / rng_env_end.  OFFSIM_ENV_GRID is refused with OFFSIM_EUNSUPPORTED (offsim_eval_env's).
 *   enc  struct offsim_latent_encoder, run in the kernel at every observation the loop visits (the f32 observation offsim_env_collect records):
 *          OFFSIM_LATENT_BOX  CartpoleBoxEncoder.get_box with offsim_encode_box's f32 literals and comparisons: -1 (out of bounds) .. 161;
 *                             OFFSIM_ENV_CARTPOLE only (OFFSIM_EUNSUPPORTED otherwise), nS >= 162.
 *          OFFSIM_LATENT_MLP  the HOMER obs_encoder Linear(dO, H) -> LeakyReLU(0.01) -> Linear(H, nZ) -> first arg max, offsim_encode_mlp's
 *                             arithmetic (per unit one k-ordered fmaf chain from 0, then the bias; a row that is all NaN gives 0); W1 [H, dO],
 *                             b1 [H], W2 [nZ, H], b2 [nZ] f32 device pointers, dO the observation's width (2 / 4), nZ <= nS.  Limits: H and nZ
 *                             at most 4096 each, and the weights (H * dO + H + nZ * H + nZ floats, staged once per workgroup) with 4 + H + nZ
 *                             floats per rollout must fit the LDS carve below: OFFSIM_EUNSUPPORTED beyond.
 *        nS: the rows of pi and Q.  The row of z is z for 0 <= z < nS and z + nS for -nS <= z < 0 -- NumPy's index wrap: the reference's Q[-1]
 *        is the last row -- the rule TransitionTable's slots follow on the PSRS side, so Q compares entry for entry.
 * Per step: z = enc(obs); p = pi[row], or the behaviour policy on Q[row] (offsim_eval_td's rules); A = Generator.choice(nA, p=p) as
 *   offsim_eval_env draws it, one draw of the action stream per step; the dynamics (offsim_env_collect's, their draws from the environment
 *   stream); z' = enc(obs'); the update of offsim_eval_td on Q[row, A] with Q[row'] (the same arithmetic and order; done is not masked, as in
 *   the reference); G = G + gamma_pow[t] * (double)reward, where the grid's -0.1f is widened to the f64 literal -0.1, the reference's
 *   Python float.  A row p without a cdf entry above u (NaN, all zeros): OFFSIM_ST_KEYERROR, the draw consumed, the environment not stepped.
 *   An episode ends at done or at run->max_episode_steps (required > 0 for CartPole, CartPole-v1's is 500; 0 on the grid: num_steps alone).
 * run  struct offsim_latent_run:
 *        reseed = 1  the reference's protocol: episode e of the call restarts the environment stream as np.random.default_rng(episode0 + e),
 *                    seeded on the device, and draws the reset from it (env.reset(seed=episode)); env->rng_env is not read;
 *        reseed = 0  the rollout's own environment stream (row r of env->rng_env) runs on across episodes;
 *        rec_max = 1 (z_expSARSA, OFFSIM_TD_EXPSARSA only) td_err records R + gamma * max_a Q[row', a] - Q[row, A] while the update stays
 *                    expected SARSA (tabular.py:229 / :232);
 *        tie_reseed_episode (needs tie_mt): the tie stream of episode e restarts as np.random.seed((episode0 + e) mod 2^32);
 *        rng_act_end / rng_env_end [R, 4] or NULL: the rows a later call continues from (with episode0 moved on by the episodes run);
 *        the trace (optional, for tests; any pointer NULL) of a rollout's first trace_cap steps: trace_z / trace_z_next [R, trace_cap] i32 as
 *        the encoder gave them (before the wrap), trace_reward [R, trace_cap] f64, trace_done [R, trace_cap] u8, trace_state /
 *        trace_next_state [R, trace_cap, 4] f64 (offsim_env's state row before and after the step).  Steps not taken are left as they were.
 * td, out, gamma_pow: offsim_eval_env's, word for word, with q [R, nS, nA]; trace_pop holds the ACTION drawn at every step (nA at the
 *   undrawable one).  On exit q and tie_mt are written back.
 * Launch shape: one wavefront per rollout; LDS per workgroup: per rollout Q (nS * nA * 8 bytes), the behaviour row and the tie stream (2496)
 *   for a learner, the shared pi when given, the encoder's weights and 4 * (4 + H + nZ) bytes per rollout; 4 rollouts per workgroup, then 2,
 *   then 1 while the carve exceeds 64 KiB, one rollout up to 160 KiB, beyond that -- or nS * nA > 40960 -- OFFSIM_EUNSUPPORTED.
 * OFFSIM_EINVAL: NULL env / enc / run / out / required outputs / q / weights / streams with S > 0, unknown kinds, a goal off the grid, nS < 1,
 *   nZ > nS, an input width that is not the observation's, CartPole without a cap, n_episodes <= 0, episode0 < 0, pi = NULL where a policy is
 *   read, flags outside 0 / 1, rec_max without OFFSIM_TD_EXPSARSA, and everything offsim_eval_env checks about td and out.
 * Argument validation happens before any HIP call; env->S = 0 launches nothing.
 *
 * offsim_eval_env_latent_pop: offsim_eval_env_latent for L policies or L learners on the same S seeds in ONE launch, behind ONE encoder.
 * env->S = L * S rollouts, member-major: rollout r = l * S + j is member l on seed j; the stream tables hold [L * S, 4] rows (the caller's S
 * rows replicated L times), so all members of a seed see the same resets, the same noise and the same action uniforms.
 *   pop != NULL  a population of learners: struct offsim_td_pop as offsim_eval_env_pop takes it with nS * nA entries per table; pi_stack,
 *                gamma, gamma_pow and n_gamma_pow are ignored (pop's are read).  A workgroup holds rollouts of one learner (grid = L *
 *                ceil(S / rollouts per workgroup)).  Rollout l * S + j equals, in every output bit, offsim_eval_env_latent run alone with
 *                learner l's setting on seed j's streams.
 *   pop == NULL  evalMC of the stack pi_stack [L, nS, nA] f64 with one gamma / gamma_pow, the same launch shape (a workgroup stages its
 *                policy); run->tie_reseed_episode and rec_max must be 0.
 * OFFSIM_EINVAL as offsim_eval_env_latent, and L outside 1..65535, S < 1, env->S != L * S, pi_stack = NULL without pop, and everything
 * offsim_eval_td_pop checks about the per-learner arrays; OFFSIM_EUNSUPPORTED as offsim_eval_env_latent.  Argument validation happens
 * before any HIP call; env->S = 0 launches nothing. */
#define OFFSIM_LATENT_BOX 0
#define OFFSIM_LATENT_MLP 1
typedef struct offsim_latent_encoder {
    int32_t kind;                      /* OFFSIM_LATENT_*                                           */
    int32_t nS;                        /* rows of pi and Q                                          */
    int32_t dO, H, nZ;                 /* MLP                                                       */
    const float *W1, *b1, *W2, *b2;    /* MLP: state_dict layout, device pointers                   */
} offsim_latent_encoder;
typedef struct offsim_latent_run {
    int32_t reseed;                    /* 1: default_rng(episode0 + e) per episode; 0: env->rng_env */
    int32_t max_episode_steps;         /* 0: none (the grid)                                        */
    int32_t rec_max;                   /* z_expSARSA's recorded TD error                            */
    int32_t tie_reseed_episode;
    int64_t episode0;
    uint64_t *rng_act_end;             /* [R,4], or NULL                                            */
    uint64_t *rng_env_end;             /* [R,4], or NULL                                            */
    int64_t trace_cap;
    int32_t *trace_z;                  /* [R,trace_cap], or NULL                                    */
    int32_t *trace_z_next;             /* likewise                                                  */
    double *trace_reward;              /* likewise                                                  */
    uint8_t *trace_done;               /* likewise                                                  */
    double *trace_state;               /* [R,trace_cap,4], or NULL                                  */
    double *trace_next_state;          /* likewise                                                  */
} offsim_latent_run;
int offsim_eval_env_latent(const offsim_env_eval *env, const offsim_latent_encoder *enc, const double *pi /* [nS,nA] or NULL */, double gamma,
                           const double *gamma_pow, int64_t n_gamma_pow, int64_t n_episodes, const offsim_evalmc_out *out,
                           const offsim_td *td /* NULL: evalMC */, const offsim_latent_run *run, void *stream);
int offsim_eval_env_latent_pop(const offsim_env_eval *env, const offsim_latent_encoder *enc, int32_t L, int32_t S, const offsim_td_pop *pop,
                               const double *pi_stack, double gamma, const double *gamma_pow, int64_t n_gamma_pow, int64_t n_episodes,
                               const offsim_evalmc_out *out, const offsim_latent_run *run, void *stream);

/* offsim_ppo_advantages: GAE-lambda advantages and rewards-to-go over step-major [T,E] records, with the path rules of the reference's
 * agent, and spinup's advantage normalisation (spinup PPOBuffer.finish_path / get, driven by offsim4rl/agents/ppo.py:106-158; E
 * environments = E MPI processes of local_steps_per_epoch = T).  Per environment e, over its valid steps t (flags & OFFSIM_COLLECT_SERVED):
 *   a path ends at a step with OFFSIM_COLLECT_TERMINATED | OFFSIM_COLLECT_TRUNCATED (end_episode), with the bootstrap
 *     OFFSIM_PPO_BOOT_REFERENCE  value[t] (end_episode's prev_v) if truncated or t = T - 1 (the epoch ended), else 0 (ppo.py:116-131);
 *     OFFSIM_PPO_BOOT_SPINUP     0 if terminated, else v_trunc[t] (the textbook rule; v_trunc is then required);
 *   a path still open after the last valid step bootstraps with final_value[e] (step's epoch cut, ppo.py:149-158, or a stopped
 *   environment);
 *   within a path (finish_path): delta_t = rew[t] + gamma V_next - value[t] (V_next: the path's next value, or the bootstrap),
 *   adv[t] = sum_k (gamma lam)^k delta_{t+k}, ret[t] = sum_k gamma^k rew[t+k] + gamma^K bootstrap.
 * Accumulated in f64, stored f32; invalid entries get 0.  adv_norm (optional): (adv - mean) / std over all valid entries of all
 * environments, mean = sum(adv) / n, std = sqrt(sum((adv - mean)^2) / n) (mpi_statistics_scalar, the population std), reduced in a fixed
 * order (the same bits every run); stats[0..1] = mean, std.  n = 0 leaves adv_norm = adv (zeros) and reports std = 0; a std of 0 with
 * n > 0 divides as spinup does.  work: OFFSIM_PPO_WORK_DOUBLES(E) doubles of device scratch (needed with adv_norm).  One launch, three
 * with adv_norm.  Argument validation happens before any HIP call. */
#define OFFSIM_PPO_BOOT_REFERENCE 0
#define OFFSIM_PPO_BOOT_SPINUP 1
#define OFFSIM_PPO_WORK_DOUBLES(E) (3 * (((E) + 255) / 256))
int offsim_ppo_advantages(const float *rew, const float *value, const uint8_t *flags, const float *final_value, const float *v_trunc,
                          int64_t T, int64_t E, double gamma, double lam, int32_t bootstrap, float *adv, float *ret, float *adv_norm,
                          double *stats, double *work, void *stream);

/* offsim_ppo_advantages_pop: offsim_ppo_advantages over the step-major [T, L * E] records of a population of L learners with E
 * environments each (learner-major columns, as offsim_vector_collect_ppo_pop leaves them; final_value [L * E]).  GAE-lambda and
 * rewards-to-go run per environment exactly as in offsim_ppo_advantages.  adv_norm, mean and std are PER LEARNER, over that learner's
 * [T, E] entries, each sum in the fixed order offsim_ppo_advantages uses on a contiguous [T, E] input: the same bits.  stats [L, 2] =
 * (mean, std) per learner; a learner without a valid entry gets std = 0 and adv_norm = adv.  work: OFFSIM_PPO_WORK_DOUBLES_POP(L, E)
 * doubles.  The same launches as offsim_ppo_advantages, on a grid (ceil(E / 256), L).  L in 1..65535, E >= 1.
 * Argument validation happens before any HIP call. */
#define OFFSIM_PPO_WORK_DOUBLES_POP(L, E) ((L) * OFFSIM_PPO_WORK_DOUBLES(E))
int offsim_ppo_advantages_pop(const float *rew, const float *value, const uint8_t *flags, const float *final_value, const float *v_trunc,
                              int64_t T, int32_t L, int64_t E, double gamma, double lam, int32_t bootstrap, float *adv, float *ret,
                              float *adv_norm, double *stats, double *work, void *stream);

/* offsim_ppo_epoch_log: what the reference's agent hands to its EpochLogger during one epoch, and spinup's statistics of it, over the
 * step-major [T, E] records of that epoch as offsim_vector_collect_ppo leaves them (offsim4rl/agents/ppo.py:103-160, :225-235; E
 * environments = E MPI processes).  valid / terminated / truncated: [T, E] bytes, non-zero = set.  open_ret [E] f64 and open_len [E] i32
 * are the caller's carried state -- self.ep_ret / self.ep_len of every environment -- read and updated in place, so an episode that an
 * epoch cuts goes on in the next call (zero them to begin).  Per environment, over its valid steps in order:
 *   open_ret += (double)rew, open_len += 1;
 *   at a step with terminated or truncated an episode ends: its return is open_ret, its length open_len - 1 under
 *     OFFSIM_EPLEN_REFERENCE (end_episode does not count its own transition, ppo.py:116-133; step does, :138-140) or open_len under
 *     OFFSIM_EPLEN_STEPS (the number of its transitions); both counters go back to zero;
 *   an environment with a valid step and no ended episode contributes the one entry (open_ret, open_len) -- _log_epoch_metrics' store
 *     when EpRet is empty (ppo.py:226-227); open_len is here the transition count so far under either mode, and the counters go on;
 *   an environment without a valid step contributes nothing;
 *   VVals are value[t] of every valid step.
 * stats [OFFSIM_PPO_LOG_STATS] f64: EpRet mean, std, min, max | EpLen mean | VVals mean, std, min, max | the number of entries, with
 * mean = sum / n and std = sqrt(sum((x - mean)^2) / n) (mpi_statistics_scalar; two passes, f64); n = 0 gives NaN.  counts [2] i64:
 * EpisodesInEpoch (ended episodes only) and the valid steps.  Optional (NULL to skip), the ENDED episodes of every environment in order:
 * ep_ret [E, ep_cap] f64, ep_len [E, ep_cap] i32 (the first ep_cap of them), n_ep [E] i32 (their number, which may pass ep_cap); the
 * open entry of an environment with n_ep = 0 and a valid step is its open_ret / open_len after the call.
 * One launch; no atomics, every sum in a fixed order (a lane's environments in order, each in step order, then an LDS tree): the same
 * bits every run.  T >= 1, E >= 1, ep_cap >= 0, a known mode, non-NULL records, state, stats and counts (otherwise OFFSIM_EINVAL);
 * argument validation happens before any HIP call.  Asynchronous on `stream`, capturable. */
#define OFFSIM_EPLEN_REFERENCE 0
#define OFFSIM_EPLEN_STEPS 1
#define OFFSIM_PPO_LOG_STATS 10
int offsim_ppo_epoch_log(const float *rew, const float *value, const uint8_t *valid, const uint8_t *terminated, const uint8_t *truncated,
                         int64_t T, int64_t E, int32_t eplen_mode, double *open_ret, int32_t *open_len, double *stats, int64_t *counts,
                         double *ep_ret, int32_t *ep_len, int32_t *n_ep, int64_t ep_cap, void *stream);

/* offsim_ppo_epoch_log_pop: offsim_ppo_epoch_log over the [T, L * E] records of a population (learner-major columns: environment r belongs
 * to learner r / E), one workgroup per learner in the same single launch.  open_ret / open_len / n_ep [L * E], ep_ret / ep_len
 * [L * E, ep_cap], stats [L, OFFSIM_PPO_LOG_STATS], counts [L, 2].  Learner l's outputs are, bit for bit, those of offsim_ppo_epoch_log on
 * its own E columns; a learner without a valid step gets NaN statistics and zero counts.  L in 1..65535. */
int offsim_ppo_epoch_log_pop(const float *rew, const float *value, const uint8_t *valid, const uint8_t *terminated, const uint8_t *truncated,
                             int64_t T, int32_t L, int64_t E, int32_t eplen_mode, double *open_ret, int32_t *open_len, double *stats,
                             int64_t *counts, double *ep_ret, int32_t *ep_len, int32_t *n_ep, int64_t ep_cap, void *stream);

/* ---- the PPO update (PPOLearner.update, ppo_grad) --------------------------------------------------------------------------------
 * PPOAgentRevealed.adapt (offsim4rl/agents/ppo.py:162-223) over M records -- a PPO buffer as offsim_vector_collect_ppo and
 * offsim_ppo_advantages leave it, [T*E] step-major, or any flat batch -- for one network at a time (kind):
 *   OFFSIM_PPO_ACTOR   logp = log_softmax(logits(obs))[act], ratio = exp(logp - logp_old),
 *                      loss = -mean(min(ratio * adv, clamp(ratio, 1 - c, 1 + c) * adv)),  kl = mean(logp_old - logp),
 *                      entropy = mean(-sum_a p_a log p_a),  clipfrac = mean(ratio > 1 + c or ratio < 1 - c)     (_compute_loss_pi);
 *   OFFSIM_PPO_CRITIC  loss = mean((v(obs) - ret)^2)  (_compute_loss_v); kl, entropy and clipfrac are 0.
 * The means run over the records with valid != 0 (valid NULL: all M) of all environments together, and the gradient is that of this
 * loss.  spinup averages per-process means and gradients over its E MPI processes instead: the same numbers whenever every environment
 * holds T valid records.  A record whose act lies outside [0, nA) counts as invalid (for the actor).  Records with valid = 0 are never compacted
 * away: they contribute nothing, and their obs / adv / logp / ret may hold anything finite or not.
 * The network is offsim_policy_mlp's / offsim_value_mlp's (1-4 layers, dO <= 128, hidden <= 256, nA <= 16 or one output for the critic,
 * the same activations; a leaky_relu slope below 0 is refused), its W and b together at most OFFSIM_COLLECT_MLP_MAX_FLOATS floats
 * (they are staged into LDS as offsim_vector_collect stages them), otherwise OFFSIM_EUNSUPPORTED.  f32 arithmetic per record (fmaf
 * chains in k order; not the bits of offsim_policy_mlp, as the reference's batched forward is not those of its per-step forward);
 * per-workgroup partial gradients in f32, summed over a fixed assignment of records to at most OFFSIM_PPO_MAX_BLOCKS workgroups and
 * then in block order in f64: no float atomics, two calls on the same input give the same bits.
 *
 * offsim_ppo_grad: one pass.  grad [P] f32: the gradient of the loss, flat in layer order, W [out,in] then b [out] of each layer (a
 * layer without b has none), P the number of parameters; stats [5] f64: n (valid records), loss, kl, entropy, clipfrac.  Two launches.
 *
 * offsim_ppo_update: the loop for one network, 2 * iters + 1 launches enqueued at once, no host round trip:
 *   for i in 0 .. iters-1:  pass i (loss, kl, ... and the gradient at the current weights);
 *                           actor only: if kl > 1.5 * target_kl: stop -- StopIter = i, nothing is changed by this or any later launch;
 *                           torch.optim.Adam's default step, in place on the layers' W / b:  t += 1,
 *                             m = b1 m + (1 - b1) g,  v = b2 v + (1 - b2) g^2,  p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 *                             with b1 = 0.9, b2 = 0.999, eps = 1e-8 and no weight decay; each line is evaluated in f64 from the f32 state and g, and m and v
 *                             are rounded to f32 before the last line reads them, as torch's f32 step reads its stored state.
 *   opt: m, v [P] f32 (flat as grad) and t [1] i64 on the device, all zero before the first call and carried from call to call.
 *   stats [6] f64: loss of pass 0, loss of the last pass computed, kl of the last pass, entropy of pass 0, clipfrac of the last pass,
 *   StopIter (the pass that stopped, else iters - 1) -- what adapt() logs as LossPi / LossV, DeltaLoss* (last - first), KL, Entropy,
 *   ClipFrac, StopIter.  trace [iters,2] f64: (loss, kl) of every pass computed, NaN for the passes after a stop.
 *   A batch without a valid record changes nothing (StopIter = 0, zeros).
 * The early stop is a flag in `work` that every launch reads first; no kernel waits for another.
 * work: OFFSIM_PPO_UPDATE_WORK_DOUBLES(P) doubles of device scratch (offsim_ppo_update_work_doubles computes P from the layers; a
 * negative return is an error code).  Argument validation happens before any HIP call; M = 0 or iters = 0 launches nothing. */
#define OFFSIM_PPO_ACTOR 0
#define OFFSIM_PPO_CRITIC 1
#define OFFSIM_PPO_MAX_BLOCKS 256
#define OFFSIM_PPO_UPDATE_WORK_DOUBLES(P) (OFFSIM_PPO_MAX_BLOCKS * 8 + 8 + OFFSIM_PPO_MAX_BLOCKS * (((P) + 1) / 2))
typedef struct offsim_ppo_layer {      /* offsim_mlp_layer's layout with writable weights: offsim_ppo_update steps W and b in place */
    float *W;                          /* [out, in] */
    float *b;                          /* [out] or NULL */
    int32_t in;
    int32_t out;
} offsim_ppo_layer;
typedef struct offsim_ppo_net {
    int32_t n_layers;                  /* layers_host[n_layers]: a HOST array, device pointers, as offsim_policy_mlp's */
    int32_t activation;
    const offsim_ppo_layer *layers_host;
    float slope;
    int32_t reserved;
} offsim_ppo_net;
typedef struct offsim_ppo_batch {
    const void *obs;                   /* [M,dO] f32 or f16 (x_dtype)                               */
    int32_t x_dtype;
    int32_t dO;
    const int32_t *act;                /* [M]   actor                                               */
    const float *adv;                  /* [M]   actor                                               */
    const float *logp;                 /* [M]   actor: logp_old                                     */
    const float *ret;                  /* [M]   critic                                              */
    const uint8_t *valid;              /* [M], or NULL: every record is valid                       */
    int64_t M;
} offsim_ppo_batch;
typedef struct offsim_ppo_adam {
    float *m;                          /* [P] in/out                                                */
    float *v;                          /* [P] in/out                                                */
    int64_t *t;                        /* [1] in/out: Adam's step count                             */
    double lr;
} offsim_ppo_adam;
int64_t offsim_ppo_update_work_doubles(const offsim_ppo_net *net);
int offsim_ppo_grad(const offsim_ppo_net *net, int32_t kind, const offsim_ppo_batch *batch, double clip_ratio, float *grad, double *stats,
                    double *work, void *stream);
int offsim_ppo_update(const offsim_ppo_net *net, int32_t kind, const offsim_ppo_batch *batch, double clip_ratio, double target_kl,
                      int32_t iters, const offsim_ppo_adam *opt, double *stats, double *trace, double *work, void *stream);

/* offsim_ppo_grad_pop / offsim_ppo_update_pop: offsim_ppo_grad / offsim_ppo_update for a population of L independent learners, in the
 * same number of launches as for one (the learner is the grid's y dimension).  batch: the step-major [T, L * E] buffer as it is, M =
 * T * L * E records (a multiple of L * E); learner l sees its records in the flat order m' = t * E + e, read at memory index
 * t * L * E + l * E + e -- its buffer is never copied out.  net: the stacked networks, W [L, out, in] and b [L, out] per layer,
 * layers_host describing learner 0 (learner l's tensors at W + l * out * in, b + l * out).  Per learner, the tile size, the assignment
 * of tiles to min(tiles, OFFSIM_PPO_MAX_BLOCKS) workgroups and the f64 block-order reduction are those of offsim_ppo_grad /
 * offsim_ppo_update on a contiguous [T * E] batch, so every learner's results equal the single call's bit for bit.
 *   offsim_ppo_grad_pop    grad [L, P] f32, stats [L, 5] f64; clip_ratio: a HOST array [L].
 *   offsim_ppo_update_pop  clip_ratio, target_kl and opt->lr: HOST arrays [L] (they ride to the device as kernel arguments: no copy the
 *                          host waits for); iters is shared.  opt->m, v [L, P] f32 and t [L] i64 on the device; stats [L, 6], trace
 *                          [L, iters, 2] f64.  Every learner has its own stop flag: one whose KL stop fires goes quiet while the others
 *                          keep stepping, and t[l] moves by learner l's own steps.  A learner without a valid record changes nothing of
 *                          its own (weights, m, v, t; StopIter = 0, zeros) and does not disturb the others.
 * No float atomics, no cooperative launch; no kernel waits for another workgroup.
 * work: offsim_ppo_update_work_doubles_pop(net, L, M) doubles of device scratch, M = T * E the records of ONE learner: per learner
 * OFFSIM_PPO_UPDATE_WORK_DOUBLES_NB(P, nb) for the nb = min(tiles, OFFSIM_PPO_MAX_BLOCKS) workgroups the learner really has (a caller
 * that does not know M passes INT64_MAX and gets the size for OFFSIM_PPO_MAX_BLOCKS); a negative return is an error code.  L in
 * 1..65535, E >= 1.  Argument validation happens before any HIP call (every learner's clip_ratio in [0, 1), target_kl >= 0, lr >= 0);
 * M = 0 or iters = 0 launches nothing. */
#define OFFSIM_PPO_UPDATE_WORK_DOUBLES_NB(P, NB) ((NB) * 8 + 8 + (NB) * (((P) + 1) / 2))
typedef struct offsim_ppo_adam_pop {
    float *m;                          /* [L,P] in/out                                              */
    float *v;                          /* [L,P] in/out                                              */
    int64_t *t;                        /* [L] in/out: every learner's Adam step count               */
    const double *lr;                  /* [L] HOST array                                            */
} offsim_ppo_adam_pop;
int64_t offsim_ppo_update_work_doubles_pop(const offsim_ppo_net *net, int32_t L, int64_t M);
int offsim_ppo_grad_pop(const offsim_ppo_net *net, int32_t kind, const offsim_ppo_batch *batch, int32_t L, int32_t E, const double *clip_ratio,
                        float *grad, double *stats, double *work, void *stream);
int offsim_ppo_update_pop(const offsim_ppo_net *net, int32_t kind, const offsim_ppo_batch *batch, int32_t L, int32_t E,
                          const double *clip_ratio, const double *target_kl, int32_t iters, const offsim_ppo_adam_pop *opt, double *stats,
                          double *trace, double *work, void *stream);

/* ---- HOMER encoder training (HOMEREncoder.train, loss_grad) ------------------------------------------------------------------------
 * The model of offsim4rl/encoders/models.py: obs_encoder = Linear(dO,H) -> LeakyReLU -> Linear(H,nZ), classifier =
 * Linear(2 nZ + nA, H) -> LeakyReLU -> Linear(H,2), the action embedding a frozen identity (a one-hot of the action).  One record m of a
 * batch is (i = idx_real[m], j = idx_impo[m], noise g[m][0..3][nZ]); the loss is HOMEREncoder._calc_loss (homer.py:170-184):
 *   e_prev = enc(obs[i]);  e_real = enc(next_obs[i]);  e_impo = enc(next_obs[j])
 *   z0 = softmax((e_prev + g0) / tau)   z1 = softmax((e_real + g1) / tau)
 *   z2 = softmax((e_prev + g2) / tau)   z3 = softmax((e_impo + g3) / tau)
 *   lp_real = log_softmax(cls([z0, onehot(act[i]), z1]));  lp_impo = log_softmax(cls([z2, onehot(act[i]), z3]))
 *   loss = (mean_m(-lp_real[m][1]) + mean_m(-lp_impo[m][0])) / 2
 * The noise and the indices are inputs: nothing is drawn on the device.  hard != 0: every z is F.gumbel_softmax(hard=True)'s forward
 * value, (onehot(argmax) - y_soft) + y_soft; forward only.  A record whose i or j lies outside [0, n_rows) or whose act[i] lies outside
 * [0, nA) is invalid: it is excluded from n and contributes nothing, and its noise may hold anything.
 * f32 arithmetic per record (fmaf chains in k order); per-workgroup partial gradients in f32 over a fixed assignment of tiles to at
 * most OFFSIM_HOMER_MAX_BLOCKS workgroups, summed in block order in f64: no float atomics, two calls on the same input give the same
 * bits.  All weights and one tile of records must fit 160 KiB of LDS and P <= OFFSIM_HOMER_MAX_FLOATS, otherwise OFFSIM_EUNSUPPORTED.
 *
 * offsim_homer_grad: one pass.  grad [P] f32 or NULL (forward only): the gradient of the loss, unclipped, flat in the order encoder
 * L1 W [H,dO], b, L2 W [nZ,H], b, classifier L1 W [H, 2 nZ + nA], b, L2 W [2,H], b.  stats [2] f64: n (valid records), loss.
 * hard != 0 requires grad == NULL.  Two launches.
 *
 * offsim_homer_step: one pass, then torch.nn.utils.clip_grad_norm_ over all trainable parameters of both networks
 * (total = sqrt(sum g^2), coef = min(1, max_grad_norm / (total + 1e-6)), g *= coef) and torch.optim.Adam's step with L2 weight decay
 * (g += weight_decay * p before the moments; b1 = 0.9, b2 = 0.999, eps = 1e-8), in place on the net's tensors, with
 * offsim_ppo_update's arithmetic: each line in f64 from the f32 state and the f32 gradient, m and v rounded to f32 before the last line
 * reads them.  adam: m, v [P] f32 (flat as grad) and t [1] i64 on the device, zero before the first call.  stats [3] f64: n, loss,
 * total_norm.  A batch without a valid record changes nothing (t included).  Three launches.
 *
 * work: OFFSIM_HOMER_WORK_DOUBLES(P) doubles of device scratch (offsim_homer_work_doubles computes P from the net; a negative return is
 * an error code).  Argument validation happens before any HIP call (tau <= 0, nZ < 2, a negative slope, NULL pointers, widths outside
 * dO <= 128, H <= 256, nZ <= 256, nA <= 16: OFFSIM_EINVAL); M = 0 launches nothing.  Asynchronous on `stream`, capturable. */
#define OFFSIM_HOMER_MAX_BLOCKS 128
#define OFFSIM_HOMER_MAX_FLOATS 20480
#define OFFSIM_HOMER_WORK_DOUBLES(P) \
    (OFFSIM_HOMER_MAX_BLOCKS * 2 + 8 + ((P) + 255) / 256 + ((P) + 1) / 2 + OFFSIM_HOMER_MAX_BLOCKS * (((P) + 1) / 2))
typedef struct offsim_homer_net {      /* state_dict layout, writable device pointers: offsim_homer_step steps them in place */
    float *enc_W1;                     /* obs_encoder.0.weight [H, dO]                              */
    float *enc_b1;                     /* obs_encoder.0.bias   [H]                                  */
    float *enc_W2;                     /* obs_encoder.2.weight [nZ, H]                              */
    float *enc_b2;                     /* obs_encoder.2.bias   [nZ]                                 */
    float *cls_W1;                     /* classifier.0.weight  [H, 2 nZ + nA]                       */
    float *cls_b1;                     /* classifier.0.bias    [H]                                  */
    float *cls_W2;                     /* classifier.2.weight  [2, H]                               */
    float *cls_b2;                     /* classifier.2.bias    [2]                                  */
    int32_t dO;
    int32_t nA;
    int32_t nZ;
    int32_t H;
    float slope;                       /* LeakyReLU's negative slope (torch's default: 0.01)        */
    int32_t reserved;
} offsim_homer_net;
typedef struct offsim_homer_batch {
    const void *obs;                   /* [n_rows, dO] f32 or f16 (x_dtype)                         */
    const void *next_obs;              /* [n_rows, dO]                                              */
    int32_t x_dtype;
    int32_t reserved;
    const int32_t *act;                /* [n_rows]                                                  */
    int64_t n_rows;
    const int32_t *idx_real;           /* [M]                                                       */
    const int32_t *idx_impo;           /* [M]                                                       */
    const float *noise;                /* [M, 4, nZ], or NULL: zeros                                */
    int64_t M;
} offsim_homer_batch;
typedef struct offsim_homer_adam {
    float *m;                          /* [P] in/out                                                */
    float *v;                          /* [P] in/out                                                */
    int64_t *t;                        /* [1] in/out: Adam's step count                             */
    double lr;
    double weight_decay;
} offsim_homer_adam;
int64_t offsim_homer_work_doubles(const offsim_homer_net *net);
int offsim_homer_grad(const offsim_homer_net *net, const offsim_homer_batch *batch, double tau, int32_t hard, float *grad, double *stats,
                      double *work, void *stream);
int offsim_homer_step(const offsim_homer_net *net, const offsim_homer_batch *batch, double tau, double max_grad_norm,
                      const offsim_homer_adam *adam, double *stats, double *work, void *stream);

/* offsim_homer_grad_pop / offsim_homer_step_pop: offsim_homer_grad / offsim_homer_step for a population of L independent encoders of one
 * architecture, in the same number of launches as for one (the learner is the grid's y dimension).  net: the stacked networks, every
 * tensor with a leading learner axis (enc_W1 [L, H, dO], enc_b1 [L, H], ..., cls_b2 [L, 2]); the struct describes learner 0 and learner
 * l's tensor is at base + l * numel.  batch: obs / next_obs / act / n_rows are shared by all learners; every learner has its own M
 * records, idx_real / idx_impo [L, M] i32 and noise [L, M, 4, nZ] f32 (or NULL: zeros) with an explicit learner stride in records,
 * idx_stride >= M: learner l's record m is at idx[l * idx_stride + m] and its noise at (l * idx_stride + m) * 4 * nZ, so a batch is a
 * column slice [:, lo:hi] of an epoch's arrays with no copy.  tau and hard are shared.  active: [L] u8 on the device, or NULL for all
 * active; every launch of learner l reads active[l] first and returns when it is 0, and nothing of that learner is written (weights,
 * m, v, t, its rows of grad and stats).  Per learner, the tile size, the assignment of tiles to min(tiles, OFFSIM_HOMER_MAX_BLOCKS)
 * workgroups, the f32 partials, the f64 block-order reduction, the norm tree and the Adam arithmetic are those of the single call on the
 * same M, so every learner's results equal the single call's bit for bit.  The LDS budget and OFFSIM_HOMER_MAX_FLOATS are per learner.
 *   offsim_homer_grad_pop  grad [L, P] f32 or NULL (forward only; hard != 0 requires NULL), stats [L, 2] f64.  Two launches.
 *   offsim_homer_step_pop  adam: m, v [L, P] f32, t [L] i64, and lr, weight_decay, max_grad_norm [L] f64, all on the DEVICE (the caller
 *                          keeps them >= 0); stats [L, 3] f64.  A learner whose batch has no valid record changes nothing of its own
 *                          (t[l] included) and does not disturb the others.  Three launches.
 * No float atomics, no cooperative launch; no kernel waits for another workgroup.
 * work: offsim_homer_work_doubles_pop(net, L, M) doubles of device scratch, M the records of ONE learner: per learner
 * OFFSIM_HOMER_WORK_DOUBLES_NB(P, nb) for the nb = min(tiles, OFFSIM_HOMER_MAX_BLOCKS) workgroups the learner really has at that M (a
 * caller that does not know M passes INT64_MAX and gets the size for OFFSIM_HOMER_MAX_BLOCKS, which serves every M); a negative return
 * is an error code.  L in 1..65535.  Argument validation happens before any HIP call (L, idx_stride < M, hard with a grad pointer, and
 * all that offsim_homer_grad refuses: OFFSIM_EINVAL; the budgets: OFFSIM_EUNSUPPORTED); M = 0 launches nothing.  Asynchronous on
 * `stream`, capturable. */
#define OFFSIM_HOMER_WORK_DOUBLES_NB(P, NB) ((NB) * 2 + 8 + ((P) + 255) / 256 + ((P) + 1) / 2 + (NB) * (((P) + 1) / 2))
typedef struct offsim_homer_batch_pop {
    const void *obs;                   /* [n_rows, dO] f32 or f16 (x_dtype), shared                 */
    const void *next_obs;              /* [n_rows, dO], shared                                      */
    int32_t x_dtype;
    int32_t reserved;
    const int32_t *act;                /* [n_rows], shared                                          */
    int64_t n_rows;
    const int32_t *idx_real;           /* [L, M], rows idx_stride apart                             */
    const int32_t *idx_impo;           /* [L, M], rows idx_stride apart                             */
    const float *noise;                /* [L, M, 4, nZ], learners idx_stride records apart, or NULL */
    int64_t M;                         /* records per learner                                       */
    int64_t idx_stride;                /* >= M, in records                                          */
} offsim_homer_batch_pop;
typedef struct offsim_homer_adam_pop {
    float *m;                          /* [L,P] in/out                                              */
    float *v;                          /* [L,P] in/out                                              */
    int64_t *t;                        /* [L] in/out: every learner's Adam step count               */
    const double *lr;                  /* [L] device array                                          */
    const double *weight_decay;        /* [L] device array                                          */
    const double *max_grad_norm;       /* [L] device array                                          */
} offsim_homer_adam_pop;
int64_t offsim_homer_work_doubles_pop(const offsim_homer_net *net, int32_t L, int64_t M);
int offsim_homer_grad_pop(const offsim_homer_net *net, const offsim_homer_batch_pop *batch, int32_t L, double tau, int32_t hard,
                          const uint8_t *active, float *grad, double *stats, double *work, void *stream);
int offsim_homer_step_pop(const offsim_homer_net *net, const offsim_homer_batch_pop *batch, int32_t L, double tau,
                          const offsim_homer_adam_pop *adam, const uint8_t *active, double *stats, double *work, void *stream);

/* offsim_replay_td: a logged memory replayed through L tabular TD learners in ONE launch -- qlearn(..., memory=...) of the reference
 * (offsim4rl/agents/tabular.py:90-104: the Q-learning update swept over logged (S, A, R, S', done) tuples in log order, no simulator), for a
 * population of step sizes and discounts, on S streams of the same log.
 *   log: device columns s, a [N] i32, r [N] f64, s_next [N] i32, done [N] u8; states in [0, nS), actions in [0, nA).
 *   rp->order [S, M] i32 or NULL.  NULL: S must be 1 and the stream is the log in log order (M is ignored, the stream has N steps).
 *     Otherwise stream j visits log rows order[j, 0 .. M - 1]; repeats are allowed and M is independent of N (shuffled replay, bootstrap
 *     resamples of the log for paired error bars).  passes >= 1: the stream is swept that many times; the episode counter carries on.
 *   Per learner, device arrays: alpha, gamma [L] f64; alpha_ep [L, n_sched] f64 or NULL with offsim_td's rule (entry min(e, n_sched - 1)
 *     serves episode e; alpha is then not read).  mode: OFFSIM_TD_QLEARN or OFFSIM_TD_EXPSARSA (one per launch).  pi [L, nS, nA] f64 with
 *     pi_stride = nS * nA, or one table shared by all learners with pi_stride = 0 (offsim_td_pop's rule); read by OFFSIM_TD_EXPSARSA only.
 *   Rollout l * S + j is learner l on stream j.
 * Per step k of a stream, with (s, a, r, s', d) its transition and e the number of done flags the stream has seen so far:
 *     target = max_b Q[s', b]                                   OFFSIM_TD_QLEARN   (tabular.py:95-96)
 *            | sum_b Q[s', b] * pi[s', b], b = 0 .. nA - 1      OFFSIM_TD_EXPSARSA (left to right from 0.0: the sum offsim_eval_td defines)
 *     td     = (r + gamma * target) - Q[s, a]
 *     Q[s,a] = Q[s, a] + alpha(e) * td
 *     if d: e += 1
 *   in f64, in exactly this order, without contraction.  done is not treated specially in the update (the reference does not either).  The
 *   row maximum is offsim_eval_td's: m = Q[s', 0], then m = Q[s', b] > m ? Q[s', b] : m for b = 1 .. nA - 1 -- a NaN in entry 0 stays, a NaN
 *   in a later entry is passed over (np.max would return it).
 * Outputs: q [L * S, nS, nA] f64, read as Q_init and written back.  td_err [S, td_cap, L] f64 (optional): the TD errors of the first td_cap
 *   steps, learner-MINOR (a wavefront stores one step of 64 learners as one contiguous vector).  q_snap [L * S, snap_cap, nS, nA] /
 *   snap_stride / snap_cap: offsim_td's rule, Q after steps 0, stride, 2 stride, ....  n_ep [S] i64: the done flags stream j saw;
 *   steps [L * S] i64; status [L * S] i32.  A step whose s, a or s' is out of range, or whose order entry is outside [0, N), stops that
 *   stream's rollouts BEFORE the step: status OFFSIM_ST_KEYERROR, steps = k, Q as step k - 1 left it (the reference raises IndexError);
 *   other streams are unaffected.  Otherwise OFFSIM_ST_OK and steps = passes * M.
 * Launch: one wavefront per workgroup, grid = S x ceil(L / LPW), the lane is the learner within its group, its Q in LDS as
 *   [nS * nA][LPW] f64.  LPW = offsim_replay_lpw(nS, nA, L): the largest of 64, 32, .., 1 that is no larger than L rounded up to a power of two
 *   and whose Q image nS * nA * LPW * 8 bytes fits 160 KiB (offsim_eval_td's dynamic-LDS budget; the stream tile is staged in registers, so
 *   nothing comes off it); 0 when one learner's table does not fit, and offsim_replay_td then returns OFFSIM_EUNSUPPORTED, the refusal of
 *   offsim_eval_td past 160 KiB.
 * OFFSIM_EINVAL, before any HIP call: NULL log columns, N < 1, L outside 1..65535, S < 1, S != 1 without an order, an order with M < 1,
 *   passes < 1, a bad mode, NULL q / alpha / gamma / n_ep / steps / status, OFFSIM_TD_EXPSARSA without pi, alpha_ep without n_sched, a bad
 *   snapshot stride (L and S are at least 1 in an accepted call, so there is no empty launch).  N or M above 2^31 - 1: OFFSIM_EUNSUPPORTED.
 *   Asynchronous on `stream`. */
typedef struct offsim_replay_log {
    int64_t N;
    int32_t nS;
    int32_t nA;
    const int32_t *s;
    const int32_t *a;
    const double *r;
    const int32_t *s_next;
    const uint8_t *done;
} offsim_replay_log;
typedef struct offsim_replay {
    int32_t mode;
    const int32_t *order;
    int64_t M;
    int64_t passes;
    const double *alpha;
    const double *gamma;
    const double *alpha_ep;
    int64_t n_sched;
    const double *pi;
    int64_t pi_stride;
    double *q;
    double *td_err;
    int64_t td_cap;
    double *q_snap;
    int64_t snap_cap;
    int64_t snap_stride;
    int64_t *n_ep;
    int64_t *steps;
    int32_t *status;
} offsim_replay;
int32_t offsim_replay_lpw(int32_t nS, int32_t nA, int32_t L);
int offsim_replay_td(const offsim_replay_log *log, int32_t L, int32_t S, const offsim_replay *rp, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* OFFSIM_H */
