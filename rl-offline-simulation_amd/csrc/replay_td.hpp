// replay_td.hpp -- a logged memory replayed through many tabular TD learners in one launch (offsim_replay_td): the `memory=` path of the
// reference's qlearn (offsim4rl/agents/tabular.py:90-104), with orders (shuffled replay, bootstrap resamples) and expected SARSA added.
//
// No simulator runs here: the transition stream is the same for every learner, so the learner is the LANE.  One wavefront per workgroup,
// grid = S streams x ceil(L / LPW) lane groups; lane i of group g is learner g * LPW + i and keeps its own Q in LDS as [nS * nA][LPW] f64
// (entry e of lane i at (e * LPW + i) * 8: at LPW = 64 a ds_read_b64 of one entry by the wave covers 512 contiguous bytes, conflict-free within
// each 32-lane half).  Each lane loads one transition of a tile of 64 stream steps (coalesced; through `order` when given), the step loop makes
// step k's fields wave-uniform with v_readlane, and every lane runs the same update on its own Q with its own alpha / gamma.  The loads of
// tile t + 1 (and the order entries of tile t + 2) are issued before the loop over tile t.  A step is one LDS round trip -- read Q[s', .] and
// Q[s, a], a handful of f64 operations, write Q[s, a], which the next step's reads queue behind in order -- inside one wavefront's serial
// chain of scalar tests and branches; DESIGN section 26 has the measured cost of a step and what is in it.
//
// Stream step g of a launch is position g % M of sweep g / M, so a tile simply runs across the end of a sweep: only the last tile of the
// launch is partial, and the episode counter carries on.  Expected SARSA reads pi[s', .] from global memory (one table or one per learner).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// the dynamic-LDS budget of a workgroup, offsim_eval_td's 160 KiB; the tile is staged in registers, so nothing comes off it
#define REPLAY_LDS_BUDGET (160 * 1024)
#define REPLAY_TILE 64

struct ReplayArgs {
    offsim_replay_log log;
    offsim_replay rp;
    int32_t L, S, lpw;
    uint32_t M;  // stream length (log.N without an order)
    int64_t T;   // steps of the launch: passes * M
};

// what a lane holds of its transition of a tile, as loaded
struct ReplayRow {
    int32_t row;  // the order entry; the columns below are those of that row clamped into the log, so every lane loads, without a branch
    int32_t s, a, sn;
    uint32_t done;
    double r;
};
enum { REPLAY_DONE = 1, REPLAY_BAD = 2 };

static __device__ __forceinline__ double replay_lane_f64(double v, int k) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), k), __builtin_amdgcn_readlane(__double2loint(v), k));
}

template <bool EXPS, bool ORD>
__global__ void __launch_bounds__(64) k_replay_td(ReplayArgs a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int lane = threadIdx.x, lpw = a.lpw;
    const int j = blockIdx.x;  // stream
    const int l = blockIdx.y * lpw + lane;
    const bool on = lane < lpw && l < a.L;
    const int nA = a.log.nA, nSA = a.log.nS * nA;
    const int64_t r = (int64_t)l * a.S + j;  // rollout: learner l on stream j
    const uint32_t M = a.M;
    const int64_t T = a.T;
    double *q_me = (double *)lds_raw + lane;  // entry e: q_me[e * lpw]
    double alpha = 0.0, gamma = 0.0;
    const double *alpha_ep = nullptr, *pi_me = nullptr;
    if (on) {
        for (int e = 0; e < nSA; e++) q_me[(size_t)e * lpw] = a.rp.q[r * nSA + e];
        gamma = a.rp.gamma[l];
        if (a.rp.alpha_ep) alpha_ep = a.rp.alpha_ep + (int64_t)l * a.rp.n_sched;
        alpha = alpha_ep ? alpha_ep[0] : a.rp.alpha[l];
        if (EXPS) pi_me = a.rp.pi + (int64_t)l * a.rp.pi_stride;
    }

    // all that was loaded so far has landed: the waits of the step loop then count the loads of the tiles in flight only
    __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0)

    const int32_t *ord = ORD ? a.rp.order + (int64_t)j * M : nullptr;
    const uint32_t hop = REPLAY_TILE % M;  // a lane's position moves by one tile, modulo M
    uint32_t pos = (uint32_t)lane % M;     // this lane's position in its sweep, of the tile whose order entry is fetched next
    // the order entry of this lane's step of the next tile (a lane past the end of the launch reads an entry it does not use; nothing looks at
    // the value before `load` does), then on to the tile after it
    auto entry = [&]() -> int32_t {
        const int32_t row = ORD ? ord[pos] : (int32_t)pos;
        pos += hop;
        pos = pos >= M ? pos - M : pos;
        return row;
    };
    auto load = [&](int32_t row) {
        const int32_t at = row < 0 ? 0 : row >= a.log.N ? (int32_t)(a.log.N - 1) : row;
        return ReplayRow{row, a.log.s[at], a.log.a[at], a.log.s_next[at], a.log.done[at], a.log.r[at]};
    };

    int64_t ep = 0, stop_at = T, snap_at = 0, snap_i = 0;
    int status = OFFSIM_ST_OK;
    // the steps of the tile that starts at g0, `cur` this lane's transition of it
    auto tile = [&](int64_t g0, const ReplayRow &cur) {
        // this lane's step, packed: the Q entries it touches and its flags
        const bool bad = cur.row < 0 || cur.row >= a.log.N || cur.s < 0 || cur.s >= a.log.nS || cur.a < 0 || cur.a >= nA || cur.sn < 0 || cur.sn >= a.log.nS;
        const int my_sa = bad ? 0 : cur.s * nA + cur.a, my_sn = bad ? 0 : cur.sn * nA;
        const int my_fl = (cur.done ? REPLAY_DONE : 0) | (bad ? REPLAY_BAD : 0);
        const int n = T - g0 < REPLAY_TILE ? (int)(T - g0) : REPLAY_TILE;
        for (int k = 0; k < n; k++) {
            const int fl = __builtin_amdgcn_readlane(my_fl, k);
            const int64_t step = g0 + k;
            if (fl & REPLAY_BAD) {  // the reference raises IndexError at Q[S_] / Q[S, A]: the stream stops before the step
                status = OFFSIM_ST_KEYERROR;
                stop_at = step;
                break;
            }
            const int e_sa = __builtin_amdgcn_readlane(my_sa, k), e_sn = __builtin_amdgcn_readlane(my_sn, k);
            const double rew = replay_lane_f64(cur.r, k);
            if (on) {
                const double *qn = q_me + (size_t)e_sn * lpw;
                const double *pn = EXPS ? pi_me + e_sn : nullptr;
                const double q_sa = q_me[(size_t)e_sa * lpw];
                // QLEARN: tabular.py:95-96, the row maximum of offsim_eval_td (a NaN is kept only in the first entry); EXPSARSA: Q[S_] @ pi[S_],
                // left to right.  Four entries are read before any is used (one LDS round trip, not nA); an index past the row reads its last
                // entry again, which the maximum does not notice and the sum skips.
                double nxt = EXPS ? 0.0 : qn[0];
                for (int b0 = EXPS ? 0 : 1; b0 < nA; b0 += 4) {
                    double v[4], p[4];
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const int b = b0 + i < nA ? b0 + i : nA - 1;
                        v[i] = qn[(size_t)b * lpw];
                        p[i] = EXPS ? pn[b] : 0.0;
                    }
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        if (!EXPS) nxt = v[i] > nxt ? v[i] : nxt;
                        else if (b0 + i < nA) nxt = nxt + v[i] * p[i];
                    }
                }
                const double td_err = rew + gamma * nxt - q_sa;
                if (a.rp.td_err && step < a.rp.td_cap) a.rp.td_err[((int64_t)j * a.rp.td_cap + step) * a.L + l] = td_err;  // learner-minor
                q_me[(size_t)e_sa * lpw] = q_sa + alpha * td_err;
                if (a.rp.q_snap && step == snap_at && snap_i < a.rp.snap_cap) {  // save_Q: Q after steps 0, stride, 2 stride, ...
                    double *dst = a.rp.q_snap + (r * a.rp.snap_cap + snap_i) * nSA;
                    for (int e = 0; e < nSA; e++) dst[e] = q_me[(size_t)e * lpw];
                }
            }
            if (a.rp.q_snap && step == snap_at) {
                snap_at += a.rp.snap_stride;
                snap_i++;
            }
            if (fl & REPLAY_DONE) {  // tabular.py:98-99; alpha(episode) of the steps that follow
                ep++;
                if (a.rp.alpha_ep) {  // (waited for here, once per episode, and not by every step's update)
                    if (alpha_ep) alpha = alpha_ep[ep < a.rp.n_sched ? ep : a.rp.n_sched - 1];
                    __builtin_amdgcn_s_waitcnt(0x0f70);
                }
            }
        }
    };
    // Two tiles per turn, so that the transitions of the tile in flight land in registers of their own (handing them over in a copy would wait
    // for them): while tile t runs, the transitions of tile t + 1 and the order entries of tile t + 2 are in flight.
    ReplayRow w0 = load(entry()), w1;
    int32_t row_nn = entry();
    for (int64_t g0 = 0; g0 < T; g0 += 2 * REPLAY_TILE) {
        w1 = load(row_nn);
        row_nn = entry();
        tile(g0, w0);
        if (status != OFFSIM_ST_OK || g0 + REPLAY_TILE >= T) break;
        w0 = load(row_nn);
        row_nn = entry();
        tile(g0 + REPLAY_TILE, w1);
        if (status != OFFSIM_ST_OK) break;
    }
    if (on) {
        for (int e = 0; e < nSA; e++) a.rp.q[r * nSA + e] = q_me[(size_t)e * lpw];
        a.rp.steps[r] = stop_at;
        a.rp.status[r] = status;
    }
    if (blockIdx.y == 0 && lane == 0) a.rp.n_ep[j] = ep;
}

// learners per wavefront: the largest of 64, 32, .., 1 that is no larger than L rounded up to a power of two and whose Q image fits the budget; 0: none
static int32_t replay_lpw(int64_t nSA, int32_t L) {
    int32_t lpw = 64;
    while (lpw > 1 && (lpw >> 1) >= L) lpw >>= 1;
    while (lpw >= 1 && nSA * lpw * 8 > REPLAY_LDS_BUDGET) lpw >>= 1;
    return lpw;
}

extern "C" int32_t offsim_replay_lpw(int32_t nS, int32_t nA, int32_t L) {
    if (nS < 1 || nA < 1 || L < 1 || L > 65535) return fail(OFFSIM_EINVAL, "replay_lpw: nS, nA >= 1 and L in 1..65535%s");
    return replay_lpw((int64_t)nS * nA, L);
}

extern "C" int offsim_replay_td(const offsim_replay_log *log, int32_t L, int32_t S, const offsim_replay *rp, void *stream) {
    static const char *who = "replay_td";
    if (!log || !rp) return fail(OFFSIM_EINVAL, "%s: bad argument", who);
    if (!log->s || !log->a || !log->r || !log->s_next || !log->done) return fail(OFFSIM_EINVAL, "%s: NULL log column", who);
    if (log->N < 1 || log->nS < 1 || log->nA < 1) return fail(OFFSIM_EINVAL, "%s: bad N / nS / nA", who);
    if (L < 1 || L > 65535 || S < 1) return fail(OFFSIM_EINVAL, "%s: L must be 1..65535 and S >= 1", who);
    if (!rp->order && S != 1) return fail(OFFSIM_EINVAL, "%s: S streams need an order (without one the stream is the log: S = 1)", who);
    if (rp->order && rp->M < 1) return fail(OFFSIM_EINVAL, "%s: an order needs M >= 1", who);
    if (rp->passes < 1) return fail(OFFSIM_EINVAL, "%s: passes must be >= 1", who);
    if ((rp->mode != OFFSIM_TD_QLEARN && rp->mode != OFFSIM_TD_EXPSARSA) || !rp->q) return fail(OFFSIM_EINVAL, "%s: bad td mode or NULL q", who);
    if (!rp->alpha || !rp->gamma || rp->pi_stride < 0) return fail(OFFSIM_EINVAL, "%s: a per-learner array is NULL (alpha, gamma)", who);
    if (rp->mode == OFFSIM_TD_EXPSARSA && !rp->pi) return fail(OFFSIM_EINVAL, "%s: expected SARSA needs pi", who);
    if (rp->alpha_ep && rp->n_sched <= 0) return fail(OFFSIM_EINVAL, "%s: schedules need n_sched > 0", who);
    if (rp->td_err && rp->td_cap < 0) return fail(OFFSIM_EINVAL, "%s: negative td_cap", who);
    if (rp->q_snap && (rp->snap_stride <= 0 || rp->snap_cap < 0)) return fail(OFFSIM_EINVAL, "%s: bad snapshot stride / capacity", who);
    if (!rp->n_ep || !rp->steps || !rp->status) return fail(OFFSIM_EINVAL, "%s: required output is NULL", who);
    const int64_t M = rp->order ? rp->M : log->N;
    if (log->N > 0x7fffffffll || M > 0x7fffffffll || rp->passes > INT64_MAX / M)
        return fail(OFFSIM_EUNSUPPORTED, "%s: more than 2^31 - 1 log rows or stream steps per sweep, or more than 2^63 - 1 steps", who);
    const int64_t nSA = (int64_t)log->nS * log->nA;
    const int32_t lpw = replay_lpw(nSA, L);
    if (lpw < 1) return fail(OFFSIM_EUNSUPPORTED, "%s: one learner's Q table exceeds 160 KiB of LDS", who);
    const size_t lds = (size_t)nSA * lpw * 8;
    const ReplayArgs args{*log, *rp, L, S, lpw, (uint32_t)M, rp->passes * M};
    const dim3 grid((unsigned)S, (unsigned)((L + lpw - 1) / lpw));
    auto launch = [&](auto exps, auto has_order) -> int {
        auto *kernel = k_replay_td<decltype(exps)::value, decltype(has_order)::value>;
        if (lds > 64 * 1024) HIP_TRY(allow_big_lds(kernel, (int)lds));
        hipLaunchKernelGGL(kernel, grid, dim3(64), lds, (hipStream_t)stream, args);
        LAUNCH_CHECK();
        return OFFSIM_OK;
    };
    if (rp->mode == OFFSIM_TD_EXPSARSA) return rp->order ? launch(std::true_type{}, std::true_type{}) : launch(std::true_type{}, std::false_type{});
    return rp->order ? launch(std::false_type{}, std::true_type{}) : launch(std::false_type{}, std::false_type{});
}
