"""The learner-in-the-loop drivers qlearn_psrs / expSARSA_psrs in plain f64 Python, one learner at a time (test infrastructure).

A restatement of documented behaviour (offsim4rl/evaluators/psrs.py:119-239, offsim4rl/agents/tabular.py:4-32, include/offsim.h:
offsim_eval_td), not of the kernel's code:

  stepping   queue orders, the initial queue, the rejection draws and the accept rule are oracle.OraclePSRS's (reset_sampler, reset,
             step(p_new, PROB_F64, reject_mode), set_rejection_seed / set_rejection_philox); f16 / f32 logging probabilities and f32
             rewards are handed to it exactly widened to f64
  behaviour  FIXED: pi[z].  EPS_GREEDY: eps / nA everywhere and 1 - eps + eps / nA at the chosen maximum, chosen by
             RandomState.choice(np.where(q == q.max())[0]) on the learner's own np.random.RandomState (which draws only when several
             actions hold the maximum); without a tie stream the first maximal action.  SOFT_GREEDY: uniform over np.isclose(q, q.max()).
             epsilon / alpha: constants or per-episode tables, clamped at their last entry.  The behaviour distribution is formed BEFORE
             the step (psrs.py:158), so a step that then finds its queue empty or missing has already drawn from the tie stream
  update     Q-learning max(Q[z']); expected SARSA sum_k Q[z'][k] * pi[z'][k] from k = 0 upwards in a Python loop; then
             td = r + gamma * nxt - Q[z, a];  Q[z, a] = Q[z, a] + alpha * td;  G = G + gamma ** t * r -- all in Python floats
  episodes   as evalmc_rows of tests/obs_policy_host.py: lengths get every episode, Gs the completed ones with the cut-short one stored
             behind them, sum_g adds the completed returns in order; status ok / exhausted / no_init / keyerror

Everything comes back in the device's layout: Q and the snapshots in slot order (slot = z - min(z, z', 0), TransitionTable's dense
map), rows as caller-buffer rows, outputs cut by trace_cap / ep_cap / snap_cap as include/offsim.h says, buffers pre-filled as
BatchedPSRS.eval_td allocates them.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle as O  # noqa: E402

ST_OK, ST_EXHAUSTED, ST_NO_INIT, ST_KEYERROR = 0, 1, 2, 3  # include/offsim.h: OFFSIM_ST_*
QLEARN, EXPSARSA = 1, 2                                    # OFFSIM_TD_*
FIXED, EPS_GREEDY, SOFT_GREEDY = 0, 1, 2                   # OFFSIM_BEHAVIOUR_*
UNLIMITED = 1 << 62


class Log:
    """The logged transitions on the host, with TransitionTable's dense state -> slot map."""

    def __init__(self, z, a, r, z_next, done, p_log, t0):
        self.z, self.a, self.z_next = (np.asarray(x, np.int64) for x in (z, a, z_next))
        self.done, self.t0 = np.asarray(done, bool), np.asarray(t0, bool)
        self.r, self.p_log = np.asarray(r), np.asarray(p_log)
        self.r64, self.p64 = self.r.astype(np.float64), self.p_log.astype(np.float64)  # exact widenings
        self.N, self.nA = len(self.z), self.p_log.shape[1]
        self.z_base = int(min(self.z.min(), self.z_next.min(), 0))
        self.n_slots = int(max(self.z.max(), self.z_next.max())) - self.z_base + 1
        assert self.n_slots <= 1024, "beyond 1024 ids the table may compact them: this helper restates the dense map only"
        self.slot_z = np.arange(self.z_base, self.z_base + self.n_slots)

    def slot(self, z):
        return int(z) - self.z_base

    def oracle(self):
        return O.OraclePSRS(self.z, self.a, self.r64, self.z_next, self.done, self.p64, self.t0)


class Learner:
    """One learner: its sampler (queues, cursors, rejection stream), its Q [n_slots, nA] and its tie stream."""

    def __init__(self, log, seed, q_init, tie_state=None, stream="pcg64", shuffle_seed=None):
        self.log, self.ora = log, log.oracle()
        if shuffle_seed is None:
            self.ora.reset_sampler(seed)
        else:  # one queue order shared by the launch, the learner's own rejection stream
            self.ora.reset_sampler(shuffle_seed)
            self.ora.set_rejection_seed(seed)
        if stream == "philox":
            self.ora.set_rejection_philox(seed)
        self.q = np.array(q_init, dtype=np.float64).reshape(log.n_slots, log.nA).copy()
        self.rs = None
        if tie_state is not None:
            w = np.asarray(tie_state, dtype=np.uint32).reshape(625)
            self.rs = np.random.RandomState()
            self.rs.set_state(("MT19937", w[:624].copy(), int(w[624])))
        self.cur_slot = -1

    def tie_words(self):
        """The tie stream as the device keeps it: 624 state words and the position."""
        if self.rs is None:
            return None
        st = self.rs.get_state()
        return np.concatenate([np.asarray(st[1], np.uint32), np.array([st[2]], np.uint32)])

    def cursors(self):
        """(per-slot cursors [n_slots], init cursor) of the sampler, from the oracle's heads."""
        keys = self.ora.orders()[0]
        heads, init_head = self.ora.heads()
        cur = np.zeros(self.log.n_slots, np.int64)
        cur[keys - self.log.z_base] = heads
        return cur, init_head


def _sched(table, const, ep):
    return float(const) if table is None else float(table[min(ep, len(table) - 1)])


def run(lr, mode, pi, gamma, alpha, behaviour=FIXED, epsilon=0.0, alpha_ep=None, epsilon_ep=None, n_episodes=None,
        reject_mode=O.REJECT_DEFAULT, trace_cap=0, ep_cap=0, snap_cap=0, snap_stride=1, keep_p=False):
    """Runs learner `lr` from where it stands until its log or `n_episodes` ends; `lr` keeps the state a second call resumes from.
    pi [n_slots, nA] f64 in slot order.  Returns the row of every output of BatchedPSRS.eval_td that belongs to this learner (keep_p: also `beh_p`, the behaviour
    distribution of every accepted step)."""
    log, ora, q, nA = lr.log, lr.ora, lr.q, lr.log.nA
    pi = np.asarray(pi, np.float64)
    gamma = float(gamma)
    n_episodes = UNLIMITED if n_episodes is None else int(n_episodes)
    snap_stride = max(int(snap_stride), 1)
    o = dict(trace_row=np.full(trace_cap, -1, np.int32), trace_pop=np.zeros(trace_cap, np.int32), td_err=np.zeros(trace_cap, np.float64),
             beh_arg=np.zeros(trace_cap, np.int32), ep_g=np.zeros(ep_cap, np.float64), ep_len=np.zeros(ep_cap + 1, np.int32),
             q_snap=np.zeros((snap_cap, log.n_slots, nA), np.float64))
    beh_p = []
    ep = n_len = steps = cand = 0
    words = 0
    sum_g = 0.0
    status, terminate = ST_OK, False
    while ep < n_episodes and not terminate:
        row0 = ora.reset()
        if row0 is None:
            status, lr.cur_slot = ST_NO_INIT, -1
            break
        s = log.slot(log.z[row0])
        G, t, done = 0.0, 0, False
        while not done:
            lr.cur_slot = s
            if behaviour == FIXED:
                p = pi[s]
            elif behaviour == EPS_GREEDY:
                tied = np.where(q[s] == q[s].max())[0]
                if lr.rs is None:
                    best = int(tied[0])
                else:
                    before = lr.rs.get_state()[2]
                    best = int(lr.rs.choice(tied))
                    after = lr.rs.get_state()[2]
                    if len(tied) > 1:  # (a draw takes a few words at most: the position wraps at most once)
                        words += after - before if after > before else (624 - before) + after
                eps = _sched(epsilon_ep, epsilon, ep)
                p = np.full(nA, eps / nA)
                p[best] = 1 - eps + eps / nA
                if steps < trace_cap:
                    o["beh_arg"][steps] = best
            else:
                close = np.isclose(q[s], q[s].max())
                p = np.where(close, 1.0 / int(close.sum()), 0.0)
            try:
                row, n = ora.step(p, O.PROB_F64, reject_mode)
            except KeyError:
                status, terminate = ST_KEYERROR, True
                break
            cand += n
            if row is None:
                status, terminate = ST_EXHAUSTED, True
                break
            if steps < trace_cap:
                o["trace_row"][steps], o["trace_pop"][steps] = row, n
            if keep_p:
                beh_p.append(np.array(p, np.float64))
            A, sn, r = int(log.a[row]), log.slot(log.z_next[row]), float(log.r64[row])
            q_sa = float(q[s, A])
            if mode == QLEARN:
                nxt = max(float(v) for v in q[sn])
            else:
                nxt = 0.0
                for k in range(nA):
                    nxt = nxt + float(q[sn, k]) * float(pi[sn, k])
            td = r + gamma * nxt - q_sa
            if steps < trace_cap:
                o["td_err"][steps] = td
            q[s, A] = q_sa + _sched(alpha_ep, alpha, ep) * td
            if snap_cap and steps % snap_stride == 0 and steps // snap_stride < snap_cap:
                o["q_snap"][steps // snap_stride] = q
            G = G + gamma ** t * r
            t += 1
            steps += 1
            s, done = sn, bool(log.done[row])
            lr.cur_slot = s
        if status == ST_KEYERROR:
            break
        if n_len <= ep_cap and ep_cap:
            o["ep_len"][n_len] = t
        n_len += 1
        if done:
            if ep < ep_cap:
                o["ep_g"][ep] = G
            sum_g += G
            ep += 1
        elif ep < ep_cap:
            o["ep_g"][ep] = G
    o.update(q=q.copy(), sum_g=sum_g, n_ep=ep, steps=steps, cand=cand, n_len=n_len, status=status, tie_mt=lr.tie_words(), mt_words=words,
             cur_slot=lr.cur_slot)
    o["cursor"], o["init_cursor"] = lr.cursors()
    if keep_p:
        o["beh_p"] = beh_p
    return o


def reset_and_step(lr, p, reject_mode=O.REJECT_DEFAULT):
    """What one further PSRS.reset() and PSRS.step(p) serve after a run: (initial row or -1, accepted row or -1, status, candidates
    popped) -- where the sampler's cursors and its rejection stream stand is what decides them.  Without an initial row left the
    learner has no state and the step is not taken (the device reports OFFSIM_ST_INACTIVE = 4)."""
    row0 = lr.ora.reset()
    if row0 is None:
        return -1, -1, 4, 0
    try:
        row, n = lr.ora.step(np.asarray(p, np.float64), O.PROB_F64, reject_mode)
    except KeyError:
        return row0, -1, ST_KEYERROR, 0
    return (row0, -1, ST_EXHAUSTED, n) if row is None else (row0, row, ST_OK, n)


_STACK = dict(q=np.float64, sum_g=np.float64, n_ep=np.int64, steps=np.int64, cand=np.int64, n_len=np.int64, status=np.int32,
              trace_row=np.int32, trace_pop=np.int32, td_err=np.float64, beh_arg=np.int32, ep_g=np.float64, ep_len=np.int32,
              q_snap=np.float64, cursor=np.int64, init_cursor=np.int64, cur_slot=np.int64, mt_words=np.int64)


def run_launch(learners, **kw):
    """run() for every learner of a launch, stacked as the device returns them ([R, ...]); tie_mt [R, 625] uint32 or None."""
    rows = [run(lr, **kw) for lr in learners]
    out = {k: np.stack([np.asarray(r[k], dt) for r in rows]) for k, dt in _STACK.items()}
    out["tie_mt"] = None if rows[0]["tie_mt"] is None else np.stack([r["tie_mt"] for r in rows])
    return out
