"""The plain loop offsim_replay_td is held to (include/offsim.h): a logged memory swept through L tabular TD learners, step by step in Python.

The learners of a stream see the same transition at every step, so the loop runs over the steps and the learner is the leading axis of NumPy
arrays: every f64 operation is the elementwise IEEE one a scalar loop would do, in the order the header states --
    target = max_b Q[s', b] (first entry, then `>` left to right)  |  sum_b Q[s', b] * pi[s', b] from 0.0, left to right
    td = (r + gamma * target) - Q[s, a];  Q[s, a] = Q[s, a] + alpha(e) * td;  e += done
-- which for one learner is the reference's qlearn(..., memory=...) (offsim4rl/agents/tabular.py:90-104) bit for bit
(tests/test_replay_host.py holds it to the recorded reference).
"""
import numpy as np

QLEARN, EXPSARSA = 1, 2
ST_OK, ST_KEYERROR = 0, 3
LDS_BUDGET = 160 * 1024  # csrc/replay_td.hpp: REPLAY_LDS_BUDGET


def lpw(nS, nA, L):
    """offsim_replay_lpw: the largest of 64, 32, .., 1 no larger than L rounded up to a power of two whose Q image fits the budget; 0: none"""
    w = 64
    while w > 1 and w // 2 >= L:
        w //= 2
    while w >= 1 and nS * nA * w * 8 > LDS_BUDGET:
        w //= 2
    return w


def stream(log, mode, alpha, gamma, q, order=None, passes=1, alpha_ep=None, pi=None, td_cap=0, snap_stride=1, snap_cap=0):
    """One stream.  log = (s, a, r, s_next, done, nS, nA); alpha, gamma [L]; q [L, nS, nA] (Q_init, not modified); order [M] or None;
    alpha_ep [L, n_sched] or None; pi [nS, nA] or [L, nS, nA].  Returns q [L,nS,nA], td_err [td_cap, L], q_snap [L, snap_cap, nS, nA], n_ep,
    steps, status."""
    s, a, r, sn, done, nS, nA = log
    N = len(s)
    alpha, gamma = np.asarray(alpha, np.float64), np.asarray(gamma, np.float64)
    n_l = len(alpha)
    Q = np.array(q, dtype=np.float64)
    order = np.arange(N) if order is None else np.asarray(order)
    M = len(order)
    td_err = np.zeros((td_cap, n_l))
    q_snap = np.zeros((n_l, snap_cap, nS, nA))
    if pi is not None:
        pi = np.broadcast_to(np.asarray(pi, np.float64), (n_l, nS, nA))
    ep, steps, status = 0, passes * M, ST_OK
    for k in range(passes * M):
        row = int(order[k % M])
        if not 0 <= row < N or not (0 <= s[row] < nS and 0 <= a[row] < nA and 0 <= sn[row] < nS):
            steps, status = k, ST_KEYERROR
            break
        S, A, R, S_ = int(s[row]), int(a[row]), np.float64(r[row]), int(sn[row])
        qn = Q[:, S_, :]
        if mode == QLEARN:
            nxt = qn[:, 0].copy()
            for b in range(1, nA):
                nxt = np.where(qn[:, b] > nxt, qn[:, b], nxt)
        else:
            nxt = np.zeros(n_l)
            for b in range(nA):
                nxt = nxt + qn[:, b] * pi[:, S_, b]
        q_sa = Q[:, S, A].copy()
        td = R + gamma * nxt - q_sa
        if k < td_cap:
            td_err[k] = td
        al = alpha if alpha_ep is None else alpha_ep[:, min(ep, alpha_ep.shape[1] - 1)]
        Q[:, S, A] = q_sa + al * td
        if snap_cap and k % snap_stride == 0 and k // snap_stride < snap_cap:
            q_snap[:, k // snap_stride] = Q
        if done[row]:
            ep += 1
    return dict(q=Q, td_err=td_err, q_snap=q_snap, n_ep=ep, steps=steps, status=status)


def run(log, mode, alpha, gamma, q, orders=None, **kw):
    """S streams in the layout of evaluators.replay.replay_td: q [L, S, nS, nA] in and out, td_err [S, td_cap, L], q_snap
    [L, S, snap_cap, nS, nA], n_ep [S], steps / status [L, S]."""
    q = np.asarray(q, np.float64)
    n_l, S = q.shape[:2]
    outs = [stream(log, mode, alpha, gamma, q[:, j], None if orders is None else orders[j], **kw) for j in range(S)]
    return dict(q=np.stack([o["q"] for o in outs], axis=1), td_err=np.stack([o["td_err"] for o in outs]),
                q_snap=np.stack([o["q_snap"] for o in outs], axis=1), n_ep=np.array([o["n_ep"] for o in outs], np.int64),
                steps=np.tile(np.array([o["steps"] for o in outs], np.int64), (n_l, 1)),
                status=np.tile(np.array([o["status"] for o in outs], np.int32), (n_l, 1)))


def synth_log(N, nS, nA, seed, p_done=0.1):
    """A random log: uniform states and actions, normal rewards, done with probability p_done."""
    g = np.random.default_rng(seed)
    return (g.integers(0, nS, N).astype(np.int32), g.integers(0, nA, N).astype(np.int32), g.standard_normal(N), g.integers(0, nS, N).astype(np.int32),
            g.random(N) < p_done, nS, nA)


def learners(n_l, nS, nA, seed):
    """Distinct settings per learner: alpha, gamma [L], Q_init [L, nS, nA]."""
    g = np.random.default_rng(seed)
    return g.uniform(0.01, 0.9, n_l), g.uniform(0.5, 0.999, n_l), g.standard_normal((n_l, nS, nA)) * 0.1
