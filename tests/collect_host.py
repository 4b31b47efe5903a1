"""NumPy restatement of VectorPSRS.collect for one environment, with the policy given as per-row tables (test infrastructure).

The loop of the reference's CartPole example (examples/cartpole/psrs_from_expert_heuristic.py:59-80) for T steps: p_new = the policy at
the current observation (P_init[i] after a reset that popped initial row i, P_next[i] after serving row i), PSRS.step as restated in
obs_policy_host.py, truncated = steps of the episode >= cap (cap 0: never), reset on terminated or truncated, stop on None, on KeyError or
when the init queue is empty.  Tables are in caller order.
"""
import numpy as np

from obs_policy_host import orders


def collect_rows(z, a, z_next, done, p_log, t0, P_next, P_init, seed, T, cap):
    """Returns dict(rows, obs_row (the observation each step was asked at, encoded as offsim_collect_state.obs_row), terminated,
    truncated, reset (an initial observation followed the step), status 'ok' | 'keyerror', end (why the loop ended: 'running' after T
    steps, 'exhausted' (step returned None), 'no_init' (reset returned None), 'keyerror'), held (the observation the environment holds at
    the end, encoded as obs_row; -1 if it never had one))."""
    init, queues = orders(z, t0, seed)
    heads = {k: 0 for k in queues}
    rng = np.random.default_rng(seed=seed)
    rows, obs_rows, term, trunc, rst = [], [], [], [], []
    status, end = "ok", "running"
    ic = 0

    def reset():
        nonlocal ic
        if ic >= len(init):
            return None
        i0 = init[ic]
        ic += 1
        return i0

    i0 = reset()
    cur = None if i0 is None else -2 - i0
    s_z = None if i0 is None else int(z[i0])
    held = -1 if cur is None else cur
    end = "running" if cur is not None else "no_init"
    n_ep = 0
    for _ in range(T):
        if cur is None:
            break
        if s_z not in queues:
            status = end = "keyerror"
            break
        p = P_next[cur] if cur >= 0 else P_init[-2 - cur]
        q, acc = queues[s_z], None
        while acc is None and heads[s_z] < len(q):
            j = q[heads[s_z]]
            heads[s_z] += 1
            aj = int(a[j])
            M = (p / p_log[j]).max()
            u = rng.random()
            if not (u > p[aj] / p_log[j][aj] / M):
                acc = j
        if acc is None:
            end = "exhausted"
            break
        n_ep += 1
        tr = bool(cap) and n_ep >= cap
        rows.append(acc)
        obs_rows.append(cur)
        term.append(bool(done[acc]))
        trunc.append(tr)
        cur, s_z = acc, int(z_next[acc])
        held = cur
        rst.append(False)
        if done[acc] or tr:
            n_ep = 0
            i0 = reset()
            cur = None if i0 is None else -2 - i0
            s_z = None if i0 is None else int(z[i0])
            if i0 is None:
                end = "no_init"
            else:
                held, rst[-1] = cur, True
    return dict(rows=np.asarray(rows, np.int64), obs_row=np.asarray(obs_rows, np.int64), terminated=np.asarray(term, bool),
                truncated=np.asarray(trunc, bool), reset=np.asarray(rst, bool), status=status, end=end, held=held)
