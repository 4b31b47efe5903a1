"""NumPy restatement of the PPO buffer rules of VectorPSRS.collect_ppo / offsim_ppo_advantages, in f64 (test infrastructure).

One environment's [T] records: a path ends at a valid step with terminated | truncated and bootstraps with (mode "reference", the agent's
rules of offsim4rl/agents/ppo.py:106-158) v of that step if truncated or if it is the last step, else 0, or (mode "spinup") 0 if terminated,
else v_trunc; a path still open after the last valid step bootstraps with final_value.  Within a path: spinup's PPOBuffer.finish_path,
deltas = r + gamma V_next - V, adv = discounted cumsum of deltas by gamma lam, ret = discounted cumsum of [r, bootstrap] by gamma minus the
last entry.  Normalisation: spinup's mpi_statistics_scalar over every valid entry of every environment.
"""
import numpy as np


def _dcs(x, d):
    out, acc = np.zeros(len(x)), 0.0
    for i in range(len(x) - 1, -1, -1):
        acc = x[i] + d * acc
        out[i] = acc
    return out


def gae(rew, val, term, trunc, valid, final_value, gamma, lam, mode="reference", v_trunc=None):
    """adv, ret [T] f64 (0 where not valid)."""
    T = len(rew)
    adv, ret = np.zeros(T), np.zeros(T)
    idx = [t for t in range(T) if valid[t]]
    paths, start = [], 0
    for k, t in enumerate(idx):
        if term[t] or trunc[t]:
            if mode == "reference":
                b = float(val[t]) if (trunc[t] or t == T - 1) else 0.0
            else:
                b = 0.0 if term[t] else float(v_trunc[t])
            paths.append((idx[start:k + 1], b))
            start = k + 1
    if start < len(idx):
        paths.append((idx[start:], float(final_value)))
    for ts, b in paths:
        r = np.append(np.asarray([rew[t] for t in ts], np.float64), b)
        v = np.append(np.asarray([val[t] for t in ts], np.float64), b)
        d = r[:-1] + gamma * v[1:] - v[:-1]
        adv[ts] = _dcs(d, gamma * lam)
        ret[ts] = _dcs(r, gamma)[:-1]
    return adv, ret


def statistics(x):
    """mpi_statistics_scalar over the float32 values x: (mean, population std), in f64."""
    x = np.asarray(x, np.float32).astype(np.float64)
    n = len(x)
    if n == 0:
        return 0.0, 0.0
    mean = x.sum() / n
    return mean, float(np.sqrt(((x - mean) ** 2).sum() / n))


def batch(rew, val, term, trunc, valid, final_value, gamma, lam, mode="reference", v_trunc=None):
    """[T, E] records -> adv_raw, ret, adv_norm [T, E] f64, mean, std (adv_norm = adv_raw where nothing is valid)."""
    T, E = rew.shape
    adv, ret = np.zeros((T, E)), np.zeros((T, E))
    for e in range(E):
        adv[:, e], ret[:, e] = gae(rew[:, e], val[:, e], term[:, e], trunc[:, e], valid[:, e], final_value[e], gamma, lam, mode,
                                   None if v_trunc is None else v_trunc[:, e])
    a32 = adv.astype(np.float32)[valid]
    mean, std = statistics(a32)
    norm = adv.copy()
    if a32.size:
        norm = np.where(valid, (adv.astype(np.float32).astype(np.float64) - mean) / std, 0.0)
    return adv, ret, norm, mean, std
