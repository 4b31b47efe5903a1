"""A NumPy restatement of the epoch log of the reference's PPO agent (include/offsim.h: offsim_ppo_epoch_log) over step-major [T, R]
records with a carry -- the rules, written plainly, for the tests to hold the kernel and the fixtures to.

Per environment, over its valid steps in order: open_ret += rew (a Python float: an f64 sum in step order), open_len += 1; at a step with
terminated or truncated an episode ends with return open_ret and length open_len - 1 ("reference": end_episode does not count its own
transition) or open_len ("steps"), and both go back to zero.  An environment with a valid step and no ended episode contributes the one
entry (open_ret, open_len), the open episode, and goes on; one without a valid step contributes nothing.  VVals: val at every valid step.
"""
import numpy as np


class Carry:
    def __init__(self, R):
        self.open_ret = [0.0] * R
        self.open_len = [0] * R


def epoch(rew, val, valid, terminated, truncated, carry, ep_len="reference"):
    """One epoch.  Returns per environment r: ended[r] = [(ret, len), ...] of the episodes that ended, entries[r] = ended[r] or the open
    episode's single entry or [], vvals[r] = [val, ...]; the carry is updated in place."""
    assert ep_len in ("reference", "steps")
    T, R = rew.shape
    ended, entries, vvals = [], [], []
    for r in range(R):
        ret, n, eps, vs = carry.open_ret[r], carry.open_len[r], [], []
        for t in range(T):
            if not valid[t, r]:
                continue
            ret += float(rew[t, r])
            n += 1
            vs.append(float(val[t, r]))
            if terminated[t, r] or truncated[t, r]:
                eps.append((ret, n - 1 if ep_len == "reference" else n))
                ret, n = 0.0, 0
        carry.open_ret[r], carry.open_len[r] = ret, n
        ended.append(eps)
        entries.append(eps if eps else [(ret, n)] if vs else [])
        vvals.append(vs)
    return ended, entries, vvals


def _stats(x):
    """mpi_statistics_scalar in f64: (mean, std, min, max, n, the summation bounds of mean and of the squared deviations)"""
    x = np.asarray(x, np.float64)
    n = len(x)
    if n == 0:
        return dict(mean=np.nan, std=np.nan, min=np.nan, max=np.nan, n=0, sum_abs=0.0, sum_sq=0.0)
    mean = x.sum() / n
    q = ((x - mean) ** 2)
    return dict(mean=mean, std=np.sqrt(q.sum() / n), min=x.min(), max=x.max(), n=n, sum_abs=np.abs(x).sum(), sum_sq=q.sum())


def learner_log(ended, entries, vvals, cols):
    """The log of one learner whose environments are `cols`: entries in environment order, then step order."""
    ent = [e for r in cols for e in entries[r]]
    return dict(ret=_stats([g for g, _ in ent]), len=_stats([n for _, n in ent]), v=_stats([v for r in cols for v in vvals[r]]),
                entries=len(ent), episodes=sum(len(ended[r]) for r in cols), steps=sum(len(vvals[r]) for r in cols))
