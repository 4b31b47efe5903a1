"""The learner's collection loop on QueueEvaluator in plain NumPy / Python, one environment at a time, and the case list of
tests/test_gpu_queue_collect.py (test infrastructure).

A restatement of documented behaviour (offsim4rl/agents/ppo.py:258-279 on offsim4rl/evaluators/queue_evaluator.py:77-131, include/offsim.h:
offsim_queue_collect), not of the kernel's code, on queue_host.Sampler:

  policy   per-row probability tables in caller order, P_next[i] = the policy at next_obs of row i, P_init[i] = at obs of row i, read
           through obs_row (i >= 0: next_obs of row i; -2 - i: obs of row i) as collect_host.collect_rows reads them -- or pi [nZ, nA] by
           state row z - z_lo
  action   draw(p, gen): cdf = cumsum(p widened to f64); cdf /= cdf[-1]; A = cdf.searchsorted(gen.random(), side='right') -- what
           Generator.choice(nA, p=p) computes, restated because choice itself refuses many f32 softmax rows once they are widened (their sum
           misses 1 by more than its f64 tolerance); test_queue_collect_host.py holds it to gen.choice(nA, p=p32).  A row whose cdf is not
           finite (NaN or all zeros) draws nothing: A = nA, the draw consumed.  One draw per asked step
  pop      Sampler.step(A): KeyError for a pair never logged (and for A = nA), None for a queue at its end; either stops the environment for
           the rest of the call with state, observation and heads as they were
  record   row, action (drawn at every asked step, the unserved last one included; -1 where nothing was asked), flags SERVED | TERMINATED
           (the row's done) | TRUNCATED (cap > 0 and steps of the episode >= cap) | RESET (an initial row followed) | ALIVE
  reset    on terminated or truncated: the next initial row; none left: ST_NO_INIT, no state, the observation recorded as -1
"""
import numpy as np

import queue_host as Q

SERVED, TERMINATED, TRUNCATED, RESET, ALIVE = 1, 2, 4, 8, 16  # include/offsim.h: OFFSIM_COLLECT_*
ST_OK, ST_EXHAUSTED, ST_NO_INIT, ST_KEYERROR, ST_INACTIVE = 0, 1, 2, 3, 4


def draw(p, gen):
    """(A, u): the action of the rule above and the uniform it used"""
    u = gen.random()
    with np.errstate(invalid="ignore", divide="ignore"):
        cdf = np.cumsum(np.asarray(p).astype(np.float64))
        cdf /= cdf[-1]
    if not np.isfinite(cdf).all():
        return len(cdf), u
    return int(cdf.searchsorted(u, side="right")), u


class Env:
    """One environment's carried state: the sampler, the action stream, ep_t, obs_row, alive."""

    def __init__(self, log, seed, action_seed):
        self.log, self.sm, self.gen = log, Q.Sampler(log, seed), np.random.default_rng(action_seed)
        self.ep_t, self.obs_row, self.alive = 0, -1, False

    def reset(self):
        row = self.sm.reset()
        self.ep_t = 0
        self.alive = row is not None
        if row is not None:
            self.obs_row = -2 - row
        return row

    def state(self):
        lg, sm = self.log, self.sm
        return dict(cursor=sm.cursors(), init_cursor=sm.init_head, cur_slot=-1 if sm.cur is None else (sm.cur - lg.z_lo) * lg.nA, ep_t=self.ep_t,
                    obs_row=self.obs_row, alive=self.alive, rng=Q.rng_words(self.gen))


def collect(env, T, cap, P_next=None, P_init=None, pi=None):
    """T steps of `env` from where it stands; returns dict(row, action, flags, asked_at (obs_row each asked step was asked at, -1 else),
    p (the row drawn from, zeros where nothing was asked), status) and leaves env where the call ended (env.state())."""
    lg, sm = env.log, env.sm
    nA = lg.nA
    row, action, flags, asked_at = np.full(T, -1, np.int32), np.full(T, -1, np.int32), np.zeros(T, np.uint8), np.full(T, -1, np.int64)
    ps = np.zeros((T, nA), np.float64)
    status = ST_OK if sm.cur is not None else ST_INACTIVE
    live = status == ST_OK
    moved = none = False
    for i in range(T):
        if live and not (0 <= sm.cur - lg.z_lo < lg.nZ):  # a state outside the table: nothing asked
            status, live, env.alive = ST_KEYERROR, False, False
        if not live:
            continue
        asked_at[i] = env.obs_row
        if pi is not None:
            p = pi[sm.cur - lg.z_lo]
        else:
            p = P_next[env.obs_row] if env.obs_row >= 0 else P_init[-2 - env.obs_row]
        ps[i] = p
        A, _ = draw(p, env.gen)
        action[i] = A
        try:
            g = sm.step(A)
        except KeyError:
            g, why = None, ST_KEYERROR
        else:
            why = ST_EXHAUSTED
        if g is None:
            status, live, env.alive = why, False, False
            continue
        assert int(lg.a[g]) == A
        env.ep_t += 1
        term, trunc = bool(lg.done[g]), cap > 0 and env.ep_t >= cap
        fl = SERVED | (TERMINATED if term else 0) | (TRUNCATED if trunc else 0)
        env.obs_row, moved = g, True
        if term or trunc:
            env.ep_t = 0
            r0 = sm.reset()
            if r0 is None:
                status, live, env.alive, none = ST_NO_INIT, False, False, True
            else:
                env.obs_row = -2 - r0
                fl |= RESET
        if env.alive:
            fl |= ALIVE
        row[i], flags[i] = g, fl
    if moved and none:
        env.obs_row = -1
    return dict(row=row, action=action, flags=flags, asked_at=asked_at, p=ps, status=status)


# ---------------------------------------------------------------------------------------------------------------------------------
# Logs with observations, and the case list
# ---------------------------------------------------------------------------------------------------------------------------------
def observations(log, dO=4, seed=0, dtype=np.float32):
    """Synthetic observations of a log: obs / next_obs [N, dO], feature 0 the state id and the rest noise (so that rows of one state
    differ), and the lookup back to the states."""
    g = np.random.default_rng(9000 + seed)
    obs = g.standard_normal((log.N, dO)).astype(dtype)
    nobs = g.standard_normal((log.N, dO)).astype(dtype)
    obs[:, 0], nobs[:, 0] = log.z, log.z_next
    return obs, nobs


def row_tables(log, seed, dtype=np.float32, nan_rows=0):
    """Random per-row policy tables P_next / P_init [N, nA] of `dtype` (rows of a softmax, so f32 rows miss 1 by rounding)."""
    g = np.random.default_rng(7000 + seed)
    def soft(x):
        e = np.exp(x - x.max(1, keepdims=True)).astype(dtype)
        return (e / e.sum(1, keepdims=True, dtype=dtype)).astype(dtype)
    pn, p0 = soft(g.standard_normal((log.N, log.nA)) * 2), soft(g.standard_normal((log.N, log.nA)) * 2)
    if nan_rows:
        pn[g.permutation(log.N)[:nan_rows]] = np.nan
    return pn, p0


class Case:
    """A case of the matrix.  form: 'mlp' | 'rows' | 'tabular'; ptype: the tables' element type (rows, tabular); xtype: the observations'
    (mlp); vf: None | 'mlp' | 'rows'; act: the networks' activation.  expect: the branch the case is there to reach -- a status some
    environment must end with, or a flag some step must carry (checked on the mirror by test_queue_collect_host.py)."""

    def __init__(self, name, N=2000, nZ=25, nA=5, E=9, T=40, cap=8, form="rows", ptype=np.float32, xtype=np.float32, vf=None, act="tanh",
                 bootstrap="reference", log_seed=1, holes=0, neg_state=False, no_init=False, p_t0=0.1, p_done=0.1, reset_envs=None, nan_rows=0,
                 record_obs=True, record_probs=True, expect=()):
        self.__dict__.update(locals())
        del self.__dict__["self"]
        self.seeds = [5 + 3 * i for i in range(E)]
        self.action_seeds = [200 + 7 * i for i in range(E)]
        self._log = None

    @property
    def log(self):
        if self._log is None:
            self._log = Q.make_log(self.N, self.nZ, self.nA, self.log_seed, r32=True, neg_state=self.neg_state, holes=self.holes, p_done=self.p_done,
                                   p_t0=self.p_t0, no_init=self.no_init)
        return self._log

    def envs(self):
        """The E mirror environments after reset_sampler / set_action_seeds / reset (reset_envs: only those environments are reset)."""
        out = []
        for k, (s, sa) in enumerate(zip(self.seeds, self.action_seeds)):
            e = Env(self.log, s, sa)
            if self.reset_envs is None or k in self.reset_envs:
                e.reset()
            out.append(e)
        return out

    def pi(self):
        """[nZ, nA] by state row (the tabular form)"""
        g = np.random.default_rng(3000 + self.log_seed)
        return g.dirichlet(np.full(self.log.nA, 1.5), self.log.nZ).astype(self.ptype)


# The base case: a 2 000-row log, 25 states, 5 actions, E = 9 (two workgroups, the second with one live wave), T = 40, cap 8.
CASES = [
    Case("mlp-f32", form="mlp", expect=(TRUNCATED, TERMINATED, RESET)),
    Case("mlp-f16", form="mlp", xtype=np.float16, log_seed=2),
    Case("mlp-relu", form="mlp", act="relu", log_seed=3),
    Case("rows-f32", form="rows", log_seed=4, expect=(TRUNCATED, TERMINATED)),
    Case("rows-f64", form="rows", ptype=np.float64, log_seed=5),
    Case("tabular-f64", form="tabular", ptype=np.float64, log_seed=6),
    Case("tabular-f32", form="tabular", ptype=np.float32, log_seed=7),
    Case("nA2", form="mlp", nA=2, nZ=12, log_seed=8),
    Case("nA16", form="mlp", nA=16, nZ=6, N=3000, log_seed=9),
    Case("vf-mlp-reference", form="mlp", vf="mlp", log_seed=10, expect=(TRUNCATED,)),
    Case("vf-mlp-spinup", form="mlp", vf="mlp", bootstrap="spinup", log_seed=11, p_done=0.02, expect=(TRUNCATED,)),
    Case("vf-rows-reference", form="mlp", vf="rows", log_seed=12),
    Case("vf-rows-spinup", form="rows", vf="rows", bootstrap="spinup", log_seed=13, p_done=0.02, expect=(TRUNCATED,)),
    Case("vf-mlp-tabular", form="tabular", ptype=np.float64, vf="mlp", log_seed=14),
    Case("vf-mlp-rows-f16", form="rows", vf="mlp", xtype=np.float16, log_seed=15),
    Case("exhausted", form="rows", N=60, nZ=3, nA=2, log_seed=16, p_t0=0.5, expect=(ST_EXHAUSTED,)),
    Case("holes-keyerror", form="rows", holes=40, log_seed=17, expect=(ST_KEYERROR,)),
    Case("nan-rows-keyerror", form="rows", nan_rows=400, log_seed=18, expect=(ST_KEYERROR,)),
    Case("no-init", form="rows", N=300, p_t0=0.0, cap=3, log_seed=19, expect=(ST_NO_INIT,)),
    Case("neg-state", form="tabular", ptype=np.float64, neg_state=True, log_seed=20),
    Case("inactive", form="mlp", reset_envs=(0, 3, 8), log_seed=21, expect=(ST_INACTIVE,)),
    Case("T0", form="mlp", T=0, log_seed=22),
    Case("no-cap", form="rows", cap=0, log_seed=23, expect=(TERMINATED,)),
    Case("no-records", form="mlp", vf=None, record_obs=False, record_probs=False, log_seed=24),
]
BY_NAME = {c.name: c for c in CASES}
