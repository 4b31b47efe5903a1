"""PSRS_Exo and the three drivers evalMC_psrs / qlearn_psrs / expSARSA_psrs in plain NumPy / Python, one rollout at a time (test
infrastructure), and the case list of the kernel matrix (tests/test_gpu_exo_drivers.py).

A restatement of documented behaviour (offsim4rl/evaluators/psrs.py:59-271, include/offsim.h: offsim_eval_mc_exo), not of the kernel's code:

  sampler    reset_sampler(seed): the initial rows in buffer order, the rows of every s value and of every x value in buffer order, each
             list shuffled by its own np.random.default_rng(seed).  reset(): the rejection stream restarts (reseed "episode":
             default_rng(episode0 + e), before the init queue is looked at), then the next initial row gives (s, x).
  step       pops the heads of s_queues[s] and x_queues[x] together; one draw u per candidate; f64: accept when
             u <= p[a] / p_log[a] / max(p / p_log) in doubles; f32: the same in float32 with u rounded to float32.  Either queue empty:
             exhausted, the state stays.  A state without rows in either family: KeyError.
  tables     pi and Q are indexed by obs_of[s slot, x slot]; -1 there: KeyError status (the reference raises IndexError).  In the learner
             drivers an accepted step whose next pair has no row stops the rollout after the environment has stepped.
  update     Q-learning max(Q[o']); expected SARSA sum_k Q[o'][k] * pi[o'][k] from k = 0 upwards; td = r + gamma * nxt - Q[o, a];
             Q[o, a] = Q[o, a] + alpha * td; G = G + gamma ** t * r -- all in Python floats
  episodes   lengths get every episode, Gs the completed ones with the cut-short one stored behind them, sum_g adds the completed
             returns in order; status ok / exhausted / no_init / keyerror

Everything comes back in the device's layout: slots are value - min(values, 0) (TransitionTable's dense map), rows are caller rows,
outputs are cut by trace_cap / ep_cap / snap_cap and pre-filled as BatchedPSRSExo allocates them.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ST_OK, ST_EXHAUSTED, ST_NO_INIT, ST_KEYERROR, ST_INACTIVE = 0, 1, 2, 3, 4  # include/offsim.h: OFFSIM_ST_*
EVALMC, QLEARN, EXPSARSA = 0, 1, 2                                       # OFFSIM_TD_*
UNLIMITED = 1 << 62
GAMMA, ALPHA = 0.95, 0.2  # of every case of the matrix


class Log:
    """The logged transitions of an exogenous-state log on the host, with TransitionTable's dense value -> slot maps."""

    def __init__(self, s, x, a, r, s_next, x_next, done, p_log, t0):
        self.s, self.x, self.a, self.s_next, self.x_next = (np.asarray(v, np.int64) for v in (s, x, a, s_next, x_next))
        self.done, self.t0 = np.asarray(done, bool), np.asarray(t0, bool)
        self.r, self.p_log = np.asarray(r), np.asarray(p_log)
        self.r64, self.p64 = self.r.astype(np.float64), self.p_log.astype(np.float64)  # exact widenings
        self.N, self.nA = len(self.s), self.p_log.shape[1]
        self.s_base = int(min(self.s.min(), self.s_next.min(), 0))
        self.x_base = int(min(self.x.min(), self.x_next.min(), 0))
        self.ns = int(max(self.s.max(), self.s_next.max())) - self.s_base + 1
        self.nx = int(max(self.x.max(), self.x_next.max())) - self.x_base + 1
        self.s_values, self.x_values = np.arange(self.s_base, self.s_base + self.ns), np.arange(self.x_base, self.x_base + self.nx)

    def obs_of(self, combine, n_rows):
        """obs_of [ns, nx] and the observation ids of its compact rows, as evaluators/psrs_exo.py: tabulate_obs lays them out."""
        grid = np.array([[combine(int(s), int(x)) for x in self.x_values] for s in self.s_values], np.int64)
        ok = (grid >= 0) & (grid < n_rows)
        ids = np.unique(grid[ok])
        out = np.full(grid.shape, -1, np.int32)
        out[ok] = np.searchsorted(ids, grid[ok])
        return out, ids


class Stream:
    """A rejection stream: default_rng(seed), or Philox draws first, first + 1, .. of `seed` (oracle.philox_doubles)."""

    def __init__(self, seed, philox=False):
        self.seed, self.philox, self.count = int(seed), philox, 0
        self.gen = None if philox else np.random.default_rng(int(seed))
        self._buf, self._at = None, 0

    def draw(self):
        self.count += 1
        if not self.philox:
            return float(self.gen.random())
        if self._buf is None or self._at == len(self._buf):
            from oracle import oracle as O
            self._buf, self._at = O.philox_doubles(self.seed, 256, self.count - 1), 0
        self._at += 1
        return float(self._buf[self._at - 1])


class Sampler:
    """One PSRS_Exo: its queue orders, heads, state (s, x as values; None: no state) and rejection stream."""

    def __init__(self, log, seed, stream="pcg64"):
        self.log = log
        self.reset_sampler(seed, stream)

    def reset_sampler(self, seed, stream="pcg64"):
        lg = self.log
        shuffled = lambda rows: (lambda l: (np.random.default_rng(seed).shuffle(l), l)[1])([int(i) for i in rows])  # noqa: E731
        self.init_queue = shuffled(np.flatnonzero(lg.t0))
        self.s_queues = {int(v): shuffled(np.flatnonzero(lg.s == v)) for v in np.unique(lg.s)}
        self.x_queues = {int(v): shuffled(np.flatnonzero(lg.x == v)) for v in np.unique(lg.x)}
        self.s_head, self.x_head, self.init_head = {k: 0 for k in self.s_queues}, {k: 0 for k in self.x_queues}, 0
        self.cur = None
        self.stream = Stream(seed, philox=stream == "philox")
        self.min_rem_at_entry = 1 << 30

    def reset(self, reseed_to=None):
        if reseed_to is not None:
            self.stream = Stream(reseed_to)
        if self.init_head >= len(self.init_queue):
            self.cur = None
            return None
        row = self.init_queue[self.init_head]
        self.init_head += 1
        self.cur = (int(self.log.s[row]), int(self.log.x[row]))
        return row

    def step(self, p, f32=False):
        """(s-row, x-row, candidates popped); rows None when a queue ran out; KeyError when a queue is missing."""
        lg = self.log
        s, x = self.cur
        if s not in self.s_queues or x not in self.x_queues:
            raise KeyError((s, x))
        qs, qx, n = self.s_queues[s], self.x_queues[x], 0
        self.min_rem_at_entry = min(self.min_rem_at_entry, min(len(qs) - self.s_head[s], len(qx) - self.x_head[x]))
        p = np.asarray(p, np.float32 if f32 else np.float64)
        while True:
            if self.s_head[s] >= len(qs) or self.x_head[x] >= len(qx):
                return None, None, n
            rs, rx = qs[self.s_head[s]], qx[self.x_head[x]]
            self.s_head[s] += 1
            self.x_head[x] += 1
            n += 1
            u, a = self.stream.draw(), int(lg.a[rs])
            with np.errstate(all="ignore"):
                pl = lg.p_log[rs].astype(np.float32) if f32 else lg.p64[rs]
                M = (p / pl).max()
                thr = p[a] / pl[a] / M
                rej = (np.float32(u) > thr) if f32 else (u > thr)
            if not rej:
                self.cur = (int(lg.s_next[rs]), int(lg.x_next[rx]))
                return rs, rx, n

    def slots(self):
        return (-1, -1) if self.cur is None else (self.cur[0] - self.log.s_base, self.cur[1] - self.log.x_base)

    def cursors(self):
        lg = self.log
        cs, cx = np.zeros(lg.ns, np.int64), np.zeros(lg.nx, np.int64)
        for k, v in self.s_head.items():
            cs[k - lg.s_base] = v
        for k, v in self.x_head.items():
            cx[k - lg.x_base] = v
        return cs, cx


def run(sm, mode, pi, obs_of, gamma, alpha=0.1, alpha_ep=None, q=None, n_episodes=None, reseed="episode", episode0=0, f32=False, trace_cap=0,
        ep_cap=0, snap_cap=0, snap_stride=1):
    """Runs sampler `sm` from where it stands until its log or `n_episodes` ends; `sm` (and `q`, updated in place) keep the state a second
    call resumes from.  pi [n_obs, nA], obs_of [ns, nx].  Returns the row of every output of BatchedPSRSExo.eval_mc / eval_td."""
    lg, nA = sm.log, sm.log.nA
    pi = np.asarray(pi, np.float32 if f32 else np.float64)
    n_obs, gamma = pi.shape[0], float(gamma)
    n_episodes = UNLIMITED if n_episodes is None else int(n_episodes)
    o = dict(trace_row=np.full(trace_cap, -1, np.int32), trace_row_x=np.full(trace_cap, -1, np.int32), trace_pop=np.zeros(trace_cap, np.int32),
             td_err=np.zeros(trace_cap, np.float64), ep_g=np.zeros(ep_cap, np.float64), ep_len=np.zeros(ep_cap + 1, np.int32),
             q_snap=np.zeros((snap_cap, n_obs, nA), np.float64), last=np.full(3, -1, np.int32))

    def row_of(cur):
        i, j = cur[0] - lg.s_base, cur[1] - lg.x_base
        v = int(obs_of[i, j]) if 0 <= i < lg.ns and 0 <= j < lg.nx else -1
        return v if 0 <= v < n_obs else -1
    ep = n_len = steps = cand = 0
    sum_g, status, terminate = 0.0, ST_OK, False
    while ep < n_episodes and not terminate:
        row0 = sm.reset(episode0 + ep if reseed == "episode" else None)
        if row0 is None:
            status = ST_NO_INIT
            break
        o["last"][:] = (-1, -1, row0)
        G, t, done = 0.0, 0, False
        while not done:
            oc = row_of(sm.cur)
            if oc < 0:
                status, terminate = ST_KEYERROR, True
                break
            try:
                rs, rx, n = sm.step(pi[oc], f32)
            except KeyError:
                status, terminate = ST_KEYERROR, True
                break
            cand += n
            if rs is None:
                status, terminate = ST_EXHAUSTED, True
                break
            o["last"][:] = (rs, rx, -1)
            A, r = int(lg.a[rs]), float(lg.r64[rs])
            if mode != EVALMC:
                on = row_of(sm.cur)
                if on < 0:
                    status, terminate = ST_KEYERROR, True
                    break
                q_sa = float(q[oc, A])
                if mode == QLEARN:
                    nxt = max(float(v) for v in q[on])
                else:
                    nxt = 0.0
                    for k in range(nA):
                        nxt = nxt + float(q[on, k]) * float(pi[on, k])
                td = r + gamma * nxt - q_sa
                if steps < trace_cap:
                    o["td_err"][steps] = td
                q[oc, A] = q_sa + (float(alpha) if alpha_ep is None else float(alpha_ep[min(ep, len(alpha_ep) - 1)])) * td
                if snap_cap and steps % snap_stride == 0 and steps // snap_stride < snap_cap:
                    o["q_snap"][steps // snap_stride] = q
            if steps < trace_cap:
                o["trace_row"][steps], o["trace_row_x"][steps], o["trace_pop"][steps] = rs, rx, n
            G = G + gamma ** t * r
            t += 1
            steps += 1
            done = bool(lg.done[rs])
        if status == ST_KEYERROR:
            break
        if ep_cap and n_len <= ep_cap:
            o["ep_len"][n_len] = t
        n_len += 1
        if done:
            if ep < ep_cap:
                o["ep_g"][ep] = G
            sum_g += G
            ep += 1
        elif ep < ep_cap:
            o["ep_g"][ep] = G
    cs, cx = sm.cursors()
    o.update(sum_g=sum_g, n_ep=ep, steps=steps, cand=cand, n_len=n_len, status=status, cursor_s=cs, cursor_x=cx, init_cursor=sm.init_head,
             cur_s=sm.slots()[0], cur_x=sm.slots()[1], draws=sm.stream.count)
    if q is not None:
        o["q"] = q.copy()
    return o


def next_step(sm, p, f32=False):
    """What one further PSRS_Exo.step(p) serves after a run, as offsim_step_exo reports it: (s-row, x-row, status, popped)."""
    if sm.cur is None:
        return -1, -1, ST_INACTIVE, 0
    try:
        rs, rx, n = sm.step(p, f32)
    except KeyError:
        return -1, -1, ST_KEYERROR, 0
    return (-1, -1, ST_EXHAUSTED, n) if rs is None else (rs, rx, ST_OK, n)


# ---------------------------------------------------------------------------------------------------------------------------------
# The LDS carve of csrc/eval_exo.hpp, restated (include/offsim.h: 4 rollouts per workgroup, then 2, then 1 while it exceeds 64 KiB;
# one rollout up to 160 KiB; beyond: refused)
# ---------------------------------------------------------------------------------------------------------------------------------
def lds_bytes(waves, ns, nx, n_obs, nA, prob_bytes=8, td=False):
    return (waves * 65 * 32 + (waves * n_obs * nA * 8 if td else 0) + n_obs * nA * prob_bytes + ns * nx * 4 + (ns + 1) * 4 + (nx + 1) * 4
            + waves * (ns + nx) * 4)


def launch_shape(ns, nx, n_obs, nA, prob_bytes=8, td=False):
    """(rollouts per workgroup, LDS bytes, refused)"""
    w = 4
    while w > 1 and lds_bytes(w, ns, nx, n_obs, nA, prob_bytes, td) > 65536:
        w //= 2
    b = lds_bytes(w, ns, nx, n_obs, nA, prob_bytes, td)
    return w, b, b > 160 * 1024


def first_n_obs_with(waves, big, ns, nx, nA, td):
    """The smallest n_obs whose launch has `waves` rollouts per workgroup (big: one rollout above 64 KiB)."""
    n = 1
    while True:
        w, b, _ = launch_shape(ns, nx, n, nA, 8, td)
        if w == waves and (b > 65536) == big:
            return n
        n += 1


# ---------------------------------------------------------------------------------------------------------------------------------
# Logs and the case list
# ---------------------------------------------------------------------------------------------------------------------------------
def make_log(N, nS, nX, nA, seed, plog=np.float64, neg_state=False, p_done=0.08, p_t0=0.1, hot=None):
    """An iid exogenous-state log.  neg_state: the s values start at -1.  hot = (rows, p): state 0 gets at least `rows` rows and the log
    took action 0 there with probability `p`."""
    g = np.random.default_rng(seed)
    s, x = g.integers(0, nS, N), g.integers(0, nX, N)
    s_next, x_next = g.integers(0, nS, N), g.integers(0, nX, N)
    if hot:
        s[: hot[0]] = 0
        s_next[g.random(N) < 0.5] = 0
    p_log = g.dirichlet(np.full(nA, 2.0), N)
    if hot:
        rest = p_log[:, 1:] / p_log[:, 1:].sum(1, keepdims=True)
        p_log = np.concatenate([np.full((N, 1), hot[1]), rest * (1 - hot[1])], axis=1)
    p_log = p_log.astype(plog)
    p64 = p_log.astype(np.float64)
    a = np.array([g.choice(nA, p=p64[i] / p64[i].sum()) for i in range(N)], np.int64)
    r = g.standard_normal(N)
    done = g.random(N) < p_done
    t0 = g.random(N) < p_t0
    t0[:3] = True
    if hot:
        g.shuffle(order := np.arange(N))
        s, x, s_next, x_next, p_log, a, r, done, t0 = (v[order] for v in (s, x, s_next, x_next, p_log, a, r, done, t0))
    if neg_state:
        s, s_next = s - 1, s_next - 1
    return Log(s, x, a, r, s_next, x_next, done, p_log, t0)


class Case:
    def __init__(self, name, N=500, nS=5, nX=2, nA=3, R=5, log_seed=1, plog=np.float64, prob="f64", reseed="episode", stream="pcg64", episode0=0,
                 n_episodes=None, mode=EVALMC, combine="4s+x", n_rows=None, neg_state=False, hot=None, pi_on_action0=None, n_obs_pad=None, snap=False,
                 alpha_sched=False):
        self.__dict__.update(locals())
        del self.__dict__["self"]
        self.seeds = [3 + 7 * i for i in range(R)]
        self._log = self._host = None

    @property
    def log(self):
        if self._log is None:
            self._log = make_log(self.N, self.nS, self.nX, self.nA, self.log_seed, self.plog, self.neg_state, hot=self.hot)
        return self._log

    def tables(self):
        """(obs_of [ns, nx], pi [n_obs, nA] in the case's probability dtype)"""
        lg = self.log
        span = lg.nx
        comb = {"4s+x": lambda s, x: (s - lg.s_base) * span + (x - lg.x_base), "s": lambda s, x: s - lg.s_base}[self.combine]
        n_rows = (lg.ns * span if self.combine == "4s+x" else lg.ns) if self.n_rows is None else self.n_rows
        obs_of, ids = lg.obs_of(comb, n_rows)
        n_obs = len(ids) if self.n_obs_pad is None else self.n_obs_pad  # (padding: rows of pi / Q no pair maps to -- they size the LDS carve)
        g = np.random.default_rng(1000 + self.log_seed)
        pi = g.dirichlet(np.full(self.nA, 1.5), n_obs)
        if self.pi_on_action0 is not None:
            pi = np.concatenate([np.full((n_obs, 1), self.pi_on_action0), np.full((n_obs, self.nA - 1), (1 - self.pi_on_action0) / (self.nA - 1))], axis=1)
        return obs_of, pi.astype(np.float32 if self.prob == "f32" else np.float64)

    def q_init(self, n_obs):
        return np.random.default_rng(7).standard_normal((self.R, n_obs, self.nA)) * 0.1

    @property
    def alpha_ep(self):
        return np.array([0.5 / (1.0 + 0.1 * e) for e in range(40)]) if self.alpha_sched else None

    def kw(self, trace_cap=None):
        cap = self.log.N + 1 if trace_cap is None else trace_cap
        return dict(n_episodes=self.n_episodes, reseed=self.reseed, episode0=self.episode0, trace_cap=cap, ep_cap=self.log.N + 1,
                    snap_cap=16 if self.snap else 0, snap_stride=3 if self.snap else 1)

    def samplers(self):
        return [Sampler(self.log, s, self.stream) for s in self.seeds]

    def host(self):
        """The mirror's outputs per rollout and the samplers as the runs left them (computed once)."""
        if self._host is None:
            obs_of, pi = self.tables()
            sms, q0 = self.samplers(), self.q_init(pi.shape[0])
            outs = [run(sm, self.mode, pi, obs_of, GAMMA, alpha=ALPHA, alpha_ep=self.alpha_ep, q=None if self.mode == EVALMC else q0[i].copy(),
                        f32=self.prob == "f32", **self.kw()) for i, sm in enumerate(sms)]
            self._host = (outs, sms)
        return self._host


_f16 = dict(plog=np.float16)
CASES = [
    Case("evalmc-f64-R5"),
    Case("evalmc-f64-R1-lone", R=1, N=300, nS=3, nX=1, nA=2, log_seed=2),
    Case("evalmc-f64-R9", R=9, N=700, nS=7, nX=3, nA=5, log_seed=3),
    Case("evalmc-plog-f32-R5", plog=np.float32, log_seed=4),
    Case("evalmc-plog-f16-R5", log_seed=5, **_f16),
    Case("evalmc-prob-f32-R5", plog=np.float32, prob="f32", log_seed=6),
    Case("evalmc-prob-f32-none-R9", plog=np.float32, prob="f32", reseed="none", R=9, log_seed=7),
    Case("evalmc-none-pcg-R5", reseed="none", log_seed=8),
    Case("evalmc-none-philox-R5", reseed="none", stream="philox", log_seed=9),
    Case("evalmc-episode0-R5", episode0=(1 << 33) + 11, log_seed=10),
    Case("evalmc-max-episodes-R5", n_episodes=2, log_seed=11),
    Case("evalmc-neg-state-R5", neg_state=True, log_seed=12),
    Case("evalmc-default-combine-R5", combine="s", nX=3, log_seed=13),
    Case("evalmc-missing-row-R9", R=9, n_rows=7, log_seed=14),  # pi has 7 rows: the pairs from o = 7 on have none, reached in mid-run
    Case("evalmc-long-pop-R5", N=700, nS=3, nX=2, nA=4, hot=(230, 0.02), pi_on_action0=0.97, log_seed=15),
    Case("qlearn-R5", mode=QLEARN, log_seed=16, snap=True),
    Case("qlearn-none-philox-R9", mode=QLEARN, R=9, reseed="none", stream="philox", log_seed=17),
    Case("qlearn-plog-f16-sched-R5", mode=QLEARN, alpha_sched=True, log_seed=18, **_f16),
    Case("qlearn-missing-row-R5", mode=QLEARN, n_rows=6, log_seed=19),
    Case("expsarsa-R5", mode=EXPSARSA, log_seed=20, snap=True),
    Case("expsarsa-plog-f32-R1", mode=EXPSARSA, R=1, plog=np.float32, log_seed=21),
    Case("expsarsa-max-episodes-neg-state-R9", mode=EXPSARSA, R=9, n_episodes=3, neg_state=True, log_seed=22),
]
# The launch shapes, forced by the rows of pi / Q (n_obs_pad: rows no pair maps to still take their place in LDS).  From the carve above with
# ns = 5, nx = 2, nA = 3 and the learner's Q (td): bytes(w) = 2080 w + 24 n_obs (w + 1) + 40 + 24 + 12 + 28 w, so
#   4 rollouts fit while 8432 + 120 n_obs + 76 <= 65536, i.e. n_obs <= 475; from 476 on the launch halves to 2 (4216 + 72 n_obs + 76),
#   which holds up to n_obs = 850; from 851 on 1 (2108 + 48 n_obs + 76), within 64 KiB up to n_obs = 1319; from 1320 on one rollout
#   above 64 KiB, and from 3368 on (163 840 bytes are the limit) the call is refused.  first_n_obs_with() finds the same numbers by search,
#   and tests/test_exo_drivers_host.py checks them against these.
_SHAPE = dict(nS=5, nX=2, nA=3, mode=QLEARN, R=5)
LDS_BOUNDS = {"waves4-last": 475, "waves2-first": 476, "waves2-last": 850, "waves1-first": 851, "waves1-last-64k": 1319, "big-first": 1320,
              "big-last": 3367, "refused-first": 3368}
CASES += [
    Case("lds-waves4-last-R5", n_obs_pad=LDS_BOUNDS["waves4-last"], log_seed=23, **_SHAPE),
    Case("lds-waves2-first-R5", n_obs_pad=LDS_BOUNDS["waves2-first"], log_seed=24, **_SHAPE),
    Case("lds-waves1-first-R5", n_obs_pad=LDS_BOUNDS["waves1-first"], log_seed=25, **_SHAPE),
    Case("lds-big-first-R5", n_obs_pad=LDS_BOUNDS["big-first"], log_seed=26, **_SHAPE),
    Case("lds-evalmc-waves2-R9", n_obs_pad=2400, log_seed=27, R=9),  # evalMC, f64 pi alone: 8 * 3 * 2400 + 8320 + .. > 64 KiB at 4, fits at 2
]
BY_NAME = {c.name: c for c in CASES}
