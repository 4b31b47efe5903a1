"""QueueEvaluator_impl and the tabular drivers evalMC / qlearn / expSARSA in plain NumPy / Python, one rollout at a time (test
infrastructure), and the case list of the kernel matrix (tests/test_gpu_queue_drivers.py).

A restatement of documented behaviour (offsim4rl/evaluators/queue_evaluator.py:90-131, offsim4rl/agents/tabular.py:4-32, :71-191, :247-270,
include/offsim.h: offsim_eval_queue), not of the kernel's code:

  sampler    reset_sampler(seed): the initial rows in buffer order and the rows of every logged (z, a) pair in buffer order, each list
             shuffled by its own np.random.default_rng(seed).  reset(): the next initial row gives z.  step(a): the head of queue (z, a);
             a pair never logged: KeyError; the queue at its end: None, the state stays.
  action     A = gen.choice(nA, p=p) -- NumPy's own Generator.choice on the rollout's action stream
  behaviour  fixed pi[z]; epsilon-greedy / soft-greedy on Q[z] as tabular.py writes them; ties of the arg max: the first maximum, a
             RandomState's choice among the maxima (np.random.choice is the global RandomState's), or that with seed(episode0 + e) at the
             start of episode e
  update     Q-learning max(Q[z']); expected SARSA sum_k Q[z'][k] * pi[z'][k] from k = 0 upwards; td = r + gamma * nxt - Q[z, a];
             Q[z, a] = Q[z, a] + alpha * td; G = G + gamma ** t * r -- all in Python floats
  stop       the *_psrs drivers' rule where the reference's tabular drivers have none: an exhausted queue ends the run, lengths get every
             episode, Gs the completed ones with the cut-short one stored behind them

Everything comes back in the device's layout: state rows are z - min(z, 0), slots (z - z_lo) * nA + a, n_slots = nZ * nA, rows are caller
rows, outputs are cut by trace_cap / ep_cap / snap_cap and pre-filled as BatchedQueueEvaluator allocates them.
"""
import numpy as np

ST_OK, ST_EXHAUSTED, ST_NO_INIT, ST_KEYERROR = 0, 1, 2, 3  # include/offsim.h: OFFSIM_ST_*
EVALMC, QLEARN, EXPSARSA = 0, 1, 2                         # OFFSIM_TD_*
FIXED, EPS_GREEDY, SOFT_GREEDY = 0, 1, 2                   # OFFSIM_BEHAVIOUR_*
UNLIMITED = 1 << 62
GAMMA, ALPHA = 0.95, 0.2  # of every case of the matrix


class Log:
    def __init__(self, z, a, r, z_next, done, p_log, t0):
        self.z, self.a, self.z_next = (np.asarray(v, np.int64) for v in (z, a, z_next))
        self.done, self.t0 = np.asarray(done, bool), np.asarray(t0, bool)
        self.r, self.p_log = np.asarray(r), np.asarray(p_log)
        self.r64 = self.r.astype(np.float64)  # an exact widening
        self.N, self.nA = len(self.z), self.p_log.shape[1]
        self.z_lo = int(min(self.z.min(), self.z_next.min(), 0))
        hi = int(max(((self.z - self.z_lo) * self.nA + self.a).max(), ((self.z_next - self.z_lo) * self.nA).max()))
        self.nZ = hi // self.nA + 1
        self.n_slots = self.nZ * self.nA

    def arrays(self):
        return self.z, self.a, self.r, self.z_next, self.done, self.p_log, self.t0


class Sampler:
    """One QueueEvaluator_impl: its queue orders, heads and state (z as a value; None: no state)."""

    def __init__(self, log, seed):
        self.log = log
        shuffled = lambda rows: (lambda l: (np.random.default_rng(seed).shuffle(l), l)[1])([int(i) for i in rows])  # noqa: E731
        self.init_queue = shuffled(np.flatnonzero(log.t0))
        keys = sorted({(int(z), int(a)) for z, a in zip(log.z, log.a)})
        self.queues = {k: shuffled(np.flatnonzero((log.z == k[0]) & (log.a == k[1]))) for k in keys}
        self.head, self.init_head, self.cur = {k: 0 for k in keys}, 0, None

    def reset(self):
        if self.init_head >= len(self.init_queue):
            self.cur = None
            return None
        row = self.init_queue[self.init_head]
        self.init_head += 1
        self.cur = int(self.log.z[row])
        return row

    def step(self, a):
        q = self.queues[(self.cur, int(a))]  # KeyError: never logged
        if self.head[(self.cur, int(a))] >= len(q):
            return None
        row = q[self.head[(self.cur, int(a))]]
        self.head[(self.cur, int(a))] += 1
        self.cur = int(self.log.z_next[row])
        return row

    def cursors(self):
        c = np.zeros(self.log.n_slots, np.int64)
        for (z, a), v in self.head.items():
            c[(z - self.log.z_lo) * self.log.nA + a] = v
        return c


def rng_words(gen):
    """The stream row of a Generator: (state.hi, state.lo, inc.hi, inc.lo) as uint64."""
    s, m = gen.bit_generator.state["state"], (1 << 64) - 1
    return np.array([s["state"] >> 64, s["state"] & m, s["inc"] >> 64, s["inc"] & m], dtype=np.uint64)


def mt_words(rs):
    st = rs.get_state()
    return np.concatenate([np.asarray(st[1], np.uint32), np.array([st[2]], np.uint32)])


def behaviour_row(kind, q_row, eps, tie_rs):
    """(p, the action the greedy mass went to or -1) for tabular.py's epsilon_greedy_policy / soft_greedy_policy on one Q row."""
    nA = len(q_row)
    if kind == EPS_GREEDY:
        best = np.where(q_row == np.max(q_row))[0]
        a_star = int(best[0]) if tie_rs is None else int(tie_rs.choice(best))  # _random_argmax (tabular.py:4-5)
        p = np.ones(nA) * eps / nA
        p[a_star] = 1 - eps + eps / nA
        return p, a_star
    p = np.zeros(nA)
    p[np.where(np.isclose(q_row, np.max(q_row)))[0]] = 1
    return p / p.sum(), -1


def run(sm, gen, mode, pi, gamma, alpha=0.1, q=None, behaviour=FIXED, epsilon=0.0, alpha_ep=None, epsilon_ep=None, tie=None, episode0=0,
        n_episodes=None, trace_cap=0, ep_cap=0, snap_cap=0, snap_stride=1):
    """Runs sampler `sm` with the action stream `gen` (a Generator) from where they stand until the log or `n_episodes` ends; sm, gen, q
    (updated in place) and a RandomState `tie` keep the state a second call resumes from.  pi, q: [nZ, nA] by state row.
    tie: None (first maximum), a RandomState, or "episode".  Returns the row of every output of BatchedQueueEvaluator.eval_mc / eval_td."""
    lg, nA = sm.log, sm.log.nA
    pi = None if pi is None else np.asarray(pi, np.float64)
    gamma = float(gamma)
    n_episodes = UNLIMITED if n_episodes is None else int(n_episodes)
    o = dict(trace_row=np.full(trace_cap, -1, np.int32), trace_pop=np.zeros(trace_cap, np.int32), td_err=np.zeros(trace_cap, np.float64),
             beh_arg=np.zeros(trace_cap, np.int32), ep_g=np.zeros(ep_cap, np.float64), ep_len=np.zeros(ep_cap + 1, np.int32),
             q_snap=np.zeros((snap_cap, lg.nZ, nA), np.float64), obs_row=-(1 << 31))
    tie_rs = tie if isinstance(tie, np.random.RandomState) else (np.random.RandomState(0) if tie == "episode" else None)
    ep = n_len = steps = 0
    sum_g, status, terminate, begun = 0.0, ST_OK, False, False
    while ep < n_episodes and not terminate:
        if tie == "episode":
            tie_rs.seed((episode0 + ep) & 0xFFFFFFFF)  # np.random.seed(episode), before env.reset
            begun = True
        row0 = sm.reset()
        if row0 is None:
            status, o["obs_row"] = ST_NO_INIT, -1
            break
        o["obs_row"] = -2 - row0
        G, t, done = 0.0, 0, False
        while not done:
            S = sm.cur - lg.z_lo
            sched = lambda tab, const: float(const) if tab is None else float(tab[min(ep, len(tab) - 1)])  # noqa: E731
            if mode != EVALMC and behaviour != FIXED:
                p, best = behaviour_row(behaviour, q[S], sched(epsilon_ep, epsilon), tie_rs)
                if behaviour == EPS_GREEDY and steps < trace_cap:
                    o["beh_arg"][steps] = best
            else:
                p = pi[S]
            A = int(gen.choice(nA, p=p))
            if steps < trace_cap:
                o["trace_pop"][steps] = A
            try:
                row = sm.step(A)
            except KeyError:
                status, terminate = ST_KEYERROR, True
                break
            if row is None:
                status, terminate = ST_EXHAUSTED, True
                break
            o["obs_row"] = row
            r = float(lg.r64[row])
            if mode != EVALMC:
                S_ = sm.cur - lg.z_lo
                q_sa = float(q[S, A])
                if mode == QLEARN:
                    nxt = max(float(v) for v in q[S_])
                else:
                    nxt = 0.0
                    for k in range(nA):
                        nxt = nxt + float(q[S_, k]) * float(pi[S_, k])
                td = r + gamma * nxt - q_sa
                if steps < trace_cap:
                    o["td_err"][steps] = td
                q[S, A] = q_sa + sched(alpha_ep, alpha) * td
                if snap_cap and steps % snap_stride == 0 and steps // snap_stride < snap_cap:
                    o["q_snap"][steps // snap_stride] = q
            if steps < trace_cap:
                o["trace_row"][steps] = row
            G = G + gamma ** t * r
            t += 1
            steps += 1
            done = bool(lg.done[row])
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
    o.update(sum_g=sum_g, n_ep=ep, steps=steps, cand=steps, n_len=n_len, status=status, cursor=sm.cursors(), init_cursor=sm.init_head,
             cur_slot=-1 if sm.cur is None else (sm.cur - lg.z_lo) * nA, rng=rng_words(gen))
    if q is not None:
        o["q"] = q.copy()
    if tie_rs is not None and (tie != "episode" or begun):
        o["tie_mt"] = mt_words(tie_rs)
    return o


# ---------------------------------------------------------------------------------------------------------------------------------
# The LDS carve of csrc/eval_queue.hpp, restated (include/offsim.h: 4 rollouts per workgroup, then 2, then 1 while it exceeds 64 KiB;
# one rollout up to 160 KiB; beyond: refused)
# ---------------------------------------------------------------------------------------------------------------------------------
def lds_bytes(waves, n_slots, nA, have_pi=True, td=False):
    return ((waves * n_slots * 8 if td else 0) + (n_slots * 8 if have_pi else 0) + (waves * nA * 8 if td else 0) + (n_slots + 1) * 4
            + waves * n_slots * 4 + (waves * 624 * 4 if td else 0))


def launch_shape(n_slots, nA, have_pi=True, td=False):
    """(rollouts per workgroup, LDS bytes, refused)"""
    w = 4
    while w > 1 and lds_bytes(w, n_slots, nA, have_pi, td) > 65536:
        w //= 2
    b = lds_bytes(w, n_slots, nA, have_pi, td)
    return w, b, b > 160 * 1024


# ---------------------------------------------------------------------------------------------------------------------------------
# Logs and the case list
# ---------------------------------------------------------------------------------------------------------------------------------
def make_log(N, nZ, nA, seed, r32=False, neg_state=False, holes=0, n_slots=None, p_done=0.1, p_t0=0.1, no_init=False):
    """An iid log over nZ states.  holes: that many (z, a) pairs are never logged.  n_slots: filler rows from states beyond the nZ that are
    never reached (every third pair down from slot n_slots - 1) stretch the table to that many slots."""
    g = np.random.default_rng(seed)
    z, z_next, a = g.integers(0, nZ, N), g.integers(0, nZ, N), g.integers(0, nA, N)
    done = g.random(N) < p_done
    t0 = g.random(N) < p_t0
    t0[:3] = True
    if holes:
        pairs = g.permutation(nZ * nA)[:holes]
        keep = ~np.isin(z * nA + a, pairs)
        a = np.where(keep, a, (a + 1) % nA)
        keep = ~np.isin(z * nA + a, pairs)
        z, z_next, a, done, t0 = (v[keep] for v in (z, z_next, a, done, t0))
        N = len(z)
    if n_slots is not None:
        comp = np.arange(n_slots - 1, nZ * nA - 1, -3)
        comp = comp[: N // 2]
        f = len(comp)
        z[:f], a[:f], t0[:f] = comp // nA, comp % nA, False
    r = g.standard_normal(N)
    r = r.astype(np.float32) if r32 else r
    p_log = g.dirichlet(np.full(nA, 2.0), N)
    if no_init:
        t0[:] = False
    if neg_state:
        z, z_next = z - 1, z_next - 1
    return Log(z, a, r, z_next, done, p_log, t0)


class Case:
    def __init__(self, name, N=600, nZ=5, nA=5, R=5, log_seed=1, mode=EVALMC, behaviour=FIXED, tie=None, r32=False, neg_state=False, holes=0,
                 n_slots=None, pi_kind="dirichlet", n_episodes=None, sched=False, snap=False, q0="rand", epsilon=0.3, no_init=False, episode0=0,
                 have_pi=True):
        self.__dict__.update(locals())
        del self.__dict__["self"]
        self.seeds = [3 + 7 * i for i in range(R)]
        self.action_seeds = [100 + 11 * i for i in range(R)]
        self._log = self._host = None

    @property
    def log(self):
        if self._log is None:
            self._log = make_log(self.N, self.nZ, self.nA, self.log_seed, self.r32, self.neg_state, self.holes, self.n_slots, no_init=self.no_init)
        return self._log

    def pi(self):
        """[nZ, nA] by state row, or None"""
        if not self.have_pi:
            return None
        lg, g = self.log, np.random.default_rng(1000 + self.log_seed)
        pi = g.dirichlet(np.full(lg.nA, 1.5), lg.nZ)
        if self.pi_kind == "zeros" and lg.nA > 1:     # rows with zeros, and one-hot rows
            pi[:, 0] = 0.0
            pi /= pi.sum(1, keepdims=True)
            pi[1::3] = np.eye(lg.nA)[g.integers(1, lg.nA, len(pi[1::3]))]
        if self.pi_kind == "short":                   # every row sums to 1 - 1e-9: cdf /= cdf[-1] matters
            pi = pi / pi.sum(1, keepdims=True) * (1 - 1e-9)
        return pi

    def q_init(self):
        lg = self.log
        if self.q0 == "zero":
            return np.zeros((self.R, lg.nZ, lg.nA))
        return np.random.default_rng(7).standard_normal((self.R, lg.nZ, lg.nA)) * 0.1

    @property
    def alpha_ep(self):
        return np.array([0.5 / (1.0 + 0.1 * e) for e in range(40)]) if self.sched else None

    @property
    def epsilon_ep(self):
        return np.array([0.9 / (1.0 + 0.2 * e) for e in range(40)]) if self.sched and self.behaviour == EPS_GREEDY else None

    def tie_states(self):
        """the [R, 625] MT19937 states of tie = "stream" """
        return np.stack([mt_words(np.random.RandomState(500 + i)) for i in range(self.R)])

    def kw(self):
        return dict(n_episodes=self.n_episodes, trace_cap=self.log.N + 1, ep_cap=self.log.N + 1, snap_cap=16 if self.snap else 0,
                    snap_stride=3 if self.snap else 1)

    def td_kw(self):
        return dict(behaviour=self.behaviour, epsilon=self.epsilon, alpha_ep=self.alpha_ep, epsilon_ep=self.epsilon_ep, episode0=self.episode0)

    def host_tie(self, i):
        return np.random.RandomState(500 + i) if self.tie == "stream" else self.tie

    def host(self):
        """The mirror's outputs per rollout (computed once)."""
        if self._host is None:
            pi, q0 = self.pi(), self.q_init()
            outs = []
            for i, (s, sa) in enumerate(zip(self.seeds, self.action_seeds)):
                sm, gen = Sampler(self.log, s), np.random.default_rng(sa)
                if self.mode == EVALMC:
                    outs.append(run(sm, gen, EVALMC, pi, GAMMA, **self.kw()))
                else:
                    outs.append(run(sm, gen, self.mode, pi, GAMMA, alpha=ALPHA, q=q0[i].copy(), tie=self.host_tie(i), **self.td_kw(), **self.kw()))
            self._host = outs
        return self._host


# The launch shapes with the learner's Q and nA = 5: bytes(w) = n (12 w + 12) + 4 + 2536 w, so 4 rollouts fit up to n = 923, 2 up to
# n = 1679, 1 within 64 KiB up to n = 2624 and within 160 KiB up to n = 6720 (n a multiple of 5).
LDS_SLOTS = {"waves4": 920, "waves2": 925, "waves1": 1680, "big": 2625, "big-last": 6720, "refused": 6725}
_Q = dict(mode=QLEARN)
CASES = [
    Case("evalmc-R5"),
    Case("evalmc-R1-nA1", R=1, nA=1, nZ=6, N=300, log_seed=2),
    Case("evalmc-R3-nA2-r32", R=3, nA=2, nZ=7, r32=True, log_seed=3),
    Case("evalmc-R9-nA70", R=9, nA=70, nZ=3, N=2000, log_seed=4),
    Case("evalmc-neg-state-zeros-R5", neg_state=True, pi_kind="zeros", log_seed=5),
    Case("evalmc-short-rows-R5", pi_kind="short", log_seed=6),
    Case("evalmc-holes-R9", R=9, holes=2, log_seed=7),
    Case("evalmc-no-init-R3", R=3, no_init=True, log_seed=8),
    Case("evalmc-max-episodes-R5", n_episodes=2, log_seed=9),
    Case("evalmc-waves2-R9", R=9, N=2000, n_slots=3275, log_seed=10),  # 28 n + 4 > 64 KiB at 4 rollouts from n = 2341 on, 20 n + 4 at 2 from 3277 on
    Case("qlearn-fixed-R5", log_seed=11, snap=True, **_Q),
    Case("qlearn-fixed-r32-sched-R3", R=3, r32=True, sched=True, log_seed=12, **_Q),
    Case("qlearn-eps-first-q0-R5", behaviour=EPS_GREEDY, q0="zero", have_pi=False, log_seed=13, **_Q),
    Case("qlearn-eps-stream-q0-R5", behaviour=EPS_GREEDY, tie="stream", q0="zero", have_pi=False, log_seed=14, **_Q),
    Case("qlearn-eps-episode-q0-R9", R=9, behaviour=EPS_GREEDY, tie="episode", q0="zero", have_pi=False, sched=True, log_seed=15, **_Q),
    Case("qlearn-eps-episode0-nA70-R3", R=3, nA=70, nZ=3, N=2000, behaviour=EPS_GREEDY, tie="episode", episode0=(1 << 32) - 2, q0="zero", log_seed=16,
         **_Q),
    Case("qlearn-greedy-episode-R5", behaviour=EPS_GREEDY, epsilon=0.0, tie="episode", q0="zero", log_seed=17, **_Q),
    Case("qlearn-soft-episode-neg-state-R5", behaviour=SOFT_GREEDY, tie="episode", q0="zero", neg_state=True, snap=True, log_seed=18, **_Q),
    Case("qlearn-fixed-episode-holes-R5", tie="episode", holes=3, log_seed=19, **_Q),
    Case("qlearn-max-episodes-nA2-R9", R=9, nA=2, nZ=7, n_episodes=3, log_seed=20, **_Q),
    Case("expsarsa-R5", mode=EXPSARSA, snap=True, log_seed=21),
    Case("expsarsa-zeros-sched-R1", mode=EXPSARSA, R=1, pi_kind="zeros", sched=True, log_seed=22),
    Case("lds-waves4-R5", N=2000, n_slots=LDS_SLOTS["waves4"], log_seed=23, **_Q),
    Case("lds-waves2-R5", N=2000, n_slots=LDS_SLOTS["waves2"], log_seed=24, **_Q),
    Case("lds-waves1-R3", R=3, N=2000, n_slots=LDS_SLOTS["waves1"], log_seed=25, **_Q),
    Case("lds-big-R3", R=3, N=2000, n_slots=LDS_SLOTS["big"], behaviour=EPS_GREEDY, tie="episode", log_seed=26, **_Q),
]
BY_NAME = {c.name: c for c in CASES}
