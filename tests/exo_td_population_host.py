"""A population of TD learners on PSRS_Exo on the host (test infrastructure): learner (l, j) of a case is a plain Python loop on its own
exo_host.Sampler of seed j, with its own Q and tie stream, under learner l's hyper-parameters -- nothing is shared between learners but
the log.  The environment and the bookkeeping are exo_host.run's (tests/exo_host.py); the behaviour rules and the MT19937 tie stream are
stated as td_host.run states them (tests/td_host.py): FIXED rejects against pi[o]; EPS_GREEDY puts 1 - eps + eps / nA on
RandomState.choice(np.where(q == q.max())[0]) of the learner's own stream (which draws only on a tie; without a stream: the first
maximum) and eps / nA elsewhere; SOFT_GREEDY is uniform over np.isclose(q, q.max()); all on the Q row of the current OBSERVATION, formed
BEFORE the step (psrs.py:158), so a step that then finds a queue missing has drawn its tie.

Also here: the LDS carve and launch shape of offsim_eval_td_exo_pop restated (include/offsim.h), the case list of
tests/test_gpu_exo_td_population.py, and the learning curves as a Python-float loop (td_population_host.curves).

Everything comes back stacked as BatchedPSRSExo.eval_td_population returns it: [L, S, ...].
"""
import functools
import os
import sys
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exo_host as X  # noqa: E402
from td_population_host import curves  # noqa: E402,F401

QLEARN, EXPSARSA = X.QLEARN, X.EXPSARSA
FIXED, EPS_GREEDY, SOFT_GREEDY = 0, 1, 2  # include/offsim.h: OFFSIM_BEHAVIOUR_*
F, E, SOFT = FIXED, EPS_GREEDY, SOFT_GREEDY
N_L, N_S = 3, 5  # S is a multiple of no launch shape's rollouts per workgroup (4, 2: a partly filled workgroup; 1)


def tie_state(words):
    """np.random.RandomState standing at the 624 words + position `words` [625]; None -> None"""
    if words is None:
        return None
    w = np.asarray(words).view(np.uint32).reshape(625) if np.asarray(words).dtype.itemsize == 4 else np.asarray(words, np.uint32).reshape(625)
    rs = np.random.RandomState()
    rs.set_state(("MT19937", w[:624].copy(), int(w[624])))
    return rs


def tie_words(rs):
    st = rs.get_state()
    return np.concatenate([np.asarray(st[1], np.uint32), np.array([st[2]], np.uint32)])


def _sched(table, const, ep):
    return float(const) if table is None else float(table[min(ep, len(table) - 1)])


def run(sm, mode, pi, obs_of, gamma, alpha, q, behaviour=FIXED, epsilon=0.0, alpha_ep=None, epsilon_ep=None, rs=None, n_episodes=None,
        reseed="episode", episode0=0, trace_cap=0, ep_cap=0, snap_cap=0, snap_stride=1):
    """Runs learner (q [n_obs, nA] updated in place, tie stream rs advanced in place) on sampler `sm` from where it stands until its log or
    `n_episodes` ends.  pi [n_obs, nA] f64, obs_of [ns, nx].  Returns the row of every output of BatchedPSRSExo.eval_td_population."""
    lg, nA = sm.log, sm.log.nA
    pi = np.asarray(pi, np.float64)
    n_obs, gamma = pi.shape[0], float(gamma)
    n_episodes = X.UNLIMITED if n_episodes is None else int(n_episodes)
    snap_stride = max(int(snap_stride), 1)
    o = dict(trace_row=np.full(trace_cap, -1, np.int32), trace_row_x=np.full(trace_cap, -1, np.int32), trace_pop=np.zeros(trace_cap, np.int32),
             td_err=np.zeros(trace_cap, np.float64), beh_arg=np.zeros(trace_cap, np.int32), ep_g=np.zeros(ep_cap, np.float64),
             ep_len=np.zeros(ep_cap + 1, np.int32), q_snap=np.zeros((snap_cap, n_obs, nA), np.float64), last=np.full(3, -1, np.int32))

    def row_of(cur):
        i, j = cur[0] - lg.s_base, cur[1] - lg.x_base
        v = int(obs_of[i, j]) if 0 <= i < lg.ns and 0 <= j < lg.nx else -1
        return v if 0 <= v < n_obs else -1
    ep = n_len = steps = cand = 0
    sum_g, status, terminate = 0.0, X.ST_OK, False
    while ep < n_episodes and not terminate:
        row0 = sm.reset(episode0 + ep if reseed == "episode" else None)
        if row0 is None:
            status = X.ST_NO_INIT
            break
        o["last"][:] = (-1, -1, row0)
        G, t, done = 0.0, 0, False
        while not done:
            oc = row_of(sm.cur)
            if oc < 0:
                status, terminate = X.ST_KEYERROR, True
                break
            if behaviour == FIXED:
                p = pi[oc]
            elif behaviour == EPS_GREEDY:
                tied = np.where(q[oc] == q[oc].max())[0]
                best = int(tied[0]) if rs is None else int(rs.choice(tied))
                eps = _sched(epsilon_ep, epsilon, ep)
                p = np.full(nA, eps / nA)
                p[best] = 1 - eps + eps / nA
                if steps < trace_cap:
                    o["beh_arg"][steps] = best
            else:
                close = np.isclose(q[oc], q[oc].max())
                p = np.where(close, 1.0 / int(close.sum()), 0.0)
            try:
                r_s, r_x, n = sm.step(p)
            except KeyError:
                status, terminate = X.ST_KEYERROR, True
                break
            cand += n
            if r_s is None:
                status, terminate = X.ST_EXHAUSTED, True
                break
            o["last"][:] = (r_s, r_x, -1)
            A, r = int(lg.a[r_s]), float(lg.r64[r_s])
            on = row_of(sm.cur)
            if on < 0:
                status, terminate = X.ST_KEYERROR, True
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
            q[oc, A] = q_sa + _sched(alpha_ep, alpha, ep) * td
            if snap_cap and steps % snap_stride == 0 and steps // snap_stride < snap_cap:
                o["q_snap"][steps // snap_stride] = q
            if steps < trace_cap:
                o["trace_row"][steps], o["trace_row_x"][steps], o["trace_pop"][steps] = r_s, r_x, n
            G = G + gamma ** t * r
            t += 1
            steps += 1
            done = bool(lg.done[r_s])
        if status == X.ST_KEYERROR:
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
    o.update(q=q.copy(), sum_g=sum_g, n_ep=ep, steps=steps, cand=cand, n_len=n_len, status=status, cursor_s=cs, cursor_x=cx, init_cursor=sm.init_head,
             cur_s=sm.slots()[0], cur_x=sm.slots()[1], draws=sm.stream.count, tie_mt=None if rs is None else tie_words(rs))
    return o


# ---------------------------------------------------------------------------------------------------------------------------------
# The LDS carve of offsim_eval_td_exo_pop, restated (include/offsim.h): offsim_eval_mc_exo's learner carve (exo_host.lds_bytes, td) plus,
# behind it, 8 bytes of alignment, nA f64 per rollout for the behaviour distribution and 624 u32 per rollout for the tie stream; 4
# rollouts per workgroup, then 2, then 1 while it exceeds 64 KiB; one rollout up to 160 KiB; beyond: refused.  A workgroup holds rollouts
# of one learner: L * ceil(S / rollouts per workgroup) workgroups.
# ---------------------------------------------------------------------------------------------------------------------------------
def lds_bytes(waves, ns, nx, n_obs, nA):
    return X.lds_bytes(waves, ns, nx, n_obs, nA, 8, True) + 8 + waves * nA * 8 + waves * 624 * 4


def launch_shape(ns, nx, n_obs, nA, L=N_L, S=N_S):
    """(rollouts per workgroup, LDS bytes, refused, workgroups)"""
    w = 4
    while w > 1 and lds_bytes(w, ns, nx, n_obs, nA) > 65536:
        w //= 2
    b = lds_bytes(w, ns, nx, n_obs, nA)
    return w, b, b > 160 * 1024, L * ((S + w - 1) // w)


def first_n_obs_with(waves, big, ns, nx, nA):
    """The smallest n_obs whose launch has `waves` rollouts per workgroup (big: one rollout above 64 KiB), as exo_host.first_n_obs_with."""
    n = 1
    while True:
        w, b, _, _ = launch_shape(ns, nx, n, nA)
        if w == waves and (b > 65536) == big:
            return n
        n += 1


# ---------------------------------------------------------------------------------------------------------------------------------
# The case list: exo_host.Case's default log (N = 500, nS = 5, nX = 2, nA = 3), L = 3 learners that agree in no hyper-parameter, S = 5 seeds
# ---------------------------------------------------------------------------------------------------------------------------------
_SCHED_A = ((0.5, 0.25, 0.125), (0.4, 0.2, 0.1), (0.3, 0.3, 0.05))
_SCHED_E = ((0.9, 0.6, 0.3), (0.8, 0.4, 0.0), (0.5, 0.5, 0.2))


@dataclass(frozen=True)
class PopCase:
    name: str
    mode: int = QLEARN
    behaviour: Tuple[int, ...] = (E, E, E)
    alpha: Tuple[float, ...] = (0.05, 0.2, 0.5)
    epsilon: Tuple[float, ...] = (0.1, 0.3, 0.6)
    gamma: Tuple[float, ...] = (0.9, 0.97, 1.0)
    alpha_ep: Optional[Tuple[Tuple[float, ...], ...]] = None
    epsilon_ep: Optional[Tuple[Tuple[float, ...], ...]] = None
    pi_per_learner: bool = False
    mt: str = "none"              # none / fresh / mid (position 600 of 624: a twist happens inside the run)
    reseed: str = "episode"
    stream: str = "pcg64"
    episode0: int = 0
    trace_cap: Optional[int] = None
    ep_cap: Optional[int] = None
    snap_cap: int = 0
    snap_stride: int = 1
    resume_k: Optional[int] = None
    n_obs_pad: Optional[int] = None
    log_seed: int = 1
    curve: bool = True

    @property
    def seeds(self):
        return [3 + 7 * j for j in range(N_S)]

    @property
    def log(self):
        return _log(self.log_seed)

    def tables(self):
        """(obs_of [ns, nx], n_obs): o = 2 s + x, padded with rows no pair maps to (they size the LDS carve)"""
        lg = self.log
        obs_of, ids = lg.obs_of(lambda s, x: (s - lg.s_base) * lg.nx + (x - lg.x_base), lg.ns * lg.nx)
        return obs_of, len(ids) if self.n_obs_pad is None else self.n_obs_pad

    @property
    def shape(self):
        lg = self.log
        return launch_shape(lg.ns, lg.nx, self.tables()[1], lg.nA)

    def caps(self):
        return (self.log.N + 1 if self.trace_cap is None else self.trace_cap, int(self.log.t0.sum()) + 1 if self.ep_cap is None else self.ep_cap)


@functools.lru_cache(maxsize=None)
def _log(seed):
    return X.make_log(500, 5, 2, 3, seed)


def pi_of(case):
    """[n_obs, nA] shared, or [L, n_obs, nA]: learner l's own mixture of a Dirichlet table and the uniform one"""
    n_obs, nA = case.tables()[1], case.log.nA
    d = lambda seed: np.random.default_rng(seed).dirichlet(np.full(nA, 1.5), n_obs)  # noqa: E731
    if not case.pi_per_learner:
        return 0.5 * d(9 + case.log_seed) + 0.5 / nA
    return np.stack([(0.3 + 0.2 * l) * d(20 + 3 * l + case.log_seed) + (0.7 - 0.2 * l) / nA for l in range(N_L)])


def q_init_of(case):
    """[L, S, n_obs, nA]: zeros (ties on every first visit)"""
    return np.zeros((N_L, N_S, case.tables()[1], case.log.nA))


def mt_of(case):
    """[L, S, 625] uint32 tie streams or None: (l, j) starts from RandomState(7000 + 31 l + 17 j); `mid` first takes 600 words out of it."""
    if case.mt == "none":
        return None
    out = np.zeros((N_L, N_S, 625), np.uint32)
    for l in range(N_L):
        for j in range(N_S):
            rs = np.random.RandomState(7000 + 31 * l + 17 * j)
            if case.mt == "mid":
                rs.bytes(4 * 600)
            out[l, j] = tie_words(rs)
    return out


def learner_args(case, l):
    trace_cap, ep_cap = case.caps()
    return dict(mode=case.mode, gamma=case.gamma[l], alpha=case.alpha[l], behaviour=case.behaviour[l], epsilon=case.epsilon[l],
                alpha_ep=None if case.alpha_ep is None else np.array(case.alpha_ep[l]),
                epsilon_ep=None if case.epsilon_ep is None else np.array(case.epsilon_ep[l]),
                trace_cap=trace_cap, ep_cap=ep_cap, snap_cap=case.snap_cap, snap_stride=case.snap_stride, reseed=case.reseed)


def population_args(case):
    """The arguments of BatchedPSRSExo.eval_td_population (obs_of apart)."""
    trace_cap, ep_cap = case.caps()
    return dict(mode=case.mode, alpha=np.array(case.alpha), gamma=np.array(case.gamma), behaviour=np.array(case.behaviour), epsilon=np.array(case.epsilon),
                pi_obs=pi_of(case), alpha_ep=None if case.alpha_ep is None else np.array(case.alpha_ep),
                epsilon_ep=None if case.epsilon_ep is None else np.array(case.epsilon_ep), trace_cap=trace_cap, ep_cap=ep_cap,
                snap_cap=case.snap_cap, snap_stride=case.snap_stride, reseed=case.reseed)


_STACK = dict(q=np.float64, sum_g=np.float64, n_ep=np.int64, steps=np.int64, cand=np.int64, n_len=np.int64, status=np.int32, trace_row=np.int32,
              trace_row_x=np.int32, trace_pop=np.int32, td_err=np.float64, beh_arg=np.int32, ep_g=np.float64, ep_len=np.int32, q_snap=np.float64,
              last=np.int32, cursor_s=np.int64, cursor_x=np.int64, init_cursor=np.int64, cur_s=np.int64, cur_x=np.int64, draws=np.int64)


def _stack(rows):
    out = {k: np.stack([np.stack([np.asarray(r[k], dt) for r in row]) for row in rows]) for k, dt in _STACK.items()}
    out["tie_mt"] = None if rows[0][0]["tie_mt"] is None else np.stack([np.stack([r["tie_mt"] for r in row]) for row in rows])
    return out


@functools.lru_cache(maxsize=None)
def host(case):
    """The host loop's outputs of the calls of the case, each {key: [L, S, ...]}: [one call], or [the first resume_k episodes, the rest
    (episode0 advanced by resume_k under the per-episode reseed)]."""
    lg, q0, mt, pi = case.log, q_init_of(case), mt_of(case), pi_of(case)
    obs_of, _ = case.tables()
    sms = [[X.Sampler(lg, s, case.stream) for s in case.seeds] for _ in range(N_L)]
    qs = [[q0[l, j].copy() for j in range(N_S)] for l in range(N_L)]
    rss = [[None if mt is None else tie_state(mt[l, j]) for j in range(N_S)] for l in range(N_L)]
    calls = [(None, case.episode0)] if case.resume_k is None else [(case.resume_k, case.episode0), (None, case.episode0 + case.resume_k)]
    return [_stack([[run(sms[l][j], pi=pi[l] if case.pi_per_learner else pi, obs_of=obs_of, q=qs[l][j], rs=rss[l][j], n_episodes=n, episode0=e0,
                         **learner_args(case, l)) for j in range(N_S)] for l in range(N_L)]) for n, e0 in calls]


def _pad(waves, big):
    lg = _log(1)
    return first_n_obs_with(waves, big, lg.ns, lg.nx, lg.nA)


CASES = [
    PopCase("qlearn-every-behaviour-mt-fresh", behaviour=(F, E, SOFT), mt="fresh"),
    PopCase("qlearn-eps-mt-mid", mt="mid", log_seed=2),
    PopCase("qlearn-eps-first-maximum", log_seed=3),
    PopCase("qlearn-greedy-schedules", epsilon=(0.0, 0.3, 0.6), alpha_ep=_SCHED_A, epsilon_ep=_SCHED_E, mt="fresh", log_seed=4),
    PopCase("qlearn-eps-none-pcg-episode0", reseed="none", episode0=0, mt="fresh", log_seed=5),
    PopCase("qlearn-eps-none-philox", reseed="none", stream="philox", mt="fresh", log_seed=6),
    PopCase("qlearn-eps-episode0", episode0=(1 << 33) + 11, mt="mid", log_seed=7),
    PopCase("expsarsa-own-pi-fixed", mode=EXPSARSA, behaviour=(F, F, F), pi_per_learner=True, log_seed=8),
    PopCase("expsarsa-own-pi-every-behaviour", mode=EXPSARSA, behaviour=(E, SOFT, F), pi_per_learner=True, mt="mid", log_seed=9),
    PopCase("expsarsa-shared-pi-soft", mode=EXPSARSA, behaviour=(SOFT, SOFT, E), log_seed=10),
    PopCase("caps-smaller-than-the-run", mt="fresh", trace_cap=50, ep_cap=2, snap_cap=7, snap_stride=3, log_seed=11, curve=False),
    PopCase("resume-after-2-episodes", mt="fresh", resume_k=2, snap_cap=30, log_seed=12, curve=False),
    PopCase("lds-waves2", mt="fresh", n_obs_pad=_pad(2, False), log_seed=13),
    PopCase("lds-waves1", mt="mid", n_obs_pad=_pad(1, False), log_seed=14),
    PopCase("lds-above-64k", mt="fresh", n_obs_pad=_pad(1, True), snap_cap=3, snap_stride=5, log_seed=15),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
CURVE_CASES = [c for c in CASES if c.curve]
