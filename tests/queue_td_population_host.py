"""A population of TD learners on QueueEvaluator on the host (test infrastructure): rollout (l, j) of a case is tests/queue_host.run -- the
plain Python loop over QueueEvaluator_impl and the reference's qlearn / expSARSA -- on its own Sampler(log, seeds[j]) and its own
default_rng(action_seeds[j]), with its own Q and tie stream, under learner l's setting.  Nothing is shared between rollouts but the log.

Also here: the launch shape of offsim_eval_queue_pop restated (include/offsim.h: offsim_eval_queue's learner carve, a workgroup holds
rollouts of one learner), the case list of tests/test_gpu_queue_td_population.py, and the learning curves as a Python-float loop in seed
order (td_population_host.curves).

Everything comes back stacked as BatchedQueueEvaluator.eval_td_population returns it: [L, S, ...], tables by state row z - z_lo.
"""
import functools
import os
import sys
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import queue_host as Q  # noqa: E402
from td_population_host import curves  # noqa: E402,F401

QLEARN, EXPSARSA = Q.QLEARN, Q.EXPSARSA
F, E, SOFT = Q.FIXED, Q.EPS_GREEDY, Q.SOFT_GREEDY
ST_OK, ST_EXHAUSTED, ST_NO_INIT, ST_KEYERROR = Q.ST_OK, Q.ST_EXHAUSTED, Q.ST_NO_INIT, Q.ST_KEYERROR
LDS_SLOTS = Q.LDS_SLOTS
N_SCHED = 40


def launch_shape(n_slots, nA, L, S, have_pi=True):
    """(rollouts per workgroup, LDS bytes, refused, workgroups): queue_host.launch_shape with the learner, L * ceil(S / rollouts per workgroup)"""
    w, b, refused = Q.launch_shape(n_slots, nA, have_pi, True)
    return w, b, refused, L * ((S + w - 1) // w)


@dataclass(frozen=True)
class PopCase:
    name: str
    L: int = 3
    S: int = 5
    N: int = 600
    nZ: int = 5
    nA: int = 5
    log_seed: int = 1
    mode: int = QLEARN
    behaviour: Tuple[int, ...] = (E, E, E)
    alpha: Tuple[float, ...] = (0.05, 0.2, 0.5)
    epsilon: Tuple[float, ...] = (0.1, 0.3, 0.6)
    gamma: Tuple[float, ...] = (0.9, 0.97, 1.0)
    sched: bool = False           # learner 0 has alpha(episode) and epsilon(episode); the others keep their constants
    pi_per_learner: bool = False
    tie: str = "first"            # first / fresh / mid (position 600 of 624: a twist happens inside the run) / episode
    episode0: int = 0
    q0: str = "zero"              # zero (every row a tie) / rand
    neg_state: bool = False
    holes: int = 0
    n_slots: Optional[int] = None
    n_episodes: Optional[int] = None
    r32: bool = False
    snap: bool = False

    @property
    def seeds(self):
        return [3 + 7 * j for j in range(self.S)]

    @property
    def action_seeds(self):
        return [100 + 11 * j for j in range(self.S)]

    @property
    def log(self):
        return _log(self.N, self.nZ, self.nA, self.log_seed, self.r32, self.neg_state, self.holes, self.n_slots)

    @property
    def shape(self):
        return launch_shape(self.log.n_slots, self.log.nA, self.L, self.S)

    def caps(self):
        """(trace_cap, ep_cap, snap_cap, snap_stride)"""
        return self.log.N + 1, self.log.N + 1, 16 if self.snap else 0, 3 if self.snap else 1

    def streams(self):
        return self.tie in ("fresh", "mid")


@functools.lru_cache(maxsize=None)
def _log(N, nZ, nA, seed, r32, neg_state, holes, n_slots):
    return Q.make_log(N, nZ, nA, seed, r32, neg_state, holes, n_slots)


def pi_of(case):
    """[nZ, nA] shared, or [L, nZ, nA]: learner l's own mixture of a Dirichlet table and the uniform one (by state row)"""
    lg = case.log
    d = lambda seed: np.random.default_rng(seed).dirichlet(np.full(lg.nA, 1.5), lg.nZ)  # noqa: E731
    if not case.pi_per_learner:
        return 0.5 * d(9 + case.log_seed) + 0.5 / lg.nA
    return np.stack([(0.3 + 0.2 * l) * d(20 + 3 * l + case.log_seed) + (0.7 - 0.2 * l) / lg.nA for l in range(case.L)])


def q_init_of(case):
    """[L, S, nZ, nA]"""
    lg = case.log
    if case.q0 == "zero":
        return np.zeros((case.L, case.S, lg.nZ, lg.nA))
    return np.random.default_rng(7).standard_normal((case.L, case.S, lg.nZ, lg.nA)) * 0.1


def schedules(case):
    """(alpha_ep, epsilon_ep) [L, N_SCHED] or (None, None): learner 0's schedules, constant rows for the others"""
    if not case.sched:
        return None, None
    a = np.stack([np.array([0.5 / (1.0 + 0.1 * e) for e in range(N_SCHED)])] + [np.full(N_SCHED, case.alpha[l]) for l in range(1, case.L)])
    e = np.stack([np.array([0.9 / (1.0 + 0.2 * e) for e in range(N_SCHED)])] + [np.full(N_SCHED, case.epsilon[l]) for l in range(1, case.L)])
    return a, e


def mt_of(case):
    """[L, S, 625] uint32 tie streams or None: (l, j) starts from RandomState(7000 + 31 l + 17 j); `mid` first takes 600 words out of it."""
    if not case.streams():
        return None
    out = np.zeros((case.L, case.S, 625), np.uint32)
    for l in range(case.L):
        for j in range(case.S):
            rs = np.random.RandomState(7000 + 31 * l + 17 * j)
            if case.tie == "mid":
                rs.bytes(4 * 600)
            out[l, j] = Q.mt_words(rs)
    return out


def tie_state(words):
    rs = np.random.RandomState()
    w = np.asarray(words, np.uint32).reshape(625)
    rs.set_state(("MT19937", w[:624].copy(), int(w[624])))
    return rs


def learner_args(case, l):
    """learner l's own setting as queue_host.run takes it (a constant where the learner has no schedule)"""
    a_ep, e_ep = schedules(case)
    own = case.sched and l == 0
    return dict(alpha=case.alpha[l], behaviour=case.behaviour[l], epsilon=case.epsilon[l], alpha_ep=a_ep[l] if own else None,
                epsilon_ep=e_ep[l] if own else None)


def population_args(case):
    """The arguments of BatchedQueueEvaluator.eval_td_population (q, tie, episode0 and the episode limit apart)."""
    a_ep, e_ep = schedules(case)
    trace_cap, ep_cap, snap_cap, snap_stride = case.caps()
    return dict(mode=case.mode, alpha=np.array(case.alpha), gamma=np.array(case.gamma), behaviour=np.array(case.behaviour), epsilon=np.array(case.epsilon),
                pi=pi_of(case), alpha_ep=a_ep, epsilon_ep=e_ep, trace_cap=trace_cap, ep_cap=ep_cap, snap_cap=snap_cap, snap_stride=snap_stride)


_STACK = dict(q=np.float64, sum_g=np.float64, n_ep=np.int64, steps=np.int64, cand=np.int64, n_len=np.int64, status=np.int32, obs_row=np.int32,
              trace_row=np.int32, trace_pop=np.int32, td_err=np.float64, beh_arg=np.int32, ep_g=np.float64, ep_len=np.int32, q_snap=np.float64,
              cursor=np.int64, init_cursor=np.int64, cur_slot=np.int64, rng=np.uint64)


def run_population(case, n_episodes="case", snap_all=False):
    """{key: [L, S, ...]}: every rollout (l, j) by queue_host.run on its own sampler, action stream, Q and tie stream."""
    lg, q0, mt, pi = case.log, q_init_of(case), mt_of(case), pi_of(case)
    trace_cap, ep_cap, snap_cap, snap_stride = case.caps()
    if snap_all:
        snap_cap, snap_stride = lg.N + 1, 1
    rows = []
    for l in range(case.L):
        row = []
        for j in range(case.S):
            tie = "episode" if case.tie == "episode" else tie_state(mt[l, j]) if mt is not None else None
            row.append(Q.run(Q.Sampler(lg, case.seeds[j]), np.random.default_rng(case.action_seeds[j]), case.mode, pi[l] if case.pi_per_learner else pi,
                             case.gamma[l], q=q0[l, j].copy(), tie=tie, episode0=case.episode0, n_episodes=case.n_episodes if n_episodes == "case" else n_episodes,
                             trace_cap=trace_cap, ep_cap=ep_cap, snap_cap=snap_cap, snap_stride=snap_stride, **learner_args(case, l)))
        rows.append(row)
    out = {k: np.stack([np.stack([np.asarray(r[k], dt) for r in row]) for row in rows]) for k, dt in _STACK.items()}
    out["tie_mt"] = np.stack([np.stack([r["tie_mt"] for r in row]) for row in rows]) if case.tie != "first" else None
    return out


@functools.lru_cache(maxsize=None)
def host(case):
    """The mirror's outputs of the case (computed once, shared by the tests, never written to)."""
    out = run_population(case)
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out


def ties_after_the_first_step(case, l, j, m):
    """How many steps s >= 1 of rollout (l, j) found two or more maxima in the Q row of their state; m: run_population(case, snap_all=True)"""
    lg, n = case.log, 0
    for s in range(1, int(m["steps"][l, j])):
        row = m["q_snap"][l, j, s - 1, int(lg.z[m["trace_row"][l, j, s]]) - lg.z_lo]
        n += int((row == row.max()).sum() >= 2)
    return n


_LDS = dict(N=2000, S=3)
CASES = [
    PopCase("qlearn-fixed", behaviour=(F, F, F), q0="rand", snap=True),
    PopCase("qlearn-eps-first", log_seed=2),
    PopCase("qlearn-greedy-fresh", epsilon=(0.0, 0.0, 0.0), tie="fresh", log_seed=3),
    PopCase("qlearn-soft-episode", behaviour=(SOFT, SOFT, SOFT), tie="episode", log_seed=4),
    PopCase("qlearn-every-behaviour-fresh", behaviour=(F, E, SOFT), tie="fresh", log_seed=5, snap=True),
    PopCase("qlearn-every-behaviour-greedy-episode", L=4, behaviour=(F, E, SOFT, E), alpha=(0.05, 0.2, 0.5, 0.3), epsilon=(0.1, 0.3, 0.6, 0.0),
            gamma=(0.9, 0.97, 1.0, 0.8), tie="episode", log_seed=6),
    PopCase("expsarsa-own-pi", mode=EXPSARSA, behaviour=(F, F, F), pi_per_learner=True, q0="rand", log_seed=7, snap=True),
    PopCase("expsarsa-shared-pi", mode=EXPSARSA, behaviour=(F, F, F), log_seed=8),
    PopCase("qlearn-eps-schedules-episode", sched=True, tie="episode", log_seed=9),
    PopCase("qlearn-eps-mid", tie="mid", log_seed=10),
    PopCase("qlearn-eps-episode0", tie="episode", episode0=(1 << 32) - 2, log_seed=11),
    PopCase("qlearn-eps-rand-q-fresh", q0="rand", tie="fresh", log_seed=12),
    PopCase("qlearn-eps-nA70-episode", nA=70, nZ=3, N=2000, tie="episode", log_seed=13),
    PopCase("qlearn-every-behaviour-neg-state", behaviour=(SOFT, F, E), neg_state=True, tie="episode", log_seed=14),
    PopCase("qlearn-eps-holes", holes=3, tie="fresh", log_seed=15),
    PopCase("qlearn-eps-two-episodes", n_episodes=2, tie="episode", log_seed=16),
    PopCase("qlearn-eps-r32", r32=True, tie="fresh", log_seed=17),
    PopCase("qlearn-eps-L1-S1", L=1, S=1, alpha=(0.2,), epsilon=(0.3,), gamma=(0.95,), behaviour=(E,), tie="episode", log_seed=18),
    PopCase("qlearn-every-behaviour-L2-S9", L=2, S=9, alpha=(0.1, 0.4), epsilon=(0.2, 0.5), gamma=(0.9, 0.99), behaviour=(E, SOFT), tie="fresh", log_seed=19),
    PopCase("lds-waves4", n_slots=LDS_SLOTS["waves4"], tie="episode", log_seed=23, **_LDS),
    PopCase("lds-waves2", n_slots=LDS_SLOTS["waves2"], tie="mid", log_seed=24, **_LDS),
    PopCase("lds-waves1", n_slots=LDS_SLOTS["waves1"], behaviour=(F, E, SOFT), tie="fresh", log_seed=25, **_LDS),
    PopCase("lds-big", n_slots=LDS_SLOTS["big"], tie="episode", snap=True, log_seed=26, **_LDS),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
TIE_CASES = [c for c in CASES if E in c.behaviour and c.q0 == "zero" and not c.holes]
