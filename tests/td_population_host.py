"""A population of TD learners on the host (test infrastructure): learner (l, j) of a population case is td_host.Learner on seed j with
its own Q and tie stream, run by td_host.run under learner l's hyper-parameters -- nothing is shared between learners but the log -- and
the learning curves are a Python-float loop in seed order.  The case list is what tests/test_gpu_td_population.py runs on the device and
what tests/test_td_population_host.py checks, without one, for being non-vacuous.

Everything comes back stacked as BatchedPSRS.eval_td_population returns it: [L, S, ...].
"""
import functools
import os
import sys
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import td_cases as K  # noqa: E402
import td_host as H  # noqa: E402
from rl_offline_simulation_amd import synth  # noqa: E402

E, SOFT, F = H.EPS_GREEDY, H.SOFT_GREEDY, H.FIXED
N_L, N_S = 3, 5  # S is a multiple of no launch shape's learners per workgroup (4, 2: a partly filled workgroup; 1)


@dataclass(frozen=True)
class PopCase:
    name: str
    table: K.Table
    mode: int = H.QLEARN
    behaviour: Tuple[int, ...] = (E, E, E)
    # the grid: no two learners agree in any of the three
    alpha: Tuple[float, ...] = (0.05, 0.2, 0.5)
    epsilon: Tuple[float, ...] = (0.1, 0.3, 0.6)
    gamma: Tuple[float, ...] = (0.9, 0.97, 1.0)
    alpha_ep: Optional[Tuple[Tuple[float, ...], ...]] = None      # [L][n_sched]
    epsilon_ep: Optional[Tuple[Tuple[float, ...], ...]] = None
    pi_per_learner: bool = False
    mt: str = "none"              # none / fresh / mid, every (learner, seed) its own state
    stream: str = "pcg64"
    trace_cap: Optional[int] = None
    ep_cap: Optional[int] = None
    snap_cap: int = 0
    snap_stride: int = 1
    resume_k: Optional[int] = None
    curve: bool = True            # a curve case: its returns go through offsim_td_curves and must be ragged over the seeds
    seed0: int = 3

    @property
    def L(self):
        return N_L

    @property
    def S(self):
        return N_S

    @property
    def seeds(self):
        return [self.seed0 + 5 * j for j in range(N_S)]

    @property
    def shape(self):
        """(learners per workgroup, LDS bytes, refused, workgroups): a workgroup holds seeds of one learner"""
        waves, lds, refused = K.launch_shape(self.table.nS, self.table.nA)
        return waves, lds, refused, N_L * ((N_S + waves - 1) // waves)


def pi_of(case):
    """[n_slots, nA] shared, or [L, n_slots, nA]: learner l's own mixture of a Dirichlet table and the uniform one"""
    t = case.table
    if not case.pi_per_learner:
        return 0.5 * synth.dirichlet_policy(t.nS, t.nA, seed=9 + t.seed) + 0.5 / t.nA
    return np.stack([(0.3 + 0.2 * l) * synth.dirichlet_policy(t.nS, t.nA, seed=20 + 3 * l + t.seed) + (0.7 - 0.2 * l) / t.nA for l in range(N_L)])


def q_init_of(case):
    """[L, S, n_slots, nA]: zeros (ties on every first visit)"""
    return np.zeros((N_L, N_S, case.table.nS, case.table.nA))


def mt_of(case):
    """[L, S, 625] uint32 tie streams or None: (l, j) starts from RandomState(7000 + 31 l + 17 j); `mid` first takes 100 + 37 (l S + j)
    words out of it, which leaves the position inside the first block."""
    if case.mt == "none":
        return None
    out = np.zeros((N_L, N_S, 625), np.uint32)
    for l in range(N_L):
        for j in range(N_S):
            rs = np.random.RandomState(7000 + 31 * l + 17 * j)
            if case.mt == "mid":
                rs.bytes(4 * (100 + 37 * (l * N_S + j)))
            st = rs.get_state()
            out[l, j, :624], out[l, j, 624] = st[1], st[2]
    return out


def caps_of(case):
    a = K.arrays(case.table)
    return (case.table.N + 1 if case.trace_cap is None else case.trace_cap, int(a["t0"].sum()) + 1 if case.ep_cap is None else case.ep_cap)


def learner_args(case, l):
    """What td_host.run and BatchedPSRS.eval_td share for learner l (under the same names), pi apart."""
    trace_cap, ep_cap = caps_of(case)
    return dict(mode=case.mode, gamma=case.gamma[l], alpha=case.alpha[l], behaviour=case.behaviour[l], epsilon=case.epsilon[l],
                alpha_ep=None if case.alpha_ep is None else np.array(case.alpha_ep[l]),
                epsilon_ep=None if case.epsilon_ep is None else np.array(case.epsilon_ep[l]),
                trace_cap=trace_cap, ep_cap=ep_cap, snap_cap=case.snap_cap, snap_stride=case.snap_stride)


def population_args(case):
    """The arguments of BatchedPSRS.eval_td_population."""
    trace_cap, ep_cap = caps_of(case)
    return dict(mode=case.mode, alpha=np.array(case.alpha), gamma=np.array(case.gamma), behaviour=np.array(case.behaviour), epsilon=np.array(case.epsilon),
                pi_slots=pi_of(case), alpha_ep=None if case.alpha_ep is None else np.array(case.alpha_ep),
                epsilon_ep=None if case.epsilon_ep is None else np.array(case.epsilon_ep), trace_cap=trace_cap, ep_cap=ep_cap,
                snap_cap=case.snap_cap, snap_stride=case.snap_stride)


def _stack(rows):
    """[L][S] dicts of td_host.run -> {key: [L, S, ...]}"""
    out = {k: np.stack([np.stack([np.asarray(r[k], dt) for r in row]) for row in rows]) for k, dt in H._STACK.items()}
    out["tie_mt"] = None if rows[0][0]["tie_mt"] is None else np.stack([np.stack([r["tie_mt"] for r in row]) for row in rows])
    return out


@functools.lru_cache(maxsize=None)
def host(case):
    """The host loop's outputs of the calls of the case, each {key: [L, S, ...]}: [one call], or [the first resume_k episodes, the rest]."""
    log, q0, mt, pi = K.log_of(case.table), q_init_of(case), mt_of(case), pi_of(case)
    ls = [[H.Learner(log, s, q0[l, j], None if mt is None else mt[l, j], stream=case.stream) for j, s in enumerate(case.seeds)] for l in range(N_L)]
    calls = [None] if case.resume_k is None else [case.resume_k, None]
    return [_stack([[H.run(ls[l][j], pi=pi[l] if case.pi_per_learner else pi, n_episodes=n, **learner_args(case, l)) for j in range(N_S)]
                    for l in range(N_L)]) for n in calls]


def curves(ep_g, n_ep):
    """(n [L, E] int64, mean [L, E], var [L, E]) of ep_g [L, S, E] and n_ep [L, S]: per learner and episode, over the seeds that completed
    the episode in order j = 0 .. S - 1, Python floats: the sum, the mean, then the mean squared deviation; NaN without a seed."""
    n_l, n_s, n_e = ep_g.shape
    n, mean, var = np.zeros((n_l, n_e), np.int64), np.zeros((n_l, n_e)), np.zeros((n_l, n_e))
    for l in range(n_l):
        for e in range(n_e):
            xs = [float(ep_g[l, j, e]) for j in range(n_s) if e < int(n_ep[l, j])]
            n[l, e] = len(xs)
            if not xs:
                mean[l, e] = var[l, e] = float("nan")
                continue
            s = 0.0
            for x in xs:
                s = s + x
            m = s / len(xs)
            ss = 0.0
            for x in xs:
                d = x - m
                ss = ss + d * d
            mean[l, e], var[l, e] = m, ss / len(xs)
    return n, mean, var


_SCHED_A = ((0.5, 0.25, 0.125), (0.4, 0.2, 0.1), (0.3, 0.3, 0.05))
_SCHED_E = ((0.9, 0.6, 0.3), (0.8, 0.4, 0.0), (0.5, 0.5, 0.2))

CASES = [
    # Q-learning under every behaviour, one learner each, in one launch (4 learners' seeds per workgroup: 2 workgroups per learner)
    PopCase("qlearn-every-behaviour-mt-fresh", K.T5, behaviour=(F, E, SOFT), mt="fresh"),
    PopCase("qlearn-eps-mt-mid", K.T5, mt="mid"),
    PopCase("qlearn-eps-first-maximum", K.T5),
    PopCase("qlearn-eps-greedy-schedules", K.T5, epsilon=(0.0, 0.3, 0.6), alpha_ep=_SCHED_A, epsilon_ep=_SCHED_E, mt="fresh"),
    PopCase("qlearn-eps-philox", K.T5, mt="fresh", stream="philox"),
    # expected SARSA with every learner its own target (and, where fixed, behaviour) policy
    PopCase("expsarsa-own-pi-waves2", K.T16, mode=H.EXPSARSA, behaviour=(F, F, F), pi_per_learner=True),
    PopCase("expsarsa-own-pi-every-behaviour", K.T5, mode=H.EXPSARSA, behaviour=(E, SOFT, F), pi_per_learner=True, mt="mid"),
    # one learner per workgroup, above 64 KiB, with snapshots
    PopCase("qlearn-eps-lds-above-64k", K.T15_BIG, mt="fresh", snap_cap=5, snap_stride=3),
    # the initial queue runs out first (every seed completes all of its episodes, so the counts are not ragged: no curve case)
    PopCase("expsarsa-few-init", K.T_FEW_INIT, mode=H.EXPSARSA, behaviour=(F, E, SOFT), pi_per_learner=True, mt="fresh", curve=False),
    # caps smaller than the run: an overrun would land in the next rollout's row
    PopCase("caps-smaller-than-the-run", K.T5, mt="fresh", trace_cap=50, ep_cap=2, snap_cap=7, snap_stride=3),
    # cut short, then resumed.  The behaviour is the fixed shared pi, so every learner of a seed walks the same rows and ONE environment
    # advanced by any of them stands where all of them stand
    PopCase("resume-after-2-episodes-fixed", K.T5, behaviour=(F, F, F), resume_k=2, snap_cap=30),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
CURVE_CASES = [c for c in CASES if c.curve and c.ep_cap is None and c.resume_k is None]
