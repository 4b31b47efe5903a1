"""The case list of the learner-kernel matrix (tests/test_gpu_td_matrix.py; checked without a device by tests/test_td_matrix_host.py).

A case names a table, the learners of one launch and every argument of BatchedPSRS.eval_td.  host(case) runs it through the plain
Python loop of tests/td_host.py, once per process; launch_shape() restates the launcher's LDS arithmetic (offsim_hip.hip:
evalmc_lds_bytes, evalmc_launch) so that a case can say which launch it gets.
"""
import functools
import os
import sys
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import td_host as H  # noqa: E402
from rl_offline_simulation_amd import synth  # noqa: E402

REJECT_DEFAULT, REJECT_NEVER = 0, 1
WAVE, SIZEOF_JUMP = 64, 32


def lds_bytes(waves, n_slots, nA):
    """evalmc_lds_bytes(waves, n_slots, nA, prob_bytes = 8, td = true): jump tables, Q per wave, pi, seg_off, cursors per wave, the
    8-byte round-up, the behaviour row and the 624 MT words per wave."""
    return (waves * (WAVE + 1) * SIZEOF_JUMP + waves * n_slots * nA * 8 + n_slots * nA * 8 + (n_slots + 1) * 4 + waves * n_slots * 4
            + 8 + waves * nA * 8 + waves * 624 * 4)


def launch_shape(n_slots, nA):
    """(waves, LDS bytes, refused): 4 learners per workgroup, halved until the carve fits 64 KiB; one learner may take up to 160 KiB."""
    waves = 4
    while waves > 1 and lds_bytes(waves, n_slots, nA) > 64 * 1024:
        waves >>= 1
    b = lds_bytes(waves, n_slots, nA)
    return waves, b, b > 160 * 1024


@dataclass(frozen=True)
class Table:
    """synth.synth_iid(N, live, nA, seed, p_done, p_init) with its `live` states spread over the ids 0 .. nS - 1 (so the table has nS
    slots, most of them without rows and never reached); p_miss: share of rows whose next state is an id without a queue."""
    N: int
    nS: int
    live: int
    nA: int
    pl: str = "f32"      # dtype of the logging probabilities: f64 / f32 / f16
    rd: str = "f32"      # dtype of the rewards: f64 / f32
    seed: int = 1
    p_done: float = 0.02
    p_init: float = 0.02
    p_miss: float = 0.0


@functools.lru_cache(maxsize=None)
def arrays(t):
    e = synth.synth_iid(t.N, t.live, t.nA, seed=t.seed, p_done=t.p_done, p_init=t.p_init)
    ids = np.round(np.linspace(0, t.nS - 1, t.live)).astype(np.int64)
    assert len(np.unique(ids)) == t.live
    z, zn = ids[e["z"]], ids[e["z_next"]]
    if t.p_miss:
        dead = next(i for i in range(t.nS) if i not in set(ids.tolist()))
        zn = np.where(np.random.default_rng(t.seed + 1000).random(t.N) < t.p_miss, dead, zn)
    p = e["action_distributions"].astype({"f64": np.float64, "f32": np.float32, "f16": np.float16}[t.pl])
    r = e["rewards"].astype({"f64": np.float64, "f32": np.float32}[t.rd])
    return dict(z=z, a=e["actions"], r=r, z_next=zn, done=e["terminals"], p_log=p, t0=e["steps"] == 0)


@functools.lru_cache(maxsize=None)
def log_of(t):
    return H.Log(**arrays(t))


@dataclass(frozen=True)
class Case:
    name: str
    table: Table
    R: int
    mode: int = H.QLEARN
    behaviour: int = H.FIXED
    epsilon: float = 0.0
    alpha: float = 0.1
    epsilon_ep: Optional[Tuple[float, ...]] = None
    alpha_ep: Optional[Tuple[float, ...]] = None
    q_init: str = "zeros"          # zeros / const (0.25 everywhere) / randn (no two entries equal)
    gamma: float = 0.97
    n_gamma_pow: int = 4096
    reject: int = REJECT_DEFAULT
    stream: str = "pcg64"          # pcg64 / philox
    reset: str = "plain"           # plain / keyed (reset_sampler(seeds, policy=...)) / shared (one queue order, seed 77)
    seed0: int = 3
    n_episodes: Optional[int] = None
    trace_cap: Optional[int] = None  # None: N + 1 (the whole run)
    ep_cap: Optional[int] = None     # None: N0 + 1 (the whole run)
    snap_cap: int = 0
    snap_stride: int = 1
    mt: str = "none"               # none / fresh (position 624) / mid (inside a block); every learner its own state
    resume_k: Optional[int] = None   # two calls: resume_k episodes, then the rest
    edge: bool = False             # exempt from the non-vacuity floor (and says why in its name)
    refused: bool = False

    @property
    def seeds(self):
        return [self.seed0 + 5 * i for i in range(self.R)]

    @property
    def shape(self):
        return launch_shape(self.table.nS, self.table.nA)


SHUFFLE_SEED = 77


def pi_of(case):
    """The tabular policy [n_slots, nA] (behaviour when FIXED, target of expected SARSA): half Dirichlet, half uniform."""
    t = case.table
    return 0.5 * synth.dirichlet_policy(t.nS, t.nA, seed=9 + t.seed) + 0.5 / t.nA


def q_init_of(case):
    t = case.table
    if case.q_init == "zeros":
        q = np.zeros((t.nS, t.nA))
    elif case.q_init == "const":
        q = np.full((t.nS, t.nA), 0.25)
    else:
        q = np.random.default_rng(99 + t.seed).standard_normal((t.nS, t.nA)) * 0.1
    return np.broadcast_to(q, (case.R, t.nS, t.nA)).copy()


def mt_of(case):
    """[R, 625] uint32 tie streams (np.random.get_state() layout), or None: learner i starts from RandomState(4000 + 17 i + seed0);
    `mid` first takes 100 + 37 i words out of it, which leaves the position inside the first block."""
    if case.mt == "none":
        return None
    out = []
    for i in range(case.R):
        rs = np.random.RandomState(4000 + 17 * i + case.seed0)
        if case.mt == "mid":
            rs.bytes(4 * (100 + 37 * i))
        st = rs.get_state()
        out.append(np.concatenate([np.asarray(st[1], np.uint32), np.array([st[2]], np.uint32)]))
    return np.stack(out)


def caps_of(case):
    a = arrays(case.table)
    return (case.table.N + 1 if case.trace_cap is None else case.trace_cap,
            int(a["t0"].sum()) + 1 if case.ep_cap is None else case.ep_cap)


def run_args(case):
    """The arguments td_host.run and BatchedPSRS.eval_td share (under the same names)."""
    trace_cap, ep_cap = caps_of(case)
    return dict(mode=case.mode, gamma=case.gamma, alpha=case.alpha, behaviour=case.behaviour, epsilon=case.epsilon,
                alpha_ep=None if case.alpha_ep is None else np.array(case.alpha_ep), epsilon_ep=None if case.epsilon_ep is None else np.array(case.epsilon_ep),
                trace_cap=trace_cap, ep_cap=ep_cap, snap_cap=case.snap_cap, snap_stride=case.snap_stride)


def learners_of(case):
    log, q0, mt = log_of(case.table), q_init_of(case), mt_of(case)
    return [H.Learner(log, s, q0[i], None if mt is None else mt[i], stream=case.stream, shuffle_seed=SHUFFLE_SEED if case.reset == "shared" else None)
            for i, s in enumerate(case.seeds)]


@functools.lru_cache(maxsize=None)
def host(case):
    """The host loop's outputs for the calls of the case: [one launch], or [first resume_k episodes, the rest]; the last one also
    holds `after` [R, 4]: td_host.reset_and_step of every learner."""
    ls, pi, kw = learners_of(case), pi_of(case), run_args(case)
    if case.resume_k is None:
        outs = [H.run_launch(ls, pi=pi, n_episodes=case.n_episodes, reject_mode=case.reject, **kw)]
    else:
        outs = [H.run_launch(ls, pi=pi, n_episodes=case.resume_k, reject_mode=case.reject, **kw),
                H.run_launch(ls, pi=pi, n_episodes=None, reject_mode=case.reject, **kw)]
    # where the sampler stands afterwards: one more reset and one more step under the uniform policy
    outs[-1]["after"] = np.array([H.reset_and_step(lr, np.full(case.table.nA, 1.0 / case.table.nA), case.reject) for lr in ls], np.int64)
    return outs


# ---- tables (n_slots x nA decides the launch; see launch_shape) ----
T5 = Table(3000, 25, 8, 5)                                   # waves 4
T5_F64 = replace(T5, pl="f64", rd="f64", seed=2)
T5_F16 = replace(T5, pl="f16", seed=3)
T2 = Table(2000, 30, 6, 2, seed=4)                           # waves 4, two actions
T16 = Table(4000, 80, 8, 16, seed=5)                         # waves 2
T16_W1 = Table(4000, 190, 8, 16, seed=6, rd="f64")           # waves 1, below 64 KiB
T15_BIG = Table(4000, 300, 8, 15, seed=7)                    # waves 1, above 64 KiB
T80 = Table(4000, 25, 6, 80, seed=8)                         # waves 2, actions wrap the wavefront
T80_F16 = replace(T80, pl="f16", seed=12)
T80_FEW = replace(T80, live=3, seed=13)                       # enough rows per state for the default reject rule at 80 actions
T_160K = Table(3000, 602, 6, 16, seed=9)                     # the last size the launcher takes
T_OVER = Table(3000, 603, 6, 16, seed=9)                     # the first it refuses
T_FEW_INIT = Table(3000, 25, 6, 5, seed=10, p_done=0.08, p_init=0.008)   # the initial queue runs out first
T_MISS = Table(3000, 25, 6, 5, seed=11, p_miss=0.0015)        # some next states have no queue

E, S, F = H.EPS_GREEDY, H.SOFT_GREEDY, H.FIXED
Q, X = H.QLEARN, H.EXPSARSA

CASES = [
    # PL instances x modes (waves 4), every behaviour under both modes
    Case("pl-f64-qlearn-eps-R4", T5_F64, 4, Q, E, epsilon=0.3, mt="fresh"),
    Case("pl-f64-expsarsa-fixed-R9", T5_F64, 9, X, F),
    Case("pl-f32-qlearn-soft-R5", T5, 5, Q, S),
    Case("pl-f32-expsarsa-eps-R1", T5, 1, X, E, epsilon=0.2, mt="fresh"),
    Case("pl-f16-qlearn-fixed-philox-R3", T5_F16, 3, Q, F, stream="philox", q_init="randn"),
    Case("pl-f16-expsarsa-soft-R6", T5_F16, 6, X, S, gamma=1.0),
    # launch shapes
    Case("waves2-R3", T16, 3, Q, E, epsilon=0.5, mt="fresh"),
    Case("waves2-R1", T16, 1, X, F, q_init="randn"),
    Case("waves1-R3", T16_W1, 3, X, E, epsilon=0.5, mt="mid"),
    Case("waves1-R1", T16_W1, 1, Q, F),
    Case("lds-above-64k-R3", T15_BIG, 3, Q, E, epsilon=0.5, mt="fresh", snap_cap=5, snap_stride=3),
    Case("lds-above-64k-R1", T15_BIG, 1, X, F),
    Case("lds-160k-last-that-fits-R2", T_160K, 2, X, E, epsilon=0.5, mt="fresh"),
    Case("lds-160k-first-refused", T_OVER, 2, Q, F, edge=True, refused=True),
    # action counts
    Case("nA2-R7", T2, 7, Q, E, epsilon=0.4, mt="fresh"),
    Case("nA80-eps-R3", T80, 3, Q, E, epsilon=0.9, mt="fresh", reject=REJECT_NEVER),
    Case("nA80-soft-f16-R5", T80_F16, 5, X, S, reject=REJECT_NEVER),
    Case("nA80-fixed-default-reject-R2", T80_FEW, 2, X, F),
    # behaviours and schedules
    Case("eps-first-maximum-no-tie-stream-R4", T5, 4, Q, E, epsilon=0.3),
    Case("greedy-epsilon-0-R3", T5, 3, Q, E, epsilon=0.0, mt="fresh", reject=REJECT_NEVER),
    Case("schedules-shorter-than-the-run-R3", T5, 3, Q, E, epsilon_ep=(0.9, 0.6, 0.3), alpha_ep=(0.5, 0.25, 0.125), mt="fresh"),
    Case("schedules-expsarsa-R2", T5, 2, X, F, alpha_ep=(0.5, 0.2), epsilon_ep=(0.0, 0.0)),
    Case("constants-R3", T5, 3, Q, E, epsilon=0.3, alpha=0.2, mt="fresh", seed0=11),
    Case("constants-as-schedules-R3", T5, 3, Q, E, epsilon_ep=(0.3, 0.3), alpha_ep=(0.2, 0.2), mt="fresh", seed0=11),
    # tie stream
    Case("ties-every-step-1300-words-R3", T5, 3, Q, E, epsilon=1.0, alpha=0.0, q_init="const", mt="fresh", reject=REJECT_NEVER),
    Case("mt-mid-block-R4", T5, 4, Q, E, epsilon=0.3, mt="mid"),
    # sampler
    Case("philox-eps-R5", T5, 5, Q, E, epsilon=0.3, mt="fresh", stream="philox"),
    Case("philox-reject-never-R2", T5, 2, X, F, stream="philox", reject=REJECT_NEVER),
    Case("keyed-reset-R4", T5_F64, 4, X, F, reset="keyed"),
    Case("keyed-reset-philox-eps-R3", T5, 3, Q, E, epsilon=0.3, mt="fresh", reset="keyed", stream="philox"),
    Case("shared-order-R4", T5, 4, Q, E, epsilon=0.3, mt="fresh", reset="shared"),
    # ends
    Case("end-no-init-R3", T_FEW_INIT, 3, Q, E, epsilon=0.5, mt="fresh"),
    Case("end-keyerror-and-others-R6", T_MISS, 6, Q, E, epsilon=0.5, mt="fresh"),
    Case("n-episodes-3-R4", T5, 4, X, F, n_episodes=3, edge=True),
    Case("n-episodes-0-R3", T5, 3, Q, E, epsilon=0.3, mt="fresh", n_episodes=0, edge=True),
    # caps smaller than the run: an overrun lands in the next learner's row
    Case("caps-smaller-than-the-run-stride3-R3", T5, 3, Q, E, epsilon=0.3, mt="fresh", trace_cap=50, ep_cap=2, snap_cap=7, snap_stride=3),
    Case("caps-smaller-than-the-run-stride1-R4", T5_F64, 4, X, F, trace_cap=33, ep_cap=1, snap_cap=40, snap_stride=1),
    # discount: a table shorter than the longest episode is exact only where it ends stationary
    Case("gamma-0-short-table-R3", T5, 3, Q, S, gamma=0.0, n_gamma_pow=2),
    Case("gamma-1-short-table-R3", T5, 3, X, F, gamma=1.0, n_gamma_pow=2),
    # resume: k episodes, then the rest, from out["q"], out["tie_mt"] and the sampler state
    Case("resume-after-2-episodes-eps-R4", T5, 4, Q, E, epsilon=0.3, mt="mid", resume_k=2),
    Case("resume-after-3-episodes-expsarsa-philox-R3", T5_F16, 3, X, F, stream="philox", resume_k=3, snap_cap=30),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
