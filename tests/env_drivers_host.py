"""The reference's tabular drivers evalMC / qlearn / expSARSA / rollout on the grid worlds as a plain Python loop over the host mirror
(GridWorld.reset / step of evaluators/true_env_drivers.py), one rollout at a time (test infrastructure), the fixtures' reader and the LDS
rule of csrc/eval_env.hpp restated.

A restatement of documented behaviour (offsim4rl/agents/tabular.py:34-191, :247-270, offsim4rl/envs/gridworld.py:14-184, include/offsim.h:
offsim_eval_env), not of the kernel's code.  The action is NumPy's own Generator.choice on the rollout's action stream, the behaviours and
their ties are tests/queue_host.py's (tabular.py's as written), the update is in Python floats: Q-learning max(Q[S']); expected SARSA
sum_k Q[S'][k] * pi[S'][k] from k = 0 upwards.  Outputs come back in the device's layout, cut by trace_cap / ep_cap / snap_cap and
pre-filled as BatchedGridWorld allocates them."""
import os

import numpy as np

from queue_host import (ST_OK, ST_KEYERROR, EVALMC, QLEARN, EXPSARSA, FIXED, EPS_GREEDY, SOFT_GREEDY,  # noqa: F401
                        behaviour_row, mt_words, rng_words)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "env_drivers")
WORLDS = {"plain": ("plain", 1), "noise2": ("noise", 2), "noise3": ("noise", 3), "counter4": ("counter", 4)}


def run(world, gen, mode, pi, gamma, alpha=0.1, q=None, behaviour=FIXED, epsilon=0.0, alpha_ep=None, epsilon_ep=None, tie=None, episode0=0,
        n_episodes=1, trace_cap=0, ep_cap=0, snap_cap=0, snap_stride=1, memory=None):
    """n_episodes episodes on GridWorld `world` with the action stream `gen` (a Generator) from where it stands; gen, q (updated in place)
    and a RandomState `tie` keep the state a second call resumes from.  tie: None (first maximum), a RandomState, or "episode".
    memory: a list that gets the reference's tuples.  Returns the row of every output of BatchedGridWorld.eval_mc / eval_td."""
    nA, nS = world.nA, world.nS
    pi = None if pi is None else np.asarray(pi, np.float64)
    gamma = float(gamma)
    o = dict(trace_pop=np.zeros(trace_cap, np.int32), td_err=np.zeros(trace_cap, np.float64), beh_arg=np.zeros(trace_cap, np.int32),
             ep_g=np.zeros(ep_cap, np.float64), ep_len=np.zeros(ep_cap + 1, np.int32), q_snap=np.zeros((snap_cap, nS, nA), np.float64))
    tie_rs = tie if isinstance(tie, np.random.RandomState) else (np.random.RandomState(0) if tie == "episode" else None)
    ep = n_len = steps = 0
    sum_g, status = 0.0, ST_OK
    sched = lambda tab, const: float(const) if tab is None else float(tab[min(ep, len(tab) - 1)])  # noqa: E731
    while ep < n_episodes and status == ST_OK:
        if tie == "episode":
            tie_rs.seed((episode0 + ep) & 0xFFFFFFFF)  # np.random.seed(episode), before env.reset
        S = world.reset(seed=episode0 + ep)
        G, t, done = 0.0, 0, False
        while not done:
            if mode != EVALMC and behaviour != FIXED:
                p, best = behaviour_row(behaviour, q[S], sched(epsilon_ep, epsilon), tie_rs)
                if behaviour == EPS_GREEDY and steps < trace_cap:
                    o["beh_arg"][steps] = best
            else:
                p = pi[S]
            # Generator.choice refuses such rows; the draw it would have made is one double (include/offsim.h: the draw is consumed)
            if np.isnan(p).any() or not p.sum() > 0:
                gen.random()
                A = nA
            else:
                A = int(gen.choice(nA, p=p))
            if steps < trace_cap:
                o["trace_pop"][steps] = A
            if A >= nA:
                status = ST_KEYERROR
                break
            S_, r, done, info = world.step(A)
            if memory is not None:
                memory.append((S, A, r, S_, done, p, {**info, "t": t}))
            if mode != EVALMC:
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
            G = G + gamma ** t * r
            t += 1
            steps += 1
            S = S_
        if status == ST_KEYERROR:
            break
        if ep_cap and n_len <= ep_cap:
            o["ep_len"][n_len] = t
        n_len += 1
        if ep < ep_cap:
            o["ep_g"][ep] = G
        sum_g += G
        ep += 1
    o.update(sum_g=sum_g, n_ep=ep, steps=steps, cand=steps, n_len=n_len, status=status, rng=rng_words(gen))
    if q is not None:
        o["q"] = q.copy()
    if tie_rs is not None:
        o["tie_mt"] = mt_words(tie_rs)
    return o


# ---- the LDS rule of the learner shape (include/offsim.h: offsim_eval_env), n = nS * 5 ----
def lds_bytes(waves, n, have_pi=True, td=True):
    return (waves * n * 8 if td else 0) + (n * 8 if have_pi else 0) + (waves * (5 * 8 + 624 * 4) if td else 0)


def launch_shape(n, have_pi=True, td=True):
    """(rollouts per workgroup, LDS bytes, refused)"""
    w = 4
    while w > 1 and lds_bytes(w, n, have_pi, td) > 65536:
        w //= 2
    b = lds_bytes(w, n, have_pi, td)
    return w, b, b > 160 * 1024 or n > 40960


def factor_for_waves(waves, have_pi=False):
    """the smallest factor of a 5 x 5 world whose learner launch holds `waves` rollouts per workgroup"""
    return next(f for f in range(1, 400) if launch_shape(25 * f * 5, have_pi)[0] == waves)


# ---- policies of the matrix ----
def uniform(nS):
    return np.full((nS, 5), 0.2)


def shortest_path(world):
    """deterministic: right until the goal's column, then up; on the goal's cell anything (noop)"""
    pi = np.zeros((world.nS, 5))
    nc = world.num_cells
    for o in range(world.nS):
        x, y = (o % world.num_states) % nc, (o % world.num_states) // nc
        pi[o, 2 if x < world.goal[0] else 4 if x > world.goal[0] else 1 if y < world.goal[1] else 3 if y > world.goal[1] else 0] = 1.0
    return pi


def gapped(nS, seed=3):
    """zero entries in front of and behind the mass: cdf ties at both ends"""
    g = np.random.default_rng(seed)
    pi = np.zeros((nS, 5))
    pi[:, 1:4] = g.dirichlet(np.full(3, 1.0), nS)
    pi[::4, 1:4] = np.eye(3)[g.integers(0, 3, len(pi[::4]))]
    return pi


def nan_second_step(world):
    """uniform over {up, right} at the start cell, NaN rows at the two cells one step away: KeyError on the second step"""
    pi = uniform(world.nS)
    nc = world.num_cells
    for e in range(world.factor):
        pi[e * world.num_states] = [0, 0.5, 0.5, 0, 0]
        if nc > 1:
            pi[e * world.num_states + 1] = np.nan
            pi[e * world.num_states + nc] = np.nan
    return pi


# ---- the fixtures ----
class Fixture:
    def __init__(self, name):
        self.name, self.d = name, np.load(os.path.join(GOLDEN, name + ".npz"))
        d = self.d
        self.kind, self.factor = WORLDS[name]
        self.runs = [str(r) for r in d["runs"]]
        self.off = np.concatenate([[0], np.cumsum(d["steps"])])
        self.td_off = np.concatenate([[0], np.cumsum(d["td_steps"])])

    def settings(self, i):
        drv, gx, gy, ns, seed = self.runs[i].split("|")
        return drv, (int(gx), int(gy)), int(ns), int(seed)

    def memory(self, i):
        a, b = self.off[i], self.off[i + 1]
        return {k: self.d[k][a:b] for k in ("S", "A", "R", "S_", "done", "p", "z", "z_next", "t")}

    def td(self, i):
        a, b = self.td_off[i], self.td_off[i + 1]
        return self.d["TD_errors"][a:b]

    def Qs(self, i):
        a, b = self.td_off[i], self.td_off[i + 1]
        nS = 25 * self.factor
        out = np.zeros((b - a + 1, nS, 5))
        for k, (j, v) in enumerate(zip(self.d["Qs_idx"][a:b], self.d["Qs_val"][a:b])):
            out[k + 1] = out[k]
            out[k + 1].flat[j] = v
        return out

    def mt(self, i):
        return np.concatenate([self.d["mt_keys"][self.d["mt_key"][i]], [self.d["mt_pos"][i]]]).astype(np.uint32)


def memory_arrays(mem):
    """a driver's memory list as the fixtures' arrays"""
    cols = {k: [m[j] for m in mem] for j, k in enumerate(("S", "A", "R", "S_", "done", "p"))}
    for k in ("z", "z_next", "t"):
        cols[k] = [m[6][k] for m in mem]
    out = {k: np.array(v, np.float64 if k in ("R", "p") else bool if k == "done" else np.int64) for k, v in cols.items()}
    out["p"] = out["p"].reshape(-1, 5)
    return out


EPS_SCHED = lambda e: 1.0 / (1.0 + e)  # noqa: E731  (the schedule the fixtures were recorded with)
# driver -> (mode, behaviour, epsilon (None: EPS_SCHED))
DRIVERS = {"evalMC": (EVALMC, FIXED, 0.0), "rollout": (EVALMC, FIXED, 0.0), "qlearn_uniform": (QLEARN, FIXED, 0.0), "qlearn_eps": (QLEARN, EPS_GREEDY, 0.3),
           "qlearn_eps_sched": (QLEARN, EPS_GREEDY, None), "qlearn_greedy": (QLEARN, EPS_GREEDY, 0.0), "qlearn_soft": (QLEARN, SOFT_GREEDY, 0.0),
           "expSARSA": (EXPSARSA, FIXED, 0.0)}
