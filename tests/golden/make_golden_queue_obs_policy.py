#!/usr/bin/env python3
"""Generate tests/golden/queue_obs_policy/*.npz by RUNNING THE REFERENCE: its own evalMC (offsim4rl/agents/tabular.py:247-270), unmodified,
on its own QueueEvaluator_impl (offsim4rl/evaluators/queue_evaluator.py:90-131), for a policy over observations.

Run from the repo root, on the CPU:   OFFSIM4RL_REFERENCE=<checkout of offsim4rl> python tests/golden/make_golden_queue_obs_policy.py
Nothing of the reference is copied -- the fixtures hold the outputs it produced for the inputs of tests/golden/queue_iid_2k.npz and
queue_grid_300x15.npz.  QueueEvaluator_impl and evalMC are compiled from their files in memory, as make_golden_queue_drivers.py does it.

evalMC asks the policy as pi[S] with S what reset / step returned.  The observation of a buffer entry is the pair ("obs" | "next", row),
unique per row, and pi is a mapping keyed by it: pi[("obs", i)] = P_init[i], pi[("next", i)] = P_next[i].  So the loop, the action draw
rng.choice(env.nA, p=p) on default_rng(seed) and the returns are the reference's own code; only env.step is wrapped to record the served
rows and the actions.  Two policies per input -- fixed per-row f64 tables (Dirichlet rows, default_rng(91)) and their f32 rounding
(choice takes the f32 row as it is) -- and three sampler seeds s each, action seed 1000 + s.  The reference's loop does not survive a
queue running out (None flows into pi[None]), so n_episodes is chosen such that all runs complete, and that is asserted here.
"""
import ast
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ["OFFSIM4RL_REFERENCE"]
OUT = os.path.join(ROOT, "tests", "golden", "queue_obs_policy")
SEEDS, GAMMA = (0, 4, 9), 0.95
N_EPISODES = {"queue_iid_2k": 6, "queue_grid_300x15": 4}


def _compiled(path, kind, name, ns):
    node = next(n for n in ast.parse(open(os.path.join(REF, path)).read()).body if isinstance(n, kind) and n.name == name)
    exec(compile(ast.Module(body=[node], type_ignores=[]), os.path.basename(path), "exec"), ns)
    return ns[name]


QueueEvaluator_impl = _compiled("offsim4rl/evaluators/queue_evaluator.py", ast.ClassDef, "QueueEvaluator_impl", {"np": np, "itertools": __import__("itertools")})
evalMC = _compiled("offsim4rl/agents/tabular.py", ast.FunctionDef, "evalMC", {"np": np})


class Recorder:
    """env with step recorded: the actions asked for and the rows served"""

    def __init__(self, env):
        self.env, self.nA, self.rows, self.actions = env, env.nA, [], []

    def reset(self, seed=None):
        return self.env.reset(seed=seed)

    def step(self, a):
        self.actions.append(int(a))
        out = self.env.step(a)
        assert out[0] is not None, "a queue ran out: choose fewer episodes"
        self.rows.append(out[0][1])
        return out


def fixture(name):
    d = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    z, a, r, zn, done, p_log, t0 = (d["in_" + k] for k in ("z", "a", "r", "z_next", "done", "p_log", "t0"))
    N, nA = len(z), p_log.shape[1]
    nS = int(max(z.max(), zn.max())) + 1
    buf = [(("obs", i), int(a[i]), float(r[i]), ("next", i), bool(done[i]), p_log[i], {"t": 0 if t0[i] else 1, "z": int(z[i]), "next_z": int(zn[i])})
           for i in range(N)]
    g = np.random.default_rng(91)
    P_next, P_init = g.dirichlet(np.full(nA, 1.5), N), g.dirichlet(np.full(nA, 1.5), N)
    n_ep = N_EPISODES[name]
    out = dict(P_next=P_next, P_init=P_init, seeds=np.array(SEEDS, np.int64), gamma=np.float64(GAMMA), n_episodes=np.int64(n_ep))
    report = []
    for tag, cast in (("f64", np.float64), ("f32", np.float32)):
        pn, p0 = P_next.astype(cast), P_init.astype(cast)
        pi = {**{("obs", i): p0[i] for i in range(N)}, **{("next", i): pn[i] for i in range(N)}}
        for s in SEEDS:
            env = QueueEvaluator_impl(buf, nS=nS, nA=nA)
            env.reset_sampler(seed=s)
            rec = Recorder(env)
            Gs, lengths = evalMC(rec, n_ep, pi, GAMMA, seed=1000 + s)
            assert len(Gs) == n_ep and len(lengths) == n_ep and sum(lengths) == len(rec.rows)
            k = f"{tag}_s{s}_"
            out.update({k + "Gs": np.asarray(Gs, np.float64), k + "lengths": np.asarray(lengths, np.int64), k + "rows": np.array(rec.rows, np.int64),
                        k + "actions": np.array(rec.actions, np.int64), k + "z": np.int64(env.z)})
            report.append((tag, s, len(rec.rows)))
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(name, report)


if __name__ == "__main__":
    for nm in ("queue_iid_2k", "queue_grid_300x15"):
        fixture(nm)
