#!/usr/bin/env python3
"""Generate tests/golden/queue_drivers/*.npz by RUNNING THE REFERENCE's QueueEvaluator_impl (offsim4rl/evaluators/queue_evaluator.py:90-131)
under its own tabular drivers evalMC, qlearn and expSARSA (offsim4rl/agents/tabular.py).

Run from the repo root:   python tests/golden/make_golden_queue_drivers.py
Needs /root/reference (read-only); nothing of it is copied -- the fixtures hold the outputs the reference produced for the inputs of
tests/golden/queue_iid_2k.npz and queue_grid_300x15.npz.  QueueEvaluator_impl is compiled from its file in memory (the module imports gym,
as make_golden.py section 12 does it); agents/tabular.py is loaded by path with tqdm stubbed, and the env.seed the drivers call, which
QueueEvaluator_impl does not have, is a no-op added to the instance here only.  Rewards enter the buffer as Python floats (an exact widening of
the f32 column), as make_golden_exo_drivers.py does: with NumPy scalars the reference's G would be summed in float32.

Per input and sampler seed s in (0, 4), with the drivers' own seed 1000 + s:
  mc    evalMC(pi)                                               Gs, lengths
  qu    qlearn, uniformly_random_policy, Q_init None             Q, Gs, TD_errors, Qs[:9] of a save_Q = 1 run
  qe    qlearn, epsilon_greedy_policy, epsilon 0.3, Q_init None  (every row of Q starts as a tie)
  qs    qlearn, epsilon_greedy_policy, epsilon(e) = 0.9 / (1 + 0.2 e), alpha(e) = 0.5 / (1 + 0.1 e), a random Q_init
  qg    qlearn, greedy_policy, Q_init None
  qf    qlearn, soft_greedy_policy, a random Q_init
  es    expSARSA(pi), Q_init None
and for each: the rows served, env.z afterwards and NumPy's global MT19937 state afterwards.  n_episodes is, per run, the largest of
(8, 6, 4, 3, 2, 1) at which the reference itself neither exhausts a queue nor raises KeyError -- asserted below.
"""
import ast
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "queue_drivers")
SEEDS = (0, 4)
GAMMA, ALPHA = 0.9, 0.1
EPS_SCHED = lambda e: 0.9 / (1.0 + 0.2 * e)    # noqa: E731
ALPHA_SCHED = lambda e: 0.5 / (1.0 + 0.1 * e)  # noqa: E731

sys.modules.setdefault("tqdm", types.SimpleNamespace(tqdm=lambda it, **kw: it))
spec = importlib.util.spec_from_file_location("ref_tabular", os.path.join(REF, "offsim4rl/agents/tabular.py"))
ref_tab = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref_tab)
_src = open(os.path.join(REF, "offsim4rl/evaluators/queue_evaluator.py")).read()
_cls = next(n for n in ast.parse(_src).body if isinstance(n, ast.ClassDef) and n.name == "QueueEvaluator_impl")
_ns = {"np": np, "itertools": __import__("itertools")}
exec(compile(ast.Module(body=[_cls], type_ignores=[]), "queue_evaluator.py", "exec"), _ns)
QueueEvaluator_impl = _ns["QueueEvaluator_impl"]


class Exhausted(Exception):
    pass


def fixture(name):
    d = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    z, a, r, zn, done, p_log, t0 = (d["in_" + k] for k in ("z", "a", "r", "z_next", "done", "p_log", "t0"))
    N, nA = len(z), p_log.shape[1]
    assert z.min() >= 0 and zn.min() >= 0
    nS = int(max(z.max(), zn.max())) + 1
    buf = [(int(z[i]), int(a[i]), float(r[i]), int(zn[i]), bool(done[i]), p_log[i], {"t": 0 if t0[i] else 1, "z": int(z[i]), "next_z": int(zn[i]), "idx": i})
           for i in range(N)]
    g = np.random.default_rng(42)
    pi = g.dirichlet(np.full(nA, 1.5), nS)
    q_init = g.standard_normal((nS, nA)) * 0.1
    out = dict(pi=pi, q_init=q_init, nS=np.int64(nS), gamma=np.float64(GAMMA), alpha=np.float64(ALPHA), seeds=np.array(SEEDS, np.int64))
    T = ref_tab
    runs = {
        "mc": lambda env, n, sd, sq: (None, dict(zip(("Gs", "lengths"), T.evalMC(env, n, pi, GAMMA, seed=sd)))),
        "qu": lambda env, n, sd, sq: T.qlearn(env, n, T.uniformly_random_policy, GAMMA, alpha=ALPHA, save_Q=sq, show_tqdm=False, seed=sd),
        "qe": lambda env, n, sd, sq: T.qlearn(env, n, T.epsilon_greedy_policy, GAMMA, alpha=ALPHA, epsilon=0.3, save_Q=sq, show_tqdm=False, seed=sd),
        "qs": lambda env, n, sd, sq: T.qlearn(env, n, T.epsilon_greedy_policy, GAMMA, alpha=ALPHA_SCHED, epsilon=EPS_SCHED, Q_init=q_init, save_Q=sq,
                                              show_tqdm=False, seed=sd),
        "qg": lambda env, n, sd, sq: T.qlearn(env, n, T.greedy_policy, GAMMA, alpha=ALPHA, Q_init=None, save_Q=sq, show_tqdm=False, seed=sd),
        "qf": lambda env, n, sd, sq: T.qlearn(env, n, T.soft_greedy_policy, GAMMA, alpha=ALPHA, Q_init=q_init, save_Q=sq, show_tqdm=False, seed=sd),
        "es": lambda env, n, sd, sq: T.expSARSA(env, n, pi, GAMMA, alpha=ALPHA, save_Q=sq, show_tqdm=False, seed=sd),
    }
    report = []
    for s in SEEDS:
        for tag, fn in runs.items():
            for n_ep in (8, 6, 4, 3, 2, 1):
                env = QueueEvaluator_impl(buf, nS=nS, nA=nA)
                env.seed = lambda seed=None: None
                rows, orig = [], env.step

                def step(act, env=env, rows=rows, orig=orig):
                    q = env.queues[env.z, int(act)]  # KeyError: never logged
                    if len(q) == 0:
                        raise Exhausted()
                    rows.append(q[0][8]["idx"])
                    return orig(act)
                env.step = step
                env.reset_sampler(seed=s)
                np.random.seed(12345)
                try:
                    Q, info = fn(env, n_ep, 1000 + s, 0)
                except (Exhausted, KeyError):
                    continue
                break
            else:
                raise AssertionError(f"{name} s{s} {tag}: the reference exhausts a queue or raises KeyError even for one episode")
            # the reference itself neither exhausted a queue nor raised KeyError
            assert len(info["Gs"]) == n_ep and all(v is not None for v in info["Gs"])
            k = f"s{s}_{tag}_"
            st = np.random.get_state()
            out.update({k + "n": np.int64(n_ep), k + "Gs": np.asarray(info["Gs"], np.float64), k + "rows": np.array(rows, np.int64), k + "z": np.int64(env.z),
                        k + "mt": np.concatenate([np.asarray(st[1], np.uint32), np.array([st[2]], np.uint32)])})
            if tag == "mc":
                out[k + "lengths"] = np.asarray(info["lengths"], np.int64)
                assert len(info["lengths"]) == n_ep
            else:
                out.update({k + "Q": Q, k + "td": np.asarray(info["TD_errors"], np.float64)})
                env2 = QueueEvaluator_impl(buf, nS=nS, nA=nA)
                env2.seed = lambda seed=None: None
                env2.reset_sampler(seed=s)
                np.random.seed(12345)
                Q2, info2 = fn(env2, n_ep, 1000 + s, 1)
                assert np.array_equal(Q, Q2) and len(info2["Qs"]) == len(rows) + 1
                out[k + "Qs9"] = info2["Qs"][:9]
            report.append((s, tag, n_ep, len(rows)))
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(name, report)


if __name__ == "__main__":
    for nm in ("queue_iid_2k", "queue_grid_300x15"):
        fixture(nm)
