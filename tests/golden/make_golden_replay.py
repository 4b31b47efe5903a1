#!/usr/bin/env python3
"""Generate tests/golden/replay/*.npz by RUNNING THE REFERENCE's qlearn(..., memory=...) (offsim4rl/agents/tabular.py:90-104): the Q-learning
update swept over logged (S, A, R, S', done) tuples in log order.

Run from the repo root:   python tests/golden/make_golden_replay.py
Needs /root/reference (read-only); nothing of it is copied -- the fixtures hold the outputs the reference produced for the inputs of
tests/golden/queue_iid_2k.npz and queue_grid_300x15.npz.  agents/tabular.py is loaded by path with tqdm stubbed, as
make_golden_queue_drivers.py does.  The memory is the fixture's in_* columns as 5-tuples of Python ints, floats and bools (rewards: an exact
widening of the f32 column).  Q_init is the one of make_golden_queue_drivers.py: the second draw of default_rng(42).

Per input, gamma = 0.9, save_Q = 1:
  c   alpha = 0.1, Q_init None (zeros)
  s   alpha(e) = 0.5 / (1 + 0.1 e), the random Q_init
and for each: Q, TD_errors, Qs[:9], Qs[::500] and the shape of Qs (the whole of it is not kept).
"""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "replay")
GAMMA, ALPHA = 0.9, 0.1
ALPHA_SCHED = lambda e: 0.5 / (1.0 + 0.1 * e)  # noqa: E731

sys.modules.setdefault("tqdm", types.SimpleNamespace(tqdm=lambda it, **kw: it))
spec = importlib.util.spec_from_file_location("ref_tabular", os.path.join(REF, "offsim4rl/agents/tabular.py"))
ref_tab = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref_tab)


def fixture(name):
    d = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    z, a, r, zn, done, p_log = (d["in_" + k] for k in ("z", "a", "r", "z_next", "done", "p_log"))
    N, nA = len(z), p_log.shape[1]
    assert z.min() >= 0 and zn.min() >= 0
    nS = int(max(z.max(), zn.max())) + 1
    memory = [(int(z[i]), int(a[i]), float(r[i]), int(zn[i]), bool(done[i])) for i in range(N)]
    g = np.random.default_rng(42)
    g.dirichlet(np.full(nA, 1.5), nS)
    q_init = g.standard_normal((nS, nA)) * 0.1
    env = types.SimpleNamespace(nS=nS, nA=nA)
    out = dict(q_init=q_init, nS=np.int64(nS), nA=np.int64(nA), gamma=np.float64(GAMMA), alpha=np.float64(ALPHA), n_ep=np.int64(int(np.sum(done != 0))))
    for tag, kw in (("c", dict(alpha=ALPHA, Q_init=None)), ("s", dict(alpha=ALPHA_SCHED, Q_init=q_init))):
        Q, info = ref_tab.qlearn(env, None, None, GAMMA, memory=memory, save_Q=1, **kw)
        Qs, td = info["Qs"], info["TD_errors"]
        assert Qs.shape == (N + 1, nS, nA) and td.shape == (N,) and np.isfinite(Q).all() and np.isfinite(td).all() and info["memory"] is memory
        assert np.array_equal(Qs[-1], Q)
        out.update({tag + "_Q": Q, tag + "_td": td, tag + "_Qs9": Qs[:9], tag + "_Qs500": Qs[::500], tag + "_Qs_shape": np.array(Qs.shape, np.int64)})
        Q1, info1 = ref_tab.qlearn(env, None, None, GAMMA, memory=memory, save_Q=0, **kw)
        assert np.array_equal(Q1, Q) and info1["Qs"].shape == (1, nS, nA)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(name, N, "steps", int(out["n_ep"]), "episodes")


if __name__ == "__main__":
    for nm in ("queue_iid_2k", "queue_grid_300x15"):
        fixture(nm)
