#!/usr/bin/env python3
"""Generate tests/golden/queue_collect/*.npz by RUNNING THE REFERENCE's QueueEvaluator_impl (offsim4rl/evaluators/queue_evaluator.py:90-131)
under the loop of its PPOAgent (offsim4rl/agents/ppo.py:258-279): reset, then step with an action the agent draws from its policy at the
current observation, until done or the step cap, then reset again.

Run from the repo root:   python tests/golden/make_golden_queue_collect.py
Needs /root/reference (read-only); nothing of it is copied -- the fixtures hold the outputs the reference produced for the inputs of
tests/golden/queue_iid_2k.npz and queue_grid_300x15.npz.  QueueEvaluator_impl is compiled from its file in memory, as
make_golden_queue_drivers.py does it.  The observation of a buffer entry is the pair ("obs" | "next", row), so that what reset and step
return names the row the policy is asked at.

The policy is a fixed per-row table (P_next[i] at next_obs of row i, P_init[i] at obs of row i; f32 softmax rows from default_rng(77)),
and the action rule is the package's, not the agent's np.random.choice on the global stream:
    cdf = cumsum(p as f64); cdf /= cdf[-1]; A = cdf.searchsorted(default_rng(action_seed).random(), side='right')
Per input, sampler seed s in (0, 4, 9) with action seed 500 + s, and cap in (8, 0 = none): T = 60 steps -- rows served, actions drawn, flags
(OFFSIM_COLLECT_*), the status the loop ended with, and where the action stream stands.
"""
import ast
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "queue_collect")
SEEDS, CAPS, T = (0, 4, 9), (8, 0), 60
SERVED, TERMINATED, TRUNCATED, RESET, ALIVE = 1, 2, 4, 8, 16
ST_OK, ST_EXHAUSTED, ST_NO_INIT, ST_KEYERROR = 0, 1, 2, 3

_src = open(os.path.join(REF, "offsim4rl/evaluators/queue_evaluator.py")).read()
_cls = next(n for n in ast.parse(_src).body if isinstance(n, ast.ClassDef) and n.name == "QueueEvaluator_impl")
_ns = {"np": np, "itertools": __import__("itertools")}
exec(compile(ast.Module(body=[_cls], type_ignores=[]), "queue_evaluator.py", "exec"), _ns)
QueueEvaluator_impl = _ns["QueueEvaluator_impl"]


def softmax32(x):
    e = np.exp(x - x.max(1, keepdims=True)).astype(np.float32)
    return (e / e.sum(1, keepdims=True, dtype=np.float32)).astype(np.float32)


def fixture(name):
    d = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    z, a, r, zn, done, p_log, t0 = (d["in_" + k] for k in ("z", "a", "r", "z_next", "done", "p_log", "t0"))
    N, nA = len(z), p_log.shape[1]
    nS = int(max(z.max(), zn.max())) + 1
    buf = [(("obs", i), int(a[i]), float(r[i]), ("next", i), bool(done[i]), p_log[i], {"t": 0 if t0[i] else 1, "z": int(z[i]), "next_z": int(zn[i])})
           for i in range(N)]
    g = np.random.default_rng(77)
    P_next, P_init = softmax32(g.standard_normal((N, nA)) * 2), softmax32(g.standard_normal((N, nA)) * 2)
    out = dict(P_next=P_next, P_init=P_init, seeds=np.array(SEEDS, np.int64), caps=np.array(CAPS, np.int64), T=np.int64(T))
    report = []
    for s in SEEDS:
        for cap in CAPS:
            env = QueueEvaluator_impl(buf, nS=nS, nA=nA)
            env.reset_sampler(seed=s)
            gen = np.random.default_rng(500 + s)
            rows, acts, flags = np.full(T, -1, np.int64), np.full(T, -1, np.int64), np.zeros(T, np.uint8)
            obs, status, ep_t = env.reset(), ST_OK, 0
            assert obs is not None
            for i in range(T):
                p = P_init[obs[1]] if obs[0] == "obs" else P_next[obs[1]]
                cdf = np.cumsum(p.astype(np.float64))
                cdf /= cdf[-1]
                A = int(cdf.searchsorted(gen.random(), side="right"))
                acts[i] = A
                try:
                    nxt, _, dn, info = env.step(A)
                except KeyError:
                    status = ST_KEYERROR
                    break
                if nxt is None:
                    status = ST_EXHAUSTED
                    break
                assert info["a"] == A and nxt[0] == "next"
                rows[i] = nxt[1]
                ep_t += 1
                trunc = cap > 0 and ep_t >= cap
                fl, obs, alive = SERVED | (TERMINATED if dn else 0) | (TRUNCATED if trunc else 0), nxt, True
                if dn or trunc:
                    ep_t = 0
                    obs = env.reset()
                    if obs is None:
                        status, alive = ST_NO_INIT, False
                    else:
                        fl |= RESET
                flags[i] = fl | (ALIVE if alive else 0)
                if obs is None:
                    break
            k = f"s{s}_cap{cap}_"
            st = gen.bit_generator.state["state"]
            out.update({k + "rows": rows, k + "actions": acts, k + "flags": flags, k + "status": np.int64(status),
                        k + "rng": np.array([st["state"] >> 64, st["state"] & ((1 << 64) - 1)], np.uint64)})
            report.append((s, cap, int((rows >= 0).sum()), status))
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(name, report)


if __name__ == "__main__":
    for nm in ("queue_iid_2k", "queue_grid_300x15"):
        fixture(nm)
