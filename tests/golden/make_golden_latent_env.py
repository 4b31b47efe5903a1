#!/usr/bin/env python3
"""Generate tests/golden/latent_env/coords_mlp.npz by RUNNING THE REFERENCE's own tabular drivers on its own MyGridNaviCoords
(offsim4rl/envs/gridworld.py:187-211) behind a seeded 2-16-25 MLP encoder:

  z_expSARSA   tabular.z_expSARSA(env, ..., latent_state_func=f) (offsim4rl/agents/tabular.py:193-245) with f the encoder's arg max;
  evalMC, qlearn_eps, qlearn_eps_sched   tabular.evalMC / tabular.qlearn with epsilon_greedy_policy (epsilon 0.3, and the schedule
               1 / (1 + episode)) on MyGridNaviCoords behind a thin adapter written here, which returns z = f(S) and has nS and nA.

Run from the repo root:   python tests/golden/make_golden_latent_env.py <path to a checkout of offsim4rl>
Nothing of the reference is copied: its classes and tabular.py are compiled from their files in memory, and the fixture holds the settings
that went in and the returns, lengths, Q tables, TD errors and NumPy global states that came out.  gym and tqdm are not installed, so the
names the sources use of them are minimal stand-ins (as in make_golden_env_drivers.py).

The encoder: f(S) = first arg max of the f64 forward Linear(2, 16) -> LeakyReLU(0.01) -> Linear(16, 25) on the observation ROUNDED TO F32
(what the device's encoder reads), weights from default_rng(7) times `scale`, stored as f32: W1 = 5 N(0, 1), b1 = -W1 (0.55, 0.55) + N(0, 1)
-- the hidden units cut through the middle of the grid, so the 25 cells spread over several latent states (a plain N(0, 1) network maps
the whole grid to one or two) --, W2 = N(0, 1), b2 = 0.1 N(0, 1); the recipe asserts at least 4 distinct z.  It ASSERTS that the
smallest top-2 logit gap over every observation of every run exceeds 1e-3 -- far above any f32 rounding of these sums, so every f32
summation order gives the same z -- doubling `scale` until it holds; the gap and the scale are stored.

Runs: goals (1, 1) and (4, 4) x num_steps 3 and 15 x seeds 0 and 9 x the four drivers, 6 episodes each, gamma 0.9, alpha 0.1, save_Q = 1,
NumPy's global stream seeded with 12345 before every run.  Arrays (run i of `runs`, "driver|gx|gy|num_steps|seed"):
  W1, b1, W2, b2, scale, min_gap, n_latent   the encoder, its smallest gap and the distinct z over all runs
  pi [25, 5]                  the policy of evalMC and z_expSARSA
  Gs [n, 6], lengths [n, 6]   returns; lengths of evalMC (-1 elsewhere)
  td_steps [n], TD_errors     TD errors of the learner runs, concatenated
  Q [n, 25, 5]                the learner's final Q (zeros elsewhere)
  Qs_idx, Qs_val              Qs of a learner run: the flat index of the entry step k changed and its new value (the recipe checks that
                              this rebuilds Qs exactly)
  mt_keys [m, 624], mt_key [n], mt_pos [n]       the global MT19937 state after the run
"""
import ast
import copy
import itertools
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "latent_env")
GOALS, NUM_STEPS, SEEDS, N_EP, GAMMA, ALPHA = ((1, 1), (4, 4)), (3, 15), (0, 9), 6, 0.9, 0.1
DRIVERS = ("evalMC", "qlearn_eps", "qlearn_eps_sched", "z_expSARSA")
EPS_SCHED = lambda e: 1.0 / (1.0 + e)  # noqa: E731
D_O, H, N_Z, NA = 2, 16, 25, 5


class _Env:
    def seed(self, seed=None):
        return [seed]


class _Space:
    def __init__(self, *a, **k):
        self.n = a[0] if a else None

    def contains(self, x):
        return 0 <= int(x) < self.n


def load_reference(ref):
    gym = types.SimpleNamespace(Env=_Env)
    spaces = types.SimpleNamespace(Box=_Space, Discrete=_Space)
    src = open(os.path.join(ref, "offsim4rl/envs/gridworld.py")).read()
    nodes = [n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name in ("MyGridNavi", "MyGridNaviCoords")]
    ns = {"np": np, "gym": gym, "spaces": spaces, "itertools": itertools, "random": random, "copy": copy}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), "gridworld.py", "exec"), ns)
    sys.modules["tqdm"] = types.SimpleNamespace(tqdm=lambda it, **k: it)
    tab = {}
    exec(compile(open(os.path.join(ref, "offsim4rl/agents/tabular.py")).read(), "tabular.py", "exec"), tab)
    return ns, tab


class Encoder:
    def __init__(self, scale):
        g = np.random.default_rng(7)
        W1 = 5 * scale * g.standard_normal((H, D_O))
        b1 = -(W1 @ np.array([0.55, 0.55])) + scale * g.standard_normal(H)  # the hidden units cut through the middle of the grid
        W2, b2 = scale * g.standard_normal((N_Z, H)), 0.1 * scale * g.standard_normal(N_Z)
        self.w = tuple(a.astype(np.float32) for a in (W1, b1, W2, b2))
        self.min_gap, self.seen = np.inf, set()

    def __call__(self, S):
        W1, b1, W2, b2 = (a.astype(np.float64) for a in self.w)
        x = np.asarray(S, np.float64).astype(np.float32).astype(np.float64)
        h = W1 @ x + b1
        lo = W2 @ np.where(h > 0, h, np.float64(np.float32(0.01)) * h) + b2
        top = np.sort(lo)[::-1]
        self.min_gap = min(self.min_gap, float(top[0] - top[1]))
        self.seen.add(int(np.argmax(lo)))
        return int(np.argmax(lo))


class Adapter:
    """MyGridNaviCoords seen through the encoder: what tabular.evalMC / qlearn index their tables with is z"""

    def __init__(self, env, f):
        self.env, self.f, self.nS, self.nA = env, f, N_Z, NA

    def seed(self, seed=None):
        return self.env.seed(seed)

    def reset(self, seed=None):
        return self.f(self.env.reset(seed=seed))

    def step(self, a):
        S_, R, done, info = self.env.step(a)
        return self.f(S_), R, done, info


def generate(ns, tab, scale):
    f = Encoder(scale)
    pi = np.random.default_rng(5).dirichlet(np.full(NA, 1.5), N_Z)
    rec = {k: [] for k in ("runs", "Gs", "lengths", "td_steps", "TD_errors", "Q", "Qs_idx", "Qs_val", "mt_key", "mt_pos")}
    keys = []
    for goal in GOALS:
        for num_steps in NUM_STEPS:
            for seed in SEEDS:
                for drv in DRIVERS:
                    env = ns["MyGridNaviCoords"](num_cells=5, num_steps=num_steps, seed=seed)
                    env.reset_task(goal)
                    np.random.seed(12345)
                    Q, info, lengths = np.zeros((N_Z, NA)), {}, np.full(N_EP, -1)
                    if drv == "evalMC":
                        Gs, lengths = tab["evalMC"](Adapter(env, f), N_EP, pi, GAMMA, seed=seed)
                        info = {"Gs": Gs}
                    elif drv == "z_expSARSA":
                        Q, info = tab["z_expSARSA"](env, N_EP, pi, GAMMA, alpha=ALPHA, save_Q=1, show_tqdm=False, seed=seed, latent_state_func=f)
                    else:
                        eps = EPS_SCHED if drv == "qlearn_eps_sched" else 0.3
                        Q, info = tab["qlearn"](Adapter(env, f), N_EP, tab["epsilon_greedy_policy"], GAMMA, alpha=ALPHA, epsilon=eps, save_Q=1,
                                                show_tqdm=False, seed=seed)
                    rec["runs"].append(f"{drv}|{goal[0]}|{goal[1]}|{num_steps}|{seed}")
                    rec["Gs"].append(info["Gs"])
                    rec["lengths"].append(lengths)
                    rec["Q"].append(Q)
                    if "Qs" in info:
                        Qs = info["Qs"]
                        n = len(info["TD_errors"])
                        assert len(Qs) == n + 1 and not Qs[0].any()
                        idx, val = [], []
                        for k in range(n):
                            ch = np.flatnonzero(Qs[k + 1].ravel() != Qs[k].ravel())
                            assert len(ch) <= 1
                            idx.append(int(ch[0]) if len(ch) else 0)
                            val.append(Qs[k + 1].flat[idx[-1]])
                        back = np.zeros_like(Qs)
                        for k, (i, v) in enumerate(zip(idx, val)):
                            back[k + 1] = back[k]
                            back[k + 1].flat[i] = v
                        assert np.array_equal(back, Qs)
                        rec["Qs_idx"].extend(idx)
                        rec["Qs_val"].extend(val)
                        rec["TD_errors"].extend(info["TD_errors"])
                        rec["td_steps"].append(n)
                    else:
                        rec["td_steps"].append(0)
                    st = np.random.get_state()
                    key = st[1].tobytes()
                    if key not in keys:
                        keys.append(key)
                    rec["mt_key"].append(keys.index(key))
                    rec["mt_pos"].append(st[2])
    i64 = lambda k: np.array(rec[k], np.int64)  # noqa: E731
    W1, b1, W2, b2 = f.w
    return f.min_gap, dict(runs=np.array(rec["runs"]), W1=W1, b1=b1, W2=W2, b2=b2, scale=np.float64(scale), min_gap=np.float64(f.min_gap), n_latent=np.int64(len(f.seen)), pi=pi,
                           gamma=np.float64(GAMMA), alpha=np.float64(ALPHA), n_episodes=np.int64(N_EP), Gs=np.array(rec["Gs"], np.float64),
                           lengths=i64("lengths"), td_steps=i64("td_steps"), TD_errors=np.array(rec["TD_errors"], np.float64),
                           Q=np.array(rec["Q"], np.float64), Qs_idx=i64("Qs_idx"), Qs_val=np.array(rec["Qs_val"], np.float64),
                           mt_keys=np.array([np.frombuffer(k, np.uint32) for k in keys]), mt_key=i64("mt_key"), mt_pos=i64("mt_pos"))


if __name__ == "__main__":
    ns, tab = load_reference(sys.argv[1])
    os.makedirs(OUT, exist_ok=True)
    scale = 1.0
    gap, data = generate(ns, tab, scale)
    while not gap > 1e-3 and scale < 1024:
        scale *= 2.0
        gap, data = generate(ns, tab, scale)
    assert gap > 1e-3, f"the smallest top-2 logit gap {gap} does not exceed 1e-3"
    assert int(data["n_latent"]) >= 4, "the encoder maps the runs to fewer than 4 latent states"
    np.savez_compressed(os.path.join(OUT, "coords_mlp.npz"), **data)
    print("wrote", OUT, "scale", scale, "min gap", gap)
