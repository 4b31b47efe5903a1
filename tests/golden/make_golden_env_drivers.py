#!/usr/bin/env python3
"""Generate tests/golden/env_drivers/*.npz by RUNNING THE REFERENCE's own tabular drivers evalMC, qlearn, expSARSA and rollout
(offsim4rl/agents/tabular.py) on its own MyGridNavi, MyGridNaviNoise (augmented_state = 2 and 3) and MyGridNaviModuloCounter
(counter_limit = 4) (offsim4rl/envs/gridworld.py) with a fixed goal.

Run from the repo root:   python tests/golden/make_golden_env_drivers.py <path to a checkout of offsim4rl>
Nothing of the reference is copied: its classes and tabular.py are compiled from their files in memory, and the fixtures hold the settings
that went in and the returns, lengths, Q tables, TD errors, memories and NumPy global states that came out.  gym and tqdm are not
installed, so the names the sources use of them (gym.Env with its seed(), spaces.Box, spaces.Discrete, tqdm) are minimal stand-ins.

One file per world.  Runs: goals (1, 1) and (4, 4) x num_steps 3 and 15 x seeds 0 and 9 x the drivers of DRIVERS, 7 episodes each, gamma 0.9,
alpha 0.1, save_Q = 1, NumPy's global stream seeded with 12345 before every run.  Arrays (run i of `runs`, "driver|gx|gy|num_steps|seed"):
  pi [nS, 5]                  the policy of evalMC, rollout and expSARSA
  Gs [n, 7], lengths [n, 7]   returns; lengths of evalMC (-1 elsewhere)
  steps [n]                   steps of the run; the per-step arrays below are the runs' concatenated (evalMC records none: 0)
  S, A, R, S_, done, p [., 5], z, z_next, t      the memory
  td_steps [n], TD_errors     TD errors of the learner runs, concatenated
  Q [n, nS, 5]                the learner's final Q (zeros elsewhere)
  Qs_idx, Qs_val              Qs of a learner run, which holds steps + 1 tables and changes one entry per step: the flat index of the entry
                              step k changed and its new value (concatenated like TD_errors; the recipe checks that this rebuilds Qs exactly)
  mt_keys [m, 624], mt_key [n], mt_pos [n]       the global MT19937 state after the run: its key words (one row per distinct key) and position
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
OUT = os.path.join(ROOT, "tests", "golden", "env_drivers")
GOALS, NUM_STEPS, SEEDS, N_EP, GAMMA, ALPHA = ((1, 1), (4, 4)), (3, 15), (0, 9), 7, 0.9, 0.1
DRIVERS = ("evalMC", "rollout", "qlearn_uniform", "qlearn_eps", "qlearn_eps_sched", "qlearn_greedy", "qlearn_soft", "expSARSA")
EPS_SCHED = lambda e: 1.0 / (1.0 + e)  # noqa: E731
WORLDS = {"plain": ("MyGridNavi", {}, 1), "noise2": ("MyGridNaviNoise", {"augmented_state": 2}, 2), "noise3": ("MyGridNaviNoise", {"augmented_state": 3}, 3),
          "counter4": ("MyGridNaviModuloCounter", {"counter_limit": 4}, 4)}


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
    nodes = [n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name in ("MyGridNavi", "MyGridNaviNoise", "MyGridNaviModuloCounter")]
    ns = {"np": np, "gym": gym, "spaces": spaces, "itertools": itertools, "random": random, "copy": copy}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), "gridworld.py", "exec"), ns)
    sys.modules["tqdm"] = types.SimpleNamespace(tqdm=lambda it, **k: it)
    tab = {}
    exec(compile(open(os.path.join(ref, "offsim4rl/agents/tabular.py")).read(), "tabular.py", "exec"), tab)
    return ns, tab


def run_world(ns, tab, cls, kw, factor):
    nS = 25 * factor
    pi = np.random.default_rng(5).dirichlet(np.full(5, 1.5), nS)
    rec = {k: [] for k in ("runs", "Gs", "lengths", "steps", "S", "A", "R", "S_", "done", "p", "z", "z_next", "t", "td_steps", "TD_errors", "Q", "Qs_idx",
                           "Qs_val", "mt_key", "mt_pos")}
    keys = []
    for goal in GOALS:
        for num_steps in NUM_STEPS:
            for seed in SEEDS:
                for drv in DRIVERS:
                    env = ns[cls](num_cells=5, num_steps=num_steps, seed=seed, **kw)
                    env.reset_task(goal)
                    np.random.seed(12345)
                    Q, info, lengths = np.zeros((nS, 5)), None, np.full(N_EP, -1)
                    if drv == "evalMC":
                        Gs, lengths = tab["evalMC"](env, N_EP, pi, GAMMA, seed=seed)
                        info = {"Gs": Gs, "memory": []}
                    elif drv == "rollout":
                        info = tab["rollout"](env, N_EP, pi, GAMMA, show_tqdm=False, seed=seed)
                    elif drv == "expSARSA":
                        Q, info = tab["expSARSA"](env, N_EP, pi, GAMMA, alpha=ALPHA, save_Q=1, show_tqdm=False, seed=seed)
                    else:
                        beh = {"qlearn_uniform": "uniformly_random_policy", "qlearn_eps": "epsilon_greedy_policy", "qlearn_eps_sched": "epsilon_greedy_policy",
                               "qlearn_greedy": "greedy_policy", "qlearn_soft": "soft_greedy_policy"}[drv]
                        eps = EPS_SCHED if drv == "qlearn_eps_sched" else 0.3
                        Q, info = tab["qlearn"](env, N_EP, tab[beh], GAMMA, alpha=ALPHA, epsilon=eps, save_Q=1, show_tqdm=False, seed=seed)
                    mem = info["memory"]
                    rec["runs"].append(f"{drv}|{goal[0]}|{goal[1]}|{num_steps}|{seed}")
                    rec["Gs"].append(info["Gs"])
                    rec["lengths"].append(lengths)
                    rec["steps"].append(len(mem))
                    for j, k in enumerate(("S", "A", "R", "S_", "done", "p")):
                        rec[k].extend(m[j] for m in mem)
                    for k in ("z", "z_next", "t"):
                        rec[k].extend(m[6][k] for m in mem)
                    assert all(np.array_equal(m[6]["task"], goal) and m[6]["task_id"] == goal[0] + 5 * goal[1] for m in mem)
                    rec["Q"].append(Q)
                    if "Qs" in info:
                        Qs = info["Qs"]
                        assert len(Qs) == len(mem) + 1 and not Qs[0].any()
                        idx = [m[0] * 5 + m[1] for m in mem]
                        val = [Qs[k + 1].flat[i] for k, i in enumerate(idx)]
                        back = np.zeros_like(Qs)
                        for k, (i, v) in enumerate(zip(idx, val)):
                            back[k + 1] = back[k]
                            back[k + 1].flat[i] = v
                        assert np.array_equal(back, Qs)
                        rec["Qs_idx"].extend(idx)
                        rec["Qs_val"].extend(val)
                        rec["TD_errors"].extend(info["TD_errors"])
                        rec["td_steps"].append(len(mem))
                    else:
                        rec["td_steps"].append(0)
                    st = np.random.get_state()
                    key = st[1].tobytes()
                    if key not in keys:
                        keys.append(key)
                    rec["mt_key"].append(keys.index(key))
                    rec["mt_pos"].append(st[2])
    i64 = lambda k: np.array(rec[k], np.int64)  # noqa: E731
    return dict(runs=np.array(rec["runs"]), pi=pi, factor=np.int64(factor), gamma=np.float64(GAMMA), alpha=np.float64(ALPHA), n_episodes=np.int64(N_EP),
                Gs=np.array(rec["Gs"], np.float64), lengths=i64("lengths"), steps=i64("steps"), S=i64("S"), A=i64("A"), R=np.array(rec["R"], np.float64),
                S_=i64("S_"), done=np.array(rec["done"], bool), p=np.array(rec["p"], np.float64).reshape(-1, 5), z=i64("z"), z_next=i64("z_next"), t=i64("t"),
                td_steps=i64("td_steps"), TD_errors=np.array(rec["TD_errors"], np.float64), Q=np.array(rec["Q"], np.float64), Qs_idx=i64("Qs_idx"),
                Qs_val=np.array(rec["Qs_val"], np.float64), mt_keys=np.array([np.frombuffer(k, np.uint32) for k in keys]), mt_key=i64("mt_key"),
                mt_pos=i64("mt_pos"))


if __name__ == "__main__":
    ns, tab = load_reference(sys.argv[1])
    os.makedirs(OUT, exist_ok=True)
    for name, (cls, kw, factor) in WORLDS.items():
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **run_world(ns, tab, cls, kw, factor))
    print("wrote", OUT)
