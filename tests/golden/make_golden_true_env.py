#!/usr/bin/env python3
"""Generate tests/golden/true_env/*.npz by RUNNING THE REFERENCE's MyGridNavi and MyGridNaviCoords (offsim4rl/envs/gridworld.py:14-124,
187-211) under a fixed action sequence: reset, then step, and reset again whenever a step returns done.

Run from the repo root:   python tests/golden/make_golden_true_env.py
Needs /root/reference (read-only); nothing of it is copied -- the fixtures hold the actions that went in and the observations, rewards,
dones and `info` entries that came out.  The two classes are compiled from their file in memory; gym is not installed, so the names the
classes use of it (gym.Env with its seed(), spaces.Box, spaces.Discrete) are minimal stand-ins.

Cases: seeds 0, 4, 9; num_steps 3 and 15; goals (1, 1) and (4, 4); num_cells 5; 60 steps; actions default_rng(77).integers(0, 5, 60).
Per class one file, arrays stacked over the cases: seed, num_steps, goal [C, 2], actions [60], obs_before / obs_after [C, 60(, 2)] (what the
environment returned before and after each step, in the f64 the reference returned for the Coords class), reward, done, z, z_next, t.
"""
import ast
import copy
import itertools
import os
import random
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "true_env")
SEEDS, NUM_STEPS, GOALS, T = (0, 4, 9), (3, 15), ((1, 1), (4, 4)), 60


class _Env:
    def seed(self, seed=None):
        return [seed]


class _Space:
    def __init__(self, *a, **k):
        self.n = a[0] if a else None

    def contains(self, x):
        return 0 <= int(x) < self.n


_gym = types.SimpleNamespace(Env=_Env)
_spaces = types.SimpleNamespace(Box=_Space, Discrete=_Space)
_src = open(os.path.join(REF, "offsim4rl/envs/gridworld.py")).read()
_nodes = [n for n in ast.parse(_src).body if isinstance(n, ast.ClassDef) and n.name in ("MyGridNavi", "MyGridNaviCoords")]
_ns = {"np": np, "gym": _gym, "spaces": _spaces, "itertools": itertools, "random": random, "copy": copy}
exec(compile(ast.Module(body=_nodes, type_ignores=[]), "gridworld.py", "exec"), _ns)


def run(cls, discrete):
    actions = np.random.default_rng(77).integers(0, 5, T)
    rec = {k: [] for k in ("seed", "num_steps", "goal", "obs_before", "obs_after", "reward", "done", "z", "z_next", "t")}
    for seed in SEEDS:
        for ns in NUM_STEPS:
            for goal in GOALS:
                env = cls(num_cells=5, num_steps=ns, seed=seed)
                env.reset_task(goal)
                obs = env.reset()
                rows = {k: [] for k in ("obs_before", "obs_after", "reward", "done", "z", "z_next", "t")}
                for a in actions:
                    rows["obs_before"].append(obs)
                    obs, r, done, info = env.step(int(a))
                    rows["obs_after"].append(obs)
                    rows["reward"].append(r)
                    rows["done"].append(done)
                    for k in ("z", "z_next", "t"):
                        rows[k].append(info[k])
                    if done:
                        obs = env.reset()
                rec["seed"].append(seed)
                rec["num_steps"].append(ns)
                rec["goal"].append(goal)
                for k, v in rows.items():
                    rec[k].append(v)
    odt = np.int64 if discrete else np.float64
    return dict(actions=actions.astype(np.int64), seed=np.array(rec["seed"], np.int64), num_steps=np.array(rec["num_steps"], np.int64),
                goal=np.array(rec["goal"], np.int64), obs_before=np.array(rec["obs_before"], odt), obs_after=np.array(rec["obs_after"], odt),
                reward=np.array(rec["reward"], np.float64), done=np.array(rec["done"], bool), z=np.array(rec["z"], np.int64),
                z_next=np.array(rec["z_next"], np.int64), t=np.array(rec["t"], np.int64))


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "grid.npz"), **run(_ns["MyGridNavi"], True))
    np.savez_compressed(os.path.join(OUT, "grid_coords.npz"), **run(_ns["MyGridNaviCoords"], False))
    print("wrote", OUT)
