#!/usr/bin/env python3
"""The tabular drivers on the true grid world (offsim_eval_env / offsim_eval_env_pop) on the 5 x 5 grid with 15 steps, goal (4, 4):

  evalMC of the uniform policy, 1 / 64 / 4096 seeds x 1000 episodes, lane-per-rollout (k_eval_env_mc);
  the same through the wavefront-per-rollout instance (k_eval_env<false>, OFFSIM_ENV_EVALMC_WAVE=1, measured in a child process because the
  library reads the variable once);
  the same for a stack of 64 policies (uniform mixed with the shortest path in 64 proportions);
  epsilon-greedy Q-learners, L = 1 / 8 / 64 on 64 seeds x 100 episodes through TDPopulation.run_env, against one qlearn_env call per learner
  and seed;
  ONE seed through the host mirror's Python loop (evalMC, 1000 episodes).

Every figure is the median of --repeats (5) synchronised wall times after one warm-up run.  Both routes must give the same values for seed 0
(asserted).  Every line goes to stdout and to --out (default profiles/env_drivers_bench.jsonl) as JSON.

  python tools/bench_env_drivers.py [--out FILE] [--repeats 5]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rl_offline_simulation_amd.evaluators import BatchedGridWorld, GridWorld, TDPopulation, qlearn_env  # noqa: E402

GAMMA, EPISODES, TD_EPISODES, TD_SEEDS = 0.9, 1000, 100, 64


def world():
    return GridWorld(5, 15, (4, 4))


def uniform(w):
    return np.full((w.nS, 5), 0.2)


def stack(w, n):
    path = np.zeros((w.nS, 5))
    for o in range(w.nS):
        x, y = o % 5, o // 5
        path[o, 2 if x < 4 else 1 if y < 4 else 0] = 1.0
    return np.stack([(1 - k / n) * uniform(w) + (k / n) * path for k in range(n)])


def timed(f, repeats):
    out, ms = None, []
    for _ in range(repeats + 1):  # (the first run warms up: module load, allocations)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = sorted(ms[1:])
    return out, dict(ms_median=ms[len(ms) // 2], ms_min=ms[0], ms_max=ms[-1], repeats=repeats)


def evalmc(w, S, repeats, n_pol=0):
    b = BatchedGridWorld(w, S)
    pi = stack(w, n_pol) if n_pol else uniform(w)

    def f():
        b.set_action_seeds(np.arange(S))
        return b.eval_mc_population(pi, GAMMA, EPISODES) if n_pol else b.eval_mc(pi, GAMMA, EPISODES)
    o, t = timed(f, repeats)
    steps = int(o["steps"].sum())
    first = (o["sum_g"][0, 0] if n_pol else o["sum_g"][0]).item() / EPISODES
    return dict(what="evalMC", kernel=o["_kernel"], seeds=S, policies=max(n_pol, 1), episodes=EPISODES, steps=steps,
                steps_per_s=steps / (t["ms_median"] * 1e-3), value_seed0=first, **t)


def host_loop(w, repeats):
    pi = uniform(w)

    def f():
        rng, total, steps = np.random.default_rng(0), 0.0, 0
        for e in range(EPISODES):
            S, G_, t, done = w.reset(seed=e), 0.0, 0, False
            while not done:
                S, R, done, _ = w.step(rng.choice(5, p=pi[S]))
                G_ = G_ + GAMMA ** t * R
                t += 1
            total += G_
            steps += t
        return total, steps
    (total, steps), t = timed(f, repeats)
    return dict(what="evalMC", kernel="host mirror, Python loop", seeds=1, policies=1, episodes=EPISODES, steps=steps, steps_per_s=steps / (t["ms_median"] * 1e-3),
                value_seed0=total / EPISODES, **t)


def eps_greedy(Q, args):
    eps = args["epsilon"]
    pi = np.ones_like(Q) * eps / Q.shape[1]
    for s in range(len(Q)):
        pi[s, np.random.choice(np.where(Q[s] == np.max(Q[s]))[0])] = 1 - eps + eps / Q.shape[1]
    return pi


def learners(w, n_l, repeats):
    alphas = [0.05 + 0.4 * k / max(n_l - 1, 1) for k in range(n_l)]
    seeds = np.arange(TD_SEEDS)
    pop = TDPopulation("qlearn", alphas, GAMMA, epsilon=0.3, behaviour="eps_greedy")
    res, t = timed(lambda: pop.run_env(w, seeds, TD_EPISODES), repeats)
    steps = int(res.steps.sum())
    line = dict(what="qlearn eps-greedy", route="TDPopulation.run_env", learners=n_l, seeds=TD_SEEDS, episodes=TD_EPISODES, steps=steps,
                steps_per_s=steps / (t["ms_median"] * 1e-3), return_l0_seed0=float(res.Gs[0, 0].sum()), **t)
    # one qlearn_env call per learner and seed; timed on the first learner's seeds and scaled (every call is one launch of one rollout)
    def f():
        return [qlearn_env(w, TD_EPISODES, eps_greedy, GAMMA, alpha=alphas[0], epsilon=0.3, seed=int(s))[1]["Gs"] for s in seeds[:8]]
    Gs, t1 = timed(f, repeats)
    assert np.array_equal(res.Gs[0, 0].cpu().numpy(), Gs[0]), "both routes must give the same returns for seed 0"
    line["return_l0_seed0"] = float(np.sum(Gs[0]))
    per_call = t1["ms_median"] / 8
    single = dict(what="qlearn eps-greedy", route="one qlearn_env call per learner and seed", learners=n_l, seeds=TD_SEEDS, episodes=TD_EPISODES,
                  ms_per_call_median=per_call, calls_timed=8, ms_all_calls_extrapolated=per_call * n_l * TD_SEEDS, return_l0_seed0=float(np.sum(Gs[0])),
                  repeats=repeats)
    return line, single


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "env_drivers_bench.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--child-wave", action="store_true", help="(internal) the evalMC lines of the wavefront-per-rollout instance, to stdout")
    a = ap.parse_args()
    w = world()
    if a.child_wave:
        for S in (1, 64, 4096):
            print(json.dumps(evalmc(w, S, a.repeats)), flush=True)
        return
    lines = [evalmc(w, S, a.repeats) for S in (1, 64, 4096)]
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-wave", "--repeats", str(a.repeats)], check=True, capture_output=True,
                           text=True, env=dict(os.environ, OFFSIM_ENV_EVALMC_WAVE="1"))
    wave = [json.loads(s) for s in child.stdout.splitlines() if s.startswith("{")]
    assert [l["kernel"] for l in wave] == ["k_eval_env_mc"] * 3  # (the Python label; the instance is the child's)
    for l in wave:
        l["kernel"] = "k_eval_env<false> (wavefront per rollout)"
    lines += wave
    lines += [evalmc(w, S, a.repeats, n_pol=64) for S in (1, 64, 4096)]
    lines.append(host_loop(w, a.repeats))
    v0 = {l["value_seed0"] for l in lines if l["seeds"] >= 1 and l["policies"] >= 1}
    assert len(v0) == 1, f"every evalMC route must give the same value for seed 0 (stack row 0 is the uniform policy): {v0}"
    for n_l in (1, 8, 64):
        lines += learners(w, n_l, a.repeats)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for l in lines:
            print(json.dumps(l))
            f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
