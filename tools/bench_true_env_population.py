#!/usr/bin/env python3
"""evalMC of a population of actors in the true environment (evalmc_rollouts_true_env, offsim_eval_env_obs): CartPole, 4-64-64-2 tanh
actors, 64 seeds x 10 episodes, max_episode_steps = 500.  For L = 1 / 8 / 64 actors, three routes to the same [L, 64] values:

  population      ONE evalmc_rollouts_true_env call for all L actors;
  per actor       one evalmc_rollouts_true_env call per actor, looped;
  collect         what there was before: per actor one VectorCartPole(64).collect of T = 10 * 500 steps (the only bound that holds 10
                  episodes of every environment), the [T, 64] records copied back and the first 10 episodes of every environment summed on
                  the host.  Timed on at most --collect-actors (8) actors and scaled to L.

Every figure is the median of --repeats (5) synchronised wall times after one warm-up run.  All routes must give the same values for
actor 0 (asserted, bit for bit).  Every line goes to stdout and to --out (default profiles/true_env_population_bench.jsonl) as JSON.

--kernel-only: run the L = 64 population call once after a warm-up and nothing else (for a rocprofv3 --kernel-trace --stats pass).

  python tools/bench_true_env_population.py [--out FILE] [--repeats 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rl_offline_simulation_amd.evaluators import MLPPolicy, VectorCartPole, evalmc_rollouts_true_env  # noqa: E402
from rl_offline_simulation_amd.evaluators.rollout_io import _gamma_pow  # noqa: E402

GAMMA, SEEDS, EPISODES, CAP = 0.99, 64, 10, 500


def actors(n):
    g = np.random.default_rng(0)
    widths = (4, 64, 64, 2)
    return [MLPPolicy([((g.standard_normal((b, a)) / np.sqrt(a)).astype(np.float32), np.zeros(b, np.float32)) for a, b in zip(widths, widths[1:])], "tanh")
            for _ in range(n)]


def timed(f, repeats):
    out, ms = None, []
    for _ in range(repeats + 1):  # (the first run warms up: module load, allocations, the weights' device copies)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = sorted(ms[1:])
    return out, dict(ms_median=ms[len(ms) // 2], ms_min=ms[0], ms_max=ms[-1], repeats=repeats)


def collect_route(nets, seeds):
    """[len(nets), S] values through VectorCartPole.collect and the host"""
    gp = _gamma_pow(GAMMA, CAP, "cpu", cap=CAP).numpy()
    T, S = EPISODES * CAP, len(seeds)
    values = np.zeros((len(nets), S))
    env = VectorCartPole(S)
    for l, net in enumerate(nets):
        env.seed(seeds)
        env.reset()
        col = env.collect(net, T, CAP, record_obs=False, record_probs=False)
        flags, reward = env.records.flags.cpu().numpy(), col.reward.cpu().numpy().astype(np.float64)
        for j in range(S):
            ends = np.flatnonzero(flags[:, j] & 6)[:EPISODES] + 1
            total, b = 0.0, 0
            for e in ends:
                total = total + np.cumsum(gp[:e - b] * reward[b:e, j])[-1]
                b = e
            values[l, j] = total / len(ends)
    return values


def lines_for(n_l, repeats, collect_actors):
    nets, seeds = actors(n_l), np.arange(SEEDS)
    res, t = timed(lambda: evalmc_rollouts_true_env("cartpole", seeds, nets, GAMMA, EPISODES, max_episode_steps=CAP), repeats)
    steps = int(res["steps"].sum())
    common = dict(what="evalMC true CartPole", network="4-64-64-2 tanh", actors=n_l, seeds=SEEDS, episodes=EPISODES, max_episode_steps=CAP, steps=steps,
                  value_actor0_seed0=float(res["value"][0, 0]))
    out = [dict(common, route="one evalmc_rollouts_true_env call", steps_per_s=steps / (t["ms_median"] * 1e-3), **t)]
    one, t1 = timed(lambda: [evalmc_rollouts_true_env("cartpole", seeds, net, GAMMA, EPISODES, max_episode_steps=CAP)["value"][0] for net in nets], repeats)
    assert np.array_equal(np.stack(one), res["value"]), "one call per actor must give the population's values"
    out.append(dict(common, route="one evalmc_rollouts_true_env call per actor", steps_per_s=steps / (t1["ms_median"] * 1e-3), **t1))
    k = min(n_l, collect_actors)
    val, t2 = timed(lambda: collect_route(nets[:k], seeds), repeats)
    assert np.array_equal(val, res["value"][:k]), "the collect route must give the population's values"
    out.append(dict(common, route="one VectorCartPole.collect of 5000 steps per actor, episodes read on the host", actors_timed=k,
                    ms_timed_median=t2["ms_median"], ms_median=t2["ms_median"] * n_l / k, extrapolated=k < n_l, repeats=repeats))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "true_env_population_bench.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--collect-actors", type=int, default=8)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    if a.kernel_only:
        nets, seeds = actors(64), np.arange(SEEDS)
        for _ in range(2):
            evalmc_rollouts_true_env("cartpole", seeds, nets, GAMMA, EPISODES, max_episode_steps=CAP)
        torch.cuda.synchronize()
        return
    lines = [l for n_l in (1, 8, 64) for l in lines_for(n_l, a.repeats, a.collect_actors)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for l in lines:
            print(json.dumps(l))
            f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
