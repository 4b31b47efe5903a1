#!/usr/bin/env python3
"""Time the tabular learners on latent states of the true CartPole (offsim_eval_env_latent_pop) and write profiles/latent_env_bench.jsonl.

Setting: CartPole behind the 162-box encoder (nS = 163), cap 500, 64 seeds x 100 episodes, epsilon-greedy Q-learners.  Three routes:
  population   L = 1 / 8 / 64 learners in one TDPopulation.run_latent_env call
  single       one single-learner call per learner (L calls), for every L
  host         the host mirror's Python loop for one learner on one seed
Medians of 5 synchronised wall times after a warm-up, for every route.  The routes must agree bit for bit on the device (the population's
entry [l, j] against the single call); the host loop's dynamics use the host's sin / cos, so its rollout may leave the device's: it is timed only.

Run from the repo root on a GPU:   python tools/bench_latent_env_drivers.py"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rl_offline_simulation_amd import _lib as L  # noqa: E402
from rl_offline_simulation_amd.encoders import CartpoleBoxEncoder  # noqa: E402
from rl_offline_simulation_amd.evaluators import BatchedLatentEnv, LatentEnv, TDPopulation  # noqa: E402

S, N_EP, GAMMA, REPS = 64, 100, 0.99, 5


def timed(fn):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), out


def learners(n):
    g = np.random.default_rng(0)
    return g.uniform(0.05, 0.5, n).tolist(), g.uniform(0.05, 0.5, n).tolist()


def host_loop(env, alpha, eps, seed, n_ep):
    g, Q, steps = np.random.default_rng(seed), np.zeros((env.nS, env.nA)), 0
    for e in range(n_ep):
        np.random.seed(e)
        z, done = env.reset(seed=e), False
        while not done:
            best = np.where(Q[z] == Q[z].max())[0]
            p = np.full(env.nA, eps / env.nA)
            p[np.random.choice(best)] = 1 - eps + eps / env.nA
            a = int(g.choice(env.nA, p=p))
            z_, r, done, _ = env.step(a)
            Q[z, a] = Q[z, a] + alpha * (r + GAMMA * Q[z_].max() - Q[z, a])
            z, steps = z_, steps + 1
    return steps


def main():
    env = LatentEnv("cartpole", CartpoleBoxEncoder(), 163)
    seeds = list(range(S))
    rows = []
    for n in (1, 8, 64):
        al, ep = learners(n)
        pop = TDPopulation("qlearn", al, GAMMA, epsilon=ep, behaviour="eps_greedy")
        t, res = timed(lambda: pop.run_latent_env(env, seeds, N_EP))
        steps = int(res.steps.sum())
        rows.append(dict(route="population", L=n, S=S, episodes=N_EP, seconds=t, steps=steps, steps_per_s=steps / t))

        def singles():
            outs = []
            for l in range(n):
                b = BatchedLatentEnv(env, S)
                b.set_seeds(seeds)
                outs.append(b.eval_td(None, GAMMA, L.TD_QLEARN, al[l], behaviour=L.BEHAVIOUR_EPS_GREEDY, epsilon=ep[l], tie="episode",
                                      n_episodes=N_EP, ep_cap=N_EP))
            return outs
        t1, outs = timed(singles)
        for l in range(n):
            assert torch.equal(res.Q[l], outs[l]["q"]) and torch.equal(res.Gs[l], outs[l]["ep_g"]), "population and single calls differ"
        rows.append(dict(route="single", L=n, S=S, episodes=N_EP, seconds=t1, calls=n, agree_bit_for_bit=True))
    al, ep = learners(1)
    mirror = LatentEnv("cartpole", CartpoleBoxEncoder(), 163)
    th, steps = timed(lambda: host_loop(mirror, al[0], ep[0], 0, N_EP))
    rows.append(dict(route="host", L=1, S=1, episodes=N_EP, seconds=th, steps=steps, steps_per_s=steps / th))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "latent_env_bench.jsonl"), "w") as f:
        for r in rows:
            r.update(device=torch.cuda.get_device_name(0), setting="cartpole + box, cap 500, eps-greedy Q-learners")
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
