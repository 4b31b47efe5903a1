#!/usr/bin/env python3
"""Ranking L PPO actors on the queue simulator: ONE evalmc_rollouts_queue_population call (one sampler reset, one forward launch per table,
one launch of offsim_eval_queue_rows_policy_pop for all L * S rollouts) against

  loop   the loop of single evalmc_rollouts_queue calls, one per actor (each resets the sampler, runs its forward and one launch of
         offsim_eval_queue_rows_policy for the S seeds)
  hand   ONE seed of ONE actor through the hand loop this replaces: per step MLPPolicy.forward on the device, the probabilities read
         back, the action drawn on the host, BatchedQueueEvaluator.step, and the reset at the end of an episode

The log is bench_queue_collect.py's (synth.synth_iid, N = 100 000, 25 states, 5 actions, synthetic 4-wide f32 observations), the actors are
4-64-64-5 tanh networks, S = 64 seeds, L in {1, 8, 64}, every rollout runs until its log is used up.  Synchronised wall time, medians of
--repeats runs after one warm-up, the routes alternating.  That the launch computes the right thing is the test suite's business
(tests/test_gpu_queue_rows_policy.py).

  python tools/bench_queue_policy_population.py [--out FILE] [--repeats 5] [--seeds 64] [--pops 1,8,64] [--only-launch L]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from rl_offline_simulation_amd import _lib as L  # noqa: E402
from rl_offline_simulation_amd.evaluators import (BatchedQueueEvaluator, MLPPolicy, PolicyPopulation, evalmc_rollouts_queue,  # noqa: E402
                                                  evalmc_rollouts_queue_population)
from rl_offline_simulation_amd.evaluators.obs_policy import obs_tensor  # noqa: E402
from bench_queue_collect import DO, HID, NA, log  # noqa: E402

GAMMA = 0.99


def actors(n):
    out = []
    for i in range(n):
        torch.manual_seed(100 + i)
        out.append(MLPPolicy.from_torch(torch.nn.Sequential(torch.nn.Linear(DO, HID), torch.nn.Tanh(), torch.nn.Linear(HID, HID), torch.nn.Tanh(),
                                                             torch.nn.Linear(HID, NA))))
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def hand_loop(cols, e, xn, x0, actor, seed):
    """evalMC of one actor on one seed by hand: forward, host draw, BatchedQueueEvaluator.step per step; returns the steps served"""
    b = BatchedQueueEvaluator(*cols, R=1)
    b.reset_sampler([seed])
    done_col, rng = np.asarray(e["terminals"]) != 0, np.random.default_rng(seed)

    def run():
        steps = 0
        while True:
            row = int(b.reset().cpu()[0])
            if row < 0:
                return steps
            x, done = x0[row:row + 1], False
            while not done:
                p = actor.forward(x).cpu().numpy()[0].astype(np.float64)
                A = int(rng.choice(NA, p=p / p.sum()))
                r, status = b.step([A])
                if int(status.cpu()[0]) != L.ST_OK:
                    return steps
                row = int(r.cpu()[0])
                steps += 1
                x, done = xn[row:row + 1], bool(done_col[row])
    return timed(run)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "queue_policy_population_bench.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--pops", default="1,8,64")
    ap.add_argument("--only-launch", type=int, default=0)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    e, ds, _ = log()
    cols = (e["z"], e["actions"], e["rewards"], e["z_next"], e["terminals"], e["action_distributions"], np.asarray(e["steps"]) == 0)
    obs, nobs = ds.experience["observations"], ds.experience["next_observations"]
    seeds = np.arange(a.seeds) + 1
    if a.only_launch:  # (for a kernel trace: two population calls, nothing else)
        pop = PolicyPopulation.from_policies(actors(a.only_launch))
        for _ in range(2):
            ms, res = timed(lambda: evalmc_rollouts_queue_population(cols, seeds, pop, GAMMA, obs=obs, next_obs=nobs))
            print(json.dumps(dict(what="population call", L=a.only_launch, S=a.seeds, ms=ms, steps=int(res["steps"].sum()))))
        return 0
    xn, x0 = obs_tensor(nobs, dev), obs_tensor(obs, dev)
    lines = []
    every = actors(max(int(v) for v in a.pops.split(",")))
    t_hand, n_hand = [], 0
    for rep in range(a.repeats + 1):
        ms, n_hand = hand_loop(cols, e, xn, x0, every[0], int(seeds[0]))
        if rep:
            t_hand.append(ms)
    hand = sorted(t_hand)[len(t_hand) // 2]
    lines.append(dict(what="hand loop: MLPPolicy.forward + host draw + BatchedQueueEvaluator.step, ONE seed of ONE actor", route="hand", L=1, S=1,
                      steps=n_hand, ms_median=hand, ms_min=min(t_hand), ms_max=max(t_hand), repeats=a.repeats, us_per_step=hand * 1e3 / max(n_hand, 1)))
    for n_pol in [int(v) for v in a.pops.split(",")]:
        pols = every[:n_pol]
        pop = PolicyPopulation.from_policies(pols)
        t, steps = {"pop": [], "loop": []}, {}
        for rep in range(a.repeats + 1):  # (the first run warms up: module load, allocations)
            ms, res = timed(lambda: evalmc_rollouts_queue_population(cols, seeds, pop, GAMMA, obs=obs, next_obs=nobs))
            steps["pop"] = int(res["steps"].sum())
            ms2, rs = timed(lambda: [evalmc_rollouts_queue(cols, seeds, p, GAMMA, obs=obs, next_obs=nobs) for p in pols])
            steps["loop"] = int(sum(r["steps"].sum() for r in rs))
            if rep:
                t["pop"].append(ms)
                t["loop"].append(ms2)
        assert steps["pop"] == steps["loop"]
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        for route, what in (("pop", "evalmc_rollouts_queue_population: one reset, one forward per table, ONE rollout launch"),
                            ("loop", "loop of evalmc_rollouts_queue, one call per actor")):
            lines.append(dict(what=what, route=route, L=n_pol, S=a.seeds, steps=steps[route], ms_median=med[route], ms_min=min(t[route]),
                              ms_max=max(t[route]), repeats=a.repeats, steps_per_s=steps[route] / (med[route] * 1e-3)))
        lines.append(dict(what="ratios of the medians", L=n_pol, S=a.seeds, loop_over_pop=med["loop"] / med["pop"],
                          hand_one_rollout_over_pop_all_rollouts=hand / med["pop"],
                          hand_us_per_step_over_pop_us_per_step=(hand / max(n_hand, 1)) / (med["pop"] / steps["pop"])))
    name = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for ln in lines:
            ln["device"] = name
            print(json.dumps(ln))
            f.write(json.dumps(ln) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
