#!/usr/bin/env python3
"""A grid of Q-learners on the queue simulator: one launch for L learners x S seeds (offsim_eval_queue_pop) against the loop a user writes
without it.  One JSON line per (behaviour, L).

  log       section 22's: synth_iid, 100 000 rows, 25 states, 5 actions; S = 64 sampler seeds, the action streams seeded like the samplers
  learners  Q-learning, a grid alpha x epsilon x gamma: L = 1 (1 x 1 x 1), 8 (2 x 2 x 2), 64 (4 x 4 x 4)
  eps_greedy   epsilon-greedy on the learner's own Q (first maximum on ties)
  fixed        the uniform behaviour policy

  pop_*    what TDPopulation.run_queue does per seed tile, on one BatchedQueueEvaluator of S rollouts: reset_sampler + set_action_seeds + ONE
           eval_td_population launch of L * S rollouts
  loop_*   the same environment without the population: per learner reset_sampler + set_action_seeds + one eval_td launch of S rollouts
The two routes alternate; times are synchronised wall times, *_s their medians; ratio = loop_s / pop_s; parity_ok: Q, the returns, the
episode counts, the step counts and the statuses of both routes are equal bit for bit.  At L = 1 the loop IS the single form: the
population should cost what it costs (l1_within_5pct on that line).

--kernel-only: run the L = 64 epsilon-greedy launch once after a warm-up and nothing else (for a rocprofv3 --kernel-trace --stats pass).

Usage: python tools/bench_td_population_queue.py [--seeds 64] [--pops 1,8,64] [--runs 5] [--out profiles/td_population_queue_bench.jsonl]
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

GRIDS = {1: ([0.1], [0.1], [0.99]), 8: ([0.05, 0.2], [0.1, 0.3], [0.95, 0.99]),
         64: ([0.02, 0.05, 0.1, 0.2], [0.05, 0.1, 0.2, 0.4], [0.9, 0.95, 0.99, 1.0])}
KEYS = ("q", "ep_g", "n_ep", "steps", "status")


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, r


def med(xs):
    return float(np.median(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--pops", default="1,8,64")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    from bench_queue_drivers import N, NA, NS, arrays
    from rl_offline_simulation_amd import _lib as L
    from rl_offline_simulation_amd.evaluators import BatchedQueueEvaluator, TDPopulation
    L.require_device()
    cols, _ = arrays()
    seeds = np.arange(a.seeds, dtype=np.uint64)
    env = BatchedQueueEvaluator(*cols, R=len(seeds))
    n_ep = env.table.N0 + 1
    uniform = np.full((env.nZ, NA), 1.0 / NA)
    beh_of = {"eps_greedy": L.BEHAVIOUR_EPS_GREEDY, "fixed": L.BEHAVIOUR_FIXED}

    def make(behaviour, n_l):
        al, ep, ga = GRIDS[n_l]
        pop = TDPopulation.grid("qlearn", alpha=al, epsilon=ep, gamma=ga, behaviour=behaviour)
        assert len(pop) == n_l
        beh = beh_of[behaviour]

        def run_pop():
            env.reset_sampler(seeds)
            env.set_action_seeds(seeds)
            o = env.eval_td_population(L.TD_QLEARN, np.array(pop.alpha), np.array(pop.gamma), beh, np.array(pop.epsilon), pi=uniform, n_episodes=n_ep, ep_cap=n_ep)
            torch.cuda.current_stream().synchronize()
            L.check_async_faults()
            return o

        def run_loop():
            outs = []
            for d in pop.learners:
                env.reset_sampler(seeds)
                env.set_action_seeds(seeds)
                o = env.eval_td(uniform, d["gamma"], L.TD_QLEARN, d["alpha"], n_episodes=n_ep, ep_cap=n_ep, behaviour=beh, epsilon=d["epsilon"])
                outs.append({k: o[k] for k in KEYS})
            torch.cuda.current_stream().synchronize()
            L.check_async_faults()
            return outs
        return run_pop, run_loop

    if a.kernel_only:
        run_pop, _ = make("eps_greedy", 64)
        run_pop()
        dt, _ = timed(run_pop)
        print(json.dumps(dict(kernel_only=True, L=64, seeds=int(a.seeds), pop_s=round(dt, 5))), flush=True)
        return
    lines = []
    for behaviour in ("eps_greedy", "fixed"):
        for n_l in [int(x) for x in a.pops.split(",")]:
            run_pop, run_loop = make(behaviour, n_l)
            res_pop, res_loop = run_pop(), run_loop()  # (warm-up of both forms)
            t_pop, t_loop = [], []
            for _ in range(a.runs):
                del res_pop, res_loop
                dt, res_pop = timed(run_pop)
                t_pop.append(dt)
                dt, res_loop = timed(run_loop)
                t_loop.append(dt)
                print(f"{behaviour} L={n_l}: pop {t_pop[-1]:.3f} s, loop {t_loop[-1]:.3f} s", file=sys.stderr, flush=True)
            steps = int(res_pop["steps"].sum())
            ok = all(torch.equal(res_pop[k][l], res_loop[l][k]) for l in range(n_l) for k in KEYS)
            line = dict(log="synth_iid", N=N, n_states=NS, nA=NA, seeds=int(a.seeds), L=n_l, learner="qlearn " + behaviour, tie="first",
                        kernel=res_pop["_kernel"], pop_s=round(med(t_pop), 5), pop_total_s=[round(x, 5) for x in t_pop], steps=steps,
                        pop_steps_per_s=float(f"{steps / med(t_pop):.4g}"), episodes_max=int(res_pop["n_ep"].max()), loop_s=round(med(t_loop), 5),
                        loop_total_s=[round(x, 5) for x in t_loop], ratio=round(med(t_loop) / med(t_pop), 3), parity_ok=bool(ok))
            if n_l == 1:
                line["l1_within_5pct"] = bool(med(t_pop) <= 1.05 * med(t_loop))
            print(json.dumps(line), flush=True)
            lines.append(line)
            if not ok:
                raise SystemExit("the population's results differ from the loop's")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
