#!/usr/bin/env python3
"""Learning curves of a grid of Q-learners on a log: TDPopulation.run against one eval_td launch per learner.  One JSON line per L.

  log       synth_iid, 1 M rows, 25 states, 5 actions; S = 64 sampler seeds
  learners  Q-learning, epsilon-greedy on the learner's own Q (first maximum on ties), a grid alpha x epsilon x gamma: L = 1 (1 x 1 x 1),
            8 (2 x 2 x 2), 64 (4 x 4 x 4)

  pop_*     TDPopulation.run: ONE sampler reset for the S seeds, one launch for all L * S rollouts (offsim_eval_td_pop), the curves on the
            device (offsim_td_curves)
  loop_*    what a user does today: per learner BatchedPSRS.reset_sampler over the same seeds and one eval_td launch of S rollouts (L
            resets, L launches); the returns stay on the device, as the population's do

Per L three runs, alternating pop / loop: *_total_s lists the three synchronised wall times and *_s their median.  parity_ok: Q, the
returns, the episode counts and the step counts of the population equal the loop's, bit for bit.

Usage: python tools/bench_td_population.py [--rows 1000000] [--seeds 64] [--pops 1,8,64] [--runs 3] [--out profiles/td_population_bench.jsonl]
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

GRIDS = {1: ([0.1], [0.1], [0.99]), 8: ([0.05, 0.2], [0.1, 0.3], [0.95, 0.99]),
         64: ([0.02, 0.05, 0.1, 0.2], [0.05, 0.1, 0.2, 0.4], [0.9, 0.95, 0.99, 1.0])}


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
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--pops", default="1,8,64")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from rl_offline_simulation_amd import _lib as L, synth
    from rl_offline_simulation_amd.evaluators import BatchedPSRS, TDPopulation
    from rl_offline_simulation_amd.table import TransitionTable
    L.require_device()
    nS, nA = 25, 5
    e = synth.synth_iid(a.rows, nS, nA, seed=1)
    table = TransitionTable(e["z"], e["actions"], e["rewards"], e["z_next"], e["terminals"], e["action_distributions"], e["steps"] == 0)
    seeds = np.arange(a.seeds, dtype=np.uint64)
    n_ep = table.N0 + 1
    pi_slots = np.full((table.n_slots, nA), 1.0 / nA)
    lines = []
    for n_l in [int(x) for x in a.pops.split(",")]:
        al, ep, ga = GRIDS[n_l]
        pop = TDPopulation.grid("qlearn", alpha=al, epsilon=ep, gamma=ga, behaviour="eps_greedy")
        assert len(pop) == n_l
        env = BatchedPSRS(table, len(seeds))

        def run_loop():
            outs = []
            for d in pop.learners:
                env.reset_sampler(seeds)
                o = env.eval_td(pi_slots, d["gamma"], L.TD_QLEARN, d["alpha"], n_episodes=n_ep, ep_cap=n_ep, behaviour=L.BEHAVIOUR_EPS_GREEDY,
                                epsilon=d["epsilon"])
                outs.append({k: o[k] for k in ("q", "ep_g", "n_ep", "steps")})
            env.check_faults()
            return outs

        run_pop = lambda: pop.run(table, seeds)  # noqa: E731
        res_pop, res_loop = run_pop(), None  # (warm-up of both forms)
        env.reset_sampler(seeds)
        env.eval_td(pi_slots, 0.99, L.TD_QLEARN, 0.1, n_episodes=n_ep, ep_cap=n_ep, behaviour=L.BEHAVIOUR_EPS_GREEDY, epsilon=0.1)
        t_pop, t_loop = [], []
        for _ in range(a.runs):
            del res_pop, res_loop
            dt, res_pop = timed(run_pop)
            t_pop.append(dt)
            dt, res_loop = timed(run_loop)
            t_loop.append(dt)
            print(f"L={n_l}: pop {t_pop[-1]:.3f} s, loop {t_loop[-1]:.3f} s", file=sys.stderr, flush=True)
        # (the ids of this log are 0 .. nS - 1: Q by state id is Q by slot)
        ok = all(torch.equal(res_pop.Q[l], res_loop[l]["q"]) and torch.equal(res_pop.Gs[l], res_loop[l]["ep_g"]) and
                 torch.equal(res_pop.n_ep[l], res_loop[l]["n_ep"]) and torch.equal(res_pop.steps[l], res_loop[l]["steps"]) for l in range(n_l))
        steps = int(res_pop.steps.sum())
        line = dict(log="synth_iid", N=int(table.N), n_states=int(table.n_slots), nA=nA, seeds=int(a.seeds), L=n_l, learner="qlearn eps_greedy",
                    pop_s=round(med(t_pop), 5), loop_s=round(med(t_loop), 5), speedup=round(med(t_loop) / med(t_pop), 3),
                    pop_total_s=[round(x, 5) for x in t_pop], loop_total_s=[round(x, 5) for x in t_loop], steps=steps,
                    pop_steps_per_s=float(f"{steps / med(t_pop):.4g}"), episodes_max=int(res_pop.n_ep.max()), best=int(res_pop.best(last=10)),
                    orders_written_bytes_pop=int(a.seeds) * 4 * int(table.N), orders_written_bytes_loop=n_l * int(a.seeds) * 4 * int(table.N), parity_ok=bool(ok))
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
