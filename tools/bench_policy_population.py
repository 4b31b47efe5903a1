#!/usr/bin/env python3
"""Ranking L actors on a log: the population evaluation against the loop of one evalmc_rollouts per actor.  One JSON line per L.

  log      cartpole_log, 1 M rows, 162 box states (CartpoleBoxEncoder); S = 64 sampler seeds
  actors   the reference agent's network, 4-64-64-2 tanh (nn.Linear's default init, seeded), L = 1, 8, 64

  pop_*    evalmc_rollouts_population: ONE sampler reset, one forward launch per table (offsim_policy_mlp_pop) and one scan launch
           (offsim_eval_mc_rows_policy_pop) for all L * S rollouts
  loop_*   for every actor evalmc_rollouts(table, seeds, MLPPolicy, ...): L resets, 2 L forward launches, L scan launches of S rollouts

Per form, three runs, alternating pop / loop: *_total_s lists the three end-to-end wall times of the driver (results on the host) and
*_s their median; *_reset_s / *_forward_s / *_scan_s are the medians of three runs of each phase on its own, synchronised (for the loop:
of one actor's phase times L).  parity_ok: every array of the population's result equals the loop's.

Usage: python tools/bench_policy_population.py [--rows 1000000] [--seeds 64] [--pops 1,8,64] [--out profiles/policy_population_bench.jsonl]
       [--scan-only]
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


def sync():
    torch.cuda.synchronize()


def timed(fn):
    sync()
    t = time.perf_counter()
    r = fn()
    sync()
    return time.perf_counter() - t, r


def med(xs):
    return float(np.median(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--pops", default="1,8,64")
    ap.add_argument("--out", default=None)
    ap.add_argument("--scan-only", action="store_true", help="only the phases on their own, not the two drivers (A/B runs of kernel variants)")
    a = ap.parse_args()
    from rl_offline_simulation_amd import _lib as L, synth
    from rl_offline_simulation_amd.encoders import CartpoleBoxEncoder
    from rl_offline_simulation_amd.evaluators import BatchedPSRS, MLPPolicy, PolicyPopulation, evalmc_rollouts, evalmc_rollouts_population
    from rl_offline_simulation_amd.table import TransitionTable
    dev = L.require_device()
    e = synth.cartpole_log(a.rows, seed=0)
    enc = CartpoleBoxEncoder()
    z, z_next = enc.encode(e["observations"]), enc.encode(e["next_observations"])
    table = TransitionTable(z, e["actions"], e["rewards"], z_next, e["terminals"], e["action_distributions"], e["steps"] == 0)
    obs, nobs = torch.from_numpy(e["observations"]).to(dev), torch.from_numpy(e["next_observations"]).to(dev)
    seeds = np.arange(a.seeds, dtype=np.uint64)
    torch.manual_seed(0)
    pops = [int(x) for x in a.pops.split(",")]
    nets = [torch.nn.Sequential(torch.nn.Linear(4, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, 2))
            for _ in range(max(pops))]
    actors = [MLPPolicy.from_torch(n) for n in nets]
    lines = []
    for n_pol in pops:
        pols = actors[:n_pol]
        pop = PolicyPopulation.from_policies(pols)
        run_pop = lambda: evalmc_rollouts_population(table, seeds, pop, 0.99, obs=obs, next_obs=nobs)
        run_loop = lambda: [evalmc_rollouts(table, seeds, p, 0.99, obs=obs, next_obs=nobs) for p in pols]
        res_pop = run_pop()  # (warm-up of every shape)
        evalmc_rollouts(table, seeds, pols[0], 0.99, obs=obs, next_obs=nobs)
        keys = ("sum_g", "n_ep", "steps", "cand", "status", "value")
        t_pop, t_loop, ok = [], [], None
        for _ in range(0 if a.scan_only else 3):
            dt, res_pop = timed(run_pop)
            t_pop.append(dt)
            dt, res_loop = timed(run_loop)
            t_loop.append(dt)
            ok = all(np.array_equal(res_pop[k][l], res_loop[l][k], equal_nan=True) for k in keys for l in range(n_pol))
            print(f"L={n_pol}: pop {t_pop[-1]:.3f} s, loop {t_loop[-1]:.3f} s", file=sys.stderr, flush=True)
        # the phases on their own
        env = BatchedPSRS(table, len(seeds))

        def reset():
            env.reset_sampler(seeds)
            env._orders_for_generic()

        ph = {k: [] for k in ("reset", "pop_fwd", "pop_scan", "one_fwd", "one_scan")}
        for _ in range(3):
            ph["reset"].append(timed(reset)[0])
            dt, (pn, p0) = timed(lambda: pop.row_tables(table, obs, nobs))
            ph["pop_fwd"].append(dt)
            ph["pop_scan"].append(timed(lambda: env.eval_mc_rows_policy_population(pn, p0, 0.99))[0])
            dt, (qn, q0) = timed(lambda: pols[0].row_tables(table, obs, nobs))
            ph["one_fwd"].append(dt)
            ph["one_scan"].append(timed(lambda: env.eval_mc_rows_policy(qn, q0, 0.99))[0])
            del pn, p0, qn, q0
        L.check_async_faults()
        if a.scan_only:
            print(json.dumps(dict(N=int(table.N), seeds=int(a.seeds), L=n_pol, pop_scan_s=[round(x, 5) for x in ph["pop_scan"]],
                                  pop_forward_s=[round(x, 5) for x in ph["pop_fwd"]], reset_s=[round(x, 5) for x in ph["reset"]],
                                  one_scan_s=[round(x, 5) for x in ph["one_scan"]], steps=int(res_pop["steps"].sum()))), flush=True)
            continue
        line = dict(log="cartpole_log", N=int(table.N), n_states=int(table.n_slots), seeds=int(a.seeds), L=n_pol, policy="mlp 4-64-64-2 tanh",
                    pop_s=round(med(t_pop), 5), loop_s=round(med(t_loop), 5), speedup=round(med(t_loop) / med(t_pop), 3),
                    pop_total_s=[round(x, 5) for x in t_pop], loop_total_s=[round(x, 5) for x in t_loop],
                    pop_reset_s=round(med(ph["reset"]), 5), pop_forward_s=round(med(ph["pop_fwd"]), 5), pop_scan_s=round(med(ph["pop_scan"]), 5),
                    loop_reset_s=round(n_pol * med(ph["reset"]), 5), loop_forward_s=round(n_pol * med(ph["one_fwd"]), 5),
                    loop_scan_s=round(n_pol * med(ph["one_scan"]), 5), steps=int(res_pop["steps"].sum()),
                    scan_steps_per_s=float(f"{int(res_pop['steps'].sum()) / med(ph['pop_scan']):.4g}"), best=int(res_pop["best"]), parity_ok=bool(ok))
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
