#!/usr/bin/env python3
"""A grid of Q-learners on an exogenous-state log: TDPopulation.run_exo, one launch for L learners x S seeds.  One JSON line per (behaviour, L).

  log       section 19's: synth_iid, 100 000 rows, 25 states, 5 actions, an exogenous x of 4 values, o = 4 s + x; S = 64 sampler seeds,
            reseed="none" (every seed's own stream)
  learners  Q-learning, a grid alpha x epsilon x gamma: L = 1 (1 x 1 x 1), 8 (2 x 2 x 2), 64 (4 x 4 x 4)

  eps_greedy   epsilon-greedy on the learner's own Q (first maximum on ties).  No device baseline exists for it on a PSRS_Exo, so the
               population is reported alone: pop_total_s lists the synchronised wall times, pop_s their median, pop_steps_per_s.
  fixed        the uniform behaviour policy.  Also loop_*: what a user writes without the population, per learner reset_sampler of both
               families over the same seeds + one BatchedPSRSExo.eval_td launch of S rollouts.  The two routes alternate; ratio =
               loop_s / pop_s (medians); parity_ok: Q, the returns, the episode counts and the step counts of both routes are equal bit for
               bit.  At L = 1 the loop IS the single form: the population should cost what it costs.

--kernel-only: run the L = 64 epsilon-greedy launch once after a warm-up and nothing else (for a rocprofv3 --kernel-trace --stats pass).

Usage: python tools/bench_td_population_exo.py [--seeds 64] [--pops 1,8,64] [--runs 5] [--out profiles/td_population_exo_bench.jsonl]
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
    from bench_exo_drivers import N, NA, NS, NX, make_env
    from rl_offline_simulation_amd import _lib as L
    from rl_offline_simulation_amd.evaluators import BatchedPSRSExo, TDPopulation
    L.require_device()
    env, _ = make_env()
    ts, tx = env.ts, env.tx
    obs_of, ids = env.obs_table(NS * NX)
    assert len(ids) == NS * NX
    seeds = np.arange(a.seeds, dtype=np.uint64)
    n_ep = ts.N0 + 1
    uniform = np.full((len(ids), NA), 1.0 / NA)
    if a.kernel_only:
        pop = TDPopulation.grid("qlearn", *GRIDS[64][:1], epsilon=GRIDS[64][1], gamma=GRIDS[64][2], behaviour="eps_greedy")
        pop.run_exo(env, seeds, reseed="none")
        dt, _ = timed(lambda: pop.run_exo(env, seeds, reseed="none"))
        print(json.dumps(dict(kernel_only=True, L=64, seeds=int(a.seeds), pop_s=round(dt, 5))), flush=True)
        return
    lines = []
    for behaviour in ("eps_greedy", "fixed"):
        for n_l in [int(x) for x in a.pops.split(",")]:
            al, ep, ga = GRIDS[n_l]
            pop = TDPopulation.grid("qlearn", alpha=al, epsilon=ep, gamma=ga, behaviour=behaviour)
            assert len(pop) == n_l
            one = BatchedPSRSExo(ts, tx, len(seeds))

            def run_loop():
                outs = []
                for d in pop.learners:
                    one.reset_sampler(seeds)
                    o = one.eval_td(uniform, obs_of, d["gamma"], L.TD_QLEARN, d["alpha"], n_episodes=n_ep, reseed="none", ep_cap=n_ep)
                    outs.append({k: o[k] for k in ("q", "ep_g", "n_ep", "steps")})
                torch.cuda.current_stream().synchronize()
                L.check_async_faults()
                return outs

            run_pop = lambda: pop.run_exo(env, seeds, reseed="none")  # noqa: E731
            res_pop, res_loop = run_pop(), (run_loop() if behaviour == "fixed" else None)  # (warm-up of both forms)
            t_pop, t_loop = [], []
            for _ in range(a.runs):
                del res_pop, res_loop
                dt, res_pop = timed(run_pop)
                t_pop.append(dt)
                res_loop = None
                if behaviour == "fixed":
                    dt, res_loop = timed(run_loop)
                    t_loop.append(dt)
                print(f"{behaviour} L={n_l}: pop {t_pop[-1]:.3f} s" + (f", loop {t_loop[-1]:.3f} s" if t_loop else ""), file=sys.stderr, flush=True)
            steps = int(res_pop.steps.sum())
            line = dict(log="synth_iid + x", N=N, n_states=NS, n_exo=NX, nA=NA, seeds=int(a.seeds), L=n_l, learner="qlearn " + behaviour, reseed="none",
                        pop_s=round(med(t_pop), 5), pop_total_s=[round(x, 5) for x in t_pop], steps=steps, pop_steps_per_s=float(f"{steps / med(t_pop):.4g}"),
                        episodes_max=int(res_pop.n_ep.max()))
            if behaviour == "fixed":
                # (the observations of this log are 0 .. nO - 1 and every one has a row: Q by observation is Q by compact row)
                ok = all(torch.equal(res_pop.Q[l], res_loop[l]["q"]) and torch.equal(res_pop.Gs[l], res_loop[l]["ep_g"]) and
                         torch.equal(res_pop.n_ep[l], res_loop[l]["n_ep"]) and torch.equal(res_pop.steps[l], res_loop[l]["steps"]) for l in range(n_l))
                line.update(loop_s=round(med(t_loop), 5), loop_total_s=[round(x, 5) for x in t_loop], ratio=round(med(t_loop) / med(t_pop), 3), parity_ok=bool(ok))
            print(json.dumps(line), flush=True)
            lines.append(line)
            if behaviour == "fixed" and not ok:
                raise SystemExit("the population's results differ from the loop's")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
