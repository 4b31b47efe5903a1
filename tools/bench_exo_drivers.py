#!/usr/bin/env python3
"""evalMC on an exogenous-state log: whole rollouts in one launch (offsim_eval_mc_exo) for 1, 64 and 1024 sampler seeds, and the hand
loop over PSRS_Exo.step -- one launch and two host reads per simulated step -- for ONE seed.

The log is the iid generator of synth.py (N = 100 000, 25 states, 5 actions) with an exogenous x of 4 values, o = 4 s + x.  Every line
goes to stdout and to --out (default profiles/exo_drivers_bench.jsonl) as JSON.

  python tools/bench_exo_drivers.py [--out FILE] [--repeats 5] [--only-launch R]   (--only-launch: one launch of R seeds, for a profiler)
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

from rl_offline_simulation_amd import synth  # noqa: E402
from rl_offline_simulation_amd.evaluators import BatchedPSRSExo, PSRS_Exo  # noqa: E402

N, NS, NA, NX, GAMMA = 100000, 25, 5, 4, 0.99


def make_env():
    e = synth.synth_iid(N, NS, NA, seed=1)
    g = np.random.default_rng(2)
    x, xn = g.integers(0, NX, N), g.integers(0, NX, N)
    p = e["action_distributions"]
    buf = [(int(e["z"][i]) * NX + int(x[i]), int(e["actions"][i]), float(e["rewards"][i]), int(e["z_next"][i]) * NX + int(xn[i]), bool(e["terminals"][i]),
            p[i], {"t": int(e["steps"][i])}) for i in range(N)]
    env = PSRS_Exo(buf, nO=NS * NX, nA=NA, o_split_func=lambda o: (o // NX, o % NX), o_combine_func=lambda s, x_: s * NX + x_)
    pi = np.repeat(synth.dirichlet_policy(NS, NA), NX, axis=0)  # pi[o] = the policy at the s of o
    return env, pi


def one_launch(env, pi, R, repeats):
    obs_of, ids = env.obs_table(pi.shape[0])
    b = BatchedPSRSExo(env.ts, env.tx, R)
    seeds = list(range(R))
    ms, o = [], None
    for _ in range(repeats + 1):  # (the first run warms up: module load, allocations)
        b.reset_sampler(seeds)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        o = b.eval_mc(pi[ids], obs_of, GAMMA)
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    ms = sorted(ms[1:])
    steps, cand = int(o["steps"].sum()), int(o["cand"].sum())
    med = ms[len(ms) // 2]
    return dict(what="one launch", kernel=o["_kernel"], seeds=R, N=N, steps=steps, candidates=cand, ms_median=med, ms_min=ms[0], ms_max=ms[-1], repeats=repeats,
                steps_per_s=steps / (med * 1e-3), value_seed0=float(o["sum_g"][0]) / max(int(o["n_ep"][0]), 1), steps_seed0=int(o["steps"][0]))


def hand_loop(env, pi, repeats):
    """The evalMC loop written by hand over PSRS_Exo.step, the only form there was before offsim_eval_mc_exo."""
    split, ms, steps, G_sum, n_ep = env.o_split_func, [], 0, 0.0, 0
    for _ in range(repeats + 1):
        env.reset_sampler(seed=0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps, G_sum, n_ep, ep, stop = 0, 0.0, 0, 0, False
        while not stop:
            o = env.reset(seed=ep)
            if o is None:
                break
            G, t, done = 0.0, 0, False
            while not done:
                o2, r, done, _ = env.step(pi[o])
                if o2 is None:
                    stop = True
                    break
                G, t, steps, o = G + GAMMA ** t * r, t + 1, steps + 1, o2
            if done:
                G_sum, n_ep, ep = G_sum + G, n_ep + 1, ep + 1
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = sorted(ms[1:])
    med = ms[len(ms) // 2]
    return dict(what="hand loop over PSRS_Exo.step", seeds=1, N=N, steps=steps, ms_median=med, ms_min=ms[0], ms_max=ms[-1], repeats=repeats,
                steps_per_s=steps / (med * 1e-3), us_per_step=med * 1e3 / max(steps, 1), value_seed0=G_sum / max(n_ep, 1), steps_seed0=steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exo_drivers_bench.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only-launch", type=int, default=0)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    env, pi = make_env()
    if a.only_launch:
        print(json.dumps(one_launch(env, pi, a.only_launch, 1)))
        return 0
    lines = [one_launch(env, pi, R, a.repeats) for R in (1, 64, 1024)]
    lines.append(hand_loop(env, pi, min(a.repeats, 3)))
    agree = lines[0]["steps_seed0"] == lines[-1]["steps_seed0"] and lines[0]["value_seed0"] == lines[-1]["value_seed0"]
    lines[-1]["equals_one_launch_on_seed0"] = bool(agree)
    dev = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for ln in lines:
            ln["device"] = dev
            print(json.dumps(ln))
            f.write(json.dumps(ln) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
