#!/usr/bin/env python3
"""The logged environments on the device (VectorCartPole / VectorGridNavi, offsim_env_collect*): what logging and a learner's epoch cost.

1. record: a log of N = 1 M and 10 M rows at E = 4096 environments under a tanh actor (CartPole 4-64-64-2, the coordinate grid 2-64-64-5),
   the OfflineDataset on the host included, against the package's host generators for the same row count (synth.cartpole_log,
   synth.grid_coords_log_fast, also 4096 environments in lock step).  The host loops only do the uniform policy: they run no network, so
   the two columns are not the same job; the device one is the dearer.
2. collect_ppo: T = 500 steps of E = 8 / 1024 / 4096 environments with a 64-64 actor and critic, beside VectorPSRS.collect_ppo on a log of
   the same environment (100 000 rows recorded the same way, states by CartpoleBoxEncoder / the cell of the coordinates).  steps_served tells how
   much of the T * E the simulator could serve before the log ran dry; the environment always serves all.
3. what a step is made of, at E = 4096 and T = 500: the same launches with 8-wide networks in the place of the 64-wide ones, and collect
   (the actor alone) beside collect_ppo (critic and actor).

Synchronised wall time, medians of --repeats runs after one warm-up run.

  python tools/bench_true_env.py [--out FILE] [--repeats 5] [--rows 1000000,10000000] [--envs 8,1024,4096] [--steps 500] [--only-bound]
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
from rl_offline_simulation_amd.encoders.heuristic import CartpoleBoxEncoder  # noqa: E402
from rl_offline_simulation_amd.evaluators import MLPPolicy, MLPValue, VectorCartPole, VectorGridNavi, VectorPSRS  # noqa: E402

HID, E_REC, N_LOG = 64, 4096, 100000


class CellEncoder:
    """the cell of a coordinate-grid observation"""

    def encode(self, x):
        x = np.asarray(x, np.float64)
        return (np.floor(x[:, 0] * 5 + 1e-6).clip(0, 4) + 5 * np.floor(x[:, 1] * 5 + 1e-6).clip(0, 4)).astype(np.int64)


def networks(dO, nA, hid=HID):
    def net(n_out, seed):
        torch.manual_seed(seed)
        return torch.nn.Sequential(torch.nn.Linear(dO, hid), torch.nn.Tanh(), torch.nn.Linear(hid, hid), torch.nn.Tanh(), torch.nn.Linear(hid, n_out))
    return MLPPolicy.from_torch(net(nA, 0)), MLPValue.from_torch(net(1, 1))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def median_of(fn, repeats):
    ts, out = [], None
    for rep in range(repeats + 1):  # (the first run warms up: module load, allocations)
        ms, out = timed(fn)
        if rep:
            ts.append(ms)
    return sorted(ts)[len(ts) // 2], min(ts), max(ts), out


ENVS = {"cartpole": (lambda E: VectorCartPole(E), 4, 2, lambda N: synth.cartpole_log(N, seed=0, n_envs=E_REC), "synth.cartpole_log",
                     lambda: (162, CartpoleBoxEncoder())),
        "grid_coords": (lambda E: VectorGridNavi(E), 2, 5, lambda N: synth.grid_coords_log_fast(N, seed=0, n_envs=E_REC), "synth.grid_coords_log_fast",
                        lambda: (25, CellEncoder()))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "true_env_bench.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", default="1000000,10000000")
    ap.add_argument("--envs", default="8,1024,4096")
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--only-bound", action="store_true", help="section 3 alone")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lines = []
    T = a.steps
    if a.only_bound:
        write(a.out, bound(a.repeats, T))
        return 0
    for name, (make, dO, nA, host, host_name, states) in ENVS.items():
        actor, critic = networks(dO, nA)
        env = make(E_REC)
        env.seed(np.arange(E_REC))
        log = env.record(actor, N_LOG, 500)
        for N in [int(v) for v in a.rows.split(",")]:
            def rec():
                env.seed(np.arange(E_REC))
                return env.record(actor, N, 500)
            med, lo, hi, ds = median_of(rec, a.repeats)
            lines.append(dict(what=f"record: {name}, {dO}-{HID}-{HID}-{nA} tanh actor, dataset on the host", route="device", env=name, rows=N, envs=E_REC,
                              ms_median=med, ms_min=lo, ms_max=hi, rows_per_s=N / (med * 1e-3), repeats=a.repeats))
            hmed, hlo, hhi, _ = median_of(lambda: host(N), a.repeats)
            lines.append(dict(what=f"{host_name}: the host generator, uniform policy only (no network)", route="host", env=name, rows=N, envs=E_REC,
                              ms_median=hmed, ms_min=hlo, ms_max=hhi, rows_per_s=N / (hmed * 1e-3), repeats=a.repeats))
            lines.append(dict(what="ratio of the medians", env=name, rows=N, host_over_device=hmed / med))
        nS, enc = states()
        for E in [int(v) for v in a.envs.split(",")]:
            true_env, sim = make(E), VectorPSRS(log, E, num_states=nS, encoder=enc)

            def in_env():
                true_env.seed(np.arange(E))
                return timed(lambda: true_env.collect_ppo(actor, critic, T, max_episode_steps=500))

            def in_sim():
                sim.reset_sampler(list(range(E)))
                sim.reset()
                return timed(lambda: sim.collect_ppo(actor, critic, T, max_episode_steps=500))

            t, served = {"env": [], "psrs": []}, {}
            for rep in range(a.repeats + 1):
                for route, fn in (("env", in_env), ("psrs", in_sim)):
                    ms, b = fn()
                    served[route] = int(b.valid.sum())
                    if rep:
                        t[route].append(ms)
            med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
            for route, what in (("env", f"{type(true_env).__name__}.collect_ppo, one launch + advantages"),
                                ("psrs", f"VectorPSRS.collect_ppo on a {len(log)}-row log of the same environment, one launch + advantages")):
                lines.append(dict(what=what, route=route, env=name, envs=E, T=T, steps_served=served[route], ms_median=med[route], ms_min=min(t[route]),
                                  ms_max=max(t[route]), repeats=a.repeats, us_per_step_of_an_env=med[route] * 1e3 / T,
                                  steps_per_s=served[route] / (med[route] * 1e-3)))
            lines.append(dict(what="ratio of the medians", env=name, envs=E, T=T, psrs_over_env=med["psrs"] / med["env"]))
    lines += bound(a.repeats, T)
    write(a.out, lines)
    return 0


def bound(repeats, T):
    """3. what a step is made of, at E = 4096: the same launch with 8-wide networks in the place of the 64-wide ones, and the actor alone"""
    lines, E = [], 4096
    for name, (make, dO, nA, _, _, _) in ENVS.items():
        env = make(E)
        for hid in (HID, 8):
            actor, critic = networks(dO, nA, hid)
            for what, fn in (("collect_ppo (critic + actor)", lambda: env.collect_ppo(actor, critic, T, max_episode_steps=500)),
                             ("collect (actor alone)", lambda: env.collect(actor, T, max_episode_steps=500))):
                def run():
                    env.seed(np.arange(E))
                    return timed(fn)[0]
                ts = sorted([run() for _ in range(repeats + 1)][1:])
                lines.append(dict(what=f"step cost: {what}, hidden width {hid}", env=name, envs=E, T=T, hidden=hid, ms_median=ts[len(ts) // 2],
                                  ms_min=ts[0], ms_max=ts[-1], us_per_step_of_an_env=ts[len(ts) // 2] * 1e3 / T, repeats=repeats))
    return lines


def write(out, lines):
    dev = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        for ln in lines:
            ln["device"] = dev
            print(json.dumps(ln))
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    sys.exit(main())
