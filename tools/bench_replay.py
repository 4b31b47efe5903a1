#!/usr/bin/env python3
"""A logged memory replayed through L Q-learners: one launch of offsim_replay_td against L launches of one learner each and against the
Python loop over the same log.  One JSON line per measurement.

  log       synth_iid, 1 000 000 rows, 25 states, 5 actions, in log order, one sweep
  learners  Q-learning, alpha spread over [0.01, 0.5], gamma over [0.9, 0.999]; Q_init zero

  launch    ONE replay_td launch for L = 1 / 8 / 64 / 1024 learners (device-event time around the launch)
  loop      L launches of one learner each, L = 1 / 8 / 64 (device-event time around all of them); their Q equals the one launch's bit for bit
  numpy     the reference's loop (offsim4rl/agents/tabular.py:94-99) for one learner over the same log on the host, wall clock; its Q equals
            learner 0's
Medians of --runs after a warm-up run; ns_per_step = the launch's time over the steps of ONE stream (what a wavefront walks);
updates_per_s counts every learner's update.

--kernel-only: the L = 64 launch twice (warm-up + one) and nothing else, for a rocprofv3 --kernel-trace --stats pass.

Usage: python tools/bench_replay.py [--rows 1000000] [--pops 1,8,64,1024] [--loops 1,8,64] [--runs 5] [--out profiles/replay_bench.jsonl]
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

NS, NA = 25, 5


def settings(n_l):
    return np.linspace(0.01, 0.5, n_l), np.linspace(0.9, 0.999, n_l)


def event_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3, r


def numpy_loop(e, alpha, gamma):
    S, A, R, S_, D = (e[k].tolist() for k in ("z", "actions", "rewards", "z_next", "terminals"))
    Q = np.zeros((NS, NA))
    for s, a, r, s_, d in zip(S, A, R, S_, D):
        Q[s, a] = Q[s, a] + alpha * (r + gamma * Q[s_].max() - Q[s, a])
    return Q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--pops", default="1,8,64,1024")
    ap.add_argument("--loops", default="1,8,64")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    from rl_offline_simulation_amd import _lib as L
    from rl_offline_simulation_amd import synth
    from rl_offline_simulation_amd.evaluators import ReplayLog, replay_lpw, replay_td
    dev = L.require_device()
    e = synth.synth_iid(a.rows, NS, NA, seed=1)
    log = ReplayLog.from_arrays(e["z"], e["actions"], e["rewards"], e["z_next"], e["terminals"], NS, NA, device=dev)

    def launch(alpha, gamma):
        q0 = torch.zeros((len(alpha), 1, NS, NA), dtype=torch.float64, device=dev)
        return replay_td(log, L.TD_QLEARN, alpha, gamma, q0)["q"]

    if a.kernel_only:
        al, ga = settings(64)
        launch(al, ga)
        dt, _ = event_time(lambda: launch(al, ga))
        print(json.dumps(dict(kernel_only=True, L=64, rows=a.rows, launch_s=round(dt, 5))), flush=True)
        return
    base = dict(log="synth_iid", N=a.rows, n_states=NS, nA=NA, passes=1)
    lines, q_of = [], {}
    for n_l in [int(x) for x in a.pops.split(",")]:
        al, ga = settings(n_l)
        launch(al, ga)
        ts = []
        for _ in range(a.runs):
            dt, q = event_time(lambda: launch(al, ga))
            ts.append(dt)
        q_of[n_l] = q
        t = float(np.median(ts))
        lines.append(dict(base, what="launch", L=n_l, lpw=replay_lpw(NS, NA, n_l), launch_s=round(t, 5), launch_all_s=[round(x, 5) for x in ts],
                          ns_per_step=round(t / a.rows * 1e9, 2), updates_per_s=float(f"{n_l * a.rows / t:.4g}")))
        print(json.dumps(lines[-1]), flush=True)
    for n_l in [int(x) for x in a.loops.split(",")]:
        al, ga = settings(n_l)
        loop = lambda: [launch(al[l:l + 1], ga[l:l + 1]) for l in range(n_l)]  # noqa: E731
        loop()
        ts = []
        for _ in range(a.runs):
            dt, qs = event_time(loop)
            ts.append(dt)
        t = float(np.median(ts))
        line = dict(base, what="loop", L=n_l, loop_s=round(t, 5), loop_all_s=[round(x, 5) for x in ts], updates_per_s=float(f"{n_l * a.rows / t:.4g}"))
        if n_l in q_of:
            line["parity_ok"] = bool(all(torch.equal(qs[l][0], q_of[n_l][l]) for l in range(n_l)))
            line["ratio_loop_over_launch"] = round(t / next(x["launch_s"] for x in lines if x["what"] == "launch" and x["L"] == n_l), 3)
        lines.append(line)
        print(json.dumps(line), flush=True)
    al, ga = settings(1)
    ts = []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        Q = numpy_loop(e, float(al[0]), float(ga[0]))
        ts.append(time.perf_counter() - t0)
    t = float(np.median(ts))
    line = dict(base, what="numpy", L=1, loop_s=round(t, 4), loop_all_s=[round(x, 4) for x in ts], updates_per_s=float(f"{a.rows / t:.4g}"))
    if 1 in q_of:
        line["parity_ok"] = bool(np.array_equal(Q, q_of[1][0, 0].cpu().numpy()))
    lines.append(line)
    print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    if not all(x.get("parity_ok", True) for x in lines):
        raise SystemExit("the routes disagree")


if __name__ == "__main__":
    main()
