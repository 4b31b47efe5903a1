"""VectorPSRS.collect (one launch per T steps, the policy network inside the kernel) against the graph-replayed driver loop of
tools/vector_env_example.py (one HIP graph replay per step: torch forward of the network + step_and_reset), on config C2: 1 M CartPole rows,
the 4 -> 64 -> 64 -> 2 tanh network of the reference's PPO actor.  Appends JSON lines to profiles/collect_bench.jsonl.

parity_ok: collect on a 2-environment twin with the seeds of environments 0 and 1 equals the eager driver loop (MLPPolicy.forward,
step_and_reset, reset of the truncated environments) row for row and flag for flag, and equals environments 0 and 1 of the timed run.

usage: python tools/bench_collect.py [--envs 4096,16384] [--steps 64,256,1024] [--rows 1000000] [--out profiles/collect_bench.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rl_offline_simulation_amd import OfflineDataset, ProbDistribution, _lib as L, spaces, synth  # noqa: E402
from rl_offline_simulation_amd.encoders import CartpoleBoxEncoder  # noqa: E402
from rl_offline_simulation_amd.evaluators import MLPPolicy, VectorPSRS  # noqa: E402
from rl_offline_simulation_amd.evaluators.obs_policy import obs_tensor  # noqa: E402

CAP = 500  # the example's time limit (psrs_from_expert_heuristic.py:76-78)


def make_env(ds, E):
    return VectorPSRS(ds, num_envs=E, num_states=162, encoder=CartpoleBoxEncoder())


def driver_loop(env, mlp, T):
    rows, flags, ep_t = [], [], torch.zeros(env.num_envs, dtype=torch.int32, device=env.obs.device)
    for _ in range(T):
        env.step_and_reset(mlp.forward(obs_tensor(env.obs, env.obs.device)))
        served = env.env._status == L.ST_OK
        term = served & env.done
        ep_t = torch.where(served, ep_t + 1, ep_t)
        trunc = served & (ep_t >= CAP)
        env.reset(mask=trunc & ~term)
        ep_t = torch.where(term | trunc, torch.zeros_like(ep_t), ep_t)
        rows.append(torch.where(served, env.env._row, torch.full_like(env.env._row, -1)))
        flags.append(term.to(torch.int32) * 2 + trunc.to(torch.int32) * 4)
    return torch.stack(rows), torch.stack(flags)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="4096,16384")
    ap.add_argument("--steps", default="64,256,1024")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "collect_bench.jsonl"))
    a = ap.parse_args()
    N = a.rows
    e = synth.cartpole_log(N, seed=0)
    ds = OfflineDataset(spaces.Box(-np.inf, np.inf, (4,), np.float32), spaces.Discrete(2), ProbDistribution.Discrete,
                        **{k: e[k] for k in ("observations", "actions", "action_distributions", "rewards", "next_observations", "terminals", "steps", "episode_ids")})
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(4, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, 2)).cuda()
    mlp = MLPPolicy.from_torch(net)
    # parity: the first two environments against the eager driver loop
    Tp = 600
    twin_a, twin_b = make_env(ds, 2), make_env(ds, 2)
    for t in (twin_a, twin_b):
        t.reset_sampler([0, 1])
        t.reset()
    cp = twin_a.collect(mlp, Tp, max_episode_steps=CAP)
    lr, lf = driver_loop(twin_b, mlp, Tp)
    fl = cp.terminated.to(torch.int32) * 2 + cp.truncated.to(torch.int32) * 4
    parity_loop = bool(torch.equal(cp.row, lr) and torch.equal(fl, lf))
    lines = []
    for E in [int(x) for x in a.envs.split(",")]:
        # the graph-replayed loop of tools/vector_env_example.py (torch forward, f64 probabilities, one replay per step)
        env = make_env(ds, E)
        env.reset_sampler(np.arange(E))
        env.reset()
        dist = lambda o: torch.softmax(net(o), dim=1).to(torch.float64)
        g, _ = env.graph_iteration(dist)
        torch.cuda.synchronize()
        n_rep = 1000
        t0 = time.perf_counter()
        for _ in range(n_rep):
            g.replay()
        torch.cuda.synchronize()
        loop_us = (time.perf_counter() - t0) / n_rep * 1e6
        loop_sps = E / (loop_us * 1e-6)
        del g
        for T in [int(x) for x in a.steps.split(",")]:
            env = make_env(ds, E)
            env.reset_sampler(np.arange(E))
            env.reset()
            c = env.collect(mlp, T, max_episode_steps=CAP)  # warm-up (the first T steps)
            torch.cuda.synchronize()
            first = c.row[:, :2].clone()
            reps, t_all, served = 3, 0.0, 0
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                c = env.collect(mlp, T, max_episode_steps=CAP)
                torch.cuda.synchronize()
                t_all += time.perf_counter() - t0
                served += int((c.row >= 0).sum())
            dt = t_all / reps
            parity = parity_loop and bool(torch.equal(first[:min(T, Tp)], cp.row[:min(T, Tp)]))
            rec = {"tool": "bench_collect", "config": "C2", "log_rows": N, "environments": E, "T": T, "network": "4-64-64-2 tanh",
                   "max_episode_steps": CAP, "collect_ms_per_call": dt * 1e3, "collect_us_per_step": dt / T * 1e6,
                   "collect_steps_per_s": E * T / dt, "collect_served_steps_per_s": served / reps / dt,
                   "loop_graph_us_per_step": loop_us, "loop_graph_steps_per_s": loop_sps, "speedup_vs_loop": (E * T / dt) / loop_sps,
                   "parity_ok": parity, "device": torch.cuda.get_device_name(0)}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del c, env
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
