"""VectorPSRS.collect_ppo (critic, logp and the PPO buffer on the device) against the routes it replaces, on config C2: 1 M CartPole rows,
4096 environments, the 4 -> 64 -> 64 -> 2 tanh actor and the 4 -> 64 -> 64 -> 1 tanh critic of the reference's PPO agent.  Three routes per
T, each from the same sampler state:

  collect       collect(actor, T): the acting half alone (no critic, no buffer)
  collect_ppo   one launch of offsim_vector_collect_ppo + the buffer kernels of offsim_ppo_advantages
  torch         collect(actor, T, record_obs=True), the critic in torch over the recorded observations, then GAE and rewards-to-go as a
                torch loop over T (what a user writes without collect_ppo) and spinup's normalisation

parity_ok: the three routes served the same rows, and the torch route's advantages equal collect_ppo's within 1e-3 (relative).
Appends JSON lines to profiles/ppo_bench.jsonl.  The kernel split comes from a run of this tool under rocprofv3 --kernel-trace --stats.

usage: python tools/bench_ppo.py [--envs 4096] [--steps 64,256,1024] [--rows 1000000] [--reps 3] [--out profiles/ppo_bench.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rl_offline_simulation_amd import OfflineDataset, ProbDistribution, spaces, synth  # noqa: E402
from rl_offline_simulation_amd.encoders import CartpoleBoxEncoder  # noqa: E402
from rl_offline_simulation_amd.evaluators import MLPPolicy, MLPValue, VectorPSRS  # noqa: E402

CAP, GAMMA, LAM = 500, 0.99, 0.97


def torch_route(env, actor, vnet, T):
    """collect with the observations recorded, then what a PPO user does in torch: the critic, GAE-lambda backwards over T, normalisation
    (the reference's bootstrap rules, as collect_ppo's default)."""
    c = env.collect(actor, T, max_episode_steps=CAP, record_obs=True)
    E = env.num_envs
    with torch.no_grad():
        val = vnet(c.obs.reshape(T * E, -1).float())[:, 0].reshape(T, E)
        fin = vnet(c.final_obs.reshape(E, -1).float())[:, 0]
    valid = c.row >= 0
    rew = c.reward.to(torch.float32)
    end = valid & (c.terminated | c.truncated)
    adv = torch.zeros((T, E), dtype=torch.float64, device=val.device)
    ret = torch.zeros_like(adv)
    nv, A, G = fin.double(), torch.zeros(E, dtype=torch.float64, device=val.device), fin.double()
    for t in range(T - 1, -1, -1):
        v, r = val[t].double(), rew[t].double()
        b = torch.where(c.truncated[t] | torch.tensor(t == T - 1, device=v.device), v, torch.zeros_like(v))
        nv, A, G = torch.where(end[t], b, nv), torch.where(end[t], torch.zeros_like(A), A), torch.where(end[t], b, G)
        d = r + GAMMA * nv - v
        A2, G2 = d + GAMMA * LAM * A, r + GAMMA * G
        A, G, nv = torch.where(valid[t], A2, A), torch.where(valid[t], G2, G), torch.where(valid[t], v, nv)
        adv[t], ret[t] = torch.where(valid[t], A2, 0.0), torch.where(valid[t], G2, 0.0)
    x = adv.float()[valid].double()
    mean = x.mean()
    std = ((x - mean) ** 2).mean().sqrt()
    return c, torch.where(valid, (adv.float() - mean) / std, 0.0).float(), ret.float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="4096")
    ap.add_argument("--steps", default="64,256,1024")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ppo_bench.jsonl"))
    a = ap.parse_args()
    N = a.rows
    e = synth.cartpole_log(N, seed=0)
    ds = OfflineDataset(spaces.Box(-np.inf, np.inf, (4,), np.float32), spaces.Discrete(2), ProbDistribution.Discrete,
                        **{k: e[k] for k in ("observations", "actions", "action_distributions", "rewards", "next_observations", "terminals", "steps", "episode_ids")})
    torch.manual_seed(0)
    pnet = torch.nn.Sequential(torch.nn.Linear(4, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, 2)).cuda()
    vnet = torch.nn.Sequential(torch.nn.Linear(4, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, 1)).cuda()
    actor, critic = MLPPolicy.from_torch(pnet), MLPValue.from_torch(vnet)
    lines = []
    for E in [int(x) for x in a.envs.split(",")]:
        for T in [int(x) for x in a.steps.split(",")]:
            def fresh():
                env = VectorPSRS(ds, num_envs=E, num_states=162, encoder=CartpoleBoxEncoder())
                env.reset_sampler(np.arange(E))
                env.reset()
                return env

            routes = {"collect": lambda env: env.collect(actor, T, max_episode_steps=CAP, record_obs=False),
                      "collect_ppo": lambda env: env.collect_ppo(actor, critic, T, max_episode_steps=CAP, gamma=GAMMA, lam=LAM),
                      "torch": lambda env: torch_route(env, actor, vnet, T)}
            rec = {"tool": "bench_ppo", "config": "C2", "log_rows": N, "environments": E, "T": T, "actor": "4-64-64-2 tanh", "critic": "4-64-64-1 tanh",
                   "max_episode_steps": CAP}
            first = {}
            for name, fn in routes.items():
                env = fresh()
                out = fn(env)  # warm-up: the first T steps (also the parity sample)
                torch.cuda.synchronize()
                first[name] = out
                t_all = 0.0
                for _ in range(a.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(env)
                    torch.cuda.synchronize()
                    t_all += time.perf_counter() - t0
                dt = t_all / a.reps
                rec[f"{name}_ms_per_call"] = dt * 1e3
                rec[f"{name}_steps_per_s"] = E * T / dt
                del env
                torch.cuda.empty_cache()
            p, (c_t, adv_t, ret_t), c0 = first["collect_ppo"], first["torch"], first["collect"]
            rows_ok = bool(torch.equal(p.collected.row, c0.row) and torch.equal(c_t.row, c0.row))
            rel = lambda x, y: float(((x - y).abs() / y.abs().clamp(min=1.0)).max())
            rec["torch_vs_collect_ppo_adv_rel"] = rel(adv_t, p.adv)
            rec["torch_vs_collect_ppo_ret_rel"] = rel(ret_t, p.ret)
            rec["parity_ok"] = rows_ok and rec["torch_vs_collect_ppo_adv_rel"] < 1e-3 and rec["torch_vs_collect_ppo_ret_rel"] < 1e-3
            rec["collect_ppo_over_collect"] = rec["collect_ppo_steps_per_s"] / rec["collect_steps_per_s"]
            rec["collect_ppo_over_torch"] = rec["collect_ppo_steps_per_s"] / rec["torch_steps_per_s"]
            rec["device"] = torch.cuda.get_device_name(0)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del first, p, c0, c_t
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
