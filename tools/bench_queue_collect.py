#!/usr/bin/env python3
"""A PPO learner's data collection on the queue simulator: ONE collect_ppo launch of VectorQueueEvaluator (offsim_queue_collect_ppo) against
the hand loop it replaces -- per simulated step MLPPolicy.forward on the device, the probabilities read back, the actions drawn on the
host, BatchedQueueEvaluator.step (two launches and a host read) and the resets -- and beside VectorPSRS.collect_ppo on the same log.

The log is bench_queue_drivers.py's (synth.synth_iid, N = 100 000, 25 states, 5 actions) with synthetic 4-wide f32 observations (feature 0
the state id, the rest noise); the actor is a 4-64-64-5 tanh network, the critic 4-64-64-1.  E in {8, 1024, 4096} environments, T = 500
steps, step cap 500.  Synchronised wall time, medians of --repeats runs, the routes alternating.  The hand loop has no critic, no logp and
no GAE (it is the cheaper job), and draws every environment's action from one host Generator, so only the step counts are comparable, not
the trajectories; that the launch computes the right thing is the test suite's business (tests/test_gpu_queue_collect.py).

  python tools/bench_queue_collect.py [--out FILE] [--repeats 5] [--steps 500] [--envs 8,1024,4096] [--only-launch E]
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

from rl_offline_simulation_amd import OfflineDataset, ProbDistribution, spaces, synth  # noqa: E402
from rl_offline_simulation_amd import _lib as L  # noqa: E402
from rl_offline_simulation_amd.evaluators import BatchedQueueEvaluator, MLPPolicy, MLPValue, VectorPSRS, VectorQueueEvaluator  # noqa: E402
from rl_offline_simulation_amd.evaluators.obs_policy import obs_tensor  # noqa: E402

N, NS, NA, DO, HID, CAP = 100000, 25, 5, 4, 64, 500


class Lookup:
    """encode(observations) -> z: the states travel with the log"""

    def __init__(self, obs, z, nobs, zn):
        self.pairs = [(obs, z), (nobs, zn)]

    def encode(self, x):
        for a, z in self.pairs:
            if x is a or np.array_equal(np.asarray(x), a):
                return z
        raise KeyError("unknown observations")


def log():
    e = synth.synth_iid(N, NS, NA, seed=1)
    g = np.random.default_rng(2)
    obs, nobs = g.standard_normal((N, DO)).astype(np.float32), g.standard_normal((N, DO)).astype(np.float32)
    obs[:, 0], nobs[:, 0] = e["z"], e["z_next"]
    ds = OfflineDataset(observation_space=spaces.Box(low=-np.inf, high=np.inf, shape=(DO,), dtype=np.float32), action_space=spaces.Discrete(NA),
                        action_dist_type=ProbDistribution.Discrete, observations=obs, actions=e["actions"],
                        action_distributions=e["action_distributions"], rewards=e["rewards"], next_observations=nobs, terminals=e["terminals"],
                        steps=e["steps"])
    return e, ds, Lookup(obs, e["z"], nobs, e["z_next"])


def networks():
    def net(n_out, seed):
        torch.manual_seed(seed)
        return torch.nn.Sequential(torch.nn.Linear(DO, HID), torch.nn.Tanh(), torch.nn.Linear(HID, HID), torch.nn.Tanh(), torch.nn.Linear(HID, n_out))
    return MLPPolicy.from_torch(net(NA, 0)), MLPValue.from_torch(net(1, 1))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def one_launch(env, actor, critic, E, T):
    env.reset_sampler(list(range(E)))
    env.reset()
    ms, b = timed(lambda: env.collect_ppo(actor, critic, T, max_episode_steps=CAP))
    return ms, int(b.valid.sum())


def hand_loop(b, e, xn, x0, actor, E, T):
    """The loop over BatchedQueueEvaluator.step: forward, host draw, step, reset of the finished environments -- per simulated step."""
    done_col = torch.as_tensor(np.asarray(e["terminals"]) != 0, device=xn.device)
    b.reset_sampler(list(range(E)))
    rng = np.random.default_rng(0)

    def run():
        row0 = b.reset().long()
        x = x0[row0.clamp(min=0)]
        ep_t = torch.zeros(E, dtype=torch.int32, device=xn.device)
        live = row0 >= 0
        served = 0
        for _ in range(T):
            p = actor.forward(x).cpu().numpy().astype(np.float64)
            cdf = np.cumsum(p, axis=1)
            cdf /= cdf[:, -1:]
            A = np.minimum((cdf <= rng.random(E)[:, None]).sum(1), NA - 1)
            row, status = b.step(A)
            ok = (status == L.ST_OK) & live
            live = ok
            served += int(ok.sum())
            rl = row.long().clamp(min=0)
            ep_t = torch.where(ok, ep_t + 1, ep_t)
            fin = ok & (done_col[rl] | (ep_t >= CAP))
            x = torch.where(ok[:, None], xn[rl], x)
            if bool(fin.any()):
                r0 = b.reset(fin.to(torch.uint8).contiguous()).long()
                x = torch.where(fin[:, None], x0[r0.clamp(min=0)], x)
                ep_t = torch.where(fin, torch.zeros_like(ep_t), ep_t)
                live = live & ~(fin & (r0 < 0))
        return served
    return timed(run)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "queue_collect_bench.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--envs", default="8,1024,4096")
    ap.add_argument("--only-launch", type=int, default=0)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    e, ds, enc = log()
    actor, critic = networks()
    T = a.steps
    if a.only_launch:
        env = VectorQueueEvaluator(ds, a.only_launch, num_states=NS, encoder=enc)
        for _ in range(2):
            print(json.dumps(dict(what="one launch", envs=a.only_launch, T=T, ms=one_launch(env, actor, critic, a.only_launch, T)[0])))
        return 0
    cols = (e["z"], e["actions"], e["rewards"], e["z_next"], e["terminals"], e["action_distributions"], np.asarray(e["steps"]) == 0)
    xn, x0 = obs_tensor(ds.experience["next_observations"], dev), obs_tensor(ds.experience["observations"], dev)
    lines = []
    for E in [int(v) for v in a.envs.split(",")]:
        q, psrs, b = VectorQueueEvaluator(ds, E, num_states=NS, encoder=enc), VectorPSRS(ds, E, num_states=NS, encoder=enc), BatchedQueueEvaluator(*cols, R=E)
        t = {"queue": [], "psrs": [], "hand": []}
        served = {}
        for rep in range(a.repeats + 1):  # (the first run warms up: module load, allocations)
            for route in ("queue", "hand", "psrs"):
                if route == "hand":
                    ms, n = hand_loop(b, e, xn, x0, actor, E, T)
                else:
                    ms, n = one_launch(q if route == "queue" else psrs, actor, critic, E, T)
                served[route] = n
                if rep:
                    t[route].append(ms)
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        for route, what in (("queue", "VectorQueueEvaluator.collect_ppo, one launch + advantages"),
                            ("hand", "hand loop: MLPPolicy.forward + host draw + BatchedQueueEvaluator.step + reset"),
                            ("psrs", "VectorPSRS.collect_ppo, one launch + advantages")):
            lines.append(dict(what=what, route=route, envs=E, T=T, N=N, steps_served=served[route], ms_median=med[route], ms_min=min(t[route]),
                              ms_max=max(t[route]), repeats=a.repeats, us_per_step_of_an_env=med[route] * 1e3 / T,
                              steps_per_s=served[route] / (med[route] * 1e-3)))
        lines.append(dict(what="ratios of the medians", envs=E, T=T, hand_over_queue=med["hand"] / med["queue"], psrs_over_queue=med["psrs"] / med["queue"]))
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
