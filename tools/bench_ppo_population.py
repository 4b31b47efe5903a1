"""A PPO epoch (collect + update) for L learners: one PPOPopulation against the same L learners run one after another.

The reference agent's shape: 4-64-64-2 / 4-64-64-1 tanh networks, T * E = 4000 steps per learner and epoch (E environments x T steps of
synth.cartpole_log), 80 + 80 iterations, a target_kl nothing reaches, so every iteration of every learner runs.  Per L one JSON line: ms
per epoch of the population route (VectorPSRS.collect_ppo_population + PPOPopulation.update on L * E environments) and of the loop route
(collect_ppo + PPOLearner.update for each learner in turn, on its own E environments), both in this process on networks of the same
weights and environments of the same seeds, with the collect / update split of each.  Timing: a warm-up epoch of each route, then
`--reps` epochs of each, alternating, every one bracketed by torch.cuda.synchronize(); the median is reported and all samples are kept.
The samplers are reset before every epoch (outside the timed window) so every epoch serves full buffers.

usage: python tools/bench_ppo_population.py [--learners 1 8 64] [--envs 8] [--steps 500] [--reps 5] [--out profiles/ppo_population_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rl_offline_simulation_amd import OfflineDataset, ProbDistribution, spaces, synth  # noqa: E402
from rl_offline_simulation_amd.encoders import CartpoleBoxEncoder  # noqa: E402
from rl_offline_simulation_amd.evaluators import MLPPolicy, MLPValue, PPOLearner, PPOPopulation, VectorPSRS  # noqa: E402


def net(sizes):
    mods = []
    for j in range(len(sizes) - 1):
        mods += [torch.nn.Linear(sizes[j], sizes[j + 1]), torch.nn.Tanh() if j < len(sizes) - 2 else torch.nn.Identity()]
    return torch.nn.Sequential(*mods)


def nets(n):
    """(actors, critics) of n learners, learner l seeded by l: every call gives fresh objects of the same weights"""
    out = []
    for l in range(n):
        torch.manual_seed(l)
        out.append((MLPPolicy.from_torch(net([4, 64, 64, 2])), MLPValue.from_torch(net([4, 64, 64, 1]))))
    return [a for a, _ in out], [c for _, c in out]


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--learners", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--rows", type=int, default=50_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/ppo_population_bench.jsonl")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    e = synth.cartpole_log(a.rows, seed=0)
    ds = OfflineDataset(observation_space=spaces.Box(low=-np.inf, high=np.inf, shape=(4,), dtype=np.float32), action_space=spaces.Discrete(2),
                        action_dist_type=ProbDistribution.Discrete, observations=e["observations"], actions=e["actions"],
                        action_distributions=e["action_distributions"], rewards=e["rewards"], next_observations=e["next_observations"],
                        terminals=e["terminals"], steps=e["steps"])
    kw = dict(train_pi_iters=80, train_v_iters=80, target_kl=1e9)
    E, T = a.envs, a.steps
    lines = []
    for nl in a.learners:
        seeds = np.arange(nl * E) + 1
        whole = VectorPSRS(ds, num_envs=nl * E, num_states=162, encoder=CartpoleBoxEncoder())
        parts = [VectorPSRS(ds, num_envs=E, num_states=162, encoder=CartpoleBoxEncoder()) for _ in range(nl)]
        pop = PPOPopulation(*nets(nl), **kw)
        actors, critics = nets(nl)
        learners = [PPOLearner(actors[l], critics[l], **kw) for l in range(nl)]
        t = {k: [] for k in ("pop", "pop_collect", "pop_update", "loop", "loop_collect", "loop_update")}

        def fresh():
            whole.reset_sampler(seeds)
            whole.reset()
            for l, p in enumerate(parts):
                p.reset_sampler(seeds[l * E:(l + 1) * E])
                p.reset()

        def epoch(keep):
            fresh()
            box = {}
            c = clock(lambda: box.update(b=whole.collect_ppo_population(pop, T)))
            u = clock(lambda: pop.update(box["b"]))
            served = int(box["b"].valid.sum())
            fresh()
            box = {}
            lc = clock(lambda: box.update(b=[parts[l].collect_ppo(actors[l], critics[l], T) for l in range(nl)]))
            lu = clock(lambda: [learners[l].update(box["b"][l]) for l in range(nl)])
            if keep:
                for k, v in (("pop", c + u), ("pop_collect", c), ("pop_update", u), ("loop", lc + lu), ("loop_collect", lc), ("loop_update", lu)):
                    t[k].append(v)
            return served

        epoch(False)  # warm-up of every shape the timed window uses
        served = [epoch(True) for _ in range(a.reps)]
        med = {k: statistics.median(v) for k, v in t.items()}
        line = dict(bench="ppo_population", L=nl, E=E, T=T, iters=[80, 80], net="4-64-64-2 tanh", reps=a.reps, served_per_epoch=served,
                    **{k + "_ms": round(v, 3) for k, v in med.items()}, loop_over_pop=round(med["loop"] / med["pop"], 3),
                    pop_ms_samples=[round(x, 3) for x in t["pop"]], loop_ms_samples=[round(x, 3) for x in t["loop"]],
                    device=torch.cuda.get_device_name(0))
        print(json.dumps(line), flush=True)
        lines.append(line)
        del whole, parts, pop, learners
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
