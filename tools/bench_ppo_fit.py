"""PPOLearner.fit / PPOPopulation.fit against the same epochs with the epoch log computed by the Python loop over the steps.

A measurement, not a threshold.  The reference agent's shape: 4-64-64-2 / 4-64-64-1 tanh networks, T * E = 4000 steps per learner and epoch
(E environments x T steps of synth.cartpole_log), 80 + 80 iterations, a target_kl nothing reaches.  Per L one JSON line: ms per epoch of

  fit    collect -> ppo_epoch_log (one launch, nothing read back) -> update, `--epochs` epochs enqueued, one synchronisation at the end;
  host   collect -> episode_returns of tools/ppo_in_psrs.py (its --log host loop: a host read at every one of the T steps) on each
         learner's own columns in turn, as a user of a population has to write it -> update.

Both routes run in this process on networks of the same weights and environments of the same seeds.  Timing: a warm-up run of each route,
then `--reps` runs of each, alternating; a run is `--epochs` epochs bracketed by torch.cuda.synchronize(); the median is reported and all
samples are kept.  The samplers are reset before every run (outside the timed window).

usage: python tools/bench_ppo_fit.py [--learners 1 8 64] [--envs 8] [--steps 500] [--epochs 2] [--reps 3] [--out profiles/ppo_fit_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_ppo_population import nets  # noqa: E402
from ppo_in_psrs import episode_returns  # noqa: E402
from rl_offline_simulation_amd import OfflineDataset, ProbDistribution, spaces, synth  # noqa: E402
from rl_offline_simulation_amd.encoders import CartpoleBoxEncoder  # noqa: E402
from rl_offline_simulation_amd.evaluators import EpisodeTracker, PPOLearner, PPOPopulation, VectorPSRS  # noqa: E402


def columns(b, sl):
    """what episode_returns reads of a batch, for the environments in `sl`"""
    c = types.SimpleNamespace(terminated=b.collected.terminated[:, sl], truncated=b.collected.truncated[:, sl])
    return types.SimpleNamespace(rew=b.rew[:, sl], valid=b.valid[:, sl], collected=c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--learners", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--rows", type=int, default=50_000)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="profiles/ppo_fit_bench.jsonl")
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
        env = VectorPSRS(ds, num_envs=nl * E, num_states=162, encoder=CartpoleBoxEncoder())

        def learner():
            actors, critics = nets(nl)
            return PPOLearner(actors[0], critics[0], **kw) if nl == 1 else PPOPopulation(actors, critics, **kw)

        fit_l, host_l = learner(), learner()
        collect = (lambda: env.collect_ppo(host_l.actor, host_l.critic, T)) if nl == 1 else (lambda: env.collect_ppo_population(host_l, T))
        t = {"fit": [], "host": []}
        served = {}

        def fresh():
            env.reset_sampler(seeds)
            env.reset()

        def run_fit():
            log = fit_l.fit(env, a.epochs, T, tracker=EpisodeTracker(nl * E, "cuda"))
            torch.cuda.synchronize()
            served["fit"] = log.StepsServed.sum(0).tolist() if nl > 1 else int(log.StepsServed.sum())

        def run_host():
            open_ret = [torch.zeros(E, device="cuda") for _ in range(nl)]
            for _ in range(a.epochs):
                b = collect()
                for l in range(nl):
                    episode_returns(columns(b, slice(l * E, (l + 1) * E)), open_ret[l])
                host_l.update(b)
            torch.cuda.synchronize()

        def clock(fn):
            fresh()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            return 1e3 * (time.perf_counter() - t0) / a.epochs

        clock(run_fit), clock(run_host)  # warm-up of every shape the timed window uses
        for _ in range(a.reps):
            t["fit"].append(clock(run_fit))
            t["host"].append(clock(run_host))
        med = {k: statistics.median(v) for k, v in t.items()}
        line = dict(bench="ppo_fit", L=nl, E=E, T=T, epochs_per_run=a.epochs, iters=[80, 80], net="4-64-64-2 tanh", reps=a.reps,
                    fit_ms_per_epoch=round(med["fit"], 3), host_log_ms_per_epoch=round(med["host"], 3), host_over_fit=round(med["host"] / med["fit"], 3),
                    fit_ms_samples=[round(x, 3) for x in t["fit"]], host_ms_samples=[round(x, 3) for x in t["host"]],
                    served_last_fit=served["fit"], device=torch.cuda.get_device_name(0))
        print(json.dumps(line), flush=True)
        lines.append(line)
        del env, fit_l, host_l
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
