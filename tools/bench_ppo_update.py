"""PPO update on the device against the torch autograd loop, on the same collect_ppo buffer in the same process.

C2 networks (4-64-64-2 / 4-64-64-1, tanh), E environments x T steps of synth.cartpole_log.  Per T one JSON line: ms per actor / critic
iteration of the device route (offsim_ppo_update; a target_kl nothing reaches, so every iteration runs), ms per whole update for the device
route and for the torch route (the loop of tools/ppo_in_psrs.py --update torch: Adam on flat() tensors, the KL read back every actor
iteration), the collect / update split of an epoch, and a parity flag (ppo_grad against torch autograd in f64 on the device, within 4 x
the error of torch's own f32 autograd, as tests/test_gpu_ppo_update.py checks it).  Timing: warm-up, then the median of `--reps` runs,
each bracketed by torch.cuda.synchronize().

usage: python tools/bench_ppo_update.py [--envs 4096] [--steps 64 256 1024] [--reps 5] [--out profiles/ppo_update_bench.jsonl]"""
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
from rl_offline_simulation_amd.evaluators import MLPPolicy, MLPValue, PPOLearner, VectorPSRS, ppo_grad  # noqa: E402


def net(sizes):
    mods = []
    for j in range(len(sizes) - 1):
        mods += [torch.nn.Linear(sizes[j], sizes[j + 1]), torch.nn.Tanh() if j < len(sizes) - 2 else torch.nn.Identity()]
    return torch.nn.Sequential(*mods)


def timed(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts)


def torch_update(pi_net, v_net, pi_opt, v_opt, d, iters, clip, target_kl):
    obs, act, adv, logp_old, ret = d["obs"].float(), d["act"].long(), d["adv"], d["logp"], d["ret"]
    for i in range(iters):
        pi_opt.zero_grad()
        logp = torch.distributions.Categorical(logits=pi_net(obs)).log_prob(act)
        ratio = torch.exp(logp - logp_old)
        loss = -(torch.min(ratio * adv, torch.clamp(ratio, 1 - clip, 1 + clip) * adv)).mean()
        if (logp_old - logp).mean().item() > 1.5 * target_kl:
            break
        loss.backward()
        pi_opt.step()
    for _ in range(iters):
        v_opt.zero_grad()
        ((v_net(obs)[:, 0] - ret) ** 2).mean().backward()
        v_opt.step()


def grad64(m, kind, f, dtype):
    m = m.to(dtype)
    t = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in f.items()}
    if kind == "actor":
        logp = torch.distributions.Categorical(logits=m(t["obs"])).log_prob(t["act"].long())
        ratio = torch.exp(logp - t["logp"])
        loss = -(torch.min(ratio * t["adv"], torch.clamp(ratio, 0.8, 1.2) * t["adv"])).mean()
    else:
        loss = ((m(t["obs"])[:, 0] - t["ret"]) ** 2).mean()
    loss.backward()
    return torch.cat([p.grad.reshape(-1) for x in m if isinstance(x, torch.nn.Linear) for p in (x.weight, x.bias)]).double()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--iters", type=int, default=80)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    e = synth.cartpole_log(a.rows, seed=0)
    ds = OfflineDataset(spaces.Box(-np.inf, np.inf, (4,), np.float32), spaces.Discrete(2), ProbDistribution.Discrete,
                        **{k: e[k] for k in ("observations", "actions", "action_distributions", "rewards", "next_observations", "terminals", "steps", "episode_ids")})
    lines = []
    for T in a.steps:
        env = VectorPSRS(ds, num_envs=a.envs, num_states=162, encoder=CartpoleBoxEncoder())
        env.reset_sampler(np.arange(a.envs))
        env.reset()
        torch.manual_seed(0)
        pi_net, v_net = net([4, 64, 64, 2]).cuda(), net([4, 64, 64, 1]).cuda()
        actor, critic = MLPPolicy.from_torch(pi_net), MLPValue.from_torch(v_net)
        b = env.collect_ppo(actor, critic, T, max_episode_steps=500)  # (warm-up; the timed call continues from its state)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b = env.collect_ppo(actor, critic, T, max_episode_steps=500)
        torch.cuda.synchronize()
        collect_ms = 1e3 * (time.perf_counter() - t0)
        flat = b.flat()
        n = int(b.valid.sum())
        # parity, as the at-scale test
        parity = True
        for nn_, mlp, kind in ((pi_net, actor, "actor"), (v_net, critic, "critic")):
            g = ppo_grad(mlp, b, kind).grad.double()
            g64 = grad64(mlp.to_torch().cuda(), kind, flat, torch.float64)
            g32 = grad64(mlp.to_torch().cuda(), kind, flat, torch.float32)
            bound = max(4.0 * float((g32 - g64).abs().max()), 4.0 * 2.0 ** -23 * float(g64.abs().max()))
            parity = parity and float((g - g64).abs().max()) <= bound
        # device route: per-iteration cost with the early stop out of reach, then the whole update at the agent's defaults
        never = PPOLearner(actor, critic, train_pi_iters=a.iters, train_v_iters=0, target_kl=1e9)
        pi_ms = timed(lambda: never.update(b), a.reps) / a.iters
        never_v = PPOLearner(actor, critic, train_pi_iters=0, train_v_iters=a.iters, target_kl=1e9)
        v_ms = timed(lambda: never_v.update(b), a.reps) / a.iters
        actor2, critic2 = MLPPolicy.from_torch(pi_net), MLPValue.from_torch(v_net)
        full = PPOLearner(actor2, critic2, train_pi_iters=a.iters, train_v_iters=a.iters, target_kl=1e9)
        dev_ms = timed(lambda: full.update(b), a.reps)
        # torch route (the same never-stopping loop: target_kl out of reach, the KL still read back every iteration as the loop does)
        pi_opt, v_opt = torch.optim.Adam(pi_net.parameters(), lr=3e-4), torch.optim.Adam(v_net.parameters(), lr=1e-3)
        torch_ms = timed(lambda: torch_update(pi_net, v_net, pi_opt, v_opt, flat, a.iters, 0.2, 1e9), a.torch_reps)
        line = dict(bench="ppo_update", net="C2 4-64-64-{2,1} tanh", envs=a.envs, T=T, records=T * a.envs, valid=n, iters=a.iters,
                    actor_iter_ms=round(pi_ms, 4), critic_iter_ms=round(v_ms, 4), update_device_ms=round(dev_ms, 3),
                    update_torch_ms=round(torch_ms, 3), torch_over_device=round(torch_ms / dev_ms, 2), collect_ms=round(collect_ms, 3),
                    epoch_device_ms=round(collect_ms + dev_ms, 3), update_share_device=round(dev_ms / (collect_ms + dev_ms), 3),
                    epoch_torch_ms=round(collect_ms + torch_ms, 3), parity=bool(parity), device=torch.cuda.get_device_name(0))
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
