"""The CartPole PPO example of the reference (examples/cartpole/psrs_from_expert_heuristic.py: PPOAgentRevealed trained inside PSRS on a
logged dataset), vectorised: E environments play E spinup MPI processes of T local steps per epoch.  Per epoch:

  1. VectorPSRS.collect_ppo(actor, critic, T): the actor and the critic inside the collect kernel, the PPO buffer on the device;
  2. the update of PPOAgentRevealed.adapt (offsim4rl/agents/ppo.py:162-201): Adam on the clipped surrogate for up to train_pi_iters
     iterations, stopping early once the approximate KL passes 1.5 * target_kl, then train_v_iters iterations on the value loss --
     --update device (default): PPOLearner.update, the HIP kernels of offsim_ppo_update on the [T, E] records, in place on the weights
     the collect kernel reads; --update torch: torch autograd over PPOBatch.flat(), the new weights read back into the MLPPolicy /
     MLPValue with from_torch every epoch (the comparison route).

  3. the epoch log of the agent (EpRet, EpLen, EpisodesInEpoch, VVals; ppo.py:225-235) --
     --log device (default): ppo_epoch_log, one launch on the records with the open episodes carried in an EpisodeTracker;
     --log host: the loop over the T steps in Python (episode_returns below, T host reads per epoch; the comparison route).

Prints per epoch the mean return of the episodes that ended in it (under either --log), the simulated steps per second of the collect, and
the split of the epoch's time between collect and update; with --log device also the reference's EpLen, EpisodesInEpoch and VVals.  Uses the
synthetic CartPole log of synth.cartpole_log (a uniform-random logging policy).

usage: python tools/ppo_in_psrs.py [--rows 1000000] [--envs 1024] [--steps 256] [--epochs 20] [--hid 64] [--l 2] [--update device|torch]
                                   [--log device|host]"""
import argparse
import os
import sys
import time

import numpy as np
import torch
from torch.optim import Adam

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rl_offline_simulation_amd import OfflineDataset, ProbDistribution, spaces, synth  # noqa: E402
from rl_offline_simulation_amd.encoders import CartpoleBoxEncoder  # noqa: E402
from rl_offline_simulation_amd.evaluators import EpisodeTracker, MLPPolicy, MLPValue, PPOLearner, VectorPSRS, ppo_epoch_log  # noqa: E402


def net(sizes):
    mods = []
    for j in range(len(sizes) - 1):
        mods += [torch.nn.Linear(sizes[j], sizes[j + 1]), torch.nn.Tanh() if j < len(sizes) - 2 else torch.nn.Identity()]
    return torch.nn.Sequential(*mods)


def episode_returns(b, open_ret):
    """Returns of the episodes that ended in this epoch (per environment, the running return carries across epochs in open_ret)."""
    rew, valid = b.rew, b.valid
    end = valid & (b.collected.terminated | b.collected.truncated)
    out = []
    for t in range(rew.shape[0]):
        open_ret += torch.where(valid[t], rew[t], torch.zeros_like(rew[t]))
        if bool(end[t].any()):
            out.append(open_ret[end[t]].clone())
            open_ret[end[t]] = 0.0
    return torch.cat(out) if out else torch.zeros(0, device=rew.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=256, help="local steps per epoch (T)")
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--hid", type=int, default=64)
    ap.add_argument("--l", type=int, default=2)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--lam", type=float, default=0.97)
    ap.add_argument("--clip-ratio", type=float, default=0.2)
    ap.add_argument("--pi-lr", type=float, default=3e-4)
    ap.add_argument("--vf-lr", type=float, default=1e-3)
    ap.add_argument("--train-pi-iters", type=int, default=80)
    ap.add_argument("--train-v-iters", type=int, default=80)
    ap.add_argument("--target-kl", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--update", choices=("device", "torch"), default="device")
    ap.add_argument("--log", choices=("device", "host"), default="device", help="the epoch log: ppo_epoch_log, or the Python loop over the steps")
    a = ap.parse_args()

    e = synth.cartpole_log(a.rows, seed=a.seed)
    ds = OfflineDataset(spaces.Box(-np.inf, np.inf, (4,), np.float32), spaces.Discrete(2), ProbDistribution.Discrete,
                        **{k: e[k] for k in ("observations", "actions", "action_distributions", "rewards", "next_observations", "terminals", "steps", "episode_ids")})
    env = VectorPSRS(ds, num_envs=a.envs, num_states=162, encoder=CartpoleBoxEncoder())
    env.reset_sampler(np.arange(a.envs) + a.seed)
    env.reset()
    torch.manual_seed(a.seed)
    pi_net = net([4] + [a.hid] * a.l + [2]).cuda()
    v_net = net([4] + [a.hid] * a.l + [1]).cuda()
    open_ret = torch.zeros(a.envs, device="cuda")  # (--log host)
    tracker = EpisodeTracker(a.envs, "cuda")  # (--log device)
    actor, critic = MLPPolicy.from_torch(pi_net), MLPValue.from_torch(v_net)
    if a.update == "device":  # (pi_net / v_net only supply the initial weights; the learner steps the device copy the kernel reads)
        learner = PPOLearner(actor, critic, pi_lr=a.pi_lr, vf_lr=a.vf_lr, clip_ratio=a.clip_ratio, train_pi_iters=a.train_pi_iters,
                             train_v_iters=a.train_v_iters, target_kl=a.target_kl)
    else:
        pi_opt, v_opt = Adam(pi_net.parameters(), lr=a.pi_lr), Adam(v_net.parameters(), lr=a.vf_lr)
    for epoch in range(a.epochs):
        if a.update == "torch":
            actor, critic = MLPPolicy.from_torch(pi_net), MLPValue.from_torch(v_net)  # the current weights, as the kernel reads them
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b = env.collect_ppo(actor, critic, a.steps, max_episode_steps=500, gamma=a.gamma, lam=a.lam)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if not bool(b.valid.any()):
            print(f"epoch {epoch}: no transition served (the log ran dry)")
            break
        if a.update == "device":
            stop = int(learner.update(b).StopIter)  # (the int() is this script's only read-back; update itself enqueues and returns)
        else:
            d = b.flat()
            obs, act, adv, logp_old, ret = d["obs"].float(), d["act"].long(), d["adv"], d["logp"], d["ret"]

            def loss_pi():
                logits = pi_net(obs)
                dist = torch.distributions.Categorical(logits=logits)
                logp = dist.log_prob(act)
                ratio = torch.exp(logp - logp_old)
                clip_adv = torch.clamp(ratio, 1 - a.clip_ratio, 1 + a.clip_ratio) * adv
                return -(torch.min(ratio * adv, clip_adv)).mean(), (logp_old - logp).mean().item()

            stop = a.train_pi_iters - 1  # (StopIter as adapt() logs it: the pass that stopped, else the last one)
            for i in range(a.train_pi_iters):
                pi_opt.zero_grad()
                loss, kl = loss_pi()
                if kl > 1.5 * a.target_kl:
                    stop = i
                    break
                loss.backward()
                pi_opt.step()
            for _ in range(a.train_v_iters):
                v_opt.zero_grad()
                ((v_net(obs)[:, 0] - ret) ** 2).mean().backward()
                v_opt.step()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        extra = ""
        if a.log == "host":
            rets = episode_returns(b, open_ret)
        else:  # one launch; the lists are read back here only because this script prints the mean over ENDED episodes under either --log
            log, eps = ppo_epoch_log(b, tracker, episodes=True)
            rets = eps.ep_ret[torch.arange(eps.ep_ret.shape[1], device="cuda")[None, :] < eps.n_ep[:, None]]
            extra = (f"  EpRet {float(log.EpRet):.2f} +- {float(log.StdEpRet):.2f} [{float(log.MinEpRet):.1f}, {float(log.MaxEpRet):.1f}] over "
                     f"{int(log.Entries)} entries  EpLen {float(log.EpLen):.1f}  EpisodesInEpoch {int(log.EpisodesInEpoch)}  VVals {float(log.VVals):.3f}")
        served = int(b.valid.sum())
        ep = f"{float(rets.mean()):8.2f} over {rets.numel():6d} episodes" if rets.numel() else "      -- (no episode ended)"
        print(f"epoch {epoch:3d}: return {ep}  {served / (t1 - t0):.3e} simulated steps/s  collect {1e3 * (t1 - t0):7.2f} ms  "
              f"update {1e3 * (t2 - t1):7.2f} ms (StopIter {stop}){extra}", flush=True)


if __name__ == "__main__":
    main()
