#!/usr/bin/env python3
"""Generate tests/golden/ppo_update/*.npz by RUNNING THE REFERENCE's PPOAgentRevealed.adapt() (offsim4rl/agents/ppo.py:162-223) on CPU torch.

Run from the repo root:   python tests/golden/make_golden_ppo_update.py
Needs /root/reference (read-only); nothing of it is copied.  The agent is loaded by path with the spinup / gym stand-ins of
make_golden_ppo.py.  Its buffer is filled through its own store() / finish_path() -- observations from a fixed generator, actions, values and
log-probabilities from the agent's own ac.step() / get_logp(), episodes of random length -- and then its own adapt() runs, with

  buf.get                       wrapped to keep what it returned (obs, act, adv, logp, ret);
  _compute_loss_pi / _loss_v    wrapped to log (loss, kl) of every call: call 0 is adapt's "old" pass, calls 1.. are the iterations;
  logger.store                  a stand-in that keeps what adapt() logs (LossPi, LossV, KL, Entropy, ClipFrac, DeltaLoss*, StopIter).

The gradient of the first pass of each network is taken with the loss functions of a second agent built from the same seed (the same
initial weights, asserted) on the data adapt() saw.
Every recorded kl must lie at least 5 % of 1.5 * target_kl away from that threshold, so ulp differences cannot move StopIter: asserted here
for the seed chosen (the first of range(50) that satisfies it and the fixture's stop requirement by the reference alone).
"""
import importlib.util
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(ROOT, "tests", "golden", "ppo_update")
MARGIN = 0.05


def _import(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def flat(mods):
    return np.concatenate([p.detach().numpy().ravel() for m in mods if isinstance(m, nn.Linear) for p in (m.weight, m.bias)])


def flat_grad(mods):
    return np.concatenate([p.grad.detach().numpy().ravel() for m in mods if isinstance(m, nn.Linear) for p in (m.weight, m.bias)])


def run(G, ppo, seed, n, obs_dim, nA, hidden, activation, hyper):
    logged = {}

    class Logger(G.EpochLogger):
        def store(self, **kw):
            logged.update(kw)

    agent = ppo.PPOAgentRevealed(G._Box(shape=(obs_dim,)), G._Discrete(nA), ac_kwargs=dict(hidden_sizes=list(hidden), activation=activation),
                                 logger=Logger(), seed=seed, steps_per_epoch=n, **hyper)
    rng = np.random.default_rng(seed)
    left = 0
    for i in range(n):  # the agent's own buffer, through its own store / finish_path
        if left == 0:
            left = int(rng.integers(5, 60))
        o = rng.normal(size=obs_dim).astype(np.float32) * np.float32(0.7)
        pi, v = agent.ac.step(torch.as_tensor(o))
        a = pi.sample().numpy()
        agent.buf.store(o, a, float(rng.normal() * 0.5 + 1.0), v, agent.ac.get_logp(pi, a).numpy())
        left -= 1
        if left == 0 or i == n - 1:
            agent.buf.finish_path(float(v) if i == n - 1 else 0.0)
    got = {}
    get = agent.buf.get

    def get_and_keep():
        d = get()
        got.update({k: v.numpy().copy() for k, v in d.items()})
        return d

    agent.buf.get = get_and_keep
    pi_mods, v_mods = list(agent.ac.pi.logits_net), list(agent.ac.v.v_net)
    before = dict(pi=flat(pi_mods), v=flat(v_mods))
    calls = dict(pi=[], v=[])
    lp, lv = agent._compute_loss_pi, agent._compute_loss_v

    def loss_pi(tr):
        loss, info = lp(tr)
        calls["pi"].append((loss.item(), info["kl"]))
        return loss, info

    def loss_v(tr):
        loss = lv(tr)
        calls["v"].append((loss.item(), 0.0))
        return loss

    agent._compute_loss_pi, agent._compute_loss_v = loss_pi, loss_v
    agent.adapt()
    data = {k: got[k] for k in ("obs", "act", "adv", "logp", "ret")}  # what adapt()'s own get() returned
    # the first pass's gradients, by the agent's own loss functions at the weights before (a second agent with the same seed)
    twin = ppo.PPOAgentRevealed(G._Box(shape=(obs_dim,)), G._Discrete(nA), ac_kwargs=dict(hidden_sizes=list(hidden), activation=activation),
                                logger=Logger(), seed=seed, steps_per_epoch=n, **hyper)
    assert np.array_equal(flat(list(twin.ac.pi.logits_net)), before["pi"])
    tr = {k: torch.as_tensor(v) for k, v in data.items()}
    l0, info0 = twin._compute_loss_pi(tr)
    l0.backward()
    twin._compute_loss_v(tr).backward()
    g_pi, g_v = flat_grad(list(twin.ac.pi.logits_net)), flat_grad(list(twin.ac.v.v_net))
    out = dict(data, pi_before=before["pi"], v_before=before["v"], pi_after=flat(pi_mods), v_after=flat(v_mods), g_pi=g_pi, g_v=g_v,
               pi_trace=np.asarray(calls["pi"][1:], np.float64), v_trace=np.asarray(calls["v"][1:], np.float64),
               pi_old=np.asarray(calls["pi"][0], np.float64), v_old=np.float64(calls["v"][0][0]), ent_old=np.float64(info0["ent"]),
               sizes_pi=np.asarray([obs_dim] + list(hidden) + [nA], np.int64), sizes_v=np.asarray([obs_dim] + list(hidden) + [1], np.int64),
               **{f"log_{k}": np.float64(v) for k, v in logged.items()})
    return out


def ok_margin(trace, target_kl):
    lim = 1.5 * target_kl
    return bool(np.all(np.abs(trace[:, 1] - lim) >= MARGIN * lim))


def main():
    G = _import("make_golden_ppo", os.path.join(HERE, "make_golden_ppo.py"))
    ppo, _ = G.load_reference()
    os.makedirs(OUT, exist_ok=True)
    base = dict(gamma=0.99, lam=0.97, clip_ratio=0.2, pi_lr=3e-4, vf_lr=1e-3, train_pi_iters=80, train_v_iters=80, target_kl=0.01)
    cases = (
        # every iteration runs (a target_kl the 80 steps stay under)
        ("ppo_update_full_tanh", dict(n=3000, obs_dim=4, nA=2, hidden=(32, 32), activation=nn.Tanh), dict(base, target_kl=0.05), "full"),
        # a larger pi_lr and a smaller target_kl: the KL test stops the actor in the middle
        ("ppo_update_stop_tanh", dict(n=3000, obs_dim=4, nA=2, hidden=(32, 32), activation=nn.Tanh), dict(base, pi_lr=1e-3, target_kl=0.003),
         "stop"),
        # three actions, ReLU, other widths
        ("ppo_update_relu_na3", dict(n=2500, obs_dim=6, nA=3, hidden=(24, 12), activation=nn.ReLU),
         dict(base, pi_lr=1e-3, train_pi_iters=40, train_v_iters=30), "any"),
    )
    for name, shape, hyper, want in cases:
        for seed in range(50):
            out = run(G, ppo, seed, hyper=hyper, **shape)
            stop, iters = int(out["log_StopIter"]), hyper["train_pi_iters"]
            stopped = len(out["pi_trace"]) < iters or out["pi_trace"][-1, 1] > 1.5 * hyper["target_kl"]
            if not ok_margin(out["pi_trace"], hyper["target_kl"]):
                continue
            if (want == "full" and stopped) or (want == "stop" and not (stopped and 3 <= stop <= iters - 10)):
                continue
            break
        else:
            raise SystemExit(f"{name}: no seed satisfies the margin and the stop requirement")
        assert ok_margin(out["pi_trace"], hyper["target_kl"])
        out.update({f"hyper_{k}": np.float64(v) for k, v in hyper.items()}, seed=np.int64(seed),
                   activation=np.asarray("tanh" if shape["activation"] is nn.Tanh else "relu"))
        np.savez_compressed(os.path.join(OUT, f"{name}.npz"), **out)
        print(name, "seed", seed, "StopIter", stop, "passes", len(out["pi_trace"]), "stopped", stopped,
              "bytes", os.path.getsize(os.path.join(OUT, f"{name}.npz")))


if __name__ == "__main__":
    main()
