#!/usr/bin/env python3
"""Generate tests/golden/ppo_log/*.npz by RUNNING THE REFERENCE's PPO agent inside its PSRS under the loop of its CartPole example and
recording what it hands to its EpochLogger.

Run from the repo root:   python tests/golden/make_golden_ppo_log.py
Needs /root/reference (read-only); nothing of it is copied -- the fixtures hold inputs, network weights and the values the reference
stored.  The stand-ins for gym / h5py / spinup and load_reference come from make_golden_ppo.py, which is left as it is.

The run: the example's loop (examples/cartpole/psrs_from_expert_heuristic.py:59-80) with steps_per_epoch = T and a step cap, three epochs
per seed, so the agent's ep_ret / ep_len cross two epoch cuts.  _on_epoch_end skips adapt() (the networks stay fixed; the buffer is
rewound as adapt()'s get() would) and keeps _log_epoch_metrics.  The logger is a recording EpochLogger: store() appends to epoch_dict,
which gives an empty list for a key never stored; dump_tabular snapshots EpRet / EpLen / VVals and the EpisodesInEpoch the agent logged,
then clears it.  The rejection draws are logged as in make_golden_ppo.py: every draw at least 1e-6 from its acceptance ratio.

Every fixture: inputs (obs, next_obs, z, a, r, z_next, done, p_log, t0), the networks (W*/b* of the actor and the critic, tanh), T, cap,
epochs, seeds; per seed s: rows, terminated, truncated, rew (f64, of the served rows), val (the stored VVals in step order), all [3 T];
per seed s and epoch j: EpRet (f64 list), EpLen (i64 list), VVals (f32 list), episodes (EpisodesInEpoch).
"""
import collections
import os
import sys

import numpy as np
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_ppo as G  # noqa: E402

OUT = os.path.join(G.ROOT, "tests", "golden", "ppo_log")
EPOCHS = 3


class RecordingLogger:
    """spinup's EpochLogger as far as the agent uses it: store() collects, dump_tabular() ends the epoch."""

    def __init__(self):
        self.epoch_dict = collections.defaultdict(list)
        self.epochs = []
        self._row = {}

    def store(self, **kw):
        for k, v in kw.items():
            self.epoch_dict[k].append(v)

    def log_tabular(self, key, val=None, **kw):
        if val is not None:
            self._row[key] = val

    def dump_tabular(self):
        d = self.epoch_dict
        self.epochs.append(dict(EpRet=list(d["EpRet"]), EpLen=list(d["EpLen"]), VVals=[np.float32(v) for v in d["VVals"]],
                                episodes=int(self._row["EpisodesInEpoch"])))
        self.epoch_dict = collections.defaultdict(list)
        self._row = {}

    def __getattr__(self, name):  # save_config, log, setup_pytorch_saver, save_state
        return lambda *a, **k: None


def run_reference(ppo, psrs, inp, seed, T, cap, hidden):
    N = len(inp["z"])
    p_rows = [np.array(inp["p_log"][i]) for i in range(N)]
    o_rows = [np.array(inp["obs"][i]) for i in range(N)]
    n_rows = [np.array(inp["next_obs"][i]) for i in range(N)]
    p2row = {id(p): i for i, p in enumerate(p_rows)}
    buf = [(o_rows[i], int(inp["a"][i]), float(inp["r"][i]), n_rows[i], bool(inp["done"][i]), p_rows[i],
            {"z": int(inp["z"][i]), "z_next": int(inp["z_next"][i]), "t": 0 if inp["t0"][i] else 1}) for i in range(N)]
    env = psrs.PSRS(buf, nS=int(max(inp["z"].max(), inp["z_next"].max())) + 1, nA=inp["p_log"].shape[1])
    env.reset_sampler(seed)

    margins, last_u = [], [0.0]
    rng = env.rejection_sampling_rng

    class LoggedRng:
        def random(self):
            last_u[0] = rng.random()
            return last_u[0]

    env.rejection_sampling_rng = LoggedRng()
    orig_reject = env._reject_func

    def reject(p_new, p_log, a):
        r = orig_reject(p_new, p_log, a)
        a = int(a)
        margins.append(abs(last_u[0] - p_new[a] / p_log[a] / (p_new / p_log).max()))
        return r

    env._reject_func = reject
    logger = RecordingLogger()

    class Agent(ppo.PPOAgentRevealed):
        def _on_epoch_end(self):  # no adapt(): the networks stay fixed; the buffer starts over as after adapt()'s get()
            self.buf.ptr, self.buf.path_start_idx = 0, 0
            self._log_epoch_metrics()
            self.epochs += 1
            self.steps = 0
            self.episodes = 0

    agent = Agent(G._Box(shape=(inp["obs"].shape[1],)), G._Discrete(inp["p_log"].shape[1]), ac_kwargs=dict(hidden_sizes=list(hidden)),
                  logger=logger, seed=0, steps_per_epoch=T)
    rows, term, trunc = [], [], []
    obs = env.reset()
    reward, steps_in_episode = None, 0
    while obs is not None and len(logger.epochs) < EPOCHS:  # examples/cartpole/psrs_from_expert_heuristic.py:59-80
        action_dist = agent.begin_episode(obs) if steps_in_episode == 0 else agent.step(reward, obs)
        if len(logger.epochs) == EPOCHS:
            break
        s_next, r, done, info = env.step(action_dist)
        if s_next is None:
            break
        agent.commit_action(info["a"])
        steps_in_episode += 1
        truncated = steps_in_episode >= cap
        rows.append(p2row[id(info["p"])])
        term.append(bool(done))
        trunc.append(bool(truncated))
        obs, reward = s_next, r
        if done or truncated:
            agent.end_episode(reward, truncated=truncated)
            obs = env.reset()
            steps_in_episode = 0
    if len(logger.epochs) < EPOCHS:  # the log ran dry first
        return None
    assert min(margins) >= 1e-6, f"seed {seed}: a rejection draw within {min(margins)} of its acceptance ratio"
    n = EPOCHS * T
    rows, term, trunc = (np.asarray(x[:n]) for x in (rows, term, trunc))
    net = {}
    for name, seq in (("pi", agent.ac.pi.logits_net), ("v", agent.ac.v.v_net)):
        for k, m in enumerate([m for m in seq if isinstance(m, nn.Linear)]):
            net[f"{name}_W{k}"] = m.weight.detach().numpy().copy()
            net[f"{name}_b{k}"] = m.bias.detach().numpy().copy()
    return rows, term, trunc, logger.epochs, net


def cover_of(term, trunc, epochs, T):
    """which of the log's rules one seed exercises"""
    end = term | trunc
    c = dict(term=int((term & ~trunc).sum()), trunc=int((trunc & ~term).sum()), span=0, no_ending=0, end_at_last=0)
    for j, ep in enumerate(epochs):
        sl = end[j * T:(j + 1) * T]
        c["end_at_last"] += int(sl[-1])
        if not sl.any():
            assert ep["episodes"] == 0 and len(ep["EpRet"]) == 1  # the open-episode entry
            c["no_ending"] += 1
        else:
            assert ep["episodes"] == len(ep["EpRet"]) == int(sl.sum())
        if j > 0 and not end[j * T - 1] and sl.any():  # the episode open at the cut ends in this epoch
            c["span"] += 1
        assert len(ep["VVals"]) == T
    return c


def fixture(ppo, psrs, name, inp, seeds, T, cap, hidden=(16, 16), want=None, n_max=None):
    out = dict(inp, T=np.int64(T), cap=np.int64(cap), epochs=np.int64(EPOCHS))
    total, used = collections.Counter(), []
    for s in seeds:
        got = run_reference(ppo, psrs, inp, int(s), T, cap, hidden)
        if got is None:
            continue
        rows, term, trunc, epochs, net = got
        c = cover_of(term, trunc, epochs, T)
        if want is not None and not want(c):
            continue
        used.append(int(s))
        total.update(c)
        out.update(net)  # the same networks for every seed (agent seed 0)
        rew = np.asarray(inp["r"], np.float64)[rows]
        assert np.array_equal(rew.astype(np.float32).astype(np.float64), rew), "a reward is not representable in f32"
        out[f"rows_{s}"], out[f"terminated_{s}"], out[f"truncated_{s}"], out[f"rew_{s}"] = rows, term, trunc, rew
        out[f"val_{s}"] = np.concatenate([np.asarray(ep["VVals"], np.float32) for ep in epochs])
        for j, ep in enumerate(epochs):
            out[f"EpRet_{s}_{j}"] = np.asarray(ep["EpRet"], np.float64)
            out[f"EpLen_{s}_{j}"] = np.asarray(ep["EpLen"], np.int64)
            out[f"VVals_{s}_{j}"] = np.asarray(ep["VVals"], np.float32)
            out[f"episodes_{s}_{j}"] = np.int64(ep["episodes"])
        if n_max is not None and len(used) == n_max:
            break
    assert len(used) >= 2, f"{name}: only {len(used)} seeds outlast {EPOCHS} epochs"
    out["seeds"] = np.asarray(used, np.int64)
    print(name, "seeds", used, dict(total))
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, f"{name}.npz"), **out)
    return total


def main():
    ppo, psrs = G.load_reference()
    synth = G._load("synth_", os.path.join(G.ROOT, "rl-offline-simulation_amd", "synth.py"))
    heur = G._load("heur_", os.path.join(G.REF, "offsim4rl/encoders/heuristic.py"))
    enc = heur.CartpoleBoxEncoder()
    cp = synth.cartpole_log(2000, seed=5)
    inp = dict(obs=cp["observations"], next_obs=cp["next_observations"], z=np.asarray(enc.encode(cp["observations"]), np.int64),
               z_next=np.asarray(enc.encode(cp["next_observations"]), np.int64), a=cp["actions"], r=cp["rewards"].astype(np.float64),
               done=cp["terminals"], p_log=cp["action_distributions"], t0=cp["steps"] == 0)
    total = collections.Counter()
    # a short epoch under the example's cap: epochs in which no episode ends, episodes that span the cuts, terminations
    total.update(fixture(ppo, psrs, "ppo_log_cartpole_T8_cap500", inp, range(40), 8, 500, want=lambda c: c["no_ending"] > 0 and c["span"] > 0, n_max=3))
    # a small cap: truncations, and (8, 16, 24 against cuts at 12, 24, 36) episodes that end on an epoch's last step
    total.update(fixture(ppo, psrs, "ppo_log_cartpole_T12_cap8", inp, range(40), 12, 8, want=lambda c: c["end_at_last"] > 0, n_max=3))
    for k in ("term", "trunc", "span", "no_ending", "end_at_last"):  # every rule of the log happens somewhere in the fixtures
        assert total[k] > 0, (k, dict(total))


if __name__ == "__main__":
    main()
