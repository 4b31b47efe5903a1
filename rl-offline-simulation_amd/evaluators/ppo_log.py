"""The epoch log of the reference's PPO agent on the device: EpRet / EpLen / EpisodesInEpoch / VVals per epoch, for one learner or L.

What PPOAgentRevealed stores in its EpochLogger while it runs (offsim4rl/agents/ppo.py:103-160) and what _log_epoch_metrics prints of it
(:225-235), computed from the [T, E] records VectorPSRS.collect_ppo / collect_ppo_population leave on the device, in ONE launch per epoch
(offsim_ppo_epoch_log, csrc/ppo_log.hpp) and with no host read: the running return and length of every environment's open episode live
in an EpisodeTracker and carry across epochs as self.ep_ret / self.ep_len do.  E environments stand for E MPI processes, so an
environment in which no episode ended contributes its open episode, as each process would (ppo.py:226-227).
"""
from collections import namedtuple

import torch

from .. import _lib as L

_EPLEN = {"reference": L.EPLEN_REFERENCE, "steps": L.EPLEN_STEPS}

_LOG_KEYS = "EpRet StdEpRet MaxEpRet MinEpRet EpLen EpisodesInEpoch VVals StdVVals MaxVVals MinVVals Entries StepsServed"
_UPDATE_KEYS = "LossPi LossV KL Entropy ClipFrac DeltaLossPi DeltaLossV StopIter"  # PPOUpdateInfo's


class PPOEpochLog(namedtuple("PPOEpochLog", _LOG_KEYS)):
    """One epoch's log, named as the reference's log keys; 0-dim device tensors, or [L] for a population.  EpRet / StdEpRet / MaxEpRet /
    MinEpRet and EpLen (mean) are over the epoch's entries -- the episodes that ended, plus the open episode of every environment in
    which none ended; VVals / StdVVals / MaxVVals / MinVVals over the critic's value at every served step (all f64; NaN where there is
    nothing to average).  EpisodesInEpoch counts ended episodes only, Entries the entries, StepsServed the served steps (i64)."""


PPOEpisodes = namedtuple("PPOEpisodes", "ep_ret ep_len n_ep open open_ret open_len")
PPOEpisodes.__doc__ = """The raw lists behind a PPOEpochLog, per environment: ep_ret [R, ep_cap] f64 / ep_len [R, ep_cap] i32 of the first
ep_cap ended episodes in order, n_ep [R] i32 their number, open [R] bool where the environment's entry is its open episode instead (a
served step, no ending), and open_ret / open_len [R]: the carry after the epoch -- that entry's values where open."""

PPOTrainLog = namedtuple("PPOTrainLog", _LOG_KEYS + " " + _UPDATE_KEYS + " TotalEnvInteracts")
PPOTrainLog.__doc__ = """The curves of PPOLearner.fit ([epochs] device tensors) / PPOPopulation.fit ([epochs, L]): every field of PPOEpochLog
and of PPOUpdateInfo per epoch, and TotalEnvInteracts = (epoch + 1) * T * E as the reference logs it (the nominal count: StepsServed is
what the log actually gave)."""


class EpisodeTracker:
    """The carry of ppo_epoch_log: open_ret [num_envs] f64 and open_len [num_envs] i32, the return and the number of transitions of every
    environment's open episode (the agent's ep_ret / ep_len).  It belongs to the caller, lives on `device` and is updated in place."""

    def __init__(self, num_envs, device):
        self.num_envs = int(num_envs)
        if self.num_envs < 1:
            raise ValueError(f"EpisodeTracker: num_envs must be >= 1, got {num_envs}")
        self.open_ret = torch.zeros(self.num_envs, dtype=torch.float64, device=device)
        self.open_len = torch.zeros(self.num_envs, dtype=torch.int32, device=device)

    def reset(self, mask=None):
        """Forget the open episode of the environments in `mask` ([num_envs] bool; all if None): begin_episode's ep_ret = ep_len = 0."""
        if mask is None:
            self.open_ret.zero_()
            self.open_len.zero_()
        else:
            m = torch.as_tensor(mask, device=self.open_ret.device).to(torch.bool)
            self.open_ret.masked_fill_(m, 0.0)
            self.open_len.masked_fill_(m, 0)


def _epoch_log(rew, val, valid, terminated, truncated, tracker, nl, ep_len, episodes, squeeze, ep_cap=None):
    if ep_len not in _EPLEN:
        raise ValueError(f"ppo_epoch_log: ep_len must be 'reference' or 'steps', got {ep_len!r}")
    if not isinstance(tracker, EpisodeTracker):
        raise TypeError(f"ppo_epoch_log: tracker must be an EpisodeTracker, got {type(tracker).__name__}")
    if rew.device.type != "cuda":
        raise ValueError("ppo_epoch_log: the records must be device tensors")
    if rew.dim() != 2:
        raise ValueError(f"ppo_epoch_log: rew must be [T, R], got shape {tuple(rew.shape)}")
    T, R = int(rew.shape[0]), int(rew.shape[1])
    nl = int(nl)
    if T < 1 or R < 1:
        raise ValueError(f"ppo_epoch_log: needs at least one step of one environment, got records of shape {(T, R)}")
    if nl < 1 or R % nl:
        raise ValueError(f"ppo_epoch_log: {R} environments do not divide among {nl} learners")
    if tracker.num_envs != R or tracker.open_ret.device != rew.device:
        raise ValueError(f"ppo_epoch_log: the tracker holds {tracker.num_envs} environments on {tracker.open_ret.device}, the records {R} on {rew.device}")
    dev = rew.device

    def rec(x, dtype, name):
        if tuple(x.shape) != (T, R) or x.dtype != dtype or x.device != dev:
            raise ValueError(f"ppo_epoch_log: {name} must be a [{T}, {R}] {dtype} tensor on {dev}, got {tuple(x.shape)} {x.dtype} on {x.device}")
        return x.contiguous()

    rew, val = rec(rew, torch.float32, "rew"), rec(val, torch.float32, "val")
    valid, terminated, truncated = (rec(x, torch.bool, n) for x, n in ((valid, "valid"), (terminated, "terminated"), (truncated, "truncated")))
    stats = torch.empty((nl, L.PPO_LOG_STATS), dtype=torch.float64, device=dev)
    counts = torch.empty((nl, 2), dtype=torch.int64, device=dev)
    ep_r = ep_l = n_ep = None
    cap = 0
    if episodes:
        cap = T if ep_cap is None else int(ep_cap)
        ep_r = torch.zeros((R, cap), dtype=torch.float64, device=dev)
        ep_l = torch.zeros((R, cap), dtype=torch.int32, device=dev)
        n_ep = torch.zeros(R, dtype=torch.int32, device=dev)
    L.check(L.load().offsim_ppo_epoch_log_pop(L.ptr(rew), L.ptr(val), L.ptr(valid), L.ptr(terminated), L.ptr(truncated), T, nl, R // nl,
                                              _EPLEN[ep_len], L.ptr(tracker.open_ret), L.ptr(tracker.open_len), L.ptr(stats), L.ptr(counts),
                                              L.ptr(ep_r) if cap else None, L.ptr(ep_l) if cap else None, L.ptr(n_ep), cap, L.stream_ptr()))
    s, c = (stats[0], counts[0]) if squeeze else (stats.t(), counts.t())
    log = PPOEpochLog(EpRet=s[0], StdEpRet=s[1], MaxEpRet=s[3], MinEpRet=s[2], EpLen=s[4], EpisodesInEpoch=c[0], VVals=s[5], StdVVals=s[6],
                      MaxVVals=s[8], MinVVals=s[7], Entries=s[9].to(torch.int64), StepsServed=c[1])
    if not episodes:
        return log
    return log, PPOEpisodes(ep_ret=ep_r, ep_len=ep_l, n_ep=n_ep, open=(n_ep == 0) & valid.any(dim=0), open_ret=tracker.open_ret.clone(),
                            open_len=tracker.open_len.clone())


def ppo_epoch_log_records(rew, val, valid, terminated, truncated, tracker, learners=1, ep_len="reference", episodes=False, ep_cap=None):
    """ppo_epoch_log on step-major [T, R] device records of any driver: rew / val f32, valid / terminated / truncated bool (an episode
    ends at a valid step with terminated | truncated).  ep_cap: how many ended episodes per environment the raw lists keep (default T)."""
    return _epoch_log(rew, val, valid, terminated, truncated, tracker, learners, ep_len, episodes, int(learners) == 1, ep_cap)


def ppo_epoch_log(batch, tracker, learners=1, ep_len="reference", episodes=False):
    """The reference's epoch log of one PPOBatch (VectorPSRS.collect_ppo, or collect_ppo_population with learners = L: environment r
    belongs to learner r // E), in one launch and with no host read; `tracker` (an EpisodeTracker over the batch's environments) carries
    every open episode into the next call.  Read in place, no flat() and no copy: rew, val, valid and collected.terminated / truncated.

    ep_len: "reference" -- an ended episode's EpLen is the number of its transitions minus one, as the agent counts it (end_episode
    does not increment ep_len, step does) -- or "steps", the number of its transitions.  The open episode of an environment in which
    none ended is logged with its transition count so far under either rule, as the agent does.

    Returns a PPOEpochLog of 0-dim device tensors (learners = 1) or [L] tensors; learner l's numbers are bit for bit those of the
    single call on its own columns.  episodes=True: (PPOEpochLog, PPOEpisodes), the raw per-environment lists."""
    c = batch.collected
    return _epoch_log(batch.rew, batch.val, batch.valid, c.terminated, c.truncated, tracker, learners, ep_len, episodes, int(learners) == 1)


def _fit(collect, update, tracker, epochs, T, E, squeeze, nl):
    """The loop of PPOLearner.fit / PPOPopulation.fit: collect, log, update per epoch, everything enqueued; the stacked curves."""
    epochs = int(epochs)
    if epochs < 1:
        raise ValueError(f"fit: epochs must be >= 1, got {epochs}")
    logs, infos = [], []
    for _ in range(epochs):
        b = collect()
        logs.append(_epoch_log(b.rew, b.val, b.valid, b.collected.terminated, b.collected.truncated, tracker, nl, "reference", False, squeeze))
        infos.append(update(b))
    cols = [torch.stack([getattr(x, k) for x in logs]) for k in PPOEpochLog._fields]
    cols += [torch.stack([getattr(x, k) for x in infos]) for k in _UPDATE_KEYS.split()]
    total = torch.arange(1, epochs + 1, dtype=torch.int64, device=tracker.open_ret.device) * (int(T) * int(E))
    return PPOTrainLog(*cols, total if squeeze else total[:, None].expand(epochs, nl).contiguous())


__all__ = ["EpisodeTracker", "PPOEpochLog", "PPOEpisodes", "PPOTrainLog", "ppo_epoch_log", "ppo_epoch_log_records"]
