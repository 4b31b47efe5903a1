"""Replay of a logged memory through tabular TD learners: "Q-learning straight on the log", the baseline of every learning curve from
offline simulation.

qlearn(..., memory=memory) of the reference (offsim4rl/agents/tabular.py:90-104) sweeps the Q-learning update over logged
(S, A, R, S', done) tuples in log order; no simulator runs.  offsim_replay_td (csrc/replay_td.hpp) does that for L learners on S streams of
the log in one launch -- the transition stream is the same for every learner, so the learner is the lane of a wavefront and its Q sits in LDS.

  ReplayLog.from_arrays / from_table / from_memory     the log's five columns on the device
  qlearn_replay(memory, gamma, alpha, ...)             the drop-in for tabular.qlearn(env, ..., memory=memory)
  replay_orders(N, S, seed, kind)                      S permutations or bootstrap resamples of the log's rows, on the device
  TDPopulation.replay(log, orders, passes, ...)        -> TDReplayResult (td_population.py)
"""
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from .. import _lib as L
from .psrs import _schedule


class ReplayLog:
    """The columns of a logged memory on the device: s, a, s_next [N] int32, r [N] float64, done [N] uint8; states in [0, nS), actions in
    [0, nA) (a row outside stops a stream with OFFSIM_ST_KEYERROR where the reference raises IndexError)."""

    def __init__(self, s, a, r, s_next, done, nS, nA):
        self.s, self.a, self.r, self.s_next, self.done = s, a, r, s_next, done
        self.N, self.nS, self.nA = int(s.numel()), int(nS), int(nA)
        if not all(int(x.numel()) == self.N for x in (a, r, s_next, done)):
            raise ValueError("ReplayLog: columns of different lengths")
        if self.N < 1 or self.nS < 1 or self.nA < 1:
            raise ValueError("ReplayLog: an empty log, or nS / nA < 1")
        self.device = s.device
        self.c = L.ReplayLog(N=self.N, nS=self.nS, nA=self.nA, s=L.ptr(s), a=L.ptr(a), r=L.ptr(r), s_next=L.ptr(s_next), done=L.ptr(done))

    @classmethod
    def from_arrays(cls, s, a, r, s_next, done, nS, nA, device=None):
        """Arrays or tensors in log order.  Rewards are widened to float64 (exact for a float32 column, as float(R) is)."""
        device = device or L.require_device()

        def col(x, dt):
            x = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
            return x.reshape(-1).to(device=device, dtype=dt).contiguous()

        done = done if isinstance(done, torch.Tensor) else np.asarray(done)
        return cls(col(s, torch.int32), col(a, torch.int32), col(r, torch.float64), col(s_next, torch.int32), col(done != 0, torch.uint8), nS, nA)

    @classmethod
    def from_table(cls, table, nS=None):
        """The transitions of a TransitionTable, rows in the caller's order (not the table's grouped order), states by the caller's ids.
        nS (None): the largest id + 1."""
        ids = torch.from_numpy(table.slot_z).to(table.device)
        order = table.order.to(torch.int64)

        def back(x):
            out = torch.empty_like(x)
            out[order] = x
            return out

        s, s_next = ids[table._slot.to(torch.int64)], back(ids[table.z_next.to(torch.int64)])
        nS = int(table.slot_z.max()) + 1 if nS is None else nS
        return cls.from_arrays(s, back(table.a), back(table.r), s_next, back(table.done), nS, table.nA, device=table.device)

    @classmethod
    def from_memory(cls, memory, nS, nA, device=None):
        """A `memory` list: the reference's 5-tuples (S, A, R, S', done), or the 7-tuples (S, A, R, S', done, p, info) the drivers of this
        package return as info["memory"], of which the first five fields are read.  R goes through float(), as Python arithmetic widens it."""
        rows = [m[:5] for m in memory]
        s, a, sn = (np.array([int(m[i]) for m in rows], dtype=np.int64) for i in (0, 1, 3))
        for k, x in (("S", s), ("A", a), ("S'", sn)):
            if len(x) and (x.min() < -2 ** 31 or x.max() >= 2 ** 31):
                raise ValueError(f"ReplayLog.from_memory: {k} does not fit int32")
        r = np.array([float(m[2]) for m in rows], dtype=np.float64)
        done = np.array([bool(m[4]) for m in rows])
        return cls.from_arrays(s, a, r, sn, done, nS, nA, device=device)


def replay_orders(N, S, seed, kind="permutation", M=None, device=None):
    """orders [S, M] int32 on the device for TDPopulation.replay: kind "permutation" -- S independent shuffles of the N log rows (M = N) --
    or "bootstrap" -- S resamples of M rows (default N) drawn with replacement.  torch's device generator seeded with `seed`."""
    device = device or L.require_device()
    g = torch.Generator(device=device)
    g.manual_seed(int(seed))
    if kind == "permutation":
        if M not in (None, N):
            raise ValueError("replay_orders: a permutation has M = N")
        return torch.stack([torch.randperm(N, generator=g, device=device) for _ in range(S)]).to(torch.int32).contiguous()
    if kind == "bootstrap":
        return torch.randint(0, N, (S, N if M is None else int(M)), generator=g, device=device).to(torch.int32).contiguous()
    raise ValueError(f"replay_orders: kind must be 'permutation' or 'bootstrap', got {kind!r}")


def replay_lpw(nS, nA, n_learners):
    """Learners per wavefront of a launch (include/offsim.h: offsim_replay_lpw); 0: one learner's Q table does not fit LDS."""
    v = L.load().offsim_replay_lpw(nS, nA, n_learners)
    if v < 0:
        L.check(v)
    return int(v)


def replay_td(log, mode, alpha, gamma, q, orders=None, passes=1, alpha_ep=None, pi=None, td_cap=0, snap_stride=0, snap_cap=0):
    """One launch of offsim_replay_td.  alpha, gamma [L]; q [L, S, nS, nA] f64 on the device (Q_init; a copy is updated and returned);
    orders [S, M] int32 or None (S = 1, the log in log order); alpha_ep [L, n_sched] or None; pi [nS, nA] or [L, nS, nA] (expected SARSA).
    Returns a dict of device tensors: q [L, S, nS, nA], n_ep [S], steps, status [L, S], td_err [S, td_cap, L] with td_cap > 0 (learner-minor,
    as the kernel stores it), q_snap [L, S, snap_cap, nS, nA] with snap_cap > 0."""
    dev = log.device

    def f64(x):
        if x is None:
            return None
        x = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x, dtype=np.float64))
        return x.to(device=dev, dtype=torch.float64).contiguous()

    alpha, gamma, alpha_ep, pi = f64(alpha), f64(gamma), f64(alpha_ep), f64(pi)
    n_l = int(alpha.numel())
    if orders is None:
        S = 1
    else:
        if orders.dim() != 2 or orders.dtype != torch.int32 or orders.device != dev:
            raise ValueError("replay: orders must be an int32 [S, M] tensor on the log's device")
        orders, S = orders.contiguous(), int(orders.shape[0])
    if int(gamma.numel()) != n_l or (alpha_ep is not None and (alpha_ep.dim() != 2 or alpha_ep.shape[0] != n_l)):
        raise ValueError("replay: alpha, gamma [L] and alpha_ep [L, n_sched] disagree on L")
    if tuple(q.shape) != (n_l, S, log.nS, log.nA) or q.dtype != torch.float64:
        raise ValueError(f"replay: q [L, S, nS, nA] = {(n_l, S, log.nS, log.nA)} float64 expected, got {tuple(q.shape)} {q.dtype}")
    if pi is not None and tuple(pi.shape) not in ((log.nS, log.nA), (n_l, log.nS, log.nA)):
        raise ValueError(f"replay: pi [nS, nA] or [L, nS, nA] expected, got {tuple(pi.shape)}")
    q = q.to(dev).contiguous().clone()
    out = dict(q=q, n_ep=torch.zeros(S, dtype=torch.int64, device=dev), steps=torch.zeros((n_l, S), dtype=torch.int64, device=dev),
               status=torch.zeros((n_l, S), dtype=torch.int32, device=dev))
    if td_cap > 0:
        out["td_err"] = torch.zeros((S, int(td_cap), n_l), dtype=torch.float64, device=dev)
    if snap_cap > 0:
        out["q_snap"] = torch.zeros((n_l, S, int(snap_cap), log.nS, log.nA), dtype=torch.float64, device=dev)
    rp = L.Replay(mode=mode, order=L.ptr(orders), M=0 if orders is None else int(orders.shape[1]), passes=int(passes), alpha=L.ptr(alpha),
                  gamma=L.ptr(gamma), alpha_ep=L.ptr(alpha_ep), n_sched=0 if alpha_ep is None else int(alpha_ep.shape[1]), pi=L.ptr(pi),
                  pi_stride=log.nS * log.nA if pi is not None and pi.dim() == 3 else 0, q=L.ptr(q), td_err=L.ptr(out.get("td_err")),
                  td_cap=int(td_cap), q_snap=L.ptr(out.get("q_snap")), snap_cap=int(snap_cap), snap_stride=int(snap_stride),
                  n_ep=L.ptr(out["n_ep"]), steps=L.ptr(out["steps"]), status=L.ptr(out["status"]))
    with torch.cuda.device(dev):
        L.check(L.load().offsim_replay_td(log.c, n_l, S, rp, L.stream_ptr()))
    return out


@dataclass
class TDReplayResult:
    """What TDPopulation.replay returns; device tensors.  Q [L,S,nS,nA]; td_err [L,S,td_cap] (a permuted view of the kernel's learner-minor
    [S,td_cap,L]; None without td_cap); q_snap [L,S,snap_cap,nS,nA] or None; n_ep [S], the done flags each stream saw; steps, status [L,S]
    (OFFSIM_ST_KEYERROR: the stream stopped before step `steps` on a row outside the tables); M and passes of the run."""
    Q: torch.Tensor
    n_ep: torch.Tensor
    steps: torch.Tensor
    status: torch.Tensor
    M: int
    passes: int
    td_err: Optional[torch.Tensor] = None
    q_snap: Optional[torch.Tensor] = None
    learners: list = field(default_factory=list)

    def last_sweep_mse(self):
        """[L, S] mean squared TD error over the steps of the last sweep that the trace holds and the run reached; NaN where there is none."""
        if self.td_err is None:
            raise ValueError("TDReplayResult: the run kept no TD errors (td_cap = 0)")
        k = torch.arange(self.td_err.shape[2], device=self.td_err.device)
        m = (k >= (self.passes - 1) * self.M)[None, None, :] & (k[None, None, :] < self.steps[:, :, None])
        n = m.sum(dim=2)
        sq = torch.where(m, self.td_err * self.td_err, torch.zeros((), dtype=torch.float64, device=k.device)).sum(dim=2)
        return torch.where(n > 0, sq / n.clamp(min=1), torch.full((), float("nan"), dtype=torch.float64, device=k.device))

    def best(self):
        """The learner with the lowest mean squared TD error of the last sweep, averaged over the streams; learners with a stream that has no
        such step (or a NaN) are never the best; -1 when there is none."""
        score = self.last_sweep_mse().mean(dim=1).cpu().numpy()
        return -1 if not np.isfinite(score).any() else int(np.nanargmin(np.where(np.isfinite(score), score, np.inf)))


def qlearn_replay(memory, gamma, alpha=0.1, Q_init=None, save_Q=0, nS=None, nA=None):
    """tabular.qlearn(env, ..., memory=memory) (offsim4rl/agents/tabular.py:90-104) in one launch: returns Q, {"Qs", "TD_errors", "memory"}
    with the reference's shapes -- Qs is [1 + steps, nS, nA] with save_Q, else [1, nS, nA].  alpha may be a callable of the episode (the number
    of done flags seen so far).  nS, nA: Q's shape, read from Q_init when it is given (the reference takes them from env).  A tuple outside
    the table raises IndexError, as the reference does (a negative index too: NumPy's wrap-around is not replayed)."""
    if Q_init is not None:
        Q0 = np.asarray(Q_init).copy().astype(float)
        nS, nA = Q0.shape
    elif nS is None or nA is None:
        raise ValueError("qlearn_replay: nS and nA, or Q_init")
    else:
        Q0 = np.zeros((nS, nA))
    if len(memory) == 0:
        return Q0, {"Qs": np.array([Q0]), "TD_errors": np.array([]), "memory": memory}
    log = memory if isinstance(memory, ReplayLog) else ReplayLog.from_memory(memory, nS, nA)
    n_ep = int(log.done.sum().item())
    a_tab = _schedule(alpha, n_ep + 1)
    o = replay_td(log, L.TD_QLEARN, [0.0 if callable(alpha) else float(alpha)], [float(gamma)], torch.from_numpy(Q0)[None, None].to(log.device),
                  alpha_ep=None if a_tab is None else a_tab[None], td_cap=log.N, snap_stride=1, snap_cap=log.N if save_Q else 0)
    if int(o["status"].cpu()[0, 0]) != L.ST_OK:
        raise IndexError(f"qlearn_replay: tuple {int(o['steps'].cpu()[0, 0])} of the memory is outside Q [{nS}, {nA}]")
    Qs = np.array([Q0]) if not save_Q else np.concatenate([Q0[None], o["q_snap"].cpu().numpy()[0, 0]], axis=0)
    return o["q"].cpu().numpy()[0, 0], {"Qs": Qs, "TD_errors": o["td_err"].cpu().numpy()[0, :, 0].copy(), "memory": memory}
