"""The PPO update on the device: PPOAgentRevealed.adapt (offsim4rl/agents/ppo.py:162-223) over the buffer VectorPSRS.collect_ppo returns.

Up to train_pi_iters Adam steps on the clipped surrogate with the KL early stop, then train_v_iters steps on the value loss, as the HIP
kernels of offsim_ppo_update (csrc/ppo_update.hpp): every pass is one fused forward / loss / backward launch and one reduce-and-Adam
launch, all of them enqueued at once -- the early stop is a flag on the device, nothing synchronises with the host.  The learner updates
the device weights the actor and the critic hand to collect_ppo in place, so the next collect_ppo(actor, critic, T) runs the new networks
with no copy; MLPPolicy / MLPValue.refresh_host / to_torch / state_dict bring the host copy up to date on demand.
"""
import ctypes as C
from collections import namedtuple

import torch

from .. import _lib as L
from .obs_policy import _ACT, MLPPolicy, MLPValue

PPOUpdateInfo = namedtuple("PPOUpdateInfo", "LossPi LossV KL Entropy ClipFrac DeltaLossPi DeltaLossV StopIter")
PPOGrad = namedtuple("PPOGrad", "grad n loss kl entropy clipfrac")
_KIND = {"actor": L.PPO_ACTOR, "critic": L.PPO_CRITIC}


def _net_struct(net, device):
    ws, arr = net._device_weights(device)
    s = L.PPONet(n_layers=len(ws), activation=_ACT[net.activation], layers_host=C.cast(arr, C.POINTER(L.MLPLayer)), slope=net.slope)
    return s, ws


def num_params(net):
    return sum(int(W.numel()) + (0 if b is None else int(b.numel())) for W, b in net.weights)


def _batch_struct(net, batch, kind):
    """offsim_ppo_batch over a PPOBatch ([T, E] records with valid, as they are) or a dict of flat tensors (obs, act, adv, logp, ret and
    optionally valid); returns (struct, device, tensors to keep alive)."""
    get = (lambda k: batch.get(k)) if isinstance(batch, dict) else (lambda k: getattr(batch, k, None))
    obs = get("obs")
    if obs is None or obs.device.type != "cuda":
        raise ValueError("ppo: the batch must hold device tensors")
    dev = obs.device
    if obs.dtype not in (torch.float32, torch.float16):
        obs = obs.to(torch.float32)
    obs = obs.contiguous()
    valid = get("valid")
    lead = tuple(valid.shape) if valid is not None else tuple(obs.shape[:-1])
    M = 1
    for d in lead:
        M *= int(d)
    if obs.numel() != M * net.dO:
        raise ValueError(f"ppo: observations of width {net.dO} expected, got shape {tuple(obs.shape)} for {M} records")
    keep = [obs]

    def col(name, dtype):
        x = get(name)
        if x is None:
            raise ValueError(f"ppo: the batch has no {name!r}")
        if x.numel() != M:
            raise ValueError(f"ppo: {name} must hold {M} entries, got shape {tuple(x.shape)}")
        x = x.to(device=dev, dtype=dtype).contiguous()
        keep.append(x)
        return L.ptr(x) if M else None

    b = L.PPOBatchC(obs=L.ptr(obs) if M else None, x_dtype=L.F32 if obs.dtype == torch.float32 else L.F16, dO=net.dO, M=M)
    if kind == L.PPO_ACTOR:
        b.act, b.adv, b.logp = col("act", torch.int32), col("adv", torch.float32), col("logp", torch.float32)
    else:
        b.ret = col("ret", torch.float32)
    if valid is not None:
        b.valid = col("valid", torch.uint8)
    return b, dev, keep


def ppo_grad(net, batch, kind, clip_ratio=0.2):
    """One forward / loss / backward pass (offsim_ppo_grad): PPOGrad(grad [P] f32 flat in layer order, W then b per layer; n, loss, kl,
    entropy, clipfrac as 0-dim f64 device tensors).  net: MLPPolicy (kind 'actor') or MLPValue ('critic'); batch: a PPOBatch (its [T, E]
    records and valid as they are) or a dict of flat device tensors obs / act / adv / logp / ret (/ valid)."""
    if kind not in _KIND:
        raise ValueError(f"ppo_grad: kind must be 'actor' or 'critic', got {kind!r}")
    b, dev, keep = _batch_struct(net, batch, _KIND[kind])
    s, ws = _net_struct(net, dev)
    P = num_params(net)
    grad = torch.zeros(P, dtype=torch.float32, device=dev)
    stats = torch.zeros(5, dtype=torch.float64, device=dev)
    work = torch.empty(L.ppo_update_work_doubles(P), dtype=torch.float64, device=dev)
    L.check(L.load().offsim_ppo_grad(C.byref(s), _KIND[kind], C.byref(b), float(clip_ratio), L.ptr(grad), L.ptr(stats), L.ptr(work), L.stream_ptr()))
    return PPOGrad(grad, *(stats[i] for i in range(5)))


class _Adam:
    """torch.optim.Adam's state for one network, on the device: m, v [P] f32, t [1] i64."""

    def __init__(self, net, lr, device):
        P = num_params(net)
        self.lr = float(lr)
        self.m = torch.zeros(P, dtype=torch.float32, device=device)
        self.v = torch.zeros(P, dtype=torch.float32, device=device)
        self.t = torch.zeros(1, dtype=torch.int64, device=device)
        self.work = torch.empty(L.ppo_update_work_doubles(P), dtype=torch.float64, device=device)

    def struct(self):
        return L.PPOAdam(m=L.ptr(self.m), v=L.ptr(self.v), t=L.ptr(self.t), lr=self.lr)


class PPOLearner:
    """adapt() of the reference's PPO agent for an MLPPolicy actor and an MLPValue critic, on the device.  The defaults are the agent's.
    The Adam states (m, v, t) persist across update() calls, as the agent's optimisers do.  One device: after update() the networks'
    host copy (net.weights) is stale until refresh_host() / to_torch() / state_dict(), and a copy made for another device before that
    would be made from the stale one."""

    def __init__(self, actor, critic, pi_lr=3e-4, vf_lr=1e-3, clip_ratio=0.2, train_pi_iters=80, train_v_iters=80, target_kl=0.01):
        if not isinstance(actor, MLPPolicy) or not isinstance(critic, MLPValue):
            raise TypeError("PPOLearner: actor must be an MLPPolicy and critic an MLPValue")
        if actor.dO != critic.dO:
            raise ValueError("PPOLearner: the actor and the critic read observations of different widths")
        if not 0.0 <= clip_ratio < 1.0 or target_kl < 0 or train_pi_iters < 0 or train_v_iters < 0 or pi_lr < 0 or vf_lr < 0:
            raise ValueError("PPOLearner: clip_ratio in [0, 1), target_kl, the learning rates and the iteration counts >= 0")
        self.actor, self.critic = actor, critic
        self.pi_lr, self.vf_lr, self.clip_ratio, self.target_kl = float(pi_lr), float(vf_lr), float(clip_ratio), float(target_kl)
        self.train_pi_iters, self.train_v_iters = int(train_pi_iters), int(train_v_iters)
        self._opt = {}

    def _state(self, device):
        key = str(device)
        if key not in self._opt:
            self._opt[key] = (_Adam(self.actor, self.pi_lr, device), _Adam(self.critic, self.vf_lr, device))
        return self._opt[key]

    def _run(self, net, kind, batch, iters, opt):
        b, dev, keep = _batch_struct(net, batch, kind)
        s, ws = _net_struct(net, dev)
        stats = torch.zeros(6, dtype=torch.float64, device=dev)
        trace = torch.full((max(iters, 0), 2), float("nan"), dtype=torch.float64, device=dev)
        a = opt.struct()
        L.check(L.load().offsim_ppo_update(C.byref(s), kind, C.byref(b), self.clip_ratio, self.target_kl, iters, C.byref(a), L.ptr(stats),
                                           L.ptr(trace) if iters else None, L.ptr(opt.work), L.stream_ptr()))
        return stats, trace

    def update(self, batch):
        """One adapt(): the actor's loop, then the critic's, on the batch's [T, E] records and valid as they are (or a dict of flat device
        tensors).  Returns PPOUpdateInfo of 0-dim device tensors named as the reference logs them; `.pi_trace` / `.v_trace` of the learner
        hold the (loss, kl) of every pass of the last call ([iters, 2] f64, NaN after a stop).  Nothing here synchronises with the host."""
        obs = batch["obs"] if isinstance(batch, dict) else batch.obs
        pi_opt, v_opt = self._state(obs.device)
        ps, self.pi_trace = self._run(self.actor, L.PPO_ACTOR, batch, self.train_pi_iters, pi_opt)
        vs, self.v_trace = self._run(self.critic, L.PPO_CRITIC, batch, self.train_v_iters, v_opt)
        return PPOUpdateInfo(LossPi=ps[0], LossV=vs[0], KL=ps[2], Entropy=ps[3], ClipFrac=ps[4], DeltaLossPi=ps[1] - ps[0],
                             DeltaLossV=vs[1] - vs[0], StopIter=ps[5].to(torch.int64))

    def fit(self, env, epochs, T, tracker=None, **collect_kwargs):
        """The training loop of the reference's example (examples/cartpole/psrs_from_expert_heuristic.py) inside the VectorPSRS `env`:
        per epoch env.collect_ppo(actor, critic, T, **collect_kwargs), ppo_epoch_log of the batch, update(batch) -- nothing more, all
        of it enqueued, nothing read back between epochs.  tracker: the EpisodeTracker that carries the open episodes (a fresh one if
        None; pass your own to go on from an earlier fit).  Returns a PPOTrainLog of [epochs] device tensors.  An epoch in which the
        log ran dry shows in StepsServed and as NaN rows; fit does not stop or synchronise for it."""
        from .ppo_log import EpisodeTracker, _fit
        if tracker is None:
            tracker = EpisodeTracker(env.num_envs, env.table.device)
        return _fit(lambda: env.collect_ppo(self.actor, self.critic, T, **collect_kwargs), self.update, tracker, epochs, T, env.num_envs, True, 1)

    def adam_state(self, device=None):
        """((m, v, t) of the actor, (m, v, t) of the critic): the device tensors of the optimiser states."""
        key = str(device) if device is not None else next(iter(self._opt))
        a, c = self._opt[key]
        return (a.m, a.v, a.t), (c.m, c.v, c.t)


__all__ = ["PPOLearner", "PPOUpdateInfo", "PPOGrad", "ppo_grad"]
