"""A population of independent PPO learners on the device: L seeds or hyperparameter settings of one agent per launch.

One learner cannot fill the device at the reference agent's sizes (DESIGN sections 13 and 15), and a learning curve wants many seeds, so
the learner is a grid dimension of the kernels PPOLearner uses: VectorPSRS.collect_ppo_population runs L * E environments, learner-major,
each with its learner's actor and critic (offsim_vector_collect_ppo_pop) and normalises the advantages per learner
(offsim_ppo_advantages_pop); PPOPopulation.update runs every learner's adapt() -- its own weights, Adam state, stop flag and
hyperparameters -- in the launches one learner takes (offsim_ppo_update_pop).  Learners never interact: learner l's numbers are, bit for
bit, those of a PPOLearner on its own E environments.

The population owns the stacked device weights (per layer W [L, out, in], b [L, out]) and updates them in place, so the next
collect_ppo_population stages the new networks with no copy; actor(l) / critic(l) / state_dict(l) / to_torch(l) export one learner.
"""
import ctypes as C

import torch

from .. import _lib as L
from .obs_policy import _ACT, MLPPolicy, MLPValue
from .ppo_learner import PPOGrad, PPOUpdateInfo, _batch_struct

_KIND = {"actor": L.PPO_ACTOR, "critic": L.PPO_CRITIC}


def _per_learner(x, n, name):
    """a scalar or a length-n sequence -> a list of n floats"""
    try:
        xs = [float(v) for v in x]
    except TypeError:
        return [float(x)] * n
    if len(xs) != n:
        raise ValueError(f"PPOPopulation: {name} must be a scalar or a sequence of {n} values, got {len(xs)}")
    return xs


class _Stack:
    """L networks of one architecture, stacked: the host copies until a device is known, then per layer W [L, out, in], b [L, out] there,
    with the optimiser state m, v [L, P], t [L] and the offsim_mlp_layer array that describes learner 0."""

    def __init__(self, nets, cls, lr):
        self.cls, self.n = cls, len(nets)
        for net in nets:
            if not isinstance(net, cls):
                raise ValueError(f"PPOPopulation: every network of this list must be an {cls.__name__}, got {type(net).__name__}")
        first = nets[0]
        self.activation, self.slope, self.dO, self.nA = first.activation, first.slope, first.dO, first.nA
        shape = [(tuple(W.shape), b is not None) for W, b in first.weights]
        for net in nets:
            if [(tuple(W.shape), b is not None) for W, b in net.weights] != shape or (net.activation, net.slope) != (self.activation, self.slope):
                raise ValueError("PPOPopulation: all learners share one architecture (layer shapes, biases, activation, slope)")
        self.host = [(torch.stack([net.weights[i][0] for net in nets]), torch.stack([net.weights[i][1] for net in nets]) if has_b else None)
                     for i, (_, has_b) in enumerate(shape)]
        self.P = sum(W[0].numel() + (0 if b is None else b[0].numel()) for W, b in self.host)
        self.lr = lr
        self.device = None

    def on(self, device):
        if self.device is None:
            self.device = torch.device(device)
            self.ws = [(W.to(device).contiguous(), None if b is None else b.to(device).contiguous()) for W, b in self.host]
            self.arr = (L.MLPLayer * len(self.ws))()
            for i, (W, b) in enumerate(self.ws):
                self.arr[i].W, self.arr[i].b = L.ptr(W), L.ptr(b)
                setattr(self.arr[i], "in", int(W.shape[2]))
                self.arr[i].out = int(W.shape[1])
            self.m = torch.zeros((self.n, self.P), dtype=torch.float32, device=device)
            self.v = torch.zeros((self.n, self.P), dtype=torch.float32, device=device)
            self.t = torch.zeros(self.n, dtype=torch.int64, device=device)
            self.work, self.lr_c = None, (C.c_double * self.n)(*self.lr)
        elif self.device != torch.device(device):
            raise ValueError(f"PPOPopulation: the population lives on {self.device}, not on {device}")
        return self

    def _device_weights(self, device):
        """(tensors, offsim_mlp_layer array of learner 0) as _MLPNet._device_weights gives them: what VectorPSRS stages a network from"""
        self.on(device)
        return self.ws, self.arr

    def net_struct(self):
        return L.PPONet(n_layers=len(self.ws), activation=_ACT[self.activation], layers_host=C.cast(self.arr, C.POINTER(L.MLPLayer)), slope=self.slope)

    def scratch(self, M):
        """device scratch for M records per learner (offsim_ppo_update_work_doubles_pop), kept between calls"""
        s = self.net_struct()
        n = L.load().offsim_ppo_update_work_doubles_pop(C.byref(s), self.n, M)
        if n < 0:
            L.check(n)
        if self.work is None or self.work.numel() < n:
            self.work = torch.empty(n, dtype=torch.float64, device=self.device)
        return self.work

    def export(self, l):
        """learner l's current weights as a network of its class (host copies; synchronises once a device copy exists)"""
        if not 0 <= l < self.n:
            raise IndexError(f"PPOPopulation: learner {l} of {self.n}")
        src = self.host if self.device is None else self.ws
        return self.cls([(W[l].detach().cpu().clone(), None if b is None else b[l].detach().cpu().clone()) for W, b in src], self.activation, self.slope)


def _records(pop, batch):
    """(T, E) of a [T, L * E, ...] batch for the population"""
    obs = batch["obs"] if isinstance(batch, dict) else batch.obs
    if obs.dim() < 3:
        raise ValueError(f"PPOPopulation: the batch must be step-major [T, L * E, ...], got observations of shape {tuple(obs.shape)}")
    T, R = int(obs.shape[0]), int(obs.shape[1])
    if R % pop.L or R == 0:
        raise ValueError(f"PPOPopulation: {R} environments do not divide among {pop.L} learners")
    return T, R // pop.L


class PPOPopulation:
    """L independent PPOLearner's of one architecture, run together.  actors / critics: lists of L MLPPolicy / MLPValue; pi_lr, vf_lr,
    clip_ratio and target_kl: a scalar or one value per learner; the iteration counts are shared.  The defaults are the reference
    agent's.  The Adam states persist across update() calls.  One device: the one the first batch (or collect) lives on."""

    def __init__(self, actors, critics, pi_lr=3e-4, vf_lr=1e-3, clip_ratio=0.2, train_pi_iters=80, train_v_iters=80, target_kl=0.01):
        actors, critics = list(actors), list(critics)
        if not actors or len(actors) != len(critics):
            raise ValueError("PPOPopulation: actors and critics must be two lists of the same, non-zero length")
        self.L = n = len(actors)
        self.pi_lr, self.vf_lr = _per_learner(pi_lr, n, "pi_lr"), _per_learner(vf_lr, n, "vf_lr")
        self.clip_ratio, self.target_kl = _per_learner(clip_ratio, n, "clip_ratio"), _per_learner(target_kl, n, "target_kl")
        if not all(0.0 <= c < 1.0 for c in self.clip_ratio) or min(self.target_kl + self.pi_lr + self.vf_lr) < 0 or train_pi_iters < 0 or train_v_iters < 0:
            raise ValueError("PPOPopulation: clip_ratio in [0, 1), target_kl, the learning rates and the iteration counts >= 0")
        self._pi, self._v = _Stack(actors, MLPPolicy, self.pi_lr), _Stack(critics, MLPValue, self.vf_lr)
        if self._pi.dO != self._v.dO:
            raise ValueError("PPOPopulation: the actors and the critics read observations of different widths")
        self.train_pi_iters, self.train_v_iters = int(train_pi_iters), int(train_v_iters)
        self._clip_c, self._kl_c = (C.c_double * n)(*self.clip_ratio), (C.c_double * n)(*self.target_kl)
        self.pi_trace = self.v_trace = None

    # ---- the device side ----
    def _stacks(self, device):
        return self._pi.on(device), self._v.on(device)

    def _run(self, st, kind, batch, T, E, iters):
        b, dev, keep = _batch_struct(st, batch, kind)
        st.on(dev)
        s = st.net_struct()
        stats = torch.zeros((self.L, 6), dtype=torch.float64, device=dev)
        trace = torch.full((self.L, max(iters, 0), 2), float("nan"), dtype=torch.float64, device=dev)
        opt = L.PPOAdamPop(m=L.ptr(st.m), v=L.ptr(st.v), t=L.ptr(st.t), lr=st.lr_c)
        L.check(L.load().offsim_ppo_update_pop(C.byref(s), kind, C.byref(b), self.L, E, self._clip_c, self._kl_c, iters, C.byref(opt), L.ptr(stats),
                                               L.ptr(trace) if iters else None, L.ptr(st.scratch(T * E)), L.stream_ptr()))
        return stats, trace

    def update(self, batch):
        """Every learner's adapt() on its own columns of the batch -- the PPOBatch of VectorPSRS.collect_ppo_population as it is, or a dict
        of step-major device tensors [T, L * E, ...] (obs, act, adv, logp, ret and optionally valid).  Returns PPOUpdateInfo of [L] device
        tensors; `.pi_trace` / `.v_trace` hold every learner's (loss, kl) per pass ([L, iters, 2] f64, NaN after that learner's stop).
        Nothing here synchronises with the host."""
        T, E = _records(self, batch)
        ps, self.pi_trace = self._run(self._pi, L.PPO_ACTOR, batch, T, E, self.train_pi_iters)
        vs, self.v_trace = self._run(self._v, L.PPO_CRITIC, batch, T, E, self.train_v_iters)
        return PPOUpdateInfo(LossPi=ps[:, 0], LossV=vs[:, 0], KL=ps[:, 2], Entropy=ps[:, 3], ClipFrac=ps[:, 4], DeltaLossPi=ps[:, 1] - ps[:, 0],
                             DeltaLossV=vs[:, 1] - vs[:, 0], StopIter=ps[:, 5].to(torch.int64))

    def fit(self, env, epochs, T, tracker=None, **collect_kwargs):
        """PPOLearner.fit for every learner at once: per epoch env.collect_ppo_population(self, T, **collect_kwargs), ppo_epoch_log over
        the L learners, update(batch); everything enqueued, nothing read back between epochs.  env: a VectorPSRS of L * E environments,
        learner-major; tracker: the EpisodeTracker over them (a fresh one if None).  Returns a PPOTrainLog of [epochs, L] device tensors:
        column l is, bit for bit, PPOLearner.fit of learner l on its own E environments."""
        from .ppo_log import EpisodeTracker, _fit
        if tracker is None:
            tracker = EpisodeTracker(env.num_envs, env.table.device)
        return _fit(lambda: env.collect_ppo_population(self, T, **collect_kwargs), self.update, tracker, epochs, T, env.num_envs // self.L, False,
                    self.L)

    def adam_state(self):
        """((m [L, P], v [L, P], t [L]) of the actors, the same of the critics): the device tensors of the optimiser states."""
        if self._pi.device is None:
            raise ValueError("PPOPopulation.adam_state: the population has not been on a device yet")
        return (self._pi.m, self._pi.v, self._pi.t), (self._v.m, self._v.v, self._v.t)

    # ---- ranking the learners on a log ----
    def evaluate(self, table, seeds, gamma, obs, next_obs, **kw):
        """evalMC_psrs of every learner's actor, with its current weights, on the same sampler seeds: evalmc_rollouts_population (batched.py)
        over PolicyPopulation.from_ppo(self) -- the stacked device weights as they are, no copy.  Returns its dict: [L, S] host arrays,
        mean_value [L] and best."""
        from .batched import evalmc_rollouts_population
        from .obs_policy import PolicyPopulation
        return evalmc_rollouts_population(table, seeds, PolicyPopulation.from_ppo(self), gamma, obs=obs, next_obs=next_obs, **kw)

    def evaluate_queue(self, env_or_arrays, seeds, gamma, obs, next_obs, **kw):
        """evalMC on the queue simulator of every learner's actor, with its current weights, on the same sampler seeds and action streams:
        evalmc_rollouts_queue_population (queue_evaluator.py) over PolicyPopulation.from_ppo(self); `env_or_arrays`, `kw` and the result
        are its."""
        from .obs_policy import PolicyPopulation
        from .queue_evaluator import evalmc_rollouts_queue_population
        return evalmc_rollouts_queue_population(env_or_arrays, seeds, PolicyPopulation.from_ppo(self), gamma, obs=obs, next_obs=next_obs, **kw)

    def evaluate_env(self, kind_or_env, seeds, gamma, n_episodes, **kw):
        """evalMC in the TRUE environment of every learner's actor, with its current weights, on the same seeds (the same resets, noise and
        action uniforms): evalmc_rollouts_true_env (true_env_population.py) over PolicyPopulation.from_ppo(self); `kind_or_env`, `kw` and
        the result are its."""
        from .obs_policy import PolicyPopulation
        from .true_env_population import evalmc_rollouts_true_env
        return evalmc_rollouts_true_env(kind_or_env, seeds, PolicyPopulation.from_ppo(self), gamma, n_episodes, **kw)

    # ---- one learner, exported ----
    def actor(self, l):
        """learner l's actor as an MLPPolicy of its current weights (a copy)"""
        return self._pi.export(l)

    def critic(self, l):
        """learner l's critic as an MLPValue of its current weights (a copy)"""
        return self._v.export(l)

    def state_dict(self, l):
        """{'actor': ..., 'critic': ...}: learner l's networks as MLPPolicy / MLPValue.state_dict() give them"""
        return {"actor": self.actor(l).state_dict(), "critic": self.critic(l).state_dict()}

    def to_torch(self, l):
        """(actor, critic) of learner l as nn.Sequential, on the CPU"""
        return self.actor(l).to_torch(), self.critic(l).to_torch()


def ppo_grad_population(population, batch, kind, clip_ratio=None):
    """One forward / loss / backward pass of every learner (offsim_ppo_grad_pop): PPOGrad(grad [L, P] f32, flat per learner as ppo_grad's;
    n, loss, kl, entropy, clipfrac as [L] f64 device tensors).  batch as PPOPopulation.update's; clip_ratio: the population's, or a scalar
    or one value per learner."""
    if kind not in _KIND:
        raise ValueError(f"ppo_grad_population: kind must be 'actor' or 'critic', got {kind!r}")
    n = population.L
    clip = population.clip_ratio if clip_ratio is None else _per_learner(clip_ratio, n, "clip_ratio")
    T, E = _records(population, batch)
    st = population._pi if kind == "actor" else population._v
    b, dev, keep = _batch_struct(st, batch, _KIND[kind])
    st.on(dev)
    s = st.net_struct()
    grad = torch.zeros((n, st.P), dtype=torch.float32, device=dev)
    stats = torch.zeros((n, 5), dtype=torch.float64, device=dev)
    L.check(L.load().offsim_ppo_grad_pop(C.byref(s), _KIND[kind], C.byref(b), n, E, (C.c_double * n)(*clip), L.ptr(grad), L.ptr(stats),
                                         L.ptr(st.scratch(T * E)), L.stream_ptr()))
    return PPOGrad(grad, *(stats[:, i] for i in range(5)))


__all__ = ["PPOPopulation", "ppo_grad_population"]
