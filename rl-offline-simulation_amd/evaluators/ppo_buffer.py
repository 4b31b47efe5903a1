"""The PPO buffer of a vectorised collect: GAE-lambda advantages, rewards-to-go and spinup's normalisation on the device.

spinup's PPOBuffer (finish_path / get) under the path rules of the reference's agent (offsim4rl/agents/ppo.py:106-158), for [T, E]
step-major records of E environments: E environments are E MPI processes of local_steps_per_epoch = T, so the advantages are normalised
with the mean and population std over every valid entry of all environments (mpi_statistics_scalar).  The work is the HIP kernels of
offsim_ppo_advantages (csrc/ppo_buffer.hpp); VectorPSRS.collect_ppo calls them on the records of its own launch, ppo_advantages on
records of any other driver (a step_and_reset loop, say).
"""
from collections import namedtuple

import torch

from .. import _lib as L

_BOOT = {"reference": L.PPO_BOOT_REFERENCE, "spinup": L.PPO_BOOT_SPINUP}


class PPOBatch(namedtuple("PPOBatch", "obs act rew val logp adv adv_raw ret valid final_value v_trunc adv_mean adv_std collected")):
    """One PPO epoch buffer per environment, step-major device tensors [T, E, ...]:
    obs (the observation the actor was asked at), act, rew (f32), val (v(obs)), logp (of act), adv (normalised when collect_ppo's
    normalize, else adv_raw), adv_raw, ret, valid (a transition was served), final_value [E] (v at the observation each environment
    holds after the call: the bootstrap of its open path), v_trunc (bootstrap="spinup": v(next_obs) at truncating steps, else None),
    adv_mean / adv_std (0-dim f64: mpi_statistics_scalar of adv_raw; 0 / 0 without normalize) and collected (collect's Collected).
    From VectorPSRS.collect_ppo_population the E axis holds L learners' environments, learner-major, adv is normalised per learner and
    adv_mean / adv_std are [L]."""

    def flat(self):
        """The valid entries, environment-major then time -- E spinup buffers concatenated, what PPOBuffer.get hands to
        ppo.py:_compute_loss_pi / _compute_loss_v: dict(obs, act, ret, adv, logp)."""
        m = self.valid.t()
        out = {}
        for k in ("obs", "act", "ret", "adv", "logp"):
            x = getattr(self, k)
            out[k] = x.transpose(0, 1)[m]
        return out


def _advantages(rew, val, flags, final_value, v_trunc, gamma, lam, normalize, bootstrap, learners=None):
    """offsim_ppo_advantages on [T, E] device tensors: (adv_raw, ret, adv (normalised or adv_raw), mean, std).  learners = L: the columns
    are L learners' environments, learner-major, normalised per learner (offsim_ppo_advantages_pop); mean and std are then [L]."""
    T, E = int(rew.shape[0]), int(rew.shape[1])
    dev = rew.device
    if learners is not None:
        return _advantages_pop(rew, val, flags, final_value, v_trunc, gamma, lam, normalize, bootstrap, T, int(learners), E // int(learners))
    adv_raw = torch.empty((T, E), dtype=torch.float32, device=dev)
    ret = torch.empty((T, E), dtype=torch.float32, device=dev)
    adv = torch.empty((T, E), dtype=torch.float32, device=dev) if normalize else adv_raw
    stats = torch.zeros(2, dtype=torch.float64, device=dev)
    work = torch.empty(max(1, L.ppo_work_doubles(E)), dtype=torch.float64, device=dev) if normalize else None
    n = T * E
    L.check(L.load().offsim_ppo_advantages(L.ptr(rew) if n else None, L.ptr(val) if n else None, L.ptr(flags) if n else None,
                                           L.ptr(final_value) if E else None, L.ptr(v_trunc) if v_trunc is not None and n else None, T, E,
                                           float(gamma), float(lam), _BOOT[bootstrap], L.ptr(adv_raw) if n else None, L.ptr(ret) if n else None,
                                           L.ptr(adv) if normalize and n else None, L.ptr(stats) if normalize else None,
                                           L.ptr(work) if normalize else None, L.stream_ptr()))
    if normalize and not n:  # (nothing launched: no valid entry, mean = std = 0)
        stats.zero_()
    return adv_raw, ret, adv, stats[0], stats[1]


def _advantages_pop(rew, val, flags, final_value, v_trunc, gamma, lam, normalize, bootstrap, T, nl, E):
    dev = rew.device
    adv_raw = torch.empty((T, nl * E), dtype=torch.float32, device=dev)
    ret = torch.empty((T, nl * E), dtype=torch.float32, device=dev)
    adv = torch.empty((T, nl * E), dtype=torch.float32, device=dev) if normalize else adv_raw
    stats = torch.zeros((nl, 2), dtype=torch.float64, device=dev)
    work = torch.empty(nl * L.ppo_work_doubles(E), dtype=torch.float64, device=dev) if normalize else None
    n = T * E
    L.check(L.load().offsim_ppo_advantages_pop(L.ptr(rew) if n else None, L.ptr(val) if n else None, L.ptr(flags) if n else None,
                                               L.ptr(final_value), L.ptr(v_trunc) if v_trunc is not None and n else None, T, nl, E,
                                               float(gamma), float(lam), _BOOT[bootstrap], L.ptr(adv_raw) if n else None, L.ptr(ret) if n else None,
                                               L.ptr(adv) if normalize and n else None, L.ptr(stats) if normalize else None,
                                               L.ptr(work) if normalize else None, L.stream_ptr()))
    return adv_raw, ret, adv, stats[:, 0], stats[:, 1]


PPOAdvantages = namedtuple("PPOAdvantages", "adv adv_raw ret mean std")


def ppo_advantages(rew, val, terminated, truncated, valid, final_value, v_trunc=None, gamma=0.99, lam=0.97, normalize=True,
                   bootstrap="reference"):
    """The buffer rules of VectorPSRS.collect_ppo on [T, E] step-major records from any driver (include/offsim.h: offsim_ppo_advantages).

    rew / val [T, E] (f32 on the device), terminated / truncated / valid [T, E] bool, final_value [E] (v at the observation each
    environment holds after the last step), v_trunc [T, E] (v(next_obs) at truncating steps; bootstrap="spinup" only).  A path ends at a
    valid step with terminated | truncated; bootstrap="reference" gives it v of that step if truncated or if it is the last step (t = T - 1),
    else 0; "spinup" gives 0 if terminated, else v_trunc.  A path open after an environment's last valid step bootstraps with final_value.
    Returns PPOAdvantages(adv (normalised if normalize, else adv_raw), adv_raw, ret, mean, std) -- f32 [T, E] tensors, 0 at invalid entries,
    and 0-dim f64 mean / std (0 / 0 without normalize)."""
    if bootstrap not in _BOOT:
        raise ValueError(f"ppo_advantages: bootstrap must be 'reference' or 'spinup', got {bootstrap!r}")
    rew = torch.as_tensor(rew)
    dev = rew.device
    if dev.type != "cuda":
        raise ValueError("ppo_advantages: the records must be device tensors")
    if rew.dim() != 2:
        raise ValueError(f"ppo_advantages: rew must be [T, E], got shape {tuple(rew.shape)}")
    T, E = int(rew.shape[0]), int(rew.shape[1])

    def f32(x, shape, name):
        x = torch.as_tensor(x, device=dev).to(torch.float32).contiguous()
        if tuple(x.shape) != shape:
            raise ValueError(f"ppo_advantages: {name} must have shape {shape}, got {tuple(x.shape)}")
        return x

    def flag(x, name):
        x = torch.as_tensor(x, device=dev)
        if tuple(x.shape) != (T, E):
            raise ValueError(f"ppo_advantages: {name} must have shape {(T, E)}, got {tuple(x.shape)}")
        return x.to(torch.bool)

    rew, val = f32(rew, (T, E), "rew"), f32(val, (T, E), "val")
    final_value = f32(final_value, (E,), "final_value")
    if bootstrap == "spinup":
        if v_trunc is None:
            raise ValueError("ppo_advantages: bootstrap='spinup' needs v_trunc")
        v_trunc = f32(v_trunc, (T, E), "v_trunc")
    else:
        v_trunc = None
    flags = (flag(valid, "valid").to(torch.uint8) * L.COLLECT_SERVED + flag(terminated, "terminated").to(torch.uint8) * L.COLLECT_TERMINATED
             + flag(truncated, "truncated").to(torch.uint8) * L.COLLECT_TRUNCATED).to(torch.uint8).contiguous()
    adv_raw, ret, adv, mean, std = _advantages(rew, val, flags, final_value, v_trunc, gamma, lam, normalize, bootstrap)
    return PPOAdvantages(adv=adv, adv_raw=adv_raw, ret=ret, mean=mean, std=std)


__all__ = ["PPOBatch", "PPOAdvantages", "ppo_advantages"]
