"""evalMC of policies over observations in the environment the log came from: L actors on S paired seeds, whole rollouts in one launch.

The package ranks a population of trained actors inside PSRS (evalmc_rollouts_population, PPOPopulation.evaluate) and inside the (z, a)
queue baseline (evalmc_rollouts_queue_population, PPOPopulation.evaluate_queue).  This module is the third number of that comparison, the
one that says whether a simulator ranks the actors correctly: their value in the true dynamics --

    res = evalmc_rollouts_true_env("cartpole", seeds, actors, 0.99, n_episodes=10)       # or "grid" / "grid_coords" / a VectorCartPole
    res["value"]        # [L, S]: actor l on seed j; every actor of a seed sees the same resets, noise and action uniforms
    res["mean_value"]   # [L]
    res["best"]

-- in offsim_eval_env_obs (csrc/eval_env_obs.hpp, include/offsim.h): the dynamics and the action rule of VectorGridNavi / VectorCartPole
(csrc/collect_env.hpp), the networks' bits of MLPPolicy.forward.  Rollout (l, j) equals, bit for bit, what VectorX(S).seed(seeds);
set_action_seeds(action_seeds); reset(); collect(policy_l, ...) records for environment j, cut into its first n_episodes episodes.
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L
from .obs_policy import _ACT, MLPPolicy, ObsPolicy, PolicyPopulation, _stacked_layers
from .rollout_io import _gamma_pow, collect_host, population_host_result, seed_tiles
from .vector_true_env import VectorCartPole, VectorGridNavi, _VectorTrueEnv

_WHO = "evalmc_rollouts_true_env"
_KINDS = {"cartpole": L.ENV_CARTPOLE, "grid": L.ENV_GRID, "grid_coords": L.ENV_GRID_COORDS}
_WIDTH = {L.ENV_CARTPOLE: (4, 2), L.ENV_GRID: (1, 5), L.ENV_GRID_COORDS: (2, 5)}  # (observation width, actions)
CARTPOLE_MAX_EPISODE_STEPS = 500  # CartPole-v1's
_KEYS = ("sum_g", "n_ep", "steps", "cand", "status", "value", "Gs", "lengths", "ended")
_TRACE = ("trace_action", "trace_state", "trace_next_state")


def _environment(kind_or_env, grid_kw):
    """(OFFSIM_ENV_* kind, the grid's parameters, make(n, device): a fresh VectorX of n environments, device or None)"""
    if isinstance(kind_or_env, _VectorTrueEnv):
        if grid_kw:
            raise TypeError(f"{_WHO}: {sorted(grid_kw)} given beside an environment, whose own parameters are taken")
        env = kind_or_env
        if env.kind == L.ENV_CARTPOLE:
            return env.kind, {}, lambda n, dev: VectorCartPole(n, device=dev), env.table.device
        par = dict(num_cells=env.num_cells, num_steps=env.num_steps, goal=env.goal)
        return env.kind, par, lambda n, dev: VectorGridNavi(n, coords=env.coords, device=dev, **par), env.table.device
    if kind_or_env not in _KINDS:
        raise ValueError(f"{_WHO}: the environment is one of {sorted(_KINDS)}, a VectorCartPole or a VectorGridNavi, got {kind_or_env!r}")
    kind = _KINDS[kind_or_env]
    if kind == L.ENV_CARTPOLE:
        if grid_kw:
            raise TypeError(f"{_WHO}: CartPole takes no parameters, got {sorted(grid_kw)}")
        return kind, {}, lambda n, dev: VectorCartPole(n, device=dev), None
    unknown = set(grid_kw) - {"num_cells", "num_steps", "goal"}
    if unknown:
        raise TypeError(f"{_WHO}: unknown grid parameters {sorted(unknown)} (num_cells, num_steps, goal)")
    par = dict(num_cells=int(grid_kw.get("num_cells", 5)), num_steps=int(grid_kw.get("num_steps", 15)), goal=tuple(int(g) for g in grid_kw.get("goal", (4, 4))))
    if not 1 <= par["num_cells"] <= 1024 or par["num_steps"] < 1:
        raise ValueError(f"{_WHO}: num_cells in 1..1024 and num_steps >= 1, got {par['num_cells']}, {par['num_steps']}")
    return kind, par, lambda n, dev: VectorGridNavi(n, coords=kind == L.ENV_GRID_COORDS, device=dev, **par), None


def _population(policies):
    """`policies` as a PolicyPopulation of stacked networks; anything that has no network is refused (there are no logged rows)."""
    no_rows = f"{_WHO}: only MLP policies run in the true environment (per-row tables and callables need a log's rows)"
    if isinstance(policies, PolicyPopulation):
        if policies._stack is None:
            raise NotImplementedError(no_rows)
        return policies
    if isinstance(policies, ObsPolicy):
        policies = [policies]
    policies = list(policies)
    if not policies:
        raise ValueError(f"{_WHO}: no policies")
    if not all(isinstance(p, MLPPolicy) for p in policies):
        if all(isinstance(p, ObsPolicy) for p in policies):
            raise NotImplementedError(no_rows)
        raise TypeError(f"{_WHO}: policies are MLPPolicy's or a PolicyPopulation, got {sorted({type(p).__name__ for p in policies})}")
    return PolicyPopulation.from_policies(policies)


def _c_env(kind, par, S, rng_env=None, rng_act=None):
    goal = par.get("goal", (0, 0))
    return L.EnvEval(kind=kind, S=S, num_cells=par.get("num_cells", 0), num_steps=par.get("num_steps", 0), goal_x=goal[0], goal_y=goal[1],
                     rng_env=L.ptr(rng_env), rng_act=L.ptr(rng_act))


def _c_policy(st, arr, n_layers):
    return L.CollectPolicy(form=L.COLLECT_MLP, n_layers=n_layers, layers_host=C.cast(arr, C.POINTER(L.MLPLayer)), activation=_ACT[st.activation],
                           slope=st.slope, x_dtype=L.F32, dO=st.dO)


def _check_arguments(kind, par, st, n_pol, cap, bound):
    """offsim_eval_env_obs's own checks (the network against the environment, the limits, the workgroup's LDS) on a descriptor of the
    stack's layer shapes with S = 0: the library validates before any HIP call and launches nothing for no seeds, so nothing here touches
    a device."""
    arr = (L.MLPLayer * len(st.host))()
    for i, (W, b) in enumerate(st.host):
        arr[i].W, arr[i].b, arr[i].out = 1, None if b is None else 1, int(W.shape[1])  # (placeholders: never read without seeds)
        setattr(arr[i], "in", int(W.shape[2]))
    gp = (C.c_double * max(bound, 1))()
    L.check(L.load().offsim_eval_env_obs(C.byref(_c_env(kind, par, 0)), C.byref(_c_policy(st, arr, len(st.host))), n_pol, 1, cap,
                                         C.cast(gp, C.c_void_p), bound, C.byref(L.EnvEvalOut()), None))


def _launch(c_env, st, arr, n_layers, n_l, S, n_ep, cap, gp, trace_cap, dev):
    """One launch of n_l policies on S seeds; returns the dict of device tensors [n_l, S, ...]."""
    o = dict(Gs=torch.empty((n_l, S, n_ep), dtype=torch.float64, device=dev), lengths=torch.empty((n_l, S, n_ep), dtype=torch.int32, device=dev),
             ended=torch.empty((n_l, S, n_ep), dtype=torch.uint8, device=dev), n_ep=torch.empty((n_l, S), dtype=torch.int64, device=dev),
             steps=torch.empty((n_l, S), dtype=torch.int64, device=dev), status=torch.empty((n_l, S), dtype=torch.int32, device=dev),
             value=torch.empty((n_l, S), dtype=torch.float64, device=dev))
    if trace_cap:
        o["trace_action"] = torch.full((n_l, S, trace_cap), -1, dtype=torch.int32, device=dev)
        o["trace_state"] = torch.full((n_l, S, trace_cap, 4), float("nan"), dtype=torch.float64, device=dev)
        o["trace_next_state"] = torch.full((n_l, S, trace_cap, 4), float("nan"), dtype=torch.float64, device=dev)
    out = L.EnvEvalOut(trace_cap=trace_cap, **{k: L.ptr(v) for k, v in o.items()})
    L.check(L.load().offsim_eval_env_obs(C.byref(c_env), C.byref(_c_policy(st, arr, n_layers)), n_l, n_ep, cap, L.ptr(gp), gp.numel(), C.byref(out),
                                         L.stream_ptr()))
    o["cand"] = o["steps"]  # one action drawn per step
    return o


def _sum_g(Gs):
    """the completed episodes' returns summed in episode order from 0.0, as the kernel sums them (the others are zeros)"""
    s = torch.zeros(Gs.shape[:2], dtype=torch.float64, device=Gs.device)
    for e in range(Gs.shape[2]):
        s = s + Gs[:, :, e]
    return s


def evalmc_rollouts_true_env(kind_or_env, seeds, policies, gamma, n_episodes, max_episode_steps=None, action_seeds=None, tile=None, policy_tile=None,
                             trace_cap=0, **grid_kw):
    """evalMC of L policies over observations in the TRUE environment on the same S seeds: evalmc_rollouts_population (batched.py) and
    evalmc_rollouts_queue_population (queue_evaluator.py) in the environment itself.  Rollout (l, j) runs policy l for n_episodes episodes
    on seed j -- reset, then per step the network at the observation, A = Generator.choice(nA, p=p) on the seed's action stream, the
    dynamics, G += gamma**t * reward -- and all L * S rollouts of a tile run in ONE launch (offsim_eval_env_obs), one wavefront each.

    kind_or_env: "cartpole", "grid" (MyGridNavi, cell-id observations) or "grid_coords" (MyGridNaviCoords) with num_cells=5, num_steps=15,
    goal=(4, 4) as keywords, or a VectorCartPole / VectorGridNavi, whose parameters are taken and whose state is left untouched (a query).
    policies: one MLPPolicy, a list of them (one architecture), or a PolicyPopulation.from_policies / from_ppo; per-row tables and callables
    (RowPolicy, CallablePolicy, from_rows) raise NotImplementedError: an environment has no logged rows.
    seeds / action_seeds: seed j's streams are what VectorX(S).seed(seeds); set_action_seeds(action_seeds) leave (default: the action
    streams from `seeds` too), shared by all policies, so differences between policies are paired.
    max_episode_steps: the step cap of an episode (truncation); default 500 for CartPole, which needs one, none on the grids.
    tile / policy_tile: seeds / policies per launch (default: all); they change no bit.  trace_cap: for tests, the first trace_cap steps
    of every rollout as trace_action [L, S, trace_cap] (-1 where no step was taken) and trace_state / trace_next_state [L, S, trace_cap, 4]
    (the state row of VectorX before the step, and after it before any reset; NaN where no step was taken).

    Returns evalmc_rollouts_population's dictionary -- host arrays [L, S] sum_g, n_ep, steps, cand, status, value; mean_value [L]; best --
    and Gs [L, S, n_episodes] f64, lengths [L, S, n_episodes], ended [L, S, n_episodes] (2: terminated, 4: truncated).  A policy row from
    which no action can be drawn (NaN or zeros) raises ValueError, as evalMC_env does."""
    kind, par, make, dev = _environment(kind_or_env, grid_kw)
    pop = _population(policies)
    st, n_pol = pop._stack, len(pop)
    dO, nA = _WIDTH[kind]
    if st.dO != dO or st.nA != nA:
        raise ValueError(f"{_WHO}: the networks map {st.dO} inputs to {st.nA} outputs, the environment has observations of width {dO} and {nA} actions")
    n_ep = int(n_episodes)
    if n_ep < 0:
        raise ValueError(f"{_WHO}: n_episodes must be >= 0, got {n_episodes}")
    cap = (CARTPOLE_MAX_EPISODE_STEPS if kind == L.ENV_CARTPOLE else 0) if max_episode_steps is None else int(max_episode_steps)
    if cap < 0 or cap >= 1 << 31 or (kind == L.ENV_CARTPOLE and cap == 0):
        raise ValueError(f"{_WHO}: max_episode_steps must be in [{1 if kind == L.ENV_CARTPOLE else 0}, 2**31), got {max_episode_steps}"
                         + (" (nothing else bounds a CartPole episode)" if kind == L.ENV_CARTPOLE else " (0 = the grid's num_steps alone)"))
    bound = cap if kind == L.ENV_CARTPOLE else (min(cap, par["num_steps"]) if cap else par["num_steps"])
    trace_cap = int(trace_cap)
    if trace_cap < 0:
        raise ValueError(f"{_WHO}: trace_cap must be >= 0, got {trace_cap}")
    seeds = np.asarray(seeds, dtype=np.uint64)
    if seeds.ndim != 1:
        raise ValueError(f"{_WHO}: seeds [S] expected, got shape {seeds.shape}")
    if action_seeds is not None:
        action_seeds = np.asarray(action_seeds, dtype=np.uint64)
        if action_seeds.shape != seeds.shape:
            raise ValueError(f"{_WHO}: one action seed per seed")
    S = len(seeds)
    tile = max(S, 1) if tile is None else int(tile)
    policy_tile = n_pol if policy_tile is None else int(policy_tile)
    if tile < 1 or policy_tile < 1:
        raise ValueError(f"{_WHO}: tile and policy_tile must be positive")
    _check_arguments(kind, par, st, min(n_pol, policy_tile), cap, bound)

    keys = _KEYS + (_TRACE if trace_cap else ())
    parts = {k: [] for k in keys}
    if S and n_ep:
        dev = L.require_device() if dev is None else dev
        ws, arr0 = st._device_weights(dev)
        gp = _gamma_pow(gamma, bound, dev, cap=bound)
        for b, sd, env in seed_tiles(seeds, tile, lambda n: make(n, dev)):
            env.seed(sd)
            if action_seeds is not None:
                env.set_action_seeds(action_seeds[b:b + len(sd)])
            c_env = _c_env(kind, par, len(sd), env.rng_env, env.rng_act)
            cols = {k: [] for k in keys}
            for lo in range(0, n_pol, policy_tile):
                hi = min(n_pol, lo + policy_tile)
                o = _launch(c_env, st, arr0 if lo == 0 else _stacked_layers(ws, lo), len(ws), hi - lo, len(sd), n_ep, cap, gp, trace_cap, dev)
                o["sum_g"] = _sum_g(o["Gs"])
                collect_host(cols, o)
            for k in keys:
                parts[k].append(np.concatenate(cols[k], axis=0))
    else:  # nothing to run: the empty result, without a launch
        shapes = dict(Gs=((n_ep,), np.float64), lengths=((n_ep,), np.int32), ended=((n_ep,), np.uint8), sum_g=((), np.float64), n_ep=((), np.int64),
                      steps=((), np.int64), cand=((), np.int64), status=((), np.int32), value=((), np.float64), trace_action=((trace_cap,), np.int32),
                      trace_state=((trace_cap, 4), np.float64), trace_next_state=((trace_cap, 4), np.float64))
        fill = dict(value=np.nan, trace_action=-1, trace_state=np.nan, trace_next_state=np.nan)
        for k in keys:
            parts[k].append(np.full((n_pol, S) + shapes[k][0], fill.get(k, 0), dtype=shapes[k][1]))
    value = np.concatenate(parts.pop("value"), axis=1)  # the kernel's own: the same division, so the same bits as sum_g / n_ep below
    res = population_host_result(parts, n_pol)
    assert np.array_equal(res["value"], value, equal_nan=True), "value: the kernel's mean differs from sum_g / n_ep"
    bad = np.argwhere(res["status"] == L.ST_KEYERROR)
    if len(bad):
        l, j = (int(v) for v in bad[0])
        raise ValueError(f"{_WHO}: no action can be drawn from policy {l}'s probabilities at step {int(res['steps'][l, j])} of seed index {j} "
                         f"(NaN, or probabilities that sum to 0); {len(bad)} of {n_pol * S} rollouts stopped this way")
    return res
