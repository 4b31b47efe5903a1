"""The reference's tabular drivers on its own grid worlds, whole rollouts per launch: the ground truth PSRS and the queue baseline are judged
against.

offsim4rl's grid experiments compare three numbers for one tabular policy or learner: its value in the true grid world, inside PSRS and
inside the (z, a) queue baseline.  The last two run on the device (evalMC_psrs / qlearn_psrs / expSARSA_psrs, their PSRS_Exo forms, the
*_queue drivers, TDPopulation.run / run_exo / run_queue); this module is the first: evalMC, qlearn, expSARSA and rollout of
offsim4rl/agents/tabular.py on MyGridNavi, MyGridNaviNoise and MyGridNaviModuloCounter (offsim4rl/envs/gridworld.py:14-184) in
offsim_eval_env / offsim_eval_env_pop (csrc/eval_env.hpp, include/offsim.h).

  GridWorld(num_cells, num_steps, goal, kind, factor)    the world: a host descriptor with the reference's nS, nA, s and reset / step
  evalMC_env, qlearn_env, expSARSA_env, rollout_env      the reference's drivers, one launch each, the reference's return shapes
  evalmc_rollouts_env(env, seeds, pi, ...)               evalMC for many action-stream seeds, one policy or a stack of L
  BatchedGridWorld(env, R)                               R rollouts' carried state (the action streams) and the launches on it
  TDPopulation.run_env (evaluators/td_population.py)     L learners x S seeds per launch

The host side of GridWorld (reset / step, ExoStream) is a mirror of the device's rules in plain Python: it serves single steps, rebuilds the
`memory` of a driver call from the recorded actions, and is what the tests hold the kernels to.
"""
import ctypes as C
import os

import numpy as np
import torch

from .. import _lib as L
from ..table import seed_streams, seeds_tensor
from .psrs import _behaviour_kind, _schedule
from .rollout_io import (HOST_KEYS, _gamma_pow, collect_host, host_result, population_host_result, population_result, rollout_outputs,
                         td_driver_schedules, td_env_launch, td_population_launch)

_KINDS = {"plain": L.GRID_PLAIN, "noise": L.GRID_NOISE, "counter": L.GRID_COUNTER}
NA = 5  # noop, up, right, down, left


class ExoStream:
    """np.random.default_rng(seed) as the grid worlds use it -- Generator.integers(n) and nothing else -- written out on the raw 64-bit
    outputs: next_uint32 hands out the low, then the high half of each output; integers(n) draws nothing for n = 1, otherwise it is Lemire's
    bounded draw on those words (numpy/random: random_bounded_uint64 for a range below 2^32, unmasked)."""

    def __init__(self, seed=None):
        self._bg = np.random.PCG64(seed)
        self._has, self._hi = False, 0

    def next32(self):
        if self._has:
            self._has = False
            return self._hi
        v = int(self._bg.random_raw())
        self._has, self._hi = True, v >> 32
        return v & 0xFFFFFFFF

    def integers(self, n):
        n = int(n)
        if n <= 1:
            return 0
        m = self.next32() * n
        leftover = m & 0xFFFFFFFF
        if leftover < n:
            threshold = (0xFFFFFFFF - (n - 1)) % n
            while leftover < threshold:
                m = self.next32() * n
                leftover = m & 0xFFFFFFFF
        return m >> 32


class GridWorld:
    """MyGridNavi (kind "plain"), MyGridNaviNoise ("noise", factor = int(augmented_state)) or MyGridNaviModuloCounter ("counter", factor =
    counter_limit) of offsim4rl/envs/gridworld.py with discrete observations and a fixed goal.  nS = num_cells^2 * factor, nA = 5; the
    observation is cell + num_cells^2 * extra with cell = x + num_cells * y.  reset(seed) / step(a) run on the host (the mirror of the
    device's rules) with the reference's return values; `s` is the current observation."""

    def __init__(self, num_cells=5, num_steps=15, goal=(4, 4), kind="plain", factor=1):
        if kind not in _KINDS:
            raise ValueError(f"GridWorld: kind must be one of {sorted(_KINDS)}, got {kind!r}")
        num_cells, num_steps, factor = int(num_cells), int(num_steps), int(factor)
        if num_cells < 1 or num_steps < 1:
            raise ValueError("GridWorld: num_cells and num_steps must be positive")
        if factor < 1:
            raise ValueError(f"GridWorld: factor must be at least 1, got {factor}")
        if kind == "plain" and factor != 1:
            raise ValueError("GridWorld: the plain world has no exogenous state (factor = 1)")
        goal = (int(goal[0]), int(goal[1]))
        if not (0 <= goal[0] < num_cells and 0 <= goal[1] < num_cells):
            raise ValueError(f"GridWorld: the goal {goal} lies off the {num_cells} x {num_cells} grid")
        self.num_cells, self.num_steps, self.goal, self.kind, self.factor = num_cells, num_steps, goal, kind, factor
        self.num_states = num_cells ** 2
        self.nS, self.nA = self.num_states * factor, NA
        self._x = self._y = self.step_count = 0
        self._extra, self._stream, self.s = 0, None, None

    def c_struct(self):
        return L.GridEnv(kind=_KINDS[self.kind], num_cells=self.num_cells, num_steps=self.num_steps, goal_x=self.goal[0], goal_y=self.goal[1],
                         factor=self.factor)

    def _obs(self):
        return self._x + self.num_cells * self._y + self.num_states * self._extra

    def reset(self, seed=None):
        self._x = self._y = self.step_count = 0
        if self.kind != "plain":
            self._stream = ExoStream(seed)
            self._extra = self._stream.integers(self.factor)
        self.s = self._obs()
        return self.s

    def step(self, action):
        a = int(action)
        if not 0 <= a < NA:
            raise ValueError(f"GridWorld.step: action {action!r} outside 0..4")
        if self.s is None:
            raise RuntimeError("GridWorld.step before reset")
        if self.kind == "noise":
            self._extra = self._stream.integers(self.factor)
        elif self.kind == "counter":
            self._extra = (self._extra + 1) % self.factor
        hi = self.num_cells - 1
        done = (self._x, self._y) == self.goal
        z = self._x + self.num_cells * self._y
        if a == 1:
            self._y = min(self._y + 1, hi)
        elif a == 2:
            self._x = min(self._x + 1, hi)
        elif a == 3:
            self._y = max(self._y - 1, 0)
        elif a == 4:
            self._x = max(self._x - 1, 0)
        self.step_count += 1
        if self.step_count >= self.num_steps:
            done = True
        if done:
            reward = 0.0
        elif (self._x, self._y) == self.goal:
            reward, done = 1.0, True
        else:
            reward = -0.1
        info = {"task": np.array(self.goal), "task_id": self.goal[0] + self.num_cells * self.goal[1], "z": z,
                "z_next": self._x + self.num_cells * self._y, "t": self.step_count - 1}
        self.s = self._obs()
        return self.s, reward, done, info


def _check_pi(who, env, pi, stack=False):
    pi = np.asarray(pi, dtype=np.float64)
    ok = pi.ndim == 2 or (stack and pi.ndim == 3 and pi.shape[0] >= 1)
    if not ok or tuple(pi.shape[-2:]) != (env.nS, env.nA):
        raise ValueError(f"{who}: pi must be a [nS, nA] = {(env.nS, env.nA)} table{' or a stack [L, nS, nA]' if stack else ''}, got {pi.shape}")
    return pi


def _check_env(who, env):
    if not isinstance(env, GridWorld):
        raise TypeError(f"{who}: `env` must be a GridWorld of this package, got {type(env).__name__}")


class BatchedGridWorld:
    """R rollouts on one GridWorld.  What a rollout carries from one call to the next is its action stream (rng [R, 4], PCG64 words), and for
    a learner its Q and tie stream, which the caller hands back in; every episode begins with a reset, so a call with episode0 moved on by
    the episodes already run continues the last."""

    def __init__(self, env, R=1, device=None):
        _check_env("BatchedGridWorld", env)
        self.world, self.R = env, int(R)
        self.device = torch.device(device) if device is not None else L.require_device()
        self.c = env.c_struct()
        self.rng = torch.zeros((self.R, 4), dtype=torch.int64, device=self.device)
        self.set_action_seeds(np.arange(self.R))

    def set_action_seeds(self, seeds):
        """rollout i draws its actions from default_rng(seeds[i]) (tabular.py:75, :145, :248)"""
        sd = seeds_tensor(seeds, self.device)
        if sd.numel() != self.R:
            raise ValueError(f"BatchedGridWorld: {self.R} action seeds expected, got {sd.numel()}")
        seed_streams(sd, out=self.rng)

    def _ro(self, rng):
        return L.EnvRollouts(R=int(rng.shape[0]), rng_kind=L.STREAM_PCG64, rng=L.ptr(rng))

    def _gp(self, gamma):
        return _gamma_pow(gamma, self.world.num_steps + 2, self.device, cap=self.world.num_steps + 2)

    def _run(self, pi, gamma, n_episodes, ep_cap, trace_cap, episode0, td):
        w, dev, R = self.world, self.device, self.R
        nS, nA = w.nS, w.nA
        pi_d = None if pi is None else torch.as_tensor(np.ascontiguousarray(_check_pi("BatchedGridWorld", w, pi))).to(dev).contiguous()
        o, oc = rollout_outputs(R, dev, ep_cap, trace_cap)
        tdc, keep, reseed = None, (), 0
        if td is not None:
            tdc, keep, reseed = td_env_launch(td, R, nS, nA, dev, o, trace_cap)
        gp = self._gp(gamma)
        ro = self._ro(self.rng)
        L.check(L.load().offsim_eval_env(C.byref(self.c), C.byref(ro), L.ptr(pi_d), float(gamma), L.ptr(gp), gp.numel(), int(n_episodes), C.byref(oc),
                                         None if tdc is None else C.byref(tdc), reseed, int(episode0), L.stream_ptr()))
        o["_keepalive"] = (pi_d, gp) + keep
        o["_kernel"] = "k_eval_env" if td is not None else "k_eval_env_mc"
        return o

    def eval_mc(self, pi, gamma, n_episodes, ep_cap=0, trace_cap=0, episode0=0):
        """evalMC (tabular.py:247-270) of pi [nS, 5] on every rollout in one launch; episode e of the call resets with seed episode0 + e.
        Returns a dict of device tensors: sum_g, n_ep, steps, cand, n_len, status (+ ep_g, ep_len and trace_pop -- the action drawn at
        every step -- when asked)."""
        return self._run(pi, gamma, n_episodes, ep_cap, trace_cap, episode0, None)

    def eval_td(self, pi, gamma, mode, alpha, q=None, n_episodes=1, ep_cap=0, trace_cap=0, behaviour=L.BEHAVIOUR_FIXED, epsilon=0.0, alpha_ep=None,
                epsilon_ep=None, snap_cap=0, snap_stride=1, tie=None, episode0=0):
        """qlearn / expSARSA (tabular.py:71-191; mode: _lib.TD_QLEARN | _lib.TD_EXPSARSA) on every rollout in one launch; the arguments are
        BatchedQueueEvaluator.eval_td's with [nS, 5] tables by observation: pi None for Q-learning with a behaviour on the rollout's own Q,
        q [R, nS, 5] (zeros if None) back as out["q"], td_err / beh_arg [R, trace_cap], schedules, snapshots, and tie: None / "first" the
        first maximum, [R, 625] MT19937 states advanced in place (out["tie_mt"]), or "episode": the stream restarts as
        np.random.seed(episode0 + e) at the start of episode e."""
        td = dict(mode=mode, alpha=alpha, q=q, behaviour=behaviour, epsilon=epsilon, alpha_ep=alpha_ep, epsilon_ep=epsilon_ep, snap_cap=int(snap_cap),
                  snap_stride=snap_stride, tie=tie)
        return self._run(pi, gamma, n_episodes, ep_cap, trace_cap, episode0, td)

    def eval_mc_population(self, pi_stack, gamma, n_episodes, ep_cap=0, trace_cap=0, episode0=0, state=False):
        """eval_mc for a stack of L policies [L, nS, 5], each on every one of the S = R rollouts: L * S rollouts in one launch
        (offsim_eval_env_pop without learners).  Entry [l, j] of every output is, bit for bit, what eval_mc gives rollout j with policy l.
        A query: it runs on copies of the action streams; with `state`, out["_state"]["rng"] holds where they stand afterwards."""
        w, dev, S = self.world, self.device, self.R
        pi = _check_pi("eval_mc_population", w, pi_stack, stack=True)
        pi = pi[None] if pi.ndim == 2 else pi
        n_pol = int(pi.shape[0])
        pi_d = torch.as_tensor(np.ascontiguousarray(pi)).to(dev).contiguous()
        o, oc = rollout_outputs(n_pol * S, dev, ep_cap, trace_cap)
        rng = self.rng.repeat(n_pol, 1)
        gp = self._gp(gamma)
        ro = self._ro(rng)
        L.check(L.load().offsim_eval_env_pop(C.byref(self.c), C.byref(ro), n_pol, S, None, L.ptr(pi_d), float(gamma), L.ptr(gp), gp.numel(),
                                             int(n_episodes), C.byref(oc), 0, int(episode0), L.stream_ptr()))
        return population_result(o, n_pol, S, dict(rng=rng), (pi_d, gp), "k_eval_env_mc", state=state)

    def eval_td_population(self, mode, alpha, gamma, behaviour=L.BEHAVIOUR_FIXED, epsilon=0.0, pi=None, q=None, alpha_ep=None, epsilon_ep=None,
                           tie=None, episode0=0, n_episodes=1, ep_cap=0, trace_cap=0, snap_cap=0, snap_stride=1, state=False):
        """eval_td for L learners, each on every one of the S = R rollouts, in one launch (offsim_eval_env_pop): the arguments and the
        result are BatchedQueueEvaluator.eval_td_population's with [nS, 5] tables by observation.  Entry [l, j] is, bit for bit, what
        eval_td gives rollout j under learner l's setting.  A query: it runs on copies of the action streams."""
        w, dev, S = self.world, self.device, self.R
        by_episode = isinstance(tie, str) and tie == "episode"
        if isinstance(tie, str) and tie not in ("episode", "first"):
            raise ValueError(f"eval_td_population: tie must be None, 'first', 'episode' or [L,S,625] states, got {tie!r}")
        n_l, o, oc, pc, keep = td_population_launch("eval_td_population", dev, S, w.nS, w.nA, w.num_steps, mode, alpha, gamma, behaviour, epsilon, pi, q,
                                                    alpha_ep, epsilon_ep, None if isinstance(tie, str) else tie, w.num_steps + 2, ep_cap, trace_cap,
                                                    snap_cap, snap_stride, names=("pi", "q", "nS"))
        R = n_l * S
        if by_episode:
            mt = o["tie_mt"] = torch.zeros((R, 625), dtype=torch.int32, device=dev)
            mt[:, 624] = 624
            pc.tie_mt = L.ptr(mt)
        rng = self.rng.repeat(n_l, 1)
        ro = self._ro(rng)
        L.check(L.load().offsim_eval_env_pop(C.byref(self.c), C.byref(ro), n_l, S, C.byref(pc), None, 0.0, None, 0, int(n_episodes), C.byref(oc),
                                             1 if by_episode else 0, int(episode0), L.stream_ptr()))
        return population_result(o, n_l, S, dict(rng=rng), keep, "k_eval_env_pop", state=state)


# ---------------------------------------------------------------------------------------------------
# Many action-stream seeds per launch
# ---------------------------------------------------------------------------------------------------
def evalmc_rollouts_env(env, seeds, pi, gamma, n_episodes, episode0=0):
    """evalMC (tabular.py:247-270) in the true grid world for many action-stream seeds in one launch: rollout i draws its actions from
    default_rng(seeds[i]) and runs n_episodes episodes, episode e reset with seed episode0 + e.  pi [nS, 5]: returns evalmc_rollouts_queue's
    dictionary (host arrays sum_g, n_ep, steps, cand, status, value = sum_g / n_ep).  pi [L, nS, 5], a stack: [L, S] arrays, mean_value [L]
    and best; all policies of a seed start from the same action stream and see the same exogenous draws, so differences are paired."""
    _check_env("evalmc_rollouts_env", env)
    pi = _check_pi("evalmc_rollouts_env", env, pi, stack=True)
    seeds = np.asarray(seeds, dtype=np.uint64)
    if int(n_episodes) < 1:
        raise ValueError("evalmc_rollouts_env: n_episodes must be positive")
    outs = {k: [] for k in HOST_KEYS}
    if len(seeds):
        b = BatchedGridWorld(env, len(seeds))
        b.set_action_seeds(seeds)
        collect_host(outs, b.eval_mc(pi, gamma, n_episodes, episode0=episode0) if pi.ndim == 2 else
                     b.eval_mc_population(pi, gamma, n_episodes, episode0=episode0))
    if pi.ndim == 2:
        return host_result(outs, empty=0)
    return population_host_result(outs, int(pi.shape[0]))


# ---------------------------------------------------------------------------------------------------
# The reference's drivers, one launch each
# ---------------------------------------------------------------------------------------------------
def _one(env, seed):
    b = BatchedGridWorld(env, 1)
    b.set_action_seeds([int.from_bytes(os.urandom(8), "little") if seed is None else int(seed)])
    return b


def _raise_undrawable(what, env, actions, n_episodes):
    """the reference's rng.choice raises on a row it cannot draw from: find the row by replaying the recorded actions"""
    S, e = env.reset(seed=0), 0
    for a in actions:
        if a >= env.nA:
            break
        S, _, done, _ = env.step(a)
        if done:
            e += 1
            S = env.reset(seed=e)
    raise ValueError(f"{what}: no action can be drawn from the policy's row of observation {S} (NaN, or probabilities that sum to 0)")


class _EnvStepMemory:
    """The `memory` list of the drivers: (S, A, R, S', done, p, {**info, 't': t}) per step (tabular.py:59, :122, :174), rebuilt on first use
    by replaying the recorded actions through the host mirror."""

    def __init__(self, env, actions, p_of_step):
        self._env, self._actions, self._p_of_step, self._items = env, actions, p_of_step, None

    def _build(self):
        if self._items is None:
            env, ps, items = self._env, self._p_of_step(), []
            e, t, S = 0, 0, None
            for i, a in enumerate(self._actions):
                if S is None:
                    S, t = env.reset(seed=e), 0
                S_, R, done, info = env.step(int(a))
                items.append((S, int(a), R, S_, done, ps[i], {**info, "t": t}))
                S, t = S_, t + 1
                if done:
                    S, e = None, e + 1
            self._items = items
        return self._items

    def __len__(self):
        return len(self._actions)

    def __iter__(self):
        return iter(self._build())

    def __getitem__(self, i):
        return self._build()[i]


def _fresh(env):
    """a GridWorld of the same settings for replays, so that the caller's `env.s` is only what the driver's own loop leaves"""
    return GridWorld(env.num_cells, env.num_steps, env.goal, env.kind, env.factor)


def _leave(env, actions):
    """env.s and the host state as the reference's loop leaves them: after the last step of the last episode"""
    S, e = None, 0
    for a in actions:
        if S is None:
            env.reset(seed=e)
        S, _, done, _ = env.step(int(a))
        if done:
            S, e = None, e + 1


def evalMC_env(env, n_episodes, pi, gamma, seed=None):
    """tabular.py:247-270 on a GridWorld: the whole loop -- env.reset(seed=episode), A = rng.choice(5, p=pi[S]), env.step(A), discounted
    returns -- in one kernel launch: (Gs, lengths)."""
    _check_env("evalMC_env", env)
    pi = _check_pi("evalMC_env", env, pi)
    n_ep = int(n_episodes)
    if n_ep <= 0:
        return np.array([]), np.array([])
    o = _one(env, seed).eval_mc(pi, gamma, n_ep, ep_cap=n_ep, trace_cap=n_ep * env.num_steps + 1)
    status, steps = int(o["status"].cpu()[0]), int(o["steps"].cpu()[0])
    L.check_async_faults()
    actions = o["trace_pop"].cpu().numpy()[0, :steps + (status == L.ST_KEYERROR)]
    if status == L.ST_KEYERROR:
        _raise_undrawable("evalMC_env", _fresh(env), actions, n_ep)
    _leave(env, actions)
    return o["ep_g"].cpu().numpy()[0, :n_ep].copy(), o["ep_len"].cpu().numpy()[0, :n_ep].astype(np.int64)


def rollout_env(env, n_episodes, pi, gamma, seed=None):
    """tabular.py:34-69 on a GridWorld, one kernel launch: {"Gs", "memory"}.  NumPy's global stream is left as the reference leaves it
    (np.random.seed(episode) of the last episode)."""
    _check_env("rollout_env", env)
    pi = _check_pi("rollout_env", env, pi)
    n_ep = int(n_episodes)
    if n_ep <= 0:
        return {"Gs": np.array([]), "memory": []}
    o = _one(env, seed).eval_mc(pi, gamma, n_ep, ep_cap=n_ep, trace_cap=n_ep * env.num_steps + 1)
    status, steps = int(o["status"].cpu()[0]), int(o["steps"].cpu()[0])
    L.check_async_faults()
    actions = o["trace_pop"].cpu().numpy()[0, :steps + (status == L.ST_KEYERROR)]
    if status == L.ST_KEYERROR:
        _raise_undrawable("rollout_env", _fresh(env), actions, n_ep)
    np.random.seed(n_ep - 1)
    _leave(env, actions)
    mem = _EnvStepMemory(_fresh(env), actions, lambda: [pi[int(s)] for s in _observations(_fresh(env), actions)])
    return {"Gs": o["ep_g"].cpu().numpy()[0, :n_ep].copy(), "memory": mem}


def _observations(env, actions):
    """S of every step of the replayed actions"""
    out, S, e = [], None, 0
    for a in actions:
        if S is None:
            S = env.reset(seed=e)
        out.append(S)
        S, _, done, _ = env.step(int(a))
        if done:
            S, e = None, e + 1
    return out


def _td_env(env, what, n_episodes, gamma, alpha, epsilon, Q_init, save_Q, mode, kind, pi_tab, seed, tie):
    """One launch of offsim_eval_env for a learner driver call; returns (Q, info) as the reference does."""
    nS, nA = env.nS, env.nA
    Q0 = np.zeros((nS, nA)) if Q_init is None else np.asarray(Q_init).copy().astype(float)
    if Q0.shape != (nS, nA):
        raise ValueError(f"{what}: Q_init must be a [nS, nA] = {(nS, nA)} table, got {Q0.shape}")
    n_ep = int(n_episodes)
    if tie not in ("episode", "global", "first", None):
        raise ValueError(f"{what}: tie must be 'episode', 'global' or 'first'")
    if n_ep <= 0:
        return Q0, {"Gs": np.array([]), "Qs": np.array([Q0]), "TD_errors": np.array([]), "memory": []}
    behaviour, a_tab, e_tab, epsilon, tie, st = td_driver_schedules(_schedule, alpha, epsilon, kind, n_ep, tie)
    cap = n_ep * env.num_steps + 1
    o = _one(env, seed).eval_td(pi_tab, gamma, mode, 0.0 if callable(alpha) else alpha, q=Q0[None], n_episodes=n_ep, ep_cap=n_ep, trace_cap=cap,
                                behaviour=behaviour, epsilon=0.0 if callable(epsilon) else epsilon, alpha_ep=a_tab,
                                epsilon_ep=e_tab if behaviour == L.BEHAVIOUR_EPS_GREEDY else None, snap_cap=cap if save_Q else 0, snap_stride=1, tie=tie)
    status, steps = int(o["status"].cpu()[0]), int(o["steps"].cpu()[0])
    L.check_async_faults()
    if "tie_mt" in o:  # np.random.seed(episode) of every episode begun (tabular.py:114, :166), or the global stream run on
        w = o["tie_mt"].cpu().numpy().view(np.uint32)[0]
        np.random.set_state(("MT19937", w[:624].copy(), int(w[624]), 0, 0.0) if isinstance(tie, str) else ("MT19937", w[:624].copy(), int(w[624]), st[3], st[4]))
    actions = o["trace_pop"].cpu().numpy()[0, :steps + (status == L.ST_KEYERROR)]
    if status == L.ST_KEYERROR:
        _raise_undrawable(what, _fresh(env), actions, n_ep)
    _leave(env, actions)
    Q = o["q"].cpu().numpy()[0].copy()
    td = o["td_err"].cpu().numpy()[0, :steps].copy()
    Qs = np.array([Q0])
    if save_Q:  # tabular.py:107, :131: Q before the first step, then after every step
        Qs = np.concatenate([Q0[None], o["q_snap"].cpu().numpy()[0, :steps]], axis=0)
    best = o["beh_arg"].cpu().numpy()[0, :steps].copy() if behaviour == L.BEHAVIOUR_EPS_GREEDY else None

    def p_of_step():
        w, obs, dones = _fresh(env), [], []
        S, e = None, 0
        for a in actions:
            if S is None:
                S = w.reset(seed=e)
            obs.append(S)
            S, _, done, _ = w.step(int(a))
            dones.append(done)
            if done:
                S, e = None, e + 1
        episode = np.concatenate([[0], np.cumsum(dones[:-1])]).astype(np.int64) if steps else np.zeros(0, np.int64)
        eps_of = (lambda i: e_tab[min(int(episode[i]), len(e_tab) - 1)]) if e_tab is not None else (lambda i: float(epsilon))
        alpha_of = (lambda i: a_tab[min(int(episode[i]), len(a_tab) - 1)]) if a_tab is not None else (lambda i: float(alpha))
        if kind == "fixed":
            return [pi_tab[int(s)] for s in obs]
        if behaviour == L.BEHAVIOUR_EPS_GREEDY:
            ps = []
            for i in range(steps):
                row = np.ones(nA) * eps_of(i) / nA
                row[int(best[i])] = 1 - eps_of(i) + eps_of(i) / nA
                ps.append(row)
            return ps
        Qr, ps = Q0.copy(), []  # soft greedy: replay Q from the TD errors
        for i, (s, a) in enumerate(zip(obs, actions)):
            row = np.zeros(nA)
            row[np.where(np.isclose(Qr[s], np.max(Qr[s])))[0]] = 1
            ps.append(row / row.sum())
            Qr[s, a] = Qr[s, a] + alpha_of(i) * td[i]
        return ps

    return Q, {"Gs": o["ep_g"].cpu().numpy()[0, :n_ep].copy(), "Qs": Qs, "TD_errors": td, "memory": _EnvStepMemory(_fresh(env), actions, p_of_step)}


def qlearn_env(env, n_episodes, behavior_policy, gamma, alpha=0.1, epsilon=1.0, Q_init=None, save_Q=0, seed=None, tie="episode"):
    """tabular.py:71-139 on a GridWorld: Q-learning with the whole loop -- the behaviour policy on the learner's own Q, the action draw from
    default_rng(seed), the environment's steps, the updates -- in one kernel launch.  `behavior_policy` must be one of the reference's
    tabular policies (recognised by probing: psrs._behaviour_kind; anything else raises NotImplementedError); alpha and epsilon may be
    callables of the episode; save_Q returns Q after every step.  tie = "episode" (the reference): ties between maximal Q values are broken
    with NumPy's global stream restarted by np.random.seed(episode) at every episode, and the global stream is left as the reference
    leaves it; "global": the global stream as it stands runs on; "first": the first maximum."""
    _check_env("qlearn_env", env)
    kind, fixed = _behaviour_kind(behavior_policy, env.nA)
    pi_tab = np.tile(np.asarray(fixed, dtype=np.float64), (env.nS, 1)) if kind == "fixed" else None
    return _td_env(env, "qlearn_env", n_episodes, gamma, alpha, epsilon, Q_init, save_Q, L.TD_QLEARN, kind, pi_tab, seed, tie)


def expSARSA_env(env, n_episodes, pi, gamma, alpha=0.1, Q_init=None, save_Q=0, seed=None, tie="episode"):
    """tabular.py:141-191 on a GridWorld: expected SARSA under the fixed behaviour / target policy pi, one kernel launch.  The reference
    sums Q[S_] @ pi[S_] in BLAS; here it runs left to right, so Q agrees to rounding."""
    _check_env("expSARSA_env", env)
    pi = _check_pi("expSARSA_env", env, pi)
    return _td_env(env, "expSARSA_env", n_episodes, gamma, alpha, 0.0, Q_init, save_Q, L.TD_EXPSARSA, "fixed", pi, seed, tie)
