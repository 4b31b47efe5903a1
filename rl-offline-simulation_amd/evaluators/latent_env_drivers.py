"""The reference's tabular drivers on the LATENT STATES of the environments with continuous observations, whole rollouts per launch: the
ground truth of a tabular policy or TD learner whose table is indexed through an encoder.

offsim4rl's headline experiments evaluate a tabular pi[z] inside PSRS, with z the 162-box encoding of CartPole's observation or a HOMER
encoder's latent state of the coordinate grid.  The value of that policy -- and the Q a learner reaches -- in the TRUE environment is this
module: evalMC, qlearn, expSARSA and z_expSARSA of offsim4rl/agents/tabular.py (:247-270, :71-139, :141-191, :193-245) on CartPole-v1 and
MyGridNaviCoords (offsim4rl/envs/gridworld.py:187-211) with the encoder run in the kernel at every observation the loop visits
(offsim_eval_env_latent / offsim_eval_env_latent_pop, csrc/eval_env_latent.hpp, include/offsim.h).

  LatentEnv(kind, encoder, num_states, ...)                      the world behind its encoder: nS, nA and a host mirror reset / step
  evalMC_latent_env, qlearn_latent_env, expSARSA_latent_env,
  z_expSARSA_env                                                 the reference's drivers, one launch each, the reference's return shapes
  evalmc_rollouts_latent_env(env, seeds, pi_or_stack, ...)       evalMC for many seeds, one policy or a stack of L
  BatchedLatentEnv(env, R)                                       R rollouts' carried state (the two streams) and the launches on it
  TDPopulation.run_latent_env (evaluators/td_population.py)      L learners x S seeds per launch

The row of a latent state z is z for 0 <= z < nS and z + nS for -nS <= z < 0: NumPy's index wrap (the box encoder's -1 is the reference's
Q[-1], the last row), the rule psrs._q_to_slots follows on the PSRS side.
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

_KINDS = {"cartpole": (L.ENV_CARTPOLE, 4, 2), "grid_coords": (L.ENV_GRID_COORDS, 2, 5)}  # kind -> (OFFSIM_ENV_*, dO, nA)
CARTPOLE_STEPS = 500  # CartPole-v1's max_episode_steps
MAX_UNITS = 4096      # the library's limit on H and nZ each (include/offsim.h)


def box_of(obs):
    """CartpoleBoxEncoder.get_box on one f32 observation: offsim_encode_box's f32 literals and comparisons; -1 out of bounds."""
    f = np.float32
    x, xd, th, thd = (f(v) for v in np.asarray(obs, np.float32).reshape(4))
    one, six, twelve, fifty = f(0.0174532), f(0.1047192), f(0.2094384), f(0.87266)
    if x < f(-2.4) or x > f(2.4) or th < -twelve or th > twelve:
        return -1
    box = 0 if x < f(-0.8) else 1 if x < f(0.8) else 2
    box += 0 if xd < f(-0.5) else 3 if xd < f(0.5) else 6
    box += 0 if th < -six else 9 if th < -one else 18 if th < f(0.0) else 27 if th < one else 36 if th < six else 45
    box += 0 if thd < -fifty else 54 if thd < fifty else 108
    return box


def _fma32(a, b, c):
    """fmaf(a, b, c) on f32 values, rounded once: the product is exact in f64; TwoSum gives the error of the f64 sum, and an inexact sum is
    moved to its odd neighbour on the error's side (round to odd), which the cast to f32 then rounds as it would the exact value (f64
    carries more than two bits beyond f32)"""
    p, c = np.float64(a) * np.float64(b), np.float64(c)
    s = p + c
    if not np.isfinite(s):
        return np.float32(s)
    t = s - p
    err = (p - (s - t)) + (c - t)
    if err != 0.0 and not int(s.view(np.int64)) & 1:
        s = np.nextafter(s, np.float64(np.inf) if err > 0 else np.float64(-np.inf))
    return np.float32(s)


def mlp_latent(weights, obs):
    """The HOMER obs_encoder on one f32 observation with the device's arithmetic: per unit one k-ordered fmaf chain from 0, then the bias,
    LeakyReLU(0.01), and the first arg max (a row that is all NaN gives 0)."""
    W1, b1, W2, b2 = weights
    x = np.asarray(obs, np.float32).reshape(-1)
    h = np.zeros(len(b1), np.float32)
    for j in range(len(b1)):
        acc = np.float32(0.0)
        for k in range(len(x)):
            acc = _fma32(x[k], W1[j, k], acc)
        acc = np.float32(acc + b1[j])
        h[j] = acc if acc > 0 else np.float32(np.float32(0.01) * acc)
    best, bv = 0, -np.inf
    for c in range(len(b2)):
        acc = np.float32(0.0)
        for k in range(len(h)):
            acc = _fma32(h[k], W2[c, k], acc)
        acc = np.float32(acc + b2[c])
        if acc > bv:
            best, bv = c, acc
    return best


class LatentEnv:
    """CartPole-v1 ("cartpole") or MyGridNaviCoords ("grid_coords") behind an encoder: what a tabular driver sees is z = encoder(observation).
    encoder: a CartpoleBoxEncoder (CartPole only; z in -1 .. 161) or a HOMEREncoder with weights (a HOMERPopulation.encoder(l) is one).
    num_states = nS, the rows of pi and Q; nA = 2 / 5.  max_episode_steps: CartPole's cap (default 500, required), optional on the grid,
    whose num_steps already bounds an episode.  reset(seed) / step(a) run on the host (the mirror of the device's rules, the dynamics in
    f64 and the encoder on the f32 observation) and return latent states; `s` is the current one, `obs` the current f32 observation."""

    def __init__(self, kind, encoder, num_states, num_cells=5, num_steps=15, goal=(4, 4), max_episode_steps=None):
        from ..encoders import CartpoleBoxEncoder, HOMEREncoder
        if kind not in _KINDS:
            raise ValueError(f"LatentEnv: kind must be one of {sorted(_KINDS)}, got {kind!r}")
        self.kind, self.encoder = kind, encoder
        self.env_kind, self.dO, self.nA = _KINDS[kind]
        self.nS = self.num_states = int(num_states)
        if self.nS < 1:
            raise ValueError("LatentEnv: num_states must be positive")
        if isinstance(encoder, CartpoleBoxEncoder):
            if kind != "cartpole":
                raise ValueError("LatentEnv: the box encoder reads CartPole's observation (kind 'cartpole')")
            if self.nS < encoder.N_BOXES:
                raise ValueError(f"LatentEnv: the box encoder gives -1 .. {encoder.N_BOXES - 1}: num_states must be at least {encoder.N_BOXES}")
            self.weights = None
        elif isinstance(encoder, HOMEREncoder):
            if encoder._w is None:
                raise ValueError("LatentEnv: the HOMER encoder has no weights (train it or load a model)")
            if encoder.obs_dim != self.dO:
                raise ValueError(f"LatentEnv: the encoder's input width {encoder.obs_dim} differs from the observation's width {self.dO}")
            if encoder.hidden_size > MAX_UNITS or encoder.latent_size > MAX_UNITS:
                raise ValueError(f"LatentEnv: hidden_size and latent_size are at most {MAX_UNITS} each")
            if encoder.latent_size > self.nS:
                raise ValueError(f"LatentEnv: the encoder gives {encoder.latent_size} latent states but num_states is {self.nS}")
            self.weights = tuple(np.ascontiguousarray(t.detach().cpu().numpy(), np.float32) for t in encoder._w)
        else:
            raise TypeError(f"LatentEnv: `encoder` must be a CartpoleBoxEncoder or a HOMEREncoder, got {type(encoder).__name__}")
        self.num_cells, self.num_steps, self.goal = int(num_cells), int(num_steps), (int(goal[0]), int(goal[1]))
        if kind == "grid_coords":
            if self.num_cells < 1 or self.num_steps < 1:
                raise ValueError("LatentEnv: num_cells and num_steps must be positive")
            if not (0 <= self.goal[0] < self.num_cells and 0 <= self.goal[1] < self.num_cells):
                raise ValueError(f"LatentEnv: the goal {self.goal} lies off the {self.num_cells} x {self.num_cells} grid")
        if max_episode_steps is None:
            max_episode_steps = CARTPOLE_STEPS if kind == "cartpole" else 0
        self.max_episode_steps = int(max_episode_steps)
        if self.max_episode_steps < (1 if kind == "cartpole" else 0):
            raise ValueError("LatentEnv: max_episode_steps must be positive for CartPole (nothing else bounds an episode) and not negative on the grid")
        self._rng, self._state, self._t, self.s, self.obs = None, None, 0, None, None

    # ---- what the launches need ----
    @property
    def bound(self):
        """the longest episode"""
        if self.kind == "cartpole":
            return self.max_episode_steps
        return min(self.max_episode_steps, self.num_steps) if self.max_episode_steps else self.num_steps

    def row(self, z):
        """the row of pi / Q of latent state z: NumPy's index wrap"""
        return int(z) + self.nS if z < 0 else int(z)

    def encode(self, obs):
        return box_of(obs) if self.weights is None else mlp_latent(self.weights, obs)

    # ---- the host mirror ----
    def _observe(self):
        if self.kind == "cartpole":
            self.obs = self._state.astype(np.float32)
        else:
            x, y, d = self._state
            self.obs = np.array([x / 5 + 0.1 + d[0], y / 5 + 0.1 + d[1]], np.float64).astype(np.float32)
        self.s = self.encode(self.obs)
        return self.s

    def reset(self, seed=None, rng=None):
        """env.reset(seed): a fresh default_rng(seed) (None: the stream runs on; rng: a Generator to draw from instead)"""
        if rng is not None:
            self._rng = rng
        elif seed is not None or self._rng is None:
            self._rng = np.random.default_rng(seed)
        self._t = 0
        if self.kind == "cartpole":
            self._state = self._rng.uniform(-0.05, 0.05, 4)
        else:
            self._state = [0, 0, self._rng.uniform(-0.1, 0.1, 2)]
        return self._observe()

    def step(self, action):
        """(z', reward, done, {}) with done at the environment's end or at max_episode_steps"""
        a = int(action)
        if not 0 <= a < self.nA:
            raise ValueError(f"LatentEnv.step: action {action!r} outside 0..{self.nA - 1}")
        if self.s is None:
            raise RuntimeError("LatentEnv.step before reset")
        if self.kind == "cartpole":
            g, mc, mp, ln, f, tau = 9.8, 1.0, 0.1, 0.5, 10.0, 0.02
            pm, tm = mp * ln, mc + mp
            x, xd, th, thd = (np.float64(v) for v in self._state)
            force = f if a == 1 else -f
            ct, sn = np.cos(th), np.sin(th)
            tmp = (force + pm * thd * thd * sn) / tm
            tha = (g * sn - ct * tmp) / (ln * (4.0 / 3.0 - mp * ct * ct / tm))
            xa = tmp - pm * tha * ct / tm
            self._state = np.array([x + tau * xd, xd + tau * xa, th + tau * thd, thd + tau * tha], np.float64)
            th_lim = 12 * 2 * 3.141592653589793 / 360
            reward = 1.0
            done = bool(self._state[0] < -2.4 or self._state[0] > 2.4 or self._state[2] < -th_lim or self._state[2] > th_lim)
        else:
            x, y, _ = self._state
            d = self._rng.uniform(-0.1, 0.1, 2)
            hi = self.num_cells - 1
            done = (x, y) == self.goal
            if a == 1:
                y = min(y + 1, hi)
            elif a == 2:
                x = min(x + 1, hi)
            elif a == 3:
                y = max(y - 1, 0)
            elif a == 4:
                x = max(x - 1, 0)
            if self._t + 1 >= self.num_steps:
                done = True
            if done:
                reward = 0.0
            elif (x, y) == self.goal:
                reward, done = 1.0, True
            else:
                reward = -0.1
            self._state = [x, y, d]
        self._t += 1
        if self.max_episode_steps and self._t >= self.max_episode_steps:
            done = True
        return self._observe(), reward, done, {}

    def state_row(self):
        """the four f64 of the device's state row (offsim_env): CartPole's state; the grid's (x, y, obs_0, obs_1)"""
        if self.kind == "cartpole":
            return self._state.copy()
        x, y, d = self._state
        return np.array([x, y, x / 5 + 0.1 + d[0], y / 5 + 0.1 + d[1]], np.float64)


def _check_env(who, env):
    if not isinstance(env, LatentEnv):
        raise TypeError(f"{who}: `env` must be a LatentEnv of this package, got {type(env).__name__}")


def _check_pi(who, env, pi, stack=False):
    pi = np.asarray(pi, dtype=np.float64)
    ok = pi.ndim == 2 or (stack and pi.ndim == 3 and pi.shape[0] >= 1)
    if not ok or tuple(pi.shape[-2:]) != (env.nS, env.nA):
        raise ValueError(f"{who}: pi must be a [nS, nA] = {(env.nS, env.nA)} table{' or a stack [L, nS, nA]' if stack else ''}, got {pi.shape}")
    return pi


def _reseed_flag(who, reseed):
    if reseed not in ("episode", "none"):
        raise ValueError(f"{who}: reseed must be 'episode' or 'none', got {reseed!r}")
    return 1 if reseed == "episode" else 0


_TRACE = (("trace_z", torch.int32, ()), ("trace_z_next", torch.int32, ()), ("trace_reward", torch.float64, ()), ("trace_done", torch.uint8, ()),
          ("trace_state", torch.float64, (4,)), ("trace_next_state", torch.float64, (4,)))


class BatchedLatentEnv:
    """R rollouts on one LatentEnv.  What a rollout carries from one call to the next is its action stream and its environment stream
    (rng_act / rng_env [R, 4], PCG64 words), and for a learner its Q and tie stream, which the caller hands back in; every episode begins
    with a reset, so a call with episode0 moved on by the episodes already run continues the last."""

    def __init__(self, env, R=1, device=None):
        _check_env("BatchedLatentEnv", env)
        self.world, self.R = env, int(R)
        self.device = torch.device(device) if device is not None else L.require_device()
        self.rng_act = torch.zeros((self.R, 4), dtype=torch.int64, device=self.device)
        self.rng_env = torch.zeros((self.R, 4), dtype=torch.int64, device=self.device)
        self._w = None if env.weights is None else tuple(torch.from_numpy(w).to(self.device).contiguous() for w in env.weights)
        self.set_seeds(np.arange(self.R))

    def set_seeds(self, seeds, action_seeds=None):
        """rollout i draws its actions from default_rng(action_seeds[i]) (None: seeds[i]) and, under reseed = 'none', its resets and noise from
        default_rng(seeds[i])"""
        sd = seeds_tensor(seeds, self.device)
        sa = sd if action_seeds is None else seeds_tensor(action_seeds, self.device)
        if sd.numel() != self.R or sa.numel() != self.R:
            raise ValueError(f"BatchedLatentEnv: {self.R} seeds and action seeds expected, got {sd.numel()} and {sa.numel()}")
        seed_streams(sd, out=self.rng_env)
        seed_streams(sa, out=self.rng_act)

    def _structs(self, rng_act, rng_env, o, reseed, episode0, trace_cap, rec_max=0, tie_reseed=0):
        w, dev = self.world, self.device
        R = int(rng_act.shape[0])
        ec = L.EnvEval(kind=w.env_kind, S=R, num_cells=w.num_cells, num_steps=w.num_steps, goal_x=w.goal[0], goal_y=w.goal[1], rng_env=L.ptr(rng_env),
                       rng_act=L.ptr(rng_act))
        if self._w is None:
            enc = L.LatentEncoder(kind=L.LATENT_BOX, nS=w.nS)
        else:
            W1, b1, W2, b2 = self._w
            enc = L.LatentEncoder(kind=L.LATENT_MLP, nS=w.nS, dO=w.dO, H=int(W1.shape[0]), nZ=int(W2.shape[0]), W1=L.ptr(W1), b1=L.ptr(b1), W2=L.ptr(W2),
                                  b2=L.ptr(b2))
        o["rng_act_end"], o["rng_env_end"] = torch.empty_like(rng_act), torch.empty_like(rng_env)
        if trace_cap:
            for k, dt, tail in _TRACE:
                o[k] = torch.full((R, trace_cap) + tail, -1, dtype=dt, device=dev) if dt == torch.int32 else torch.zeros((R, trace_cap) + tail, dtype=dt, device=dev)
        run = L.LatentRun(reseed=reseed, max_episode_steps=w.max_episode_steps, rec_max=int(rec_max), tie_reseed_episode=int(tie_reseed), episode0=int(episode0),
                          rng_act_end=L.ptr(o["rng_act_end"]), rng_env_end=L.ptr(o["rng_env_end"]), trace_cap=int(trace_cap),
                          **{k: L.ptr(o.get(k)) for k, _, _ in _TRACE})
        return ec, enc, run

    def _gp(self, gamma):
        return _gamma_pow(gamma, self.world.bound + 2, self.device, cap=self.world.bound + 2)

    def _run(self, pi, gamma, n_episodes, ep_cap, trace_cap, episode0, reseed, td):
        w, dev, R = self.world, self.device, self.R
        nS, nA = w.nS, w.nA
        flag = _reseed_flag("BatchedLatentEnv", reseed)
        pi_d = None if pi is None else torch.as_tensor(np.ascontiguousarray(_check_pi("BatchedLatentEnv", w, pi))).to(dev).contiguous()
        o, oc = rollout_outputs(R, dev, ep_cap, trace_cap)
        tdc, keep, tie_reseed, rec_max = None, (), 0, 0
        if td is not None:
            tdc, keep, tie_reseed = td_env_launch(td, R, nS, nA, dev, o, trace_cap)
            rec_max = int(td["rec_max"])
        gp = self._gp(gamma)
        ec, enc, run = self._structs(self.rng_act, self.rng_env, o, flag, episode0, trace_cap, rec_max, tie_reseed)
        L.check(L.load().offsim_eval_env_latent(C.byref(ec), C.byref(enc), L.ptr(pi_d), float(gamma), L.ptr(gp), gp.numel(), int(n_episodes), C.byref(oc),
                                                None if tdc is None else C.byref(tdc), C.byref(run), L.stream_ptr()))
        self.rng_act = o["rng_act_end"]  # the carried state: where the streams stand
        if not flag:
            self.rng_env = o["rng_env_end"]
        o["_keepalive"] = (pi_d, gp) + keep
        o["_kernel"] = "k_eval_env_latent"
        return o

    def eval_mc(self, pi, gamma, n_episodes, ep_cap=0, trace_cap=0, episode0=0, reseed="episode"):
        """evalMC (tabular.py:247-270) of pi [nS, nA] on every rollout in one launch.  Returns a dict of device tensors: sum_g, n_ep, steps,
        cand, n_len, status, rng_act_end / rng_env_end (+ ep_g, ep_len, trace_pop -- the action drawn at every step -- and the step trace
        trace_z / trace_z_next / trace_reward / trace_done / trace_state / trace_next_state when asked)."""
        return self._run(pi, gamma, n_episodes, ep_cap, trace_cap, episode0, reseed, None)

    def eval_td(self, pi, gamma, mode, alpha, q=None, n_episodes=1, ep_cap=0, trace_cap=0, behaviour=L.BEHAVIOUR_FIXED, epsilon=0.0, alpha_ep=None,
                epsilon_ep=None, snap_cap=0, snap_stride=1, tie=None, episode0=0, reseed="episode", rec_max=False):
        """qlearn / expSARSA / z_expSARSA (rec_max) on every rollout in one launch; the arguments are BatchedGridWorld.eval_td's with
        [nS, nA] tables by latent row."""
        td = dict(mode=mode, alpha=alpha, q=q, behaviour=behaviour, epsilon=epsilon, alpha_ep=alpha_ep, epsilon_ep=epsilon_ep, snap_cap=int(snap_cap),
                  snap_stride=snap_stride, tie=tie, rec_max=rec_max)
        return self._run(pi, gamma, n_episodes, ep_cap, trace_cap, episode0, reseed, td)

    def eval_mc_population(self, pi_stack, gamma, n_episodes, ep_cap=0, trace_cap=0, episode0=0, reseed="episode", state=False):
        """eval_mc for a stack of L policies [L, nS, nA], each on every one of the S = R rollouts: L * S rollouts in one launch.  Entry [l, j]
        of every output is, bit for bit, what eval_mc gives rollout j with policy l.  A query: the streams are not advanced; with `state`,
        out["_state"] holds where they stand afterwards."""
        w, dev, S = self.world, self.device, self.R
        flag = _reseed_flag("eval_mc_population", reseed)
        pi = _check_pi("eval_mc_population", w, pi_stack, stack=True)
        pi = pi[None] if pi.ndim == 2 else pi
        n_pol = int(pi.shape[0])
        pi_d = torch.as_tensor(np.ascontiguousarray(pi)).to(dev).contiguous()
        o, oc = rollout_outputs(n_pol * S, dev, ep_cap, trace_cap)
        rng_act, rng_env = self.rng_act.repeat(n_pol, 1), self.rng_env.repeat(n_pol, 1)
        gp = self._gp(gamma)
        ec, enc, run = self._structs(rng_act, rng_env, o, flag, episode0, trace_cap)
        L.check(L.load().offsim_eval_env_latent_pop(C.byref(ec), C.byref(enc), n_pol, S, None, L.ptr(pi_d), float(gamma), L.ptr(gp), gp.numel(),
                                                    int(n_episodes), C.byref(oc), C.byref(run), L.stream_ptr()))
        copies = dict(rng_act=o.pop("rng_act_end"), rng_env=o.pop("rng_env_end"))
        return population_result(o, n_pol, S, copies, (pi_d, gp, rng_act, rng_env), "k_eval_env_latent_pop", state=state)

    def eval_td_population(self, mode, alpha, gamma, behaviour=L.BEHAVIOUR_FIXED, epsilon=0.0, pi=None, q=None, alpha_ep=None, epsilon_ep=None,
                           tie=None, episode0=0, n_episodes=1, ep_cap=0, trace_cap=0, snap_cap=0, snap_stride=1, reseed="episode", rec_max=False,
                           state=False):
        """eval_td for L learners, each on every one of the S = R rollouts, in one launch (offsim_eval_env_latent_pop): the arguments and
        the result are BatchedGridWorld.eval_td_population's with [nS, nA] tables by latent row.  Entry [l, j] is, bit for bit, what eval_td
        gives rollout j under learner l's setting.  A query: the streams are not advanced."""
        w, dev, S = self.world, self.device, self.R
        flag = _reseed_flag("eval_td_population", reseed)
        by_episode = isinstance(tie, str) and tie == "episode"
        if isinstance(tie, str) and tie not in ("episode", "first"):
            raise ValueError(f"eval_td_population: tie must be None, 'first', 'episode' or [L,S,625] states, got {tie!r}")
        n_l, o, oc, pc, keep = td_population_launch("eval_td_population", dev, S, w.nS, w.nA, w.bound, mode, alpha, gamma, behaviour, epsilon, pi, q,
                                                    alpha_ep, epsilon_ep, None if isinstance(tie, str) else tie, w.bound + 2, ep_cap, trace_cap,
                                                    snap_cap, snap_stride, names=("pi", "q", "nS"))
        R = n_l * S
        if by_episode:
            mt = o["tie_mt"] = torch.zeros((R, 625), dtype=torch.int32, device=dev)
            mt[:, 624] = 624
            pc.tie_mt = L.ptr(mt)
        rng_act, rng_env = self.rng_act.repeat(n_l, 1), self.rng_env.repeat(n_l, 1)
        ec, enc, run = self._structs(rng_act, rng_env, o, flag, episode0, trace_cap, rec_max, 1 if by_episode else 0)
        L.check(L.load().offsim_eval_env_latent_pop(C.byref(ec), C.byref(enc), n_l, S, C.byref(pc), None, 0.0, None, 0, int(n_episodes), C.byref(oc),
                                                    C.byref(run), L.stream_ptr()))
        copies = dict(rng_act=o.pop("rng_act_end"), rng_env=o.pop("rng_env_end"))
        return population_result(o, n_l, S, copies, tuple(keep) + (rng_act, rng_env), "k_eval_env_latent_pop", state=state)


# ---------------------------------------------------------------------------------------------------
# Many seeds per launch
# ---------------------------------------------------------------------------------------------------
def evalmc_rollouts_latent_env(env, seeds, pi, gamma, n_episodes, reseed="episode", action_seeds=None, episode0=0):
    """evalMC (tabular.py:247-270) of a tabular policy over latent states in the true environment, many seeds in one launch: rollout i
    draws its actions from default_rng(action_seeds[i]) (None: seeds[i]) and runs n_episodes episodes.  reseed = "episode" (the reference):
    episode e resets with default_rng(episode0 + e); "none": rollout i's resets and noise come from default_rng(seeds[i]), which runs on
    across episodes.  pi [nS, nA]: evalmc_rollouts_env's dictionary (host arrays sum_g, n_ep, steps, cand, status, value = sum_g / n_ep).
    pi [L, nS, nA], a stack: [L, S] arrays, mean_value [L] and best; all policies of a seed see the same resets, the same noise and the
    same action uniforms, so differences are paired."""
    _check_env("evalmc_rollouts_latent_env", env)
    pi = _check_pi("evalmc_rollouts_latent_env", env, pi, stack=True)
    _reseed_flag("evalmc_rollouts_latent_env", reseed)
    seeds = np.asarray(seeds, dtype=np.uint64)
    if action_seeds is not None and len(np.asarray(action_seeds)) != len(seeds):
        raise ValueError(f"evalmc_rollouts_latent_env: one action seed per seed expected, got {len(np.asarray(action_seeds))} for {len(seeds)}")
    if int(n_episodes) < 1:
        raise ValueError("evalmc_rollouts_latent_env: n_episodes must be positive")
    outs = {k: [] for k in HOST_KEYS}
    if len(seeds):
        b = BatchedLatentEnv(env, len(seeds))
        b.set_seeds(seeds, action_seeds)
        collect_host(outs, b.eval_mc(pi, gamma, n_episodes, episode0=episode0, reseed=reseed) if pi.ndim == 2 else
                     b.eval_mc_population(pi, gamma, n_episodes, episode0=episode0, reseed=reseed))
    if pi.ndim == 2:
        return host_result(outs, empty=0)
    return population_host_result(outs, int(pi.shape[0]))


# ---------------------------------------------------------------------------------------------------
# The reference's drivers, one launch each
# ---------------------------------------------------------------------------------------------------
def _one(env, seed):
    b = BatchedLatentEnv(env, 1)
    b.set_seeds([int.from_bytes(os.urandom(8), "little") if seed is None else int(seed)])
    return b


def _undrawable(what, z):
    raise ValueError(f"{what}: no action can be drawn from the policy's row of latent state {z} (NaN, or probabilities that sum to 0)")


def _last_z(o, steps):
    """the latent state the loop stood in when it stopped, from the trace (None before the first step of an episode)"""
    if steps == 0 or bool(o["trace_done"].cpu()[0, steps - 1]):
        return None
    return int(o["trace_z_next"].cpu()[0, steps - 1])


def evalMC_latent_env(env, n_episodes, pi, gamma, seed=None):
    """tabular.py:247-270 on a LatentEnv with p = pi[z]: the whole loop -- env.reset(seed=episode), z = encoder(S), A = rng.choice(nA,
    p=pi[z]), env.step(A), discounted returns -- in one kernel launch: (Gs, lengths)."""
    _check_env("evalMC_latent_env", env)
    pi = _check_pi("evalMC_latent_env", env, pi)
    n_ep = int(n_episodes)
    if n_ep <= 0:
        return np.array([]), np.array([])
    o = _one(env, seed).eval_mc(pi, gamma, n_ep, ep_cap=n_ep, trace_cap=n_ep * env.bound + 1)
    status, steps = int(o["status"].cpu()[0]), int(o["steps"].cpu()[0])
    L.check_async_faults()
    if status == L.ST_KEYERROR:
        _undrawable("evalMC_latent_env", _last_z(o, steps))
    return o["ep_g"].cpu().numpy()[0, :n_ep].copy(), o["ep_len"].cpu().numpy()[0, :n_ep].astype(np.int64)


def _td_latent(env, what, n_episodes, gamma, alpha, epsilon, Q_init, save_Q, mode, kind, pi_tab, seed, tie, rec_max=False):
    """One launch of offsim_eval_env_latent for a learner driver call; returns (Q, info) as the reference does."""
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
    cap = n_ep * env.bound + 1
    o = _one(env, seed).eval_td(pi_tab, gamma, mode, 0.0 if callable(alpha) else alpha, q=Q0[None], n_episodes=n_ep, ep_cap=n_ep, trace_cap=cap,
                                behaviour=behaviour, epsilon=0.0 if callable(epsilon) else epsilon, alpha_ep=a_tab,
                                epsilon_ep=e_tab if behaviour == L.BEHAVIOUR_EPS_GREEDY else None, snap_cap=cap if save_Q else 0, snap_stride=1, tie=tie,
                                rec_max=rec_max)
    status, steps = int(o["status"].cpu()[0]), int(o["steps"].cpu()[0])
    L.check_async_faults()
    if "tie_mt" in o:  # np.random.seed(episode) of every episode begun (tabular.py:114, :166, :218), or the global stream run on
        w = o["tie_mt"].cpu().numpy().view(np.uint32)[0]
        np.random.set_state(("MT19937", w[:624].copy(), int(w[624]), 0, 0.0) if isinstance(tie, str) else ("MT19937", w[:624].copy(), int(w[624]), st[3], st[4]))
    if status == L.ST_KEYERROR:
        _undrawable(what, _last_z(o, steps))
    host = lambda k: o[k].cpu().numpy()[0, :steps].copy()  # noqa: E731
    Q = o["q"].cpu().numpy()[0].copy()
    td = host("td_err")
    Qs = np.array([Q0])
    if save_Q:  # Q before the first step, then after every step
        Qs = np.concatenate([Q0[None], o["q_snap"].cpu().numpy()[0, :steps]], axis=0)
    z, A, R, z_, done = host("trace_z"), host("trace_pop"), host("trace_reward"), host("trace_z_next"), host("trace_done").astype(bool)
    best = host("beh_arg") if behaviour == L.BEHAVIOUR_EPS_GREEDY else None
    episode = np.concatenate([[0], np.cumsum(done[:-1])]).astype(np.int64) if steps else np.zeros(0, np.int64)
    t_of = np.zeros(steps, np.int64)
    for i in range(1, steps):
        t_of[i] = 0 if done[i - 1] else t_of[i - 1] + 1

    def memory():
        eps_of = (lambda i: e_tab[min(int(episode[i]), len(e_tab) - 1)]) if e_tab is not None else (lambda i: float(epsilon))
        alpha_of = (lambda i: a_tab[min(int(episode[i]), len(a_tab) - 1)]) if a_tab is not None else (lambda i: float(alpha))
        ps, Qr = [], Q0.copy()
        for i in range(steps):
            if kind == "fixed":
                row = pi_tab[int(z[i])]
            elif behaviour == L.BEHAVIOUR_EPS_GREEDY:
                row = np.ones(nA) * eps_of(i) / nA
                row[int(best[i])] = 1 - eps_of(i) + eps_of(i) / nA
            else:  # soft greedy (Q-learning only: the recorded error is the update's): replay Q from the TD errors
                row = np.zeros(nA)
                row[np.where(np.isclose(Qr[z[i]], np.max(Qr[z[i]])))[0]] = 1
                row = row / row.sum()
                Qr[z[i], A[i]] = Qr[z[i], A[i]] + alpha_of(i) * td[i]
            ps.append(row)
        return [(int(z[i]), int(A[i]), float(R[i]), int(z_[i]), bool(done[i]), ps[i], {"t": int(t_of[i])}) for i in range(steps)]

    return Q, {"Gs": o["ep_g"].cpu().numpy()[0, :n_ep].copy(), "Qs": Qs, "TD_errors": td, "memory": memory()}


def qlearn_latent_env(env, n_episodes, behavior_policy, gamma, alpha=0.1, epsilon=1.0, Q_init=None, save_Q=0, seed=None, tie="episode"):
    """tabular.py:71-139 on a LatentEnv with Q indexed by z = encoder(S): Q-learning with the whole loop -- the encoder, the behaviour
    policy on the learner's own Q, the action draw from default_rng(seed), the environment's steps, the updates -- in one kernel launch.
    The arguments are qlearn_env's.  memory holds (z, A, R, z', done, p, {'t': t}), rebuilt from the kernel's trace."""
    _check_env("qlearn_latent_env", env)
    kind, fixed = _behaviour_kind(behavior_policy, env.nA)
    pi_tab = np.tile(np.asarray(fixed, dtype=np.float64), (env.nS, 1)) if kind == "fixed" else None
    return _td_latent(env, "qlearn_latent_env", n_episodes, gamma, alpha, epsilon, Q_init, save_Q, L.TD_QLEARN, kind, pi_tab, seed, tie)


def expSARSA_latent_env(env, n_episodes, pi, gamma, alpha=0.1, Q_init=None, save_Q=0, seed=None, tie="episode"):
    """tabular.py:141-191 on a LatentEnv: expected SARSA under the fixed behaviour / target policy pi [nS, nA] over latent rows, one
    kernel launch.  The reference sums Q[z_] @ pi[z_] in BLAS; here it runs left to right, so Q agrees to rounding."""
    _check_env("expSARSA_latent_env", env)
    pi = _check_pi("expSARSA_latent_env", env, pi)
    return _td_latent(env, "expSARSA_latent_env", n_episodes, gamma, alpha, 0.0, Q_init, save_Q, L.TD_EXPSARSA, "fixed", pi, seed, tie)


def z_expSARSA_env(env, n_episodes, pi, gamma, alpha=0.1, Q_init=None, save_Q=0, seed=None, tie="episode"):
    """tabular.py:193-245, z_expSARSA(env, ..., latent_state_func=encoder): expSARSA_latent_env, except that TD_errors records
    R + gamma * Q[z_].max() - Q[z, A] (:229) while the update stays expected SARSA (:232)."""
    _check_env("z_expSARSA_env", env)
    pi = _check_pi("z_expSARSA_env", env, pi)
    return _td_latent(env, "z_expSARSA_env", n_episodes, gamma, alpha, 0.0, Q_init, save_Q, L.TD_EXPSARSA, "fixed", pi, seed, tie, rec_max=True)
