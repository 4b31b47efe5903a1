"""VectorGridNavi / VectorCartPole: the environments that produced the logs, many of them, a learner's loop in one launch.

The reference's experiments set a learner's curve inside a simulator built from a log (PSRS, QueueEvaluator) beside the same learner's
curve in the environment the log came from.  VectorPSRS and VectorQueueEvaluator run the first on the device; these classes run the
second, through the same calls and with the same records, so that both curves come from the same networks' bits and the same action rule:

    env = VectorCartPole(num_envs=4096)                 # or VectorGridNavi(num_envs, num_cells=5, num_steps=15, goal=(4, 4), coords=True)
    env.seed(env_seeds)                                 # environment k is default_rng(env_seeds[k]); resets every environment
    env.set_action_seeds(action_seeds)                  # environment k draws its actions from default_rng(action_seeds[k]) (default: env_seeds)
    batch = env.collect_ppo(actor, critic, 500)         # a PPOBatch: PPOLearner.update / ppo_epoch_log / PPOLearner.fit(env, ...) as they are
    dataset = env.record(actor, 1_000_000)              # the reference's record_dataset_in_memory: an OfflineDataset for VectorPSRS(dataset, ...)

VectorGridNavi is the reference's MyGridNavi (coords=False: the observation is the cell id) / MyGridNaviCoords (coords=True)
(offsim4rl/envs/gridworld.py:14-124, 187-211) with the goal a parameter; VectorCartPole is CartPole-v1, the equations of
synth.cartpole_log in f64.  The dynamics run inside the kernel (offsim_env_collect, csrc/collect_env.hpp); every environment has two PCG64
streams, one for its actions and one for the environment's own noise and resets.  The action rule is the package's, as
VectorQueueEvaluator's: A = Generator.choice(nA, p=p) on the action stream with p the policy's f32 probabilities widened exactly to f64.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from .. import _lib as L
from .. import spaces
from ..data import OfflineDataset, ProbDistribution
from ..table import seed_streams, seeds_tensor
from .obs_policy import _ACT, MLPPolicy, MLPValue
from .vector_env import Collected


class _VectorTrueEnv:
    """What the two environments share: the carried state, seeding, reset, the three collects and record."""

    def _init_env(self, kind, num_envs, nA, obs_shape, obs_dtype, device, num_cells=0, num_steps=0, goal=(0, 0)):
        dev = L.require_device() if device is None else torch.device(device)
        L.load()
        self.num_envs = E = int(num_envs)
        if E < 0:
            raise ValueError(f"num_envs must be >= 0, got {num_envs}")
        self.kind, self.nA = kind, nA
        self.table = SimpleNamespace(device=dev, nA=nA)  # what PPOLearner.fit / PPOPopulation.fit read of an environment
        self._obs_shape, self._obs_dtype = tuple(obs_shape), obs_dtype
        self.rng_env = torch.zeros((E, 4), dtype=torch.int64, device=dev)
        self.rng_act = torch.zeros((E, 4), dtype=torch.int64, device=dev)
        self.state = torch.zeros((E, 4), dtype=torch.float64, device=dev)
        self.step_count = torch.zeros(E, dtype=torch.int32, device=dev)
        self._ep_t = torch.zeros(E, dtype=torch.int32, device=dev)
        self.alive = torch.ones(E, dtype=torch.bool, device=dev)
        self.records = None
        self.c = L.Env(kind=kind, R=E, num_cells=int(num_cells), num_steps=int(num_steps), goal_x=int(goal[0]), goal_y=int(goal[1]),
                       rng_env=L.ptr(self.rng_env), rng_act=L.ptr(self.rng_act), state=L.ptr(self.state), step_count=L.ptr(self.step_count),
                       ep_t=L.ptr(self._ep_t))
        self.seed(np.arange(E))

    # ---- seeding and reset ----
    def seed(self, env_seeds):
        """Environment k becomes the reference environment constructed with seed=env_seeds[k] and reset(): its env stream is
        default_rng(env_seeds[k]), from which the reset takes its draws.  The action streams are set to the same seeds."""
        s = seeds_tensor(env_seeds, self.table.device)
        if s.numel() != self.num_envs:
            raise ValueError(f"seed: {self.num_envs} seeds expected, got {s.numel()}")
        seed_streams(s, out=self.rng_env)
        seed_streams(s, out=self.rng_act)
        self.reset()

    def set_action_seeds(self, seeds):
        """Environment k draws its actions from np.random.default_rng(seeds[k])."""
        s = seeds_tensor(seeds, self.table.device)
        if s.numel() != self.num_envs:
            raise ValueError(f"set_action_seeds: {self.num_envs} seeds expected, got {s.numel()}")
        seed_streams(s, out=self.rng_act)

    def reset(self, mask=None):
        """reset() of the environments in `mask` (all if None): the start state, the episode counters at 0, the reset's draws taken from
        the env stream as the reference's reset() without a seed takes them.  Returns (obs [E, ...], alive [E])."""
        m = None if mask is None else torch.as_tensor(mask, device=self.table.device).to(torch.uint8).contiguous()
        if m is not None and m.numel() != self.num_envs:
            raise ValueError(f"reset: a mask of {self.num_envs} entries expected, got {m.numel()}")
        L.check(L.load().offsim_env_collect_reset(C.byref(self.c), L.ptr(m), L.stream_ptr()))
        self._keep = m
        return self.obs, self.alive

    @property
    def obs(self):
        """The observation every environment holds, [E, ...] (a fresh tensor made from the carried f64 state)."""
        return self._obs_of(self.state)

    # ---- the policy's and the critic's descriptors ----
    def _mlp(self, c, form, net, what):
        dO = int(np.prod(self._obs_shape, dtype=np.int64)) if self._obs_shape else 1
        if net.dO != dO:
            raise ValueError(f"{what} takes observations of width {net.dO}, the environment's have {dO}")
        ws, arr = net._device_weights(self.table.device)
        c.form, c.n_layers, c.layers_host = form, len(ws), C.cast(arr, C.POINTER(L.MLPLayer))
        c.activation, c.slope, c.x_dtype, c.dO = _ACT[net.activation], net.slope, L.F32, net.dO
        return [ws]

    def _policy(self, policy, form):
        pol = L.CollectPolicy()
        if form == "auto":
            form = "mlp" if isinstance(policy, MLPPolicy) else "tabular"
        if form == "mlp":
            if not isinstance(policy, MLPPolicy):
                raise TypeError(f"collect: form='mlp' needs an MLPPolicy, got {type(policy).__name__}")
            if policy.nA != self.nA:
                raise ValueError(f"collect: the network has {policy.nA} outputs, the environment {self.nA} actions")
            return pol, self._mlp(pol, L.COLLECT_MLP, policy, "collect: the network")
        if form != "tabular":
            raise ValueError(f"collect: form must be 'auto', 'mlp' or 'tabular' (an environment has no logged rows), got {form!r}")
        nS = getattr(self, "nS", None)
        if nS is None:
            raise TypeError("collect: a tabular policy needs a grid environment; pass an MLPPolicy")
        pi = policy.detach().cpu().numpy() if isinstance(policy, torch.Tensor) else np.asarray(policy)
        if pi.ndim != 2 or pi.shape != (nS, self.nA):
            raise ValueError(f"collect: pi must be a [{nS}, {self.nA}] table indexed by the cell id, got shape {pi.shape}")
        f32 = pi.dtype == np.float32
        ps = torch.from_numpy(np.ascontiguousarray(pi.astype(np.float32 if f32 else np.float64))).to(self.table.device)
        pol.form, pol.pi, pol.x_dtype = L.COLLECT_TABULAR, L.ptr(ps), L.F32 if f32 else L.F64
        return pol, [ps]

    @staticmethod
    def _steps(who, num_steps, max_episode_steps):
        T = int(num_steps)
        if T < 0:
            raise ValueError(f"{who}: num_steps must be >= 0, got {num_steps}")
        cap = 0 if max_episode_steps is None else int(max_episode_steps)
        if cap < 0 or cap >= 1 << 31:
            raise ValueError(f"{who}: max_episode_steps must be None or in [0, 2**31), got {max_episode_steps} (0 = no limit)")
        return T, cap

    # ---- the launch and its records ----
    def _launch(self, pol, keep, T, cap, record_obs, record_probs, record_state, ppo=None, learners=None):
        E, dev, lib = self.num_envs, self.table.device, L.load()
        grid = self.kind != L.ENV_CARTPOLE

        def buf(shape, dtype, want=True):
            return torch.empty((T, E) + tuple(shape), dtype=dtype, device=dev) if want else None

        obs, next_obs = buf(self._obs_shape, self._obs_dtype, record_obs), buf(self._obs_shape, self._obs_dtype)
        sshape, sdtype = ((), torch.int32) if grid else ((4,), torch.float64)
        state, next_state = buf(sshape, sdtype, record_state), buf(sshape, sdtype, record_state)
        probs = buf((self.nA,), torch.float32, record_probs)
        action, reward = buf((), torch.int32), buf((), torch.float32)
        flags, ep_step = buf((), torch.uint8), buf((), torch.int32)
        status = torch.full((E,), L.ST_OK, dtype=torch.int32, device=dev)
        out = L.EnvOut(obs=L.ptr(obs), next_obs=L.ptr(next_obs), state=L.ptr(state), next_state=L.ptr(next_state), probs=L.ptr(probs),
                       action=L.ptr(action), reward=L.ptr(reward), flags=L.ptr(flags), ep_step=L.ptr(ep_step), status=L.ptr(status))
        if ppo is None:
            L.check(lib.offsim_env_collect(C.byref(self.c), C.byref(pol), T, cap, C.byref(out), L.stream_ptr()))
        elif learners is not None:
            L.check(lib.offsim_env_collect_ppo_pop(C.byref(self.c), C.byref(pol), C.byref(ppo[0]), learners, E // learners, T, cap, C.byref(out),
                                                   C.byref(ppo[1]), L.stream_ptr()))
        else:
            L.check(lib.offsim_env_collect_ppo(C.byref(self.c), C.byref(pol), C.byref(ppo[0]), T, cap, C.byref(out), C.byref(ppo[1]),
                                               L.stream_ptr()))
        self._keep = keep
        served = (flags & L.COLLECT_SERVED) != 0
        # the transition's index in this call's env-major record (record()'s row order)
        idx = torch.arange(E, dtype=torch.int32, device=dev).unsqueeze(0) * T + torch.arange(T, dtype=torch.int32, device=dev).unsqueeze(1)
        row = torch.where(served, idx, torch.full((), -1, dtype=torch.int32, device=dev))
        self.drawn_action = action
        self.records = SimpleNamespace(state=state, next_state=next_state, ep_step=ep_step, flags=flags)
        return Collected(obs=obs, probs=probs, row=row, action=torch.where(served, action, torch.zeros((), dtype=torch.int32, device=dev)).to(torch.int64),
                         reward=reward, next_obs=next_obs, terminated=(flags & L.COLLECT_TERMINATED) != 0,
                         truncated=(flags & L.COLLECT_TRUNCATED) != 0, reset=(flags & L.COLLECT_RESET) != 0,
                         alive=(flags & L.COLLECT_ALIVE) != 0, final_obs=self.obs, status=status)

    def collect(self, policy, num_steps, max_episode_steps=None, record_obs=True, record_probs=True, form="auto"):
        """VectorPSRS.collect in the real environment: `num_steps` steps of every environment in ONE launch (offsim_env_collect), reset
        inside the loop at terminated or at max_episode_steps (None: no limit besides the environment's own).

        policy: an MLPPolicy (the network runs inside the kernel, probs bit-equal to MLPPolicy.forward at the recorded observation) or, on
        a grid, an [num_cells ** 2, 5] f32 / f64 array indexed by the cell id.  Returns VectorPSRS's Collected, step-major [T, E, ...]:
        obs, probs, action, reward, next_obs (the true next observation, not the reset's), terminated, truncated, reset, alive, final_obs,
        status (all OFFSIM_ST_OK: a real environment never runs dry), and row = e * T + i, the transition's index in this call's env-major
        record, so every row is valid.  self.records keeps the last call's state / next_state (CartPole: [T, E, 4] f64; grids: the cell ids
        z / z_next), ep_step and flags.  The open episode -- state, counters and both streams -- carries over to the next call."""
        T, cap = self._steps("collect", num_steps, max_episode_steps)
        pol, keep = self._policy(policy, form)
        return self._launch(pol, keep, T, cap, record_obs, record_probs, True)

    def collect_ppo(self, actor, critic, num_steps, max_episode_steps=500, gamma=0.99, lam=0.97, normalize=True, bootstrap="reference", form="auto"):
        """VectorPSRS.collect_ppo in the real environment (offsim_env_collect_ppo): the keyword arguments and the PPOBatch are its own; the
        critic is an MLPValue (there are no logged rows to tabulate one over)."""
        T, cap = self._steps("collect_ppo", num_steps, max_episode_steps)
        if bootstrap not in ("reference", "spinup"):
            raise ValueError(f"collect_ppo: bootstrap must be 'reference' or 'spinup', got {bootstrap!r}")
        if not isinstance(critic, MLPValue):
            raise TypeError(f"collect_ppo: the critic must be an MLPValue, got {type(critic).__name__}")
        pol, keep = self._policy(actor, form)
        val = L.CollectValue()
        keep += self._mlp(val, L.VALUE_MLP, critic, "collect_ppo: the critic")
        return self._ppo_records(pol, val, keep, T, cap, gamma, lam, normalize, bootstrap)

    def collect_ppo_population(self, population, num_steps, max_episode_steps=500, gamma=0.99, lam=0.97, normalize=True, bootstrap="reference",
                               form="auto"):
        """VectorPSRS.collect_ppo_population in the real environment (offsim_env_collect_ppo_pop): num_envs = L * E, learner-major."""
        from .ppo_population import PPOPopulation
        if not isinstance(population, PPOPopulation):
            raise TypeError(f"collect_ppo_population: needs a PPOPopulation, got {type(population).__name__}")
        nl = population.L
        if self.num_envs % nl or self.num_envs == 0:
            raise ValueError(f"collect_ppo_population: num_envs = {self.num_envs} must be a positive multiple of the population's {nl} learners")
        T, cap = self._steps("collect_ppo_population", num_steps, max_episode_steps)
        if bootstrap not in ("reference", "spinup"):
            raise ValueError(f"collect_ppo_population: bootstrap must be 'reference' or 'spinup', got {bootstrap!r}")
        if form not in ("auto", "mlp"):
            raise ValueError(f"collect_ppo_population: form must be 'auto' or 'mlp', got {form!r}")
        pi, v = population._stacks(self.table.device)
        pol, val = L.CollectPolicy(), L.CollectValue()
        keep = self._mlp(pol, L.COLLECT_MLP, pi, "collect_ppo_population: the actors") + \
            self._mlp(val, L.VALUE_MLP, v, "collect_ppo_population: the critics")
        return self._ppo_records(pol, val, keep, T, cap, gamma, lam, normalize, bootstrap, learners=nl)

    def _ppo_records(self, pol, val, keep, T, cap, gamma, lam, normalize, bootstrap, learners=None):
        from .ppo_buffer import PPOBatch, _advantages
        E, dev = self.num_envs, self.table.device
        value = torch.zeros((T, E), dtype=torch.float32, device=dev)
        logp = torch.zeros((T, E), dtype=torch.float32, device=dev)
        final_value = torch.zeros((E,), dtype=torch.float32, device=dev)
        v_trunc = torch.zeros((T, E), dtype=torch.float32, device=dev) if bootstrap == "spinup" else None
        out = L.CollectPPOOut(value=L.ptr(value), logp=L.ptr(logp), final_value=L.ptr(final_value), v_trunc=L.ptr(v_trunc))
        c = self._launch(pol, keep, T, cap, True, True, True, ppo=(val, out), learners=learners)
        flags = self.records.flags & (L.COLLECT_SERVED | L.COLLECT_TERMINATED | L.COLLECT_TRUNCATED)
        adv_raw, ret, adv, mean, std = _advantages(c.reward, value, flags, final_value, v_trunc, gamma, lam, normalize, bootstrap, learners)
        return PPOBatch(obs=c.obs, act=c.action, rew=c.reward, val=value, logp=logp, adv=adv, adv_raw=adv_raw, ret=ret, valid=c.row >= 0,
                        final_value=final_value, v_trunc=v_trunc, adv_mean=mean, adv_std=std, collected=c)

    # ---- the reference's record_dataset_in_memory ----
    def record(self, policy, num_samples, max_episode_steps=None):
        """record_dataset_in_memory(env, agent, num_samples) (offsim4rl/utils/dataset_utils.py:36-131) on the device, with any policy
        collect takes: one collect of ceil(num_samples / num_envs) steps, its rows emitted environment-major (each environment a run of
        consecutive episodes) and cut to num_samples.  Returns an OfflineDataset with the reference's keys -- episode_ids
        (cumsum(steps == 0) - 1), steps, observations, actions, action_distributions (the policy's f32 probabilities), rewards,
        next_observations, terminals -- plus truncateds and, on the grids, infos/z and infos/z_next.  It goes straight into
        VectorPSRS(dataset, ...), VectorQueueEvaluator, HOMEREncoder.train and save_npz."""
        N = int(num_samples)
        if N < 0:
            raise ValueError(f"record: num_samples must be >= 0, got {num_samples}")
        E = self.num_envs
        if N > 0 and E == 0:
            raise ValueError("record: no environments")
        T = -(-N // E) if E else 0
        grid = self.kind != L.ENV_CARTPOLE
        _, cap = self._steps("record", T, max_episode_steps)
        pol, keep = self._policy(policy, "auto")
        c = self._launch(pol, keep, T, cap, True, True, grid)
        if not bool((c.row >= 0).all()):
            raise L.OffsimError("record: an environment stopped (the policy gave a row of NaN or zeros)")

        def em(x):  # env-major flatten, cut to N rows
            return x.transpose(0, 1).reshape((E * T,) + tuple(x.shape[2:]))[:N].cpu().numpy()

        steps = em(self.records.ep_step).astype(np.int64)
        exp = dict(episode_ids=np.cumsum(steps == 0).astype(np.int64) - 1, steps=steps, observations=em(c.obs), actions=em(c.action),
                   action_distributions=em(c.probs), rewards=em(c.reward), next_observations=em(c.next_obs), terminals=em(c.terminated),
                   truncateds=em(c.truncated))
        if grid:
            exp["infos/z"], exp["infos/z_next"] = em(self.records.state).astype(np.int64), em(self.records.next_state).astype(np.int64)
            if self.kind == L.ENV_GRID:
                exp["observations"], exp["next_observations"] = exp["observations"].astype(np.int64), exp["next_observations"].astype(np.int64)
        return OfflineDataset(self.observation_space, self.action_space, ProbDistribution.Discrete, **exp)


class VectorGridNavi(_VectorTrueEnv):
    """`num_envs` grid worlds of the reference (MyGridNaviCoords with coords=True, MyGridNavi's cell-id observations otherwise)."""

    def __init__(self, num_envs, num_cells=5, num_steps=15, goal=(4, 4), coords=True, device=None):
        if not 1 <= int(num_cells) <= 1024 or int(num_steps) < 1:
            raise ValueError(f"VectorGridNavi: num_cells in 1..1024 and num_steps >= 1, got {num_cells}, {num_steps}")
        self.num_cells, self.num_steps, self.goal, self.coords = int(num_cells), int(num_steps), (int(goal[0]), int(goal[1])), bool(coords)
        self.nS = self.num_cells ** 2
        self.action_space = spaces.Discrete(5)
        # the reference's spaces: MyGridNavi declares Box(0, num_cells - 1, (2,)) whatever it observes; the discrete form is used as Discrete
        self.observation_space = spaces.Box(0.0, float(self.num_cells - 1), (2,), np.float32) if self.coords else spaces.Discrete(self.nS)
        if self.coords:
            self._init_env(L.ENV_GRID_COORDS, num_envs, 5, (2,), torch.float32, device, num_cells, num_steps, self.goal)
        else:
            self._init_env(L.ENV_GRID, num_envs, 5, (), torch.int32, device, num_cells, num_steps, self.goal)

    def _obs_of(self, state):
        if self.coords:
            return state[:, 2:4].to(torch.float32)
        return (state[:, 0] + self.num_cells * state[:, 1]).to(torch.int32)


class VectorCartPole(_VectorTrueEnv):
    """`num_envs` CartPole-v1 environments (the dynamics of synth.cartpole_log, in f64; observations f32)."""

    def __init__(self, num_envs, device=None):
        self.action_space = spaces.Discrete(2)
        hi = np.array([4.8, np.finfo(np.float32).max, 24 * 2 * np.pi / 360, np.finfo(np.float32).max], np.float32)
        self.observation_space = spaces.Box(-hi, hi, (4,), np.float32)
        self._init_env(L.ENV_CARTPOLE, num_envs, 2, (4,), torch.float32, device)

    def _obs_of(self, state):
        return state.to(torch.float32)


__all__ = ["VectorGridNavi", "VectorCartPole"]
