"""VectorPSRS: many PerStateRejectionSampling environments behind one call per step.

The reference evaluator (offsim4rl/evaluators/per_state_rejection.py:7-98) is one environment driven by one Python call
per simulated step (examples/cartpole/psrs_from_expert_heuristic.py:59-80); a neural learner that reveals an action
distribution per step cannot be moved into a kernel.  What can be done for it is to step thousands of independent
environments (sampler seeds) with ONE launch: this class is `PerStateRejectionSampling` vectorised over `num_envs`,
every environment identical to the reference evaluator constructed from the same dataset and reset_sampler(seed_k).

    env = VectorPSRS(dataset, num_envs=4096, num_states=162, encoder=CartpoleBoxEncoder())
    env.reset_sampler(seeds)                  # PSRS.reset_sampler(seed_k) for every environment k
    obs, alive = env.reset()                  # [R, ...] device tensor, alive[k] False where reset() returned None
    a, next_obs, r, done, alive = env.step_dist_batch(probs)   # probs [R, nA] (tensor or torch Distribution)

Rows of environments that are exhausted (step_dist would return the all-None tuple) have alive == False and keep their
previous observation.  Everything stays on the device; no per-environment Python work and (with strict=False) no host
synchronisation per call.  `obs` and `alive` are updated in place, and a call is nothing but kernel launches on the current
stream, so a whole driver iteration (policy forward -> step_dist_batch -> reset of the finished environments) can be
captured once in a HIP graph and replayed (`torch.cuda.graph`, see `graph_iteration`): the loop is launch-bound otherwise.
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from .. import _lib as L
from ..spaces import is_discrete
from ..table import TransitionTable
from .obs_policy import _ACT, MLPPolicy, MLPValue, ObsPolicy, RowPolicy, RowValue, obs_tensor
from .psrs import BatchedPSRS

try:
    from torch.distributions import Distribution
except Exception:  # pragma: no cover
    class Distribution:  # type: ignore
        pass


class _Collector:
    """collect / collect_ppo / collect_ppo_population of VectorPSRS and VectorQueueEvaluator (evaluators/vector_queue.py): argument checks,
    the policy's and the critic's descriptors, the records' assembly.  A class that mixes this in has table, env (the BatchedPSRS holding the
    rollout state), num_envs, strict, obs, alive, _ep_t, _obs_row, _obs, _next_obs, _a, _r, _encoded and _x_rows, and gives the simulator's part:
      _launch_collect(pol, f32, T, cap, st, out, ppo, learners)  the library call; returns the drawn actions [T, E] or None (the served row's)
      _raise_keyerror(status, action)                            strict mode's KeyError for the first environment that met one
      _policy_f32(dtype)                                         whether a policy table of torch dtype `dtype` is passed as f32
      _tabular_policy(pi, f32)                                   the device table of the TABULAR form from a host [nS, nA] array"""

    # ---- a learner's data collection: T steps in one launch ----------------------------------------------------------------------
    def _init_payload(self, dataset, encoded):
        """The log's columns in caller order, the environments' observation / alive / ep_t / obs_row buffers and the gather descriptors of
        reset and the per-step calls (needs table and num_envs)."""
        e, dev = dataset.experience, self.table.device
        n = len(e["actions"])
        # payload columns in the caller's row order (the kernels report rows of the caller's buffer)
        self._obs = torch.as_tensor(np.asarray(e["observations"])).to(dev)
        self._next_obs = torch.as_tensor(np.asarray(e["next_observations"])).to(dev)
        self._a = torch.as_tensor(np.asarray(e["actions"])).to(dev)
        self._r = torch.as_tensor(np.asarray(e["rewards"])).to(dev)
        self._done = torch.as_tensor(np.asarray(e["terminals"]) != 0).to(dev)
        self.observation_space, self.action_space = dataset.observation_space, dataset.action_space
        self.obs = torch.zeros((self.num_envs,) + tuple(self._obs.shape[1:]), dtype=self._obs.dtype, device=dev)
        # alive [E] and the episode step counter of collect, ep_t [E] i32, share one buffer: reset_sampler clears both with one fill
        ea = (self.num_envs + 3) // 4 * 4
        self._sbuf = torch.zeros(ea + 4 * self.num_envs, dtype=torch.uint8, device=dev)
        self.alive = self._sbuf[:self.num_envs].view(torch.bool)
        self._ep_t = self._sbuf[ea:].view(torch.int32)
        # where each environment's observation comes from (include/offsim.h: offsim_collect_state.obs_row): kept by reset, step_dist_batch
        # and step_and_reset through extra gather columns (no extra launch): src_next[i] = i, src_init[i] = -2 - i, zero[i] = 0
        self._obs_row = torch.full((self.num_envs,), -1, dtype=torch.int32, device=dev)
        self._src_next = torch.arange(n, dtype=torch.int32, device=dev)
        self._src_init = -2 - self._src_next
        self._src_zero = torch.zeros(n, dtype=torch.int32, device=dev)
        self._encoded = bool(encoded)
        self._x_rows = None
        # outputs of step_dist_batch (overwritten by every call) and the column descriptors of offsim_vector_gather
        self._obs, self._next_obs, self._a, self._r, self._done = (x.contiguous() for x in (self._obs, self._next_obs, self._a, self._r, self._done))
        self.action = torch.zeros(self.num_envs, dtype=self._a.dtype, device=dev)
        self.reward = torch.zeros(self.num_envs, dtype=self._r.dtype, device=dev)
        self.done = torch.zeros(self.num_envs, dtype=torch.bool, device=dev)

        def cols(*pairs):
            arr = (L.Column * len(pairs))()
            for c, (src, dst, zero) in zip(arr, pairs):
                nb = src.element_size() * int(np.prod(src.shape[1:], dtype=np.int64))
                assert nb == dst.element_size() * int(np.prod(dst.shape[1:], dtype=np.int64))
                c.src, c.dst, c.row_bytes, c.zero_if_not_ok = src.data_ptr(), dst.data_ptr(), nb, int(zero)
            return arr

        self._cols_step = cols((self._next_obs, self.obs, False), (self._a, self.action, False), (self._r, self.reward, False), (self._done, self.done, True),
                               (self._src_next, self._obs_row, False))
        self._cols_reset = cols((self._obs, self.obs, False), (self._src_init, self._obs_row, False), (self._src_zero, self._ep_t, False))

    def _reset_envs(self, mask):
        """The simulator's reset for the environments in `mask` (all if None), with obs, obs_row, ep_t and alive kept in step"""
        m = None if mask is None else mask.to(torch.uint8).contiguous()
        row = self.env.reset(m)
        L.check(L.load().offsim_vector_gather(L.ptr(row), None, L.ptr(m), self.num_envs, self._cols_reset, len(self._cols_reset),
                                              L.ptr(self.alive), L.stream_ptr()))
        return self.obs, self.alive

    def collect(self, policy, num_steps, max_episode_steps=None, record_obs=True, record_probs=True, form="auto"):
        """The loop a learner runs inside PSRS (examples/cartpole/psrs_from_expert_heuristic.py:59-80, an epoch of a fixed network,
        offsim4rl/agents/ppo.py:122-160) for `num_steps` steps of every environment, in ONE launch (offsim_vector_collect):

            probs = policy(obs); step_and_reset(probs); reset(mask=truncated & ~terminated)     # T times

        with the episode's step counter kept on the device: truncated = ep_t >= max_episode_steps after a served step (None: no limit;
        terminated and truncated may both be set, as in the example).  An environment whose step returns None (or raises KeyError:
        strict=True raises it here) or whose reset finds no initial row stops for the rest of the call.

        policy: MLPPolicy (the network runs inside the kernel, p_new bit-equal to MLPPolicy.forward), any other ObsPolicy (its per-row
        tables), or an [nS, nA] array indexed by the state (only where observations are states, as evalMC_psrs).  form: "auto", or
        "mlp" / "rows" / "tabular" to pick one ("rows" also takes an MLPPolicy, through its row_tables).  p_new is compared in f32 where
        the policy's probabilities and p_log are both f32, in f64 otherwise (step_and_reset's rule).

        Returns a Collected of device tensors, step-major [T, E, ...]: obs (the observation the policy was asked at; record_obs),
        probs (f32; record_probs), row (served caller row, -1 where nothing was served), action / reward / next_obs of the served row
        (zeros where none), terminated, truncated, reset (an initial observation follows), alive (after the step), final_obs [E, ...]
        (self.obs after the last step: the bootstrap observation of ppo.py:127-131), status [E] (include/offsim.h: OFFSIM_ST_*).
        self.obs / self.alive and the sampler state carry over, so collect mixes freely with reset / step_dist_batch / step_and_reset.
        ep_t counts the steps collect served since the environment's last reset; step_dist_batch / step_and_reset do not advance it
        (they have no time limit) but their resets clear it, as reset() and reset_sampler() do."""
        T = int(num_steps)
        if T < 0:
            raise ValueError(f"collect: num_steps must be >= 0, got {num_steps}")
        cap = 0 if max_episode_steps is None else int(max_episode_steps)
        if cap < 0 or cap >= 1 << 31:
            raise ValueError(f"collect: max_episode_steps must be None or in [0, 2**31), got {max_episode_steps} (0 = no limit)")
        env, t = self.env, self.table
        env._quiesce()
        env._orders_for_generic()
        pol, keep, f32 = self._collect_policy(policy, form)
        return self._collect_launch(pol, keep, f32, T, cap, record_obs, record_probs)

    def _collect_launch(self, pol, keep, f32, T, cap, record_obs, record_probs, ppo=None, learners=None):
        """The simulator's collect (ppo None) or collect_ppo (ppo = (offsim_collect_value, offsim_collect_ppo_out)) over T steps -- its
        population form where the environments are those of `learners` learners with stacked networks (_launch_collect); returns the
        Collected records."""
        env, t = self.env, self.table
        E, dev = self.num_envs, t.device
        row = torch.empty((T, E), dtype=torch.int32, device=dev)
        flags = torch.empty((T, E), dtype=torch.uint8, device=dev)
        obs = torch.empty((T,) + tuple(self.obs.shape), dtype=self.obs.dtype, device=dev) if record_obs else None
        probs = torch.empty((T, E, t.nA), dtype=torch.float32, device=dev) if record_probs else None
        status = torch.full((E,), L.ST_OK, dtype=torch.int32, device=dev)
        st = L.CollectState()
        st.ep_t, st.obs_row, st.alive, st.obs = L.ptr(self._ep_t), L.ptr(self._obs_row), L.ptr(self.alive), L.ptr(self.obs)
        st.obs_next, st.obs_init = L.ptr(self._next_obs), L.ptr(self._obs)
        st.obs_bytes = self.obs.element_size() * int(np.prod(self.obs.shape[1:], dtype=np.int64))
        out = L.CollectOut()
        out.row, out.flags, out.obs, out.probs, out.status = L.ptr(row), L.ptr(flags), L.ptr(obs), L.ptr(probs), L.ptr(status)
        drawn = self._launch_collect(pol, f32, T, cap, st, out, ppo, learners)
        self._keep = keep
        if self.strict and bool((status == L.ST_KEYERROR).any()):
            self._raise_keyerror(status, drawn)
        served = (flags & L.COLLECT_SERVED) != 0
        rl = row.clamp(min=0).to(torch.int64)

        def take(col):
            if t.N == 0:
                return torch.zeros((T, E) + tuple(col.shape[1:]), dtype=col.dtype, device=dev)
            v = col[rl]
            return torch.where(served.reshape(served.shape + (1,) * (v.dim() - 2)), v, torch.zeros((), dtype=v.dtype, device=dev))

        action = take(self._a) if drawn is None else torch.where(served, drawn, torch.zeros((), dtype=drawn.dtype, device=dev)).to(self._a.dtype)
        return Collected(obs=obs, probs=probs, row=row, action=action, reward=take(self._r), next_obs=take(self._next_obs),
                         terminated=(flags & L.COLLECT_TERMINATED) != 0, truncated=(flags & L.COLLECT_TRUNCATED) != 0,
                         reset=(flags & L.COLLECT_RESET) != 0, alive=(flags & L.COLLECT_ALIVE) != 0, final_obs=self.obs.clone(), status=status)

    def collect_ppo(self, actor, critic, num_steps, max_episode_steps=500, gamma=0.99, lam=0.97, normalize=True, bootstrap="reference",
                    form="auto"):
        """One PPO epoch buffer per environment from one call: collect(actor, num_steps, max_episode_steps) with the critic and logp of the
        served action recorded in the same launch (offsim_vector_collect_ppo), then GAE-lambda advantages, rewards-to-go and spinup's
        normalisation on the device (offsim_ppo_advantages).  E environments are E spinup MPI processes of local_steps_per_epoch =
        num_steps: PPOAgentRevealed (offsim4rl/agents/ppo.py:30-158) driven by the CartPole example's loop
        (examples/cartpole/psrs_from_expert_heuristic.py:59-80), with the networks fixed for the epoch.  The defaults are the agent's and
        the example's.

        actor: as collect's policy (form likewise).  critic: MLPValue (evaluated inside the kernel at the observation the actor is asked
        at) or RowValue (per-row tables of any critic).  bootstrap: "reference" -- the agent's rules: a path that ends truncated, or ends
        at the call's last step even if terminated, bootstraps with v(obs) of its last step, one that terminates earlier with 0 -- or
        "spinup" -- terminated 0, truncated v(next_obs) of the truncating row.  Either way a path the call leaves open (the epoch cut,
        or an environment that stopped) bootstraps with v at the observation it holds (final_value), and stays open for the next call.

        Returns a PPOBatch of step-major [T, E] device tensors (flat() gives the loss inputs of ppo.py:_compute_loss_pi / _v).  The sampler
        state, observations and episode counters carry over exactly as for collect: the trajectory is collect's."""
        T = int(num_steps)
        if T < 0:
            raise ValueError(f"collect_ppo: num_steps must be >= 0, got {num_steps}")
        cap = 0 if max_episode_steps is None else int(max_episode_steps)
        if cap < 0 or cap >= 1 << 31:
            raise ValueError(f"collect_ppo: max_episode_steps must be None or in [0, 2**31), got {max_episode_steps} (0 = no limit)")
        if bootstrap not in ("reference", "spinup"):
            raise ValueError(f"collect_ppo: bootstrap must be 'reference' or 'spinup', got {bootstrap!r}")
        env, t = self.env, self.table
        dev = t.device
        env._quiesce()
        env._orders_for_generic()
        pol, keep, f32 = self._collect_policy(actor, form)
        val = L.CollectValue()
        if isinstance(critic, MLPValue):
            keep += self._collect_mlp(val, L.VALUE_MLP, critic, "collect_ppo: the critic")
        elif isinstance(critic, RowValue):
            vn, v0 = critic.tables(t.N, dev)
            val.form, val.v_next, val.v_init = L.VALUE_ROWS, L.ptr(vn), L.ptr(v0)
            keep += [vn, v0]
        else:
            raise TypeError(f"collect_ppo: the critic must be an MLPValue or a RowValue, got {type(critic).__name__}")
        return self._collect_ppo_records(pol, val, keep, f32, T, cap, gamma, lam, normalize, bootstrap)

    def _collect_ppo_records(self, pol, val, keep, f32, T, cap, gamma, lam, normalize, bootstrap, learners=None):
        """The launch and the advantages of collect_ppo / collect_ppo_population from the actor's and the critic's descriptors."""
        from .ppo_buffer import PPOBatch, _advantages
        E, dev = self.num_envs, self.table.device
        value = torch.zeros((T, E), dtype=torch.float32, device=dev)
        logp = torch.zeros((T, E), dtype=torch.float32, device=dev)
        final_value = torch.zeros((E,), dtype=torch.float32, device=dev)
        v_trunc = torch.zeros((T, E), dtype=torch.float32, device=dev) if bootstrap == "spinup" else None
        out = L.CollectPPOOut(value=L.ptr(value), logp=L.ptr(logp), final_value=L.ptr(final_value), v_trunc=L.ptr(v_trunc))
        c = self._collect_launch(pol, keep, f32, T, cap, True, True, ppo=(val, out), learners=learners)
        rew = c.reward.to(torch.float32)
        flags = ((c.row >= 0).to(torch.uint8) * L.COLLECT_SERVED + c.terminated.to(torch.uint8) * L.COLLECT_TERMINATED
                 + c.truncated.to(torch.uint8) * L.COLLECT_TRUNCATED).to(torch.uint8)
        adv_raw, ret, adv, mean, std = _advantages(rew, value, flags, final_value, v_trunc, gamma, lam, normalize, bootstrap, learners)
        return PPOBatch(obs=c.obs, act=c.action, rew=rew, val=value, logp=logp, adv=adv, adv_raw=adv_raw, ret=ret, valid=c.row >= 0,
                        final_value=final_value, v_trunc=v_trunc, adv_mean=mean, adv_std=std, collected=c)

    def collect_ppo_population(self, population, num_steps, max_episode_steps=500, gamma=0.99, lam=0.97, normalize=True, bootstrap="reference",
                               form="auto"):
        """collect_ppo for a PPOPopulation of L learners in the same launches (offsim_vector_collect_ppo_pop, offsim_ppo_advantages_pop): the
        num_envs = L * E environments are the learners', learner-major -- environment r belongs to learner r // E and runs that learner's
        actor and critic out of the population's stacked device weights.  The keyword arguments are collect_ppo's (form: "auto" or "mlp",
        the networks run inside the kernel).  Returns a PPOBatch over [T, L * E]: learner l's buffer is the columns l * E .. (l + 1) * E - 1,
        adv is normalised per learner, and adv_mean / adv_std are [L]; PPOPopulation.update consumes it as it is.  Every environment's
        records and carried state are those of collect_ppo with its learner's networks, bit for bit; the sampler state, observations and
        episode counters carry over as for collect_ppo, so the call mixes with reset, collect and the rest."""
        from .ppo_population import PPOPopulation
        if not isinstance(population, PPOPopulation):
            raise TypeError(f"collect_ppo_population: needs a PPOPopulation, got {type(population).__name__}")
        nl = population.L
        if self.num_envs % nl or self.num_envs == 0:
            raise ValueError(f"collect_ppo_population: num_envs = {self.num_envs} must be a positive multiple of the population's {nl} learners")
        T = int(num_steps)
        if T < 0:
            raise ValueError(f"collect_ppo_population: num_steps must be >= 0, got {num_steps}")
        cap = 0 if max_episode_steps is None else int(max_episode_steps)
        if cap < 0 or cap >= 1 << 31:
            raise ValueError(f"collect_ppo_population: max_episode_steps must be None or in [0, 2**31), got {max_episode_steps} (0 = no limit)")
        if bootstrap not in ("reference", "spinup"):
            raise ValueError(f"collect_ppo_population: bootstrap must be 'reference' or 'spinup', got {bootstrap!r}")
        if form not in ("auto", "mlp"):
            raise ValueError(f"collect_ppo_population: form must be 'auto' or 'mlp', got {form!r}")
        env, t = self.env, self.table
        env._quiesce()
        env._orders_for_generic()
        pi, v = population._stacks(t.device)
        pol, val = L.CollectPolicy(), L.CollectValue()
        keep = self._collect_mlp(pol, L.COLLECT_MLP, pi, "collect_ppo_population: the actors") + \
            self._collect_mlp(val, L.VALUE_MLP, v, "collect_ppo_population: the critics")
        return self._collect_ppo_records(pol, val, keep, self._policy_f32(torch.float32), T, cap, gamma, lam, normalize, bootstrap, learners=nl)

    def _collect_policy(self, policy, form):
        """offsim_collect_policy for collect / collect_ppo: (struct, tensors to keep alive, whether p_new is compared in f32)."""
        if form == "auto":
            form = "mlp" if isinstance(policy, MLPPolicy) else "rows" if isinstance(policy, ObsPolicy) else "tabular"
        t = self.table
        pol, keep = L.CollectPolicy(), []
        if form == "mlp":
            if not isinstance(policy, MLPPolicy):
                raise TypeError(f"collect: form='mlp' needs an MLPPolicy, got {type(policy).__name__}")
            keep += self._collect_mlp(pol, L.COLLECT_MLP, policy, "collect: the network")
            f32 = self._policy_f32(torch.float32)
        elif form == "rows":
            if not isinstance(policy, ObsPolicy):
                raise TypeError(f"collect: form='rows' needs an ObsPolicy, got {type(policy).__name__}")
            pn, p0 = self._caller_tables(policy)
            f32 = self._policy_f32(pn.dtype)
            pn, p0 = (x.to(torch.float32 if f32 else torch.float64).contiguous() for x in (pn, p0))
            pol.form, pol.p_next, pol.p_init = L.COLLECT_ROWS, L.ptr(pn), L.ptr(p0)
            keep += [pn, p0]
        elif form == "tabular":
            if isinstance(policy, ObsPolicy):
                raise TypeError("collect: form='tabular' needs an [nS, nA] array")
            if self._encoded:
                raise NotImplementedError("collect: the observations of this environment differ from its latent states, but a tabular policy is "
                                          "indexed by the observation (psrs.py:158, :255); pass a policy over observations (MLPPolicy, RowPolicy)")
            pi = policy.detach().cpu().numpy() if isinstance(policy, torch.Tensor) else np.asarray(policy)
            if pi.ndim != 2 or pi.shape[1] != t.nA:
                raise ValueError(f"collect: pi must be a [nS, {t.nA}] table, got shape {pi.shape}")
            f32 = self._policy_f32(torch.float32 if pi.dtype == np.float32 else torch.float64)
            ps = self._tabular_policy(pi, f32)
            pol.form, pol.pi = L.COLLECT_TABULAR, L.ptr(ps)
            keep.append(ps)
        else:
            raise ValueError(f"collect: form must be 'auto', 'mlp', 'rows' or 'tabular', got {form!r}")
        return pol, keep, f32

    def _collect_mlp(self, c, form, net, what):
        """The MLP form of an offsim_collect_policy / offsim_collect_value `c` from the _MLPNet `net` (`what` names it in the width
        error); returns the tensors to keep alive."""
        x_next, x_init = self._x_tables()
        if net.dO != x_next.shape[1]:
            raise ValueError(f"{what} takes observations of width {net.dO}, the log's have {x_next.shape[1]}")
        x_start = self.obs.reshape(self.num_envs, -1).to(x_next.dtype).contiguous()
        ws, arr = net._device_weights(self.table.device)  # (a population's stack: learner 0's descriptor of the stacked tensors)
        c.form, c.n_layers, c.layers_host = form, len(ws), C.cast(arr, C.POINTER(L.MLPLayer))
        c.activation, c.slope = _ACT[net.activation], net.slope
        c.x_dtype, c.dO = (L.F32 if x_next.dtype == torch.float32 else L.F16), net.dO
        c.x_start, c.x_next, c.x_init = L.ptr(x_start), L.ptr(x_next), L.ptr(x_init)
        return [x_start, x_next, x_init, ws]

    def _x_tables(self):
        """The log's observations as the in-kernel network reads them: next_obs / obs [N, dO], f16 kept, anything else f32 (MLPPolicy.forward's
        rule), made once."""
        if self._x_rows is None:
            dev = self.table.device
            self._x_rows = (obs_tensor(self._next_obs, dev), obs_tensor(self._obs, dev))
        return self._x_rows

    def _caller_tables(self, policy):
        """p_next [N, nA] / p_init [N, nA] in CALLER row order: the policy at next_obs / obs of every logged row (offsim_collect_policy's
        ROWS form; only initial rows of p_init are read)."""
        t = self.table
        if isinstance(policy, RowPolicy):
            return policy.caller_tables(t)
        pg, pk = policy.row_tables(t, self._obs, self._next_obs)  # grouped order / initial-row order
        pn = torch.zeros((t.N, t.nA), dtype=pg.dtype, device=t.device)
        p0 = torch.zeros((t.N, t.nA), dtype=pk.dtype, device=t.device)
        if t.N:
            pn[t.order.to(torch.int64)] = pg
        if t.N0:
            p0[t.init_orig.to(torch.int64)] = pk
        if pn.dtype != p0.dtype:
            pn, p0 = pn.to(torch.float64), p0.to(torch.float64)
        return pn.contiguous(), p0.contiguous()


class VectorPSRS(_Collector):
    def __init__(self, dataset, num_envs, num_states=None, encoder=None, device=None, strict=False):
        # the validation of per_state_rejection.py:16-25
        if not is_discrete(dataset.observation_space) and num_states is None and encoder is None:
            raise ValueError("PerStateRejectionSampling only supports discrete observation spaces")
        if (num_states is None or encoder is None) and (num_states != encoder):
            raise ValueError("num_states and encoder either both need to be None, or both need to be specified")
        if not is_discrete(dataset.action_space):
            raise ValueError("PerStateRejectionSampling currently only supports discrete action spaces")
        e = dataset.experience
        if encoder is not None:
            zs, next_zs = np.asarray(encoder.encode(e["observations"])), np.asarray(encoder.encode(e["next_observations"]))
        else:
            zs, next_zs = np.asarray(e["observations"]), np.asarray(e["next_observations"])
        n = len(zs)
        t0 = (np.asarray(e["steps"]) == 0) if "steps" in e else None
        self.num_envs = int(num_envs)
        self.strict = bool(strict)  # raise KeyError like the reference (costs a host sync per call); otherwise such environments just stop
        self.table = TransitionTable(zs, e["actions"], e["rewards"], next_zs, e["terminals"],
                                     np.asarray(e["action_distributions"]).reshape(n, -1), t0, device=device)
        dev = self.table.device
        self.env = BatchedPSRS(self.table, self.num_envs)
        self._init_payload(dataset, encoder is not None)

    # ---- the simulator's part of collect / collect_ppo / collect_ppo_population (_Collector) ----
    def _launch_collect(self, pol, f32, T, cap, st, out, ppo, learners):
        """offsim_vector_collect (ppo None), offsim_vector_collect_ppo, or offsim_vector_collect_ppo_pop for `learners` learners"""
        env, t = self.env, self.table
        if ppo is None:
            L.check(L.load().offsim_vector_collect(C.byref(t.c), C.byref(env.state.c), C.byref(pol), L.PROB_F32 if f32 else L.PROB_F64,
                                                   env.reject_mode, T, cap, C.byref(st), C.byref(out), L.stream_ptr()))
        elif learners is not None:
            L.check(L.load().offsim_vector_collect_ppo_pop(C.byref(t.c), C.byref(env.state.c), C.byref(pol), C.byref(ppo[0]), learners,
                                                           self.num_envs // learners, L.PROB_F32 if f32 else L.PROB_F64, env.reject_mode, T, cap,
                                                           C.byref(st), C.byref(out), C.byref(ppo[1]), L.stream_ptr()))
        else:
            L.check(L.load().offsim_vector_collect_ppo(C.byref(t.c), C.byref(env.state.c), C.byref(pol), C.byref(ppo[0]),
                                                       L.PROB_F32 if f32 else L.PROB_F64, env.reject_mode, T, cap, C.byref(st), C.byref(out),
                                                       C.byref(ppo[1]), L.stream_ptr()))
        return None

    def _raise_keyerror(self, status, drawn):
        k = int(torch.nonzero(status == L.ST_KEYERROR)[0])
        raise KeyError(self.table.z_of(int(self.env.state.cur_slot[k])))

    def _policy_f32(self, dtype):
        """p_new is compared in f32 where the policy's probabilities and p_log are both f32 (step_and_reset's rule)"""
        return dtype == torch.float32 and self.table.p_log.dtype == torch.float32

    def _tabular_policy(self, pi, f32):
        t = self.table
        if t.N and pi.shape[0] <= int(t.slot_z.max()):
            raise IndexError("pi has no row for some latent state")
        return torch.from_numpy(np.ascontiguousarray(t.policy_slots(pi).astype(np.float32 if f32 else np.float64))).to(t.device)

    def reset_sampler(self, seeds, rejection="pcg64"):
        """PSRS.reset_sampler(seed_k) for every environment (rejection: BatchedPSRS.reset_sampler's provider of the rejection stream)."""
        self.env.reset_sampler(seeds, rejection=rejection)
        self._sbuf.zero_()  # alive and ep_t
        if self.strict:  # (strict mode synchronises with the host anyway: a sampler reset that gave up a bounded wait raises here)
            self.check_faults()

    def check_faults(self):
        """Synchronise and raise OffsimError if the sampler reset gave up a bounded wait (include/offsim.h: offsim_async_faults).  With
        strict=False nothing synchronises with the host, so the caller does this once after reset_sampler (or whenever it reads results)."""
        self.env.check_faults()

    def reset(self, mask=None):
        """PSRS.reset (psrs.py:32-37) for the environments in `mask` (all if None).  Returns (obs [R, ...], alive [R])."""
        return self._reset_envs(mask)

    def step_dist_batch(self, action_dists):
        """per_state_rejection.py:85-95 for every environment at once.  action_dists: [R, nA] probabilities (tensor / array /
        torch Distribution with .probs).  Returns device tensors (action, next_obs, reward, done, alive) -- the environment's own
        buffers, overwritten by the next call (clone what has to outlive it); entries of environments with alive == False are
        meaningless (the reference returns the all-None tuple there; action / reward keep their last value, done is False)."""
        if isinstance(action_dists, Distribution):
            action_dists = action_dists.probs
        row, status, _ = self.env.step(action_dists)
        if self.strict and bool((status == L.ST_KEYERROR).any()):  # psrs.py:44: the state has no queue
            k = int(torch.nonzero(status == L.ST_KEYERROR)[0])
            raise KeyError(self.table.z_of(int(self.env.state.cur_slot[k])))
        L.check(L.load().offsim_vector_gather(L.ptr(row), L.ptr(status), None, self.num_envs, self._cols_step, len(self._cols_step),
                                              L.ptr(self.alive), L.stream_ptr()))
        return self.action, self.obs, self.reward, self.done, self.alive

    def step_and_reset(self, action_dists):
        """step_dist_batch followed by reset(mask=done) -- a whole driver iteration of the environments -- as ONE launch
        (offsim_vector_step).  Returns (action, obs, reward, done, alive): obs is the next observation, or the initial observation of
        the next episode where `done`; the same buffers as step_dist_batch's."""
        if isinstance(action_dists, Distribution):
            action_dists = action_dists.probs
        env, t = self.env, self.table
        env._orders_for_generic()
        p = action_dists if isinstance(action_dists, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(action_dists))
        f32 = p.dtype == torch.float32 and t.p_log.dtype == torch.float32
        p = p.to(device=t.device, dtype=torch.float32 if f32 else torch.float64).reshape(self.num_envs, t.nA).contiguous()
        L.check(L.load().offsim_vector_step(C.byref(t.c), C.byref(env.state.c), L.ptr(p), L.PROB_F32 if f32 else L.PROB_F64, env.reject_mode,
                                            self._cols_step, len(self._cols_step), self._cols_reset, len(self._cols_reset), L.ptr(self.alive),
                                            L.ptr(env._row), L.ptr(env._status), L.stream_ptr()))
        if self.strict and bool((env._status == L.ST_KEYERROR).any()):
            k = int(torch.nonzero(env._status == L.ST_KEYERROR)[0])
            raise KeyError(self.table.z_of(int(env.state.cur_slot[k])))
        self._keep = p
        return self.action, self.obs, self.reward, self.done, self.alive

    def graph_iteration(self, dist_fn, warmup=3, fused=True):
        """Capture one driver iteration in a HIP graph: probs = dist_fn(self.obs); step_and_reset(probs) (fused=False: the four
        launches of step_dist_batch(probs); reset(mask=done)).
        Returns (graph, (action, reward, done)): every graph.replay() advances all environments by one step and leaves the
        step's outputs in those three tensors (and in self.obs / self.alive).  `warmup` eager iterations run first on a side
        stream (PyTorch's capture recipe; they are real steps of the environments).  strict must be False."""
        if self.strict:
            raise ValueError("graph capture needs strict=False (the KeyError check synchronises with the host)")

        def iteration():
            if fused:  # one launch for the environments' whole iteration
                a, _, r, done, _ = self.step_and_reset(dist_fn(self.obs))
                return a, r, done
            a, _, r, done, _ = self.step_dist_batch(dist_fn(self.obs))
            self.reset(mask=done)
            return a, r, done

        side = torch.cuda.Stream(device=self.table.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(warmup):
                iteration()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g), torch.no_grad():
            outs = iteration()
        return g, outs

Collected = namedtuple("Collected", "obs probs row action reward next_obs terminated truncated reset alive final_obs status")
