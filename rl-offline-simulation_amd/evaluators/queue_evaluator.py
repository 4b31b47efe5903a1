"""QueueEvaluator (offsim4rl/evaluators/queue_evaluator.py:8-131) on the device tables.

Queues are keyed by (z, a); the agent samples its own action and the simulator pops the head of queue (z, a) -- no
rejection.  That is the PSRS machinery with the composite key z*nA + a as the grouping state and the "always accept,
pop one" rule: offsim_group_by_state / offsim_shuffle_queues / offsim_env_set_state / offsim_step_batch are reused as is.

Whole rollouts -- the reference's tabular drivers evalMC / qlearn / expSARSA (offsim4rl/agents/tabular.py), which draw the action
themselves and pop one row per step -- run in offsim_eval_queue (csrc/eval_queue.hpp), one launch: BatchedQueueEvaluator.eval_mc /
eval_td, evalmc_rollouts_queue for many sampler seeds, and the drop-ins evalMC_queue / qlearn_queue / expSARSA_queue on a QueueEvaluator.
Many learners on the same seeds in one launch (offsim_eval_queue_pop, csrc/td_pop.hpp): BatchedQueueEvaluator.eval_td_population,
driven over seed tiles by TDPopulation.run_queue (evaluators/td_population.py).

Policies over observations (evaluators/obs_policy.py: the PPO actor, ppo.py:258-279) are evaluated by offsim_eval_queue_rows_policy
(csrc/eval_queue_rows.hpp) from their per-row tables: BatchedQueueEvaluator.eval_mc_rows_policy, evalmc_rollouts_queue and evalMC_queue with
an ObsPolicy; L of them on the same seeds in one launch (offsim_eval_queue_rows_policy_pop): eval_mc_rows_policy_population and
evalmc_rollouts_queue_population.
"""
import ctypes as C
import os

import numpy as np
import torch

from .. import _lib as L
from ..spaces import is_discrete
from ..table import TransitionTable, gather_rows
from .psrs import BatchedPSRS, SHUFFLE_PER_ROLLOUT, _behaviour_kind, _schedule
from .obs_policy import MLPPolicy, ObsPolicy, PolicyPopulation
from .rollout_io import (HOST_KEYS, _gamma_pow, collect_host, episode_bound, host_result, population_host_result, population_result, population_state,
                         rollout_outputs, seed_tiles, td_outputs, td_population_launch, tie_stream)


class BatchedQueueEvaluator:
    """R independent QueueEvaluator_impl environments (queue_evaluator.py:90-131) over one table."""

    def __init__(self, z, a, r, z_next, done, p_log, t0=None, R=1, device=None):
        z = np.asarray(z, np.int64)
        a = np.asarray(a, np.int64)
        z_next = np.asarray(z_next, np.int64)
        self.nA = int(np.asarray(p_log).reshape(len(z), -1).shape[1]) if len(z) else 1
        self.z_lo = int(min(z.min(), z_next.min(), 0)) if len(z) else 0
        nA = self.nA
        comp = (z - self.z_lo) * nA + a                      # sorted(buffer, key=(z, a)), queue_evaluator.py:105
        comp_next = (z_next - self.z_lo) * nA                # base slot of the next state; the action is added per step
        self.table = TransitionTable(comp, a, r, comp_next, done, p_log, t0, device=device)
        t = self.table
        # the init queue holds (z, s): its slot is the base slot of z, not the composite of the logged action
        t.init_slot = (torch.div(t.init_slot, nA, rounding_mode="floor") * nA).to(torch.int32).contiguous()
        t.c.init_slot = L.ptr(t.init_slot)
        # whole states: empty segments up to the next multiple of nA (a step into them is the KeyError it was beyond the last slot), so
        # that the table is [nZ, nA] for the one-launch drivers (offsim_eval_queue)
        if t.z_base is not None and t.n_slots % nA:
            pad = nA - t.n_slots % nA
            t.seg_off = torch.cat([t.seg_off, t.seg_off[-1:].expand(pad)]).contiguous()
            t.n_slots += pad
            t.slot_z = np.arange(t.z_base, t.z_base + t.n_slots, dtype=np.int64)
            t.c.n_slots, t.c.seg_off = t.n_slots, L.ptr(t.seg_off)
        self.nZ = t.n_slots // nA if t.z_base is not None else None
        self.R = int(R)
        self.env = BatchedPSRS(t, R, L.REJECT_NEVER)
        self._dummy_p = torch.zeros((R, nA), dtype=torch.float64, device=t.device)
        self.cur_row = torch.full((R,), -1, dtype=torch.int32, device=t.device)  # eval_mc_rows_policy: the table row each rollout stands at

    def reset_sampler(self, seeds):
        self.env.reset_sampler(seeds, SHUFFLE_PER_ROLLOUT)
        self.cur_row.fill_(-1)

    def set_action_seeds(self, seeds):
        """The action streams of the one-launch drivers: rollout i draws its actions from default_rng(seeds[i]) (tabular.py:75, :145, :248).
        reset_sampler leaves them at the sampler seeds."""
        self.env.set_rejection_seeds(seeds, "pcg64")

    # -- the tabular drivers (offsim4rl/agents/tabular.py) for all rollouts in one launch: offsim_eval_queue --
    def state_rows(self, tab, fill=np.nan):
        """A [nS, nA] table indexed by the state as the reference does (tab[z], NumPy's wrap for z = -1) as the [nZ, nA] rows of this
        table's states, row z - z_lo; `fill` where tab has no row."""
        tab = np.asarray(tab, dtype=np.float64)
        zs = self.z_lo + np.arange(self.nZ)
        idx = np.where(zs < 0, zs + tab.shape[0], zs)
        ok = (idx >= 0) & (idx < tab.shape[0])
        out = np.full((self.nZ, self.nA), fill, dtype=np.float64)
        out[ok] = tab[idx[ok]]
        return out

    def rows_to_state(self, rows, tab):
        """rows [..., nZ, nA] back into copies of the [nS, nA] table `tab` (rows of tab without a state here keep their values)."""
        rows = np.asarray(rows)
        out = np.broadcast_to(np.asarray(tab, dtype=np.float64), rows.shape[:-2] + np.shape(tab)).copy()
        for i in range(self.nZ):
            z = self.z_lo + i
            if -out.shape[-2] <= z < out.shape[-2]:
                out[..., z, :] = rows[..., i, :]
        return out

    def _run(self, pi, gamma, n_episodes, ep_cap, trace_cap, n_gamma_pow, td):
        if self.nZ is None:
            raise L.OffsimError("the one-launch queue drivers need dense state ids (this log's ids were compacted to ranks)")
        env, t = self.env, self.table
        env._quiesce()
        env._orders_for_generic()
        dev, R, nZ, nA = t.device, self.R, self.nZ, self.nA
        pi_d = None
        if pi is not None:
            pi_d = torch.as_tensor(pi if isinstance(pi, torch.Tensor) else np.ascontiguousarray(pi), dtype=torch.float64).to(dev).reshape(nZ, nA).contiguous()
        o, oc = rollout_outputs(R, dev, ep_cap, trace_cap)
        o["obs_row"] = torch.full((R,), -(1 << 31), dtype=torch.int32, device=dev)
        tdc, keep, reseed, episode0 = None, (), 0, 0
        if td is not None:
            q = td["q"]
            q = torch.zeros((R, nZ, nA), dtype=torch.float64, device=dev) if q is None else \
                torch.as_tensor(q, dtype=torch.float64).to(dev).reshape(R, nZ, nA).contiguous().clone()
            behaviour = int(td["behaviour"])
            td_outputs(o, q, trace_cap, td["snap_cap"], beh_arg=behaviour == L.BEHAVIOUR_EPS_GREEDY)
            a_ep, e_ep = (None if x is None else torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).to(dev) for x in (td["alpha_ep"], td["epsilon_ep"]))
            n_sched = max(a_ep.numel() if a_ep is not None else 0, e_ep.numel() if e_ep is not None else 0)
            assert all(x is None or x.numel() == n_sched for x in (a_ep, e_ep)), "alpha_ep and epsilon_ep cover the same episodes"
            tie, mt = td["tie"], None
            if isinstance(tie, str) and tie == "episode":
                reseed, episode0 = 1, int(td["episode0"])
                mt = torch.zeros((R, 625), dtype=torch.int32, device=dev)
                mt[:, 624] = 624
            elif tie is not None and not (isinstance(tie, str) and tie == "first"):
                mt = tie_stream(tie, dev).reshape(R, 625).contiguous()
            if mt is not None:
                o["tie_mt"] = mt
            tdc = L.TD(mode=int(td["mode"]), alpha=float(td["alpha"]), q=L.ptr(q), td_err=L.ptr(o.get("td_err")), td_cap=trace_cap, behaviour=behaviour,
                       epsilon=float(td["epsilon"]), alpha_ep=L.ptr(a_ep), epsilon_ep=L.ptr(e_ep), n_sched=n_sched, q_snap=L.ptr(o.get("q_snap")),
                       snap_cap=td["snap_cap"], snap_stride=max(int(td["snap_stride"]), 1), tie_mt=L.ptr(mt), beh_arg=L.ptr(o.get("beh_arg")))
            o["q"] = q
            keep = (a_ep, e_ep)
        gp = _gamma_pow(gamma, n_gamma_pow, dev, cap=t.N + 2)
        L.check(L.load().offsim_eval_queue(C.byref(t.c), C.byref(env.state.c), nA, L.ptr(pi_d), float(gamma), L.ptr(gp), gp.numel(),
                                           int(episode_bound(n_episodes)), C.byref(oc), None if tdc is None else C.byref(tdc), reseed, episode0,
                                           L.ptr(o["obs_row"]), L.stream_ptr()))
        o["_keepalive"] = (pi_d, gp) + keep
        o["_kernel"] = "k_eval_queue"
        return o

    def eval_mc(self, pi, gamma, n_episodes=None, ep_cap=0, trace_cap=0, n_gamma_pow=4096):
        """evalMC (tabular.py:247-270) on every rollout in one launch.  pi [nZ, nA] f64: the policy per state, row z - z_lo (state_rows).
        Returns a dict of device tensors: sum_g, n_ep, steps, cand, n_len, status, obs_row (+ ep_g, ep_len, trace_row and trace_pop --
        the action drawn at every step -- when asked)."""
        return self._run(pi, gamma, n_episodes, ep_cap, trace_cap, n_gamma_pow, None)

    def eval_td(self, pi, gamma, mode, alpha, q=None, n_episodes=None, ep_cap=0, trace_cap=0, n_gamma_pow=4096, behaviour=L.BEHAVIOUR_FIXED,
                epsilon=0.0, alpha_ep=None, epsilon_ep=None, snap_cap=0, snap_stride=1, tie=None, episode0=0):
        """qlearn / expSARSA (tabular.py:71-191; mode: _lib.TD_QLEARN | _lib.TD_EXPSARSA) on every rollout in one launch.  pi [nZ, nA]:
        the fixed behaviour (and expected SARSA's target); None for Q-learning with behaviour = _lib.BEHAVIOUR_EPS_GREEDY /
        BEHAVIOUR_SOFT_GREEDY, which act on the rollout's own Q row.  q [R, nZ, nA] (Q_init; zeros if None) comes back updated as
        out["q"]; td_err / beh_arg [R, trace_cap]; alpha_ep / epsilon_ep: per-episode schedules; snap_cap > 0: out["q_snap"].
        tie: None the first maximum; [R, 625] MT19937 states, advanced in place (out["tie_mt"]); "episode": the stream restarts as
        np.random.seed(episode0 + e) at the start of episode e, out["tie_mt"] is where it stands afterwards."""
        td = dict(mode=mode, alpha=alpha, q=q, behaviour=behaviour, epsilon=epsilon, alpha_ep=alpha_ep, epsilon_ep=epsilon_ep, snap_cap=int(snap_cap),
                  snap_stride=snap_stride, tie=tie, episode0=episode0)
        return self._run(pi, gamma, n_episodes, ep_cap, trace_cap, n_gamma_pow, td)

    def eval_td_population(self, mode, alpha, gamma, behaviour=L.BEHAVIOUR_FIXED, epsilon=0.0, pi=None, q=None, alpha_ep=None, epsilon_ep=None,
                           tie=None, episode0=0, n_episodes=None, ep_cap=0, trace_cap=0, snap_cap=0, snap_stride=1, n_gamma_pow=4096, state=False):
        """eval_td for L learners, each on every one of this environment's S = R rollouts (its sampler seeds and action streams): L * S
        rollouts in one launch that share the S queue orders (include/offsim.h, offsim_eval_queue_pop).  alpha, gamma, behaviour
        (_lib.BEHAVIOUR_*) and epsilon are each a scalar or [L]; pi [nZ,nA] or [L,nZ,nA] by state row (state_rows; None: uniform);
        q [nZ,nA], [L,...], [L,S,...] or None (zeros); alpha_ep / epsilon_ep [n_sched] or [L,n_sched].  L is the common length of the
        per-learner arguments (1 when every one is shared); lengths that disagree raise ValueError.  mode is one value for the launch.
        tie: None / "first" the first maximum; "episode": every rollout's stream restarts as np.random.seed(episode0 + e) at the start of
        episode e; [L,S,625] MT19937 states (copied: the caller's stay where they were).  out["tie_mt"] [L,S,625] is where the streams stand.
        Returns eval_td's dict with [L, S, ...] leading dimensions; entry [l, j] is, bit for bit, what eval_td gives rollout j under learner
        l's setting, for every behaviour.  It is a query: it runs on copies of the rollout state (every learner of seed j sees the same
        queues and starts from the same action stream), and this environment's own cursors, action streams and current slots are left as
        they were; with `state`, out["_state"] holds where every learner's rollouts stand afterwards (rng, cursor, init_cursor, cur_slot)."""
        if self.nZ is None:
            raise L.OffsimError("the one-launch queue drivers need dense state ids (this log's ids were compacted to ranks)")
        env, t = self.env, self.table
        env._quiesce()
        env._orders_for_generic()
        dev, S, nZ, nA = t.device, self.R, self.nZ, self.nA
        by_episode = isinstance(tie, str) and tie == "episode"
        if isinstance(tie, str) and tie not in ("episode", "first"):
            raise ValueError(f"eval_td_population: tie must be None, 'first', 'episode' or [L,S,625] states, got {tie!r}")
        n_l, o, oc, pc, keep = td_population_launch("eval_td_population", dev, S, nZ, nA, t.N, mode, alpha, gamma, behaviour, epsilon, pi, q, alpha_ep,
                                                    epsilon_ep, None if isinstance(tie, str) else tie, n_gamma_pow, ep_cap, trace_cap, snap_cap,
                                                    snap_stride, names=("pi", "q", "nZ"))
        R = n_l * S
        if by_episode:
            mt = o["tie_mt"] = torch.zeros((R, 625), dtype=torch.int32, device=dev)
            mt[:, 624] = 624
            pc.tie_mt = L.ptr(mt)
        o["obs_row"] = torch.full((R,), -(1 << 31), dtype=torch.int32, device=dev)
        ro, copies = population_state(env.state, n_l)
        L.check(L.load().offsim_eval_queue_pop(C.byref(t.c), C.byref(ro), nA, n_l, S, C.byref(pc), int(episode_bound(n_episodes)), C.byref(oc),
                                               1 if by_episode else 0, int(episode0), L.ptr(o["obs_row"]), L.stream_ptr()))
        return population_result(o, n_l, S, copies, keep, "k_eval_queue_pop", state=state)

    # -- evalMC for policies over observations (evaluators/obs_policy.py): offsim_eval_queue_rows_policy --
    def _row_tables(self, who, p_next, p_init, lead):
        """p_next [*lead, N, nA] and p_init [*lead, N0, nA] on the device, contiguous, f32 when both are (widened in the kernel), else f64"""
        t = self.table
        dt = torch.float32 if p_next.dtype == p_init.dtype == torch.float32 else torch.float64
        if tuple(p_next.shape) != (*lead, t.N, self.nA) or tuple(p_init.shape) != (*lead, t.N0, self.nA):
            raise ValueError(f"{who}: p_next {[*lead, t.N, self.nA]} and p_init {[*lead, t.N0, self.nA]} expected, got {tuple(p_next.shape)} and "
                             f"{tuple(p_init.shape)}")
        return p_next.to(device=t.device, dtype=dt).contiguous(), p_init.to(device=t.device, dtype=dt).contiguous(), L.F32 if dt == torch.float32 else L.F64

    def eval_mc_rows_policy(self, p_next, p_init, gamma, n_episodes=None, ep_cap=0, trace_cap=0, n_gamma_pow=4096):
        """evalMC (tabular.py:247-270) of a policy over observations on every rollout in one launch, on this environment's own state.
        p_next [N,nA]: the policy at next_obs of every GROUPED row (self.table.order); p_init [N0,nA]: at obs of every initial row
        (self.table.init_orig) -- what ObsPolicy.row_tables(self.table, obs, next_obs) returns, as it is.  f32 tables stay f32 and are widened
        in the kernel; anything else is f64.  Returns eval_mc's dict, and cur_row [R] (also kept as self.cur_row; reset_sampler sets it to
        -1): g >= 0 the last served grouped row, -2 - k initial row k with no step since, -1 none."""
        if self.nZ is None:
            raise L.OffsimError("the one-launch queue drivers need dense state ids (this log's ids were compacted to ranks)")
        env, t = self.env, self.table
        env._quiesce()
        env._orders_for_generic()
        dev, R = t.device, self.R
        pn, p0, dt = self._row_tables("eval_mc_rows_policy", p_next, p_init, ())
        o, oc = rollout_outputs(R, dev, ep_cap, trace_cap)
        o["obs_row"] = torch.full((R,), -(1 << 31), dtype=torch.int32, device=dev)
        o["cur_row"] = self.cur_row
        gp = _gamma_pow(gamma, n_gamma_pow, dev, cap=t.N + 2)
        L.check(L.load().offsim_eval_queue_rows_policy(C.byref(t.c), C.byref(env.state.c), self.nA, L.ptr(pn) if t.N else None, L.ptr(p0) if t.N0 else None,
                                                       dt, float(gamma), L.ptr(gp), gp.numel(), int(episode_bound(n_episodes)), C.byref(oc),
                                                       L.ptr(self.cur_row), L.ptr(o["obs_row"]), L.stream_ptr()))
        o["_keepalive"] = (pn, p0, gp)
        o["_kernel"] = "k_eval_queue_rows"
        return o

    def eval_mc_rows_policy_population(self, p_next, p_init, gamma, n_episodes=None, ep_cap=0, trace_cap=0, n_gamma_pow=4096, state=False):
        """eval_mc_rows_policy for L policies, each on every one of this environment's S = R rollouts (its sampler seeds and action
        streams): L * S rollouts in one launch that share the S queue orders (include/offsim.h, offsim_eval_queue_rows_policy_pop).
        p_next [L,N,nA], p_init [L,N0,nA]: the tables stacked (PolicyPopulation.row_tables).  Returns eval_mc_rows_policy's dict with [L, S]
        leading dimensions; entry [l, j] is, bit for bit, what eval_mc_rows_policy gives rollout j with policy l.  It is a query: it runs
        on copies of the rollout state, and this environment's own cursors, action streams, current slots and cur_row are left as they
        were; with `state`, out["_state"] holds where every policy's rollouts stand afterwards."""
        if self.nZ is None:
            raise L.OffsimError("the one-launch queue drivers need dense state ids (this log's ids were compacted to ranks)")
        env, t = self.env, self.table
        env._quiesce()
        env._orders_for_generic()
        dev, S = t.device, self.R
        if p_next.dim() != 3 or p_init.dim() != 3 or p_next.shape[0] != p_init.shape[0] or p_next.shape[0] < 1:
            raise ValueError(f"eval_mc_rows_policy_population: p_next [L,N,nA] and p_init [L,N0,nA] expected, got {tuple(p_next.shape)} and "
                             f"{tuple(p_init.shape)}")
        n_pol = int(p_next.shape[0])
        R = n_pol * S
        pn, p0, dt = self._row_tables("eval_mc_rows_policy_population", p_next, p_init, (n_pol,))
        o, oc = rollout_outputs(R, dev, ep_cap, trace_cap)
        o["obs_row"] = torch.full((R,), -(1 << 31), dtype=torch.int32, device=dev)
        o["cur_row"] = self.cur_row.repeat(n_pol)
        ro, copies = population_state(env.state, n_pol)
        gp = _gamma_pow(gamma, n_gamma_pow, dev, cap=t.N + 2)
        L.check(L.load().offsim_eval_queue_rows_policy_pop(C.byref(t.c), C.byref(ro), self.nA, L.ptr(pn) if t.N else None, L.ptr(p0) if t.N0 else None,
                                                           dt, n_pol, S, float(gamma), L.ptr(gp), gp.numel(), int(episode_bound(n_episodes)),
                                                           C.byref(oc), L.ptr(o["cur_row"]), L.ptr(o["obs_row"]), L.stream_ptr()))
        return population_result(o, n_pol, S, copies, (pn, p0, gp), "k_eval_queue_rows_pop", state=state)

    def reset(self, mask=None):
        return self.env.reset(mask)

    def step(self, actions):
        """actions [R] int: pops the head of queue (z, a) for every rollout; returns device tensors (row, status).
        status: 0 ok, 1 queue empty (None), 3 KeyError (no such (z, a) queue), 4 no current state."""
        st = self.env.state
        act = torch.as_tensor(np.asarray(actions), dtype=torch.int32).to(self.table.device)
        base = st.cur_slot
        comp = torch.where(base >= 0, base + act, base).to(torch.int32).contiguous()
        self.env.set_state(comp)
        row, status, _ = self.env.step(self._dummy_p, advance=True, reject_mode=L.REJECT_NEVER)
        # a rollout whose pop failed keeps its state (queue_evaluator.py:122-123): undo the composite slot
        failed = status != L.ST_OK
        if bool(failed.any()):
            self.env.set_state(base.clone(), mask=failed)
        return row, status


class QueueEvaluator:
    """Drop-in for offsim4rl.evaluators.queue_evaluator.QueueEvaluator (queue_evaluator.py:8-88)."""

    def __init__(self, dataset, num_states=None, encoder=None):
        if not is_discrete(dataset.observation_space) and num_states is None and encoder is None:
            raise ValueError("QueueEvaluator only supports discrete observation spaces")
        if (num_states is None or encoder is None) and (num_states != encoder):
            raise ValueError("num_states and encoder either both need to be None, or both need to be specified")
        if not is_discrete(dataset.action_space):
            raise ValueError("QueueEvaluator currently only supports discrete action spaces")
        self._dataset = dataset
        e = dataset.experience
        if encoder is not None:
            zs, next_zs = np.asarray(encoder.encode(e["observations"])), np.asarray(encoder.encode(e["next_observations"]))
        else:
            zs, next_zs = np.asarray(e["observations"]), np.asarray(e["next_observations"])
        n = len(zs)
        t0 = (np.asarray(e["steps"]) == 0) if "steps" in e else None
        p_log = np.asarray(e["action_distributions"]).reshape(n, -1) if "action_distributions" in e else np.zeros((n, dataset.action_space.n))
        self._arrays = (zs, e["actions"], e["rewards"], next_zs, e["terminals"], p_log, t0)
        self._impl = BatchedQueueEvaluator(*self._arrays, R=1)
        self._z, self._zn = zs, next_zs
        self.nS = num_states if num_states is not None else 25
        self.nA = dataset.action_space.n
        self.s, self.z = None, None
        self.reset_sampler()
        self.reset()

    @property
    def observation_space(self):
        return self._dataset.observation_space

    @property
    def action_space(self):
        return self._dataset.action_space

    def reset_sampler(self, seed=None):
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little")
        self._impl.reset_sampler([seed])

    def reset(self, seed=None):
        row = int(self._impl.reset().cpu()[0])
        if row < 0:
            self.s = None
            return None
        self.z = int(self._z[row])
        self.s = self._dataset.experience["observations"][row]
        return self.s

    def step(self, action):
        z = self.z
        a = int(action)
        if a < 0 or a >= self._impl.nA:
            raise KeyError((z, a))
        row, status = self._impl.step([a])
        row, status = int(row.cpu()[0]), int(status.cpu()[0])
        if status == L.ST_KEYERROR:
            raise KeyError((z, a))
        if status != L.ST_OK:
            return None, None, None, None
        e = self._dataset.experience
        self.s, self.z = e["next_observations"][row], int(self._zn[row])
        p = e["action_distributions"][row] if "action_distributions" in e else None
        return self.s, e["rewards"][row], bool(e["terminals"][row]), {"z": z, "next_z": self.z, "a": int(e["actions"][row]), "p": p}

    def step_dist(self, action_dist):
        a = action_dist.sample()
        next_obs, r, done, info = self.step(a)
        if next_obs is None:
            return None, None, None, None, None
        return info["a"], next_obs, r, done, info


# ---------------------------------------------------------------------------------------------------
# Many sampler seeds per launch
# ---------------------------------------------------------------------------------------------------
def _queue_arrays(env_or_arrays):
    return env_or_arrays._arrays if isinstance(env_or_arrays, QueueEvaluator) else tuple(env_or_arrays)


def _queue_obs(who, env_or_arrays, obs, next_obs, needed):
    """the log's observations for a policy over observations: the caller's, or a QueueEvaluator's own dataset's"""
    if (obs is None or next_obs is None) and isinstance(env_or_arrays, QueueEvaluator):
        e = env_or_arrays._dataset.experience
        obs, next_obs = e["observations"], e["next_observations"]
    if (obs is None or next_obs is None) and needed:
        raise ValueError(f"{who}: a policy over observations needs the log's obs= and next_obs=")
    return obs, next_obs


def evalmc_rollouts_queue(env_or_arrays, seeds, pi, gamma, n_episodes=None, action_seeds=None, tile=None, obs=None, next_obs=None):
    """evalMC (tabular.py:247-270) on the queue simulator for many sampler seeds, one launch per tile of seeds.  `env_or_arrays`: a
    QueueEvaluator, or the columns (z, a, r, z_next, done, p_log, t0) BatchedQueueEvaluator takes.  `pi` [nS, nA] is indexed by the state
    as the reference does; rollout i shuffles its queues with seeds[i] and draws its actions from default_rng(action_seeds[i])
    (default: seeds).  Returns the dictionary of evalmc_rollouts_exo: host arrays sum_g, n_ep, steps, cand, status and
    value = sum_g / n_ep.
    `pi` may also be a policy over observations (evaluators/obs_policy.py: MLPPolicy, RowPolicy, CallablePolicy) with the log's observations
    `obs` / `next_obs` [N, dO] in caller order (default: the QueueEvaluator's dataset's): its per-row tables are computed once and every
    tile is one launch of offsim_eval_queue_rows_policy."""
    seeds = np.asarray(seeds, dtype=np.uint64)
    action_seeds = seeds if action_seeds is None else np.asarray(action_seeds, dtype=np.uint64)
    if len(action_seeds) != len(seeds):
        raise ValueError("evalmc_rollouts_queue: one action seed per sampler seed")
    arrays = _queue_arrays(env_or_arrays)
    rows = isinstance(pi, ObsPolicy)
    if rows:
        obs, next_obs = _queue_obs("evalmc_rollouts_queue", env_or_arrays, obs, next_obs, not hasattr(pi, "p_next"))
    tile = len(seeds) if tile is None else int(tile)
    outs, tables = {k: [] for k in HOST_KEYS}, None
    for b, sd, env in seed_tiles(seeds, max(tile, 1), lambda n: BatchedQueueEvaluator(*arrays, R=n)):
        env.reset_sampler(sd)
        env.set_action_seeds(action_seeds[b:b + len(sd)])
        if rows and tables is None:  # (every environment of the same columns groups them alike)
            tables = pi.row_tables(env.table, obs, next_obs)
        collect_host(outs, env.eval_mc_rows_policy(*tables, gamma, n_episodes) if rows else env.eval_mc(env.state_rows(pi), gamma, n_episodes))
    return host_result(outs, empty=0)


def evalmc_rollouts_queue_population(env_or_arrays, seeds, policies, gamma, n_episodes=None, action_seeds=None, tile=None, policy_tile=None,
                                     obs=None, next_obs=None):
    """evalMC on the queue simulator of L policies over observations on the same S sampler seeds: evalmc_rollouts_population (batched.py) on
    QueueEvaluator.  Every policy sees the same queue orders and the same action streams (default_rng(action_seeds[i]); default: seeds), so
    the differences between policies are paired.  `policies`: a PolicyPopulation, or a list of policies over observations (MLPPolicy's of
    one architecture are stacked, anything else goes through its own row tables); obs / next_obs [N, dO]: the log's observations in caller
    order (default: the QueueEvaluator's dataset's).  One sampler reset per tile of `tile` seeds (default: all), and per seed tile one
    forward launch and one launch of offsim_eval_queue_rows_policy_pop per tile of `policy_tile` policies (default: as many as keep the
    [L, N + N0, nA] tables within a quarter of the free memory; with more than one policy tile the tables are recomputed per seed tile).
    Returns evalmc_rollouts_population's dictionary: host arrays [L, S] sum_g, n_ep, steps, cand, status, value; mean_value [L]; best."""
    seeds = np.asarray(seeds, dtype=np.uint64)
    action_seeds = seeds if action_seeds is None else np.asarray(action_seeds, dtype=np.uint64)
    if len(action_seeds) != len(seeds):
        raise ValueError("evalmc_rollouts_queue_population: one action seed per sampler seed")
    if not isinstance(policies, PolicyPopulation):
        policies = list(policies)
        policies = PolicyPopulation.from_policies(policies) if policies and all(isinstance(p, MLPPolicy) for p in policies) else PolicyPopulation.from_rows(policies)
    n_pol = len(policies)
    arrays = _queue_arrays(env_or_arrays)
    obs, next_obs = _queue_obs("evalmc_rollouts_queue_population", env_or_arrays, obs, next_obs, policies.needs_obs())
    tile = len(seeds) if tile is None else int(tile)
    outs, tables = {k: [] for k in HOST_KEYS}, None
    for b, sd, env in seed_tiles(seeds, max(tile, 1), lambda n: BatchedQueueEvaluator(*arrays, R=n)):
        t = env.table
        if policy_tile is None:
            per_policy = max(1, (int(t.N) + int(t.N0)) * int(t.nA) * 8)
            policy_tile = (torch.cuda.mem_get_info(t.device)[0] // 4) // per_policy
        policy_tile = int(max(1, min(n_pol, policy_tile)))
        env.reset_sampler(sd)
        env.set_action_seeds(action_seeds[b:b + len(sd)])
        if tables is None and policy_tile >= n_pol:  # (one policy tile: computed once)
            tables = policies.row_tables(t, obs, next_obs)
        cols = {k: [] for k in HOST_KEYS}
        for lo in range(0, n_pol, policy_tile):
            p_next, p_init = tables if tables is not None else policies.row_tables(t, obs, next_obs, lo, min(n_pol, lo + policy_tile))
            collect_host(cols, env.eval_mc_rows_policy_population(p_next, p_init, gamma, n_episodes))
        for k in HOST_KEYS:
            outs[k].append(np.concatenate(cols[k], axis=0))
    return population_host_result(outs, n_pol)


# ---------------------------------------------------------------------------------------------------
# The reference's tabular drivers (offsim4rl/agents/tabular.py) on a QueueEvaluator, one launch each
# ---------------------------------------------------------------------------------------------------
def _launch_queue(env, what, seed, run, by_state=True):
    """One driver call on `env`: the action stream default_rng(seed) (tabular.py:75, :145, :248; None: OS entropy), the launch on the
    environment's own rollout state, the KeyError the reference raises, and env.s / env.z as its loop leaves them."""
    from .psrs import _all_equal
    if not isinstance(env, QueueEvaluator):
        raise TypeError(f"{what}: `env` must be the device-backed QueueEvaluator of this package, got {type(env).__name__}")
    e = env._dataset.experience
    if by_state and not (_all_equal(e["observations"], env._z) and _all_equal(e["next_observations"], env._zn)):
        raise NotImplementedError(f"{what}: the observations of this QueueEvaluator differ from its states, but the tabular drivers index their "
                                  "tables by the observation (tabular.py:119, :171, :258)")
    impl = env._impl
    impl.set_action_seeds([int.from_bytes(os.urandom(8), "little") if seed is None else int(seed)])
    o = run(impl)
    status, row, steps = int(o["status"].cpu()[0]), int(o["obs_row"].cpu()[0]), int(o["steps"].cpu()[0])
    L.check_async_faults()  # (the copies above synchronised the stream)
    if row == -1:
        env.s = None
    elif row >= 0:
        env.s, env.z = e["next_observations"][row], int(env._zn[row])
    elif row > -(1 << 31):
        env.s, env.z = e["observations"][-2 - row], int(env._z[-2 - row])
    if status == L.ST_KEYERROR:
        a = int(o["trace_pop"].cpu()[0, steps])
        if a >= impl.nA:
            raise IndexError(f"{what}: the policy has no distribution for state {env.z}")
        raise KeyError((env.z, a))
    return o, status, steps


def evalMC_queue(env, n_episodes, pi, gamma, seed=None):
    """tabular.py:247-270 on a QueueEvaluator: the whole loop -- env.reset(), A = rng.choice(nA, p=pi[S]), env.step(A), discounted returns
    -- in one kernel launch: (Gs, lengths).  A queue that runs out ends the run (the reference's loop does not survive it): Gs holds the
    completed episodes, lengths also the cut-short one.
    `pi` may be a policy over observations (evaluators/obs_policy.py): p = pi(S) with S the dataset's own observation, whatever the
    encoder makes of it (what evalMC_psrs does for PSRS); its per-row tables are computed once, then offsim_eval_queue_rows_policy runs
    the loop.  A [nS, nA] table needs observations that are the states (NotImplementedError otherwise)."""
    if isinstance(pi, ObsPolicy):
        e, t = env._dataset.experience, env._impl.table
        n_ep = int(min(n_episodes, t.N0 + 1))
        p_next, p_init = pi.row_tables(t, e["observations"], e["next_observations"])
        o, _, _ = _launch_queue(env, "evalMC_queue", seed, lambda b: b.eval_mc_rows_policy(p_next, p_init, gamma, n_ep, ep_cap=max(n_ep, 1),
                                                                                           trace_cap=t.N + 1), by_state=False)
        ne, nl = int(o["n_ep"].cpu()[0]), int(o["n_len"].cpu()[0])
        return o["ep_g"].cpu().numpy()[0, :ne].copy(), o["ep_len"].cpu().numpy()[0, :nl].astype(np.int64)
    pi = np.asarray(pi, dtype=np.float64)
    if pi.ndim != 2:
        raise ValueError("evalMC_queue: pi must be a [nS, nA] table")
    t = env._impl.table
    n_ep = int(min(n_episodes, t.N0 + 1))
    o, _, _ = _launch_queue(env, "evalMC_queue", seed, lambda b: b.eval_mc(b.state_rows(pi), gamma, n_ep, ep_cap=max(n_ep, 1), trace_cap=t.N + 1))
    ne, nl = int(o["n_ep"].cpu()[0]), int(o["n_len"].cpu()[0])
    return o["ep_g"].cpu().numpy()[0, :ne].copy(), o["ep_len"].cpu().numpy()[0, :nl].astype(np.int64)


class _QueueStepMemory:
    """The `memory` list of the learner drivers: (S, A, R, S', done, p, {**info, 't': t}) per step (tabular.py:122, :174), p the
    distribution the action was drawn from.  Built on first use."""

    def __init__(self, env, rows, p_of_step):
        self._env, self._rows, self._p_of_step, self._items = env, rows, p_of_step, None

    def _build(self):
        if self._items is None:
            env, e, ps, items, t = self._env, self._env._dataset.experience, self._p_of_step(), [], 0
            for i, r in enumerate(self._rows):
                p_log = e["action_distributions"][r] if "action_distributions" in e else None
                info = {"z": int(env._z[r]), "next_z": int(env._zn[r]), "a": int(e["actions"][r]), "p": p_log, "t": t}
                done = bool(e["terminals"][r])
                items.append((e["observations"][r], int(e["actions"][r]), e["rewards"][r], e["next_observations"][r], done, ps[i], info))
                t = 0 if done else t + 1
            self._items = items
        return self._items

    def __len__(self):
        return len(self._rows)

    def __iter__(self):
        return iter(self._build())

    def __getitem__(self, i):
        return self._build()[i]


def _td_queue(env, what, n_episodes, gamma, alpha, epsilon, Q_init, save_Q, mode, kind, pi_tab, seed, tie):
    """One launch of offsim_eval_queue for a learner driver call; returns (Q, info) as the reference does."""
    impl = env._impl
    t, nA = impl.table, env.nA
    Q0 = np.zeros((env.nS, nA)) if Q_init is None else np.asarray(Q_init).copy().astype(float)
    n_ep = int(min(n_episodes, t.N0 + 1))
    a_tab, e_tab = _schedule(alpha, n_ep), _schedule(epsilon, n_ep)
    if kind == "greedy":
        e_tab, epsilon = None, 0.0
    behaviour = {"fixed": L.BEHAVIOUR_FIXED, "eps_greedy": L.BEHAVIOUR_EPS_GREEDY, "greedy": L.BEHAVIOUR_EPS_GREEDY,
                 "soft_greedy": L.BEHAVIOUR_SOFT_GREEDY}[kind]
    if a_tab is not None and e_tab is None:
        e_tab = np.full(len(a_tab), float(epsilon) if not callable(epsilon) else 0.0)
    if e_tab is not None and a_tab is None:
        a_tab = np.full(len(e_tab), float(alpha))
    st = np.random.get_state()
    if tie == "global":  # _random_argmax draws from NumPy's global stream as it stands: the device continues it
        if st[0] != "MT19937":
            raise NotImplementedError("np.random's global bit generator is not MT19937")
        tie = np.concatenate([np.asarray(st[1], dtype=np.uint32), np.array([st[2]], dtype=np.uint32)])[None, :]
    elif tie not in ("episode", "first", None):
        raise ValueError(f"{what}: tie must be 'episode', 'global' or 'first'")
    cap = t.N + 1
    o, status, steps = _launch_queue(env, what, seed, lambda b: b.eval_td(
        None if pi_tab is None else b.state_rows(pi_tab), gamma, mode, 0.0 if callable(alpha) else alpha, q=b.state_rows(Q0, fill=0.0)[None],
        n_episodes=n_ep, ep_cap=n_ep + 1, trace_cap=cap, behaviour=behaviour, epsilon=0.0 if callable(epsilon) else epsilon, alpha_ep=a_tab,
        epsilon_ep=e_tab if behaviour == L.BEHAVIOUR_EPS_GREEDY else None, snap_cap=cap if save_Q else 0, snap_stride=1, tie=tie))
    if "tie_mt" in o and (n_ep > 0 or not isinstance(tie, str)):  # np.random.seed(episode) of every episode begun (tabular.py:114, :166)
        w = o["tie_mt"].cpu().numpy().view(np.uint32)[0]
        np.random.set_state(("MT19937", w[:624].copy(), int(w[624]), 0, 0.0) if isinstance(tie, str) else ("MT19937", w[:624].copy(), int(w[624]), st[3], st[4]))
    ne = int(o["n_ep"].cpu()[0])
    n_g = ne + (1 if status == L.ST_EXHAUSTED else 0)  # the cut-short episode's return is kept too
    Q = impl.rows_to_state(o["q"].cpu().numpy()[0], Q0)
    rows = o["trace_row"].cpu().numpy()[0, :steps]
    td = o["td_err"].cpu().numpy()[0, :steps].copy()
    Qs = np.array([Q0])
    if save_Q:  # tabular.py:107, :131: Q before the first step, then after every step
        Qs = np.concatenate([Q0[None], impl.rows_to_state(o["q_snap"].cpu().numpy()[0, :steps], Q0)], axis=0)
    e = env._dataset.experience
    done = np.asarray(e["terminals"])[rows].astype(bool) if steps else np.zeros(0, bool)
    episode = np.concatenate([[0], np.cumsum(done[:-1])]).astype(np.int64) if steps else np.zeros(0, np.int64)
    eps_of = (lambda i: e_tab[min(int(episode[i]), len(e_tab) - 1)]) if e_tab is not None else (lambda i: float(epsilon))
    alpha_of = (lambda i: a_tab[min(int(episode[i]), len(a_tab) - 1)]) if a_tab is not None else (lambda i: float(alpha))

    def p_of_step():
        if kind == "fixed":
            return [pi_tab[int(env._z[r])] for r in rows]
        if behaviour == L.BEHAVIOUR_EPS_GREEDY:
            best, ps = o["beh_arg"].cpu().numpy()[0, :steps], []
            for i in range(steps):
                w = np.ones(nA) * eps_of(i) / nA
                w[int(best[i])] = 1 - eps_of(i) + eps_of(i) / nA
                ps.append(w)
            return ps
        Qr, ps = Q0.copy(), []  # soft greedy: replay Q from the TD errors
        for i, r in enumerate(rows):
            S, A = int(env._z[r]), int(e["actions"][r])
            w = np.zeros(nA)
            w[np.where(np.isclose(Qr[S], np.max(Qr[S])))[0]] = 1
            ps.append(w / w.sum())
            Qr[S, A] = Qr[S, A] + alpha_of(i) * td[i]
        return ps

    return Q, {"Gs": o["ep_g"].cpu().numpy()[0, :n_g].copy(), "Qs": Qs, "TD_errors": td, "memory": _QueueStepMemory(env, rows, p_of_step)}


def qlearn_queue(env, n_episodes, behavior_policy, gamma, alpha=0.1, epsilon=1.0, Q_init=None, save_Q=0, seed=None, tie="episode"):
    """tabular.py:71-139 on a QueueEvaluator: Q-learning with the whole loop -- the behaviour policy on the learner's own Q, the action
    draw from default_rng(seed), the pops, the updates -- in one kernel launch.  `behavior_policy` must be one of the reference's tabular
    policies (recognised by probing: psrs._behaviour_kind; anything else raises NotImplementedError); alpha and epsilon may be callables
    of the episode; save_Q returns Q after every step.  tie = "episode" (the reference): ties between maximal Q values are broken with
    NumPy's global stream restarted by np.random.seed(episode) at every episode, and the global stream is left as the reference leaves
    it; "global": the global stream as it stands runs on; "first": the first maximum."""
    kind, fixed = _behaviour_kind(behavior_policy, env.nA)
    n_rows = env.nS if Q_init is None else int(np.shape(Q_init)[0])
    pi_tab = np.tile(np.asarray(fixed, dtype=np.float64), (max(n_rows, env._impl.nZ or 1), 1)) if kind == "fixed" else None
    return _td_queue(env, "qlearn_queue", n_episodes, gamma, alpha, epsilon, Q_init, save_Q, L.TD_QLEARN, kind, pi_tab, seed, tie)


def expSARSA_queue(env, n_episodes, pi, gamma, alpha=0.1, Q_init=None, save_Q=0, seed=None, tie="episode"):
    """tabular.py:141-191 on a QueueEvaluator: expected SARSA under the fixed behaviour / target policy pi, one kernel launch.  The
    reference sums Q[S_] @ pi[S_] in BLAS; here it runs left to right, so Q agrees to rounding."""
    pi = np.asarray(pi, dtype=np.float64)
    if pi.ndim != 2:
        raise ValueError("expSARSA_queue: pi must be a [nS, nA] table")
    return _td_queue(env, "expSARSA_queue", n_episodes, gamma, alpha, 0.0, Q_init, save_Q, L.TD_EXPSARSA, "fixed", pi, seed, tie)
