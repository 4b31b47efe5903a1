"""A population of tabular TD learners inside the simulator: a grid of step sizes, exploration rates and discounts per launch.

qlearn_psrs / expSARSA_psrs (offsim4rl/evaluators/psrs.py:119-239) run one hyper-parameter setting on one sampler seed per call.  What
they are used for is the comparison of learning curves -- every setting over many seeds -- so the learner is a grid dimension of the
learner kernel here: BatchedPSRS.eval_td_population runs L learners on each of S seeds in one launch (offsim_eval_td_pop), all learners of
a seed on the same queue orders and the same rejection draws (paired comparisons), and offsim_td_curves reduces the returns to one curve
per learner on the device.  Learners never interact: learner l on seed j is, bit for bit, what eval_td gives that setting on that seed.

  TDPopulation(mode, alpha, gamma, epsilon, behaviour, pi, Q_init)   the settings, each a scalar or one value per learner
  TDPopulation.grid(mode, alpha=[..], epsilon=[..], gamma=[..])      their Cartesian product
  population.run(table, seeds, ...)                                  -> TDPopulationResult of device tensors
  population.run_exo(env_or_tables, seeds, ...)                      the same on an exogenous-state log (PSRS_Exo), tables by observation
  population.run_queue(env_or_arrays, seeds, ...)                    the same on the queue simulator (QueueEvaluator), tables by state
  population.run_env(grid_world, seeds, n_episodes, ...)             the same in the true grid world: the ground truth of the three above
  population.replay(log, orders, passes, ...)                        no simulator: the logged memory itself replayed through every learner
"""
import itertools
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from .. import _lib as L
from .batched import SHUFFLE_PER_ROLLOUT, BatchedPSRS, default_tile
from .psrs import _schedule
from .rollout_io import seed_tiles, tie_stream

_MODE = {"qlearn": L.TD_QLEARN, "expsarsa": L.TD_EXPSARSA, L.TD_QLEARN: L.TD_QLEARN, L.TD_EXPSARSA: L.TD_EXPSARSA}
_BEHAVIOUR = {"fixed": L.BEHAVIOUR_FIXED, "eps_greedy": L.BEHAVIOUR_EPS_GREEDY, "greedy": L.BEHAVIOUR_EPS_GREEDY, "soft_greedy": L.BEHAVIOUR_SOFT_GREEDY}


def _is_seq(x):
    return isinstance(x, (list, tuple, np.ndarray)) or (isinstance(x, torch.Tensor) and x.dim() > 0)


def _per_learner(x):
    """a scalar, a callable or a string -> [x]; a sequence -> its list"""
    return list(x) if _is_seq(x) else [x]


@dataclass
class TDPopulationResult:
    """What TDPopulation.run returns; every array is a tensor on the table's device.
    Q [L,S,nS,nA] by caller state id; Gs [L,S,ep_cap] the returns in episode order (entry n_ep of a row: the episode the end of the log
    cut short, as qlearn_psrs appends it); n_ep, steps, status [L,S]; curve_n / curve_mean / curve_var [L,ep_cap]: per learner and
    episode, over the seeds that completed that episode, their number, the mean return and its population variance (NaN where no seed
    did); td_err [L,S,trace_cap] when the run was asked for the trace; tie_mt [L,S,625] int32 (run_exo with tie streams): where every
    rollout's MT19937 stream stands afterwards."""
    Q: torch.Tensor
    Gs: torch.Tensor
    n_ep: torch.Tensor
    steps: torch.Tensor
    status: torch.Tensor
    curve_mean: torch.Tensor
    curve_var: torch.Tensor
    curve_n: torch.Tensor
    learners: list = field(default_factory=list)
    td_err: Optional[torch.Tensor] = None
    tie_mt: Optional[torch.Tensor] = None

    def best(self, last=1):
        """The learner with the highest mean of its last `last` curve points that every seed reached (curve_n == S); points fewer
        seeds completed are ignored, a learner without such a point is never the best; -1 when no learner has one."""
        S = int(self.Gs.shape[1])
        n, mean = self.curve_n.cpu().numpy(), self.curve_mean.cpu().numpy()
        score = np.full(n.shape[0], -np.inf)
        for l in range(n.shape[0]):
            full = np.nonzero(n[l] == S)[0][-max(int(last), 1):]
            if len(full):
                score[l] = float(np.mean(mean[l, full]))
        return -1 if not np.isfinite(score).any() else int(np.argmax(score))


class TDPopulation:
    """L tabular TD learners.  mode: "qlearn" or "expsarsa" (one for the population).  alpha, gamma, epsilon, behaviour: a scalar or one
    value per learner; alpha and epsilon may be callables of the episode (psrs.py:128-135), tabulated per run as the single-learner
    drivers do.  behaviour: "fixed" (the tabular pi, e.g. uniformly random), "eps_greedy", "greedy" (epsilon 0) or "soft_greedy" on the
    learner's own Q (offsim4rl/agents/tabular.py:7-32).  pi [nS,nA] or [L,nS,nA] by caller state id: the behaviour policy when fixed and
    the target of expected SARSA (None: uniform).  Q_init [nS,nA] or [L,nS,nA] (None: zeros).  L is the common length of the per-learner
    arguments; lengths that disagree raise ValueError."""

    def __init__(self, mode, alpha, gamma, epsilon=1.0, behaviour="fixed", pi=None, Q_init=None):
        if mode not in _MODE:
            raise ValueError(f"TDPopulation: mode must be 'qlearn' or 'expsarsa', got {mode!r}")
        self.mode = _MODE[mode]
        given = {"alpha": alpha, "gamma": gamma, "epsilon": epsilon, "behaviour": behaviour}
        per = {k: _per_learner(x) for k, x in given.items()}
        self.pi = None if pi is None else np.asarray(pi, dtype=np.float64)
        self.Q_init = None if Q_init is None else np.asarray(Q_init, dtype=np.float64)
        lens = {k: len(per[k]) for k, x in given.items() if _is_seq(x)}
        for k, x in (("pi", self.pi), ("Q_init", self.Q_init)):
            if x is not None:
                if x.ndim not in (2, 3):
                    raise ValueError(f"TDPopulation: {k} must be [nS,nA] or [L,nS,nA], got {x.shape}")
                if x.ndim == 3:
                    lens[k] = x.shape[0]
        if len(set(lens.values())) > 1:
            raise ValueError(f"TDPopulation: per-learner arguments of different lengths: {lens}")
        self.L = next(iter(lens.values())) if lens else 1
        if self.L < 1:
            raise ValueError("TDPopulation: no learner")
        self.alpha, self.gamma, self.epsilon, self.behaviour = (v * self.L if len(v) == 1 else v for v in (per[k] for k in ("alpha", "gamma", "epsilon", "behaviour")))
        for b in self.behaviour:
            if b not in _BEHAVIOUR or not isinstance(b, str):
                raise ValueError(f"TDPopulation: behaviour must be one of {sorted(k for k in _BEHAVIOUR if isinstance(k, str))}, got {b!r}")
        self.gamma = [float(g) for g in self.gamma]

    @classmethod
    def grid(cls, mode, alpha, epsilon=(1.0,), gamma=(0.99,), behaviour="fixed", pi=None, Q_init=None):
        """The Cartesian product of the listed values, alpha slowest and gamma fastest: learner i is (alpha, epsilon, gamma) =
        list(itertools.product(alpha, epsilon, gamma))[i]; behaviour, pi and Q_init are shared."""
        alpha, epsilon, gamma = (list(x) if _is_seq(x) else [x] for x in (alpha, epsilon, gamma))
        cells = list(itertools.product(alpha, epsilon, gamma))
        if not cells:
            raise ValueError("TDPopulation.grid: an empty axis")
        return cls(mode, [c[0] for c in cells], [c[2] for c in cells], [c[1] for c in cells], behaviour, pi, Q_init)

    def __len__(self):
        return self.L

    @property
    def learners(self):
        """The settings, one dict per learner."""
        return [dict(alpha=self.alpha[l], epsilon=self.epsilon[l], gamma=self.gamma[l], behaviour=self.behaviour[l]) for l in range(self.L)]

    def tabulate(self, n_ep):
        """The per-learner constants and schedules of a run of at most n_ep episodes: (alpha [L], epsilon [L], alpha_ep, epsilon_ep), the
        last two [L, max(n_ep, 1)] or None when no learner has a callable.  A callable is evaluated per episode (_schedule of psrs.py)
        and its constant is 0; a learner with a constant gets a constant row; "greedy" is epsilon 0 whatever epsilon says (_td_run)."""
        eps = [0.0 if b == "greedy" else e for e, b in zip(self.epsilon, self.behaviour)]
        a_const = np.array([0.0 if callable(a) else float(a) for a in self.alpha])
        e_const = np.array([0.0 if callable(e) else float(e) for e in eps])
        if not any(callable(x) for x in list(self.alpha) + eps):
            return a_const, e_const, None, None
        n = max(int(n_ep), 1)
        a_tab = np.stack([_schedule(a, n) if callable(a) else np.full(n, float(a)) for a in self.alpha])
        e_tab = np.stack([_schedule(e, n) if callable(e) else np.full(n, float(e)) for e in eps])
        return a_const, e_const, a_tab, e_tab

    def _n_rows(self, table):
        for x in (self.Q_init, self.pi):
            if x is not None:
                return int(x.shape[-2])
        return max(int(table.slot_z.max()) + 1 if table.N else 1, 1)

    def _slots(self, table, x, nan=None):
        """[nS,nA] or [L,nS,nA] by caller state id -> the same in slot order (TransitionTable.policy_slots per learner)"""
        out = table.policy_slots(x) if x.ndim == 2 else np.stack([table.policy_slots(v) for v in x])
        return out if nan is None else np.nan_to_num(out, nan=nan)

    def _seeds(self, who, seeds):
        seeds = np.asarray(seeds, dtype=np.uint64)
        if len(seeds) < 1:
            raise ValueError(f"TDPopulation.{who}: no seed")
        return seeds, len(seeds)

    def _run_tiles(self, who, seeds, N0, n_episodes, tile, make_env, launch, Q_of, tie=None, tie_one=True, tie_out=False, trace_cap=0):
        """What run, run_exo and run_queue do alike once their tables are laid out: at most min(n_episodes, N0 + 1) episodes, the
        schedules and behaviour codes, the tie states -- `tie` [L,S,625], or with tie_one one [625] every rollout starts from; a string or
        None passes through -- then per tile of `tile` seeds make_env(n), launch(env, b, sd, tie of the tile, hp) with hp the keyword
        arguments every eval_td_population takes, and the fault check; the tiles concatenated along the seeds, Q_of(q) the launch's Q
        rows back by the caller's row ids, and offsim_td_curves over all seeds (_result)."""
        S, n_l = len(seeds), self.L
        n_ep = int(min(n_episodes if n_episodes is not None else N0 + 1, N0 + 1))
        ep_cap = max(n_ep, 1)
        a_const, e_const, a_tab, e_tab = self.tabulate(n_ep)
        hp = dict(mode=self.mode, alpha=a_const, gamma=self.gamma, behaviour=np.array([_BEHAVIOUR[b] for b in self.behaviour], dtype=np.int32),
                  epsilon=e_const, alpha_ep=a_tab, epsilon_ep=e_tab, n_episodes=n_ep, ep_cap=ep_cap, trace_cap=int(trace_cap))
        states = tie is not None and not isinstance(tie, str)
        if states:
            tie = tie_stream(tie)
            if tie_one and tuple(tie.shape) == (625,):
                tie = tie.expand(n_l, S, 625)
            if tuple(tie.shape) != (n_l, S, 625):
                raise ValueError(f"TDPopulation.{who}: tie_mt {'[625] or ' if tie_one else ''}[L,S,625] = {(n_l, S, 625)} expected, got {tuple(tie.shape)}")
        keys = ["q", "ep_g", "n_ep", "steps", "status"] + (["td_err"] if trace_cap else []) + (["tie_mt"] if tie_out else [])
        parts = {k: [] for k in keys}
        for b, sd, env in seed_tiles(seeds, int(tile(S) if callable(tile) else tile), make_env):
            o = launch(env, b, sd, tie[:, b:b + len(sd)] if states else tie, hp)
            for k in keys:
                parts[k].append(o[k])
            BatchedPSRS.check_faults()
        res = {k: v[0] if len(v) == 1 else torch.cat(v, dim=1).contiguous() for k, v in parts.items()}
        return self._result(res, Q_of(res["q"]), ep_cap)

    def run(self, table, seeds, n_episodes=None, shuffle=SHUFFLE_PER_ROLLOUT, tile=None, tie_mt=None, rejection="pcg64", shuffle_seed=None,
            trace_cap=0, reject_mode=L.REJECT_DEFAULT):
        """Every learner on every seed.  One reset_sampler per tile of `tile` seeds (default: resident_rollouts(keyed=False), as
        evalmc_rollouts_population -- the queue orders are the seeds', shared by all learners, so the tile does not shrink with L), one
        launch per tile, then offsim_td_curves over all seeds.  n_episodes: at most that many episodes per learner and seed (None: until
        the log ends).  tie_mt [L,S,625]: NumPy MT19937 states for ties between maximal Q values (None: the first maximum).
        trace_cap > 0 also returns the TD errors of the first trace_cap steps."""
        seeds, S = self._seeds("run", seeds)
        nS = self._n_rows(table)
        Q0 = np.zeros((nS, table.nA)) if self.Q_init is None else self.Q_init
        pi = np.full((nS, table.nA), 1.0 / table.nA) if self.pi is None else self.pi
        if table.N and pi.shape[-2] <= int(table.slot_z.max()):
            raise IndexError("pi has no row for some latent state")
        pi_slots, q_slots = self._slots(table, pi), self._slots(table, Q0, nan=0.0)

        def launch(env, b, sd, tie, hp):
            env.reset_sampler(sd, shuffle, shuffle_seed, rejection=rejection)
            return env.eval_td_population(pi_slots=pi_slots, q_slots=q_slots, tie_mt=tie, **hp)

        # slot s goes to row slot_z[s] (the rule of psrs._slots_to_q)
        return self._run_tiles("run", seeds, table.N0, n_episodes, (lambda S: default_tile(table, S, shuffle, keyed=False)) if tile is None else tile,
                               lambda n: BatchedPSRS(table, n, reject_mode), launch,
                               lambda q: self._rows_into(Q0, q, [table.z_of(s) for s in range(table.n_slots)], range(table.n_slots), self.L, S),
                               tie=tie_mt, tie_one=False, trace_cap=trace_cap)

    def _result(self, res, Q, ep_cap):
        """The TDPopulationResult of the concatenated tiles `res` ([L, S, ...]): offsim_td_curves over all seeds."""
        n_l, S = res["n_ep"].shape
        dev = res["n_ep"].device
        curve_n = torch.empty((n_l, ep_cap), dtype=torch.int64, device=dev)
        curve_mean, curve_var = (torch.empty((n_l, ep_cap), dtype=torch.float64, device=dev) for _ in range(2))
        L.check(L.load().offsim_td_curves(L.ptr(res["ep_g"]), L.ptr(res["n_ep"]), n_l, S, ep_cap, L.ptr(curve_n), L.ptr(curve_mean), L.ptr(curve_var),
                                          L.stream_ptr()))
        return TDPopulationResult(Q=Q, Gs=res["ep_g"], n_ep=res["n_ep"], steps=res["steps"], status=res["status"], curve_mean=curve_mean,
                                  curve_var=curve_var, curve_n=curve_n, learners=self.learners, td_err=res.get("td_err"), tie_mt=res.get("tie_mt"))

    def run_exo(self, env_or_tables, seeds, obs_of=None, n_episodes=None, reseed="episode", tile=None, tie_mt=None, rejection="pcg64", trace_cap=0):
        """Every learner on every seed of an exogenous-state log (PSRS_Exo: two queue families, tables indexed by the observation
        o = o_combine_func(s, x)), with any behaviour policy of the reference on the learner's own Q; one learner is qlearn_psrs /
        expSARSA_psrs with a greedy behaviour, which those drivers refuse on a PSRS_Exo.
        env_or_tables: a PSRS_Exo -- pi and Q_init are then [nO,nA] (or [L,nO,nA]) tables BY OBSERVATION, compacted through env.obs_table --
        or a pair (ts, tx) of TransitionTables with obs_of [ns_slots, nx_slots] (tabulate_obs) and pi / Q_init in its compact rows.
        One reset_sampler of both families per tile of seeds, one launch per tile (BatchedPSRSExo.eval_td_population), then offsim_td_curves
        over all seeds.  reseed = "episode": episode e of every rollout draws from default_rng(e), the reference's protocol (PCG64);
        "none": every seed's own stream (`rejection`: "pcg64" or "philox"), the learners of a seed starting from the same state.
        tile (None): the queue orders of BOTH families stay resident per seed, so it is resident_rollouts(ts, keyed=False) scaled by
        bytes(ts) / (bytes(ts) + bytes(tx)) with rollout_resident_bytes(table, keyed=False) each, at least 1, at most S; it does not shrink
        with L (the orders are the seeds', shared by all learners).  tie_mt: None (the first maximum, as run), or NumPy MT19937 states
        [L,S,625], or one [625] every rollout starts from; the advanced states come back as result.tie_mt [L,S,625].
        Returns a TDPopulationResult with Q [L,S,nO,nA] by observation (rows the slot grid has no observation for keep Q_init's values;
        for a pair of tables: the compact rows)."""
        from .psrs_exo import PSRS_Exo, BatchedPSRSExo
        from .batched import rollout_resident_bytes, resident_rollouts
        seeds, S = self._seeds("run_exo", seeds)
        given = next((x for x in (self.Q_init, self.pi) if x is not None), None)
        if isinstance(env_or_tables, PSRS_Exo):
            ts, tx = env_or_tables.ts, env_or_tables.tx
            nO = int(given.shape[-2]) if given is not None else int(env_or_tables.nO)
            obs_of, ids = env_or_tables.obs_table(nO)
        else:
            ts, tx = env_or_tables
            if obs_of is None:
                raise ValueError("TDPopulation.run_exo: a pair of tables needs obs_of")
            obs_of = np.ascontiguousarray(obs_of.cpu().numpy() if isinstance(obs_of, torch.Tensor) else obs_of, dtype=np.int32)
            nO = int(given.shape[-2]) if given is not None else max(int(obs_of.max()) + 1, 1)
            ids = np.arange(nO)
        for k, x in (("pi", self.pi), ("Q_init", self.Q_init)):
            if x is not None and x.shape[-2:] != (nO, ts.nA):
                raise ValueError(f"TDPopulation.run_exo: {k} [nO,nA] = {(nO, ts.nA)} expected, got {x.shape}")
        Q0 = np.zeros((nO, ts.nA)) if self.Q_init is None else self.Q_init
        pi = np.full((nO, ts.nA), 1.0 / ts.nA) if self.pi is None else self.pi

        def default(S):
            n_res, per_s = resident_rollouts(ts, keyed=False)[:2]
            return max(1, min(S, n_res * per_s // (per_s + rollout_resident_bytes(tx, keyed=False))))

        def launch(env, b, sd, tie, hp):
            env.reset_sampler(sd, rejection=rejection)
            return env.eval_td_population(obs_of=obs_of, pi_obs=pi[..., ids, :], q_obs=Q0[..., ids, :], reseed=reseed, tie_mt=tie, **hp)

        return self._run_tiles("run_exo", seeds, ts.N0, n_episodes, default if tile is None else tile, lambda n: BatchedPSRSExo(ts, tx, n), launch,
                               lambda q: self._rows_into(Q0, q, ids, range(len(ids)), self.L, S), tie=tie_mt, tie_out=tie_mt is not None,
                               trace_cap=trace_cap)

    def run_queue(self, env_or_arrays, seeds, n_episodes=None, action_seeds=None, tie="episode", episode0=0, tile=None, trace_cap=0):
        """Every learner on every seed of the queue simulator (QueueEvaluator: queues keyed by (z, a), the agent draws its own action;
        qlearn / expSARSA of offsim4rl/agents/tabular.py:71-191), the baseline run() on PSRS is compared against.
        env_or_arrays: a QueueEvaluator, or the columns (z, a, r, z_next, done, p_log, t0) BatchedQueueEvaluator takes.  pi / Q_init are
        [nS,nA] or [L,nS,nA] tables indexed by the state as the reference does (pi None: uniform).  Rollout (l, j) shuffles its queues
        with seeds[j] and draws its actions from default_rng(action_seeds[j]) (default: seeds): all learners of a seed see the same queues
        and start from the same action stream, so comparisons are paired.  One reset_sampler + set_action_seeds and one launch per tile of
        seeds (BatchedQueueEvaluator.eval_td_population), then offsim_td_curves over all seeds.  tile (None):
        default_tile(table, S, SHUFFLE_PER_ROLLOUT, keyed=False), as run -- the orders are the seeds', so it does not shrink with L.
        tie: "episode" (the reference: ties between maximal Q values are broken with a stream restarted as np.random.seed(episode0 + e) at
        every episode e), "first" (the first maximum), or NumPy MT19937 states [625] (every rollout starts from it) / [L,S,625].
        Returns a TDPopulationResult with Q [L,S,nS,nA] by caller state id (rows without a state keep Q_init's values), tie_mt [L,S,625]
        whenever a stream ran, td_err with trace_cap.  OFFSIM_ST_KEYERROR / _EXHAUSTED do not raise: they are in result.status."""
        from .queue_evaluator import BatchedQueueEvaluator, QueueEvaluator
        seeds, S = self._seeds("run_queue", seeds)
        action_seeds = seeds if action_seeds is None else np.asarray(action_seeds, dtype=np.uint64)
        if len(action_seeds) != S:
            raise ValueError("TDPopulation.run_queue: one action seed per sampler seed (action_seeds)")
        if isinstance(env_or_arrays, QueueEvaluator):
            arrays, probe, nS = env_or_arrays._arrays, env_or_arrays._impl, int(env_or_arrays.nS)
        else:
            arrays = tuple(env_or_arrays)
            probe, nS = BatchedQueueEvaluator(*arrays, R=1), None
        if probe.nZ is None:
            raise L.OffsimError("the one-launch queue drivers need dense state ids (this log's ids were compacted to ranks)")
        t, nZ, nA = probe.table, probe.nZ, probe.nA
        given = next((x for x in (self.Q_init, self.pi) if x is not None), None)
        nS = int(given.shape[-2]) if given is not None else nZ if nS is None else nS
        for k, x in (("pi", self.pi), ("Q_init", self.Q_init)):
            if x is not None and x.shape[-2:] != (nS, nA):
                raise ValueError(f"TDPopulation.run_queue: {k} [nS,nA] = {(nS, nA)} expected, got {x.shape}")
        Q0 = np.zeros((nS, nA)) if self.Q_init is None else self.Q_init
        rows = lambda x, fill: probe.state_rows(x, fill) if x.ndim == 2 else np.stack([probe.state_rows(v, fill) for v in x])  # noqa: E731
        pi_rows, q_rows = None if self.pi is None else rows(self.pi, np.nan), rows(Q0, 0.0)
        if isinstance(tie, str) and tie not in ("episode", "first"):
            raise ValueError(f"TDPopulation.run_queue: tie must be 'episode', 'first' or MT19937 states, got {tie!r}")

        def launch(env, b, sd, tie, hp):
            env.reset_sampler(sd)
            env.set_action_seeds(action_seeds[b:b + len(sd)])
            return env.eval_td_population(pi=pi_rows, q=q_rows, tie=tie, episode0=episode0, **hp)

        # rows_to_state on the device: row i of the table's states goes to row z_lo + i of Q0's copy
        return self._run_tiles("run_queue", seeds, t.N0, n_episodes, (lambda S: default_tile(t, S, SHUFFLE_PER_ROLLOUT, keyed=False)) if tile is None else tile,
                               lambda n: BatchedQueueEvaluator(*arrays, R=n), launch,
                               lambda q: self._rows_into(Q0, q, range(probe.z_lo, probe.z_lo + nZ), range(nZ), self.L, S), tie=tie,
                               tie_out=not (isinstance(tie, str) and tie == "first"), trace_cap=trace_cap)

    def run_env(self, env, seeds, n_episodes, tie="episode", episode0=0, tile=None, trace_cap=0):
        """Every learner on every seed in the TRUE grid world (a GridWorld of evaluators/true_env_drivers.py; qlearn / expSARSA of
        offsim4rl/agents/tabular.py:71-191 on the reference's own environment): the ground truth run(), run_exo() and run_queue() are
        judged against.  pi / Q_init are [nS,5] or [L,nS,5] tables by observation (pi None: uniform).  Rollout (l, j) draws its actions
        from default_rng(seeds[j]) and runs n_episodes episodes, episode e reset with seed episode0 + e: all learners of a seed start from
        the same action stream and see the same exogenous draws, so comparisons are paired.  One launch per tile of seeds (default: all;
        BatchedGridWorld.eval_td_population), then offsim_td_curves over all seeds.  tie: "episode" (the reference: ties between maximal Q
        values are broken with a stream restarted as np.random.seed(episode0 + e) at every episode e), "first" (the first maximum), or
        NumPy MT19937 states [625] (every rollout starts from it) / [L,S,625].  Returns a TDPopulationResult with Q [L,S,nS,5], tie_mt
        [L,S,625] whenever a stream ran, td_err with trace_cap.  OFFSIM_ST_KEYERROR does not raise: it is in result.status."""
        from .true_env_drivers import BatchedGridWorld, GridWorld
        if not isinstance(env, GridWorld):
            raise TypeError(f"TDPopulation.run_env: `env` must be a GridWorld, got {type(env).__name__}")
        seeds, S = self._seeds("run_env", seeds)
        n_episodes = int(n_episodes)
        if n_episodes < 1:
            raise ValueError("TDPopulation.run_env: n_episodes must be positive (an environment never runs dry)")
        for k, x in (("pi", self.pi), ("Q_init", self.Q_init)):
            if x is not None and x.shape[-2:] != (env.nS, env.nA):
                raise ValueError(f"TDPopulation.run_env: {k} [nS,nA] = {(env.nS, env.nA)} expected, got {x.shape}")
        if isinstance(tie, str) and tie not in ("episode", "first"):
            raise ValueError(f"TDPopulation.run_env: tie must be 'episode', 'first' or MT19937 states, got {tie!r}")
        Q0 = np.zeros((env.nS, env.nA)) if self.Q_init is None else self.Q_init

        def launch(b, lo, sd, tie, hp):
            b.set_action_seeds(sd)
            return b.eval_td_population(pi=self.pi, q=Q0, tie=tie, episode0=episode0, **hp)

        # (_run_tiles bounds the episodes by a log's initial rows: none here, so N0 = n_episodes leaves n_episodes as it is)
        return self._run_tiles("run_env", seeds, n_episodes, n_episodes, S if tile is None else tile, lambda n: BatchedGridWorld(env, n), launch,
                               lambda q: q, tie=tie, tie_out=tie is not None and not (isinstance(tie, str) and tie == "first"), trace_cap=trace_cap)

    def run_latent_env(self, env, seeds, n_episodes, tie="episode", reseed="episode", episode0=0, tile=None, trace_cap=0):
        """Every learner on every seed in the TRUE environment behind its encoder (a LatentEnv of evaluators/latent_env_drivers.py: CartPole
        with the box or a HOMER encoder, the coordinate grid with a HOMER encoder; qlearn / expSARSA of offsim4rl/agents/tabular.py with the
        tables indexed by z = encoder(observation)): the ground truth run() and run_queue() on a log encoded by the same encoder are judged
        against.  pi / Q_init are [nS,nA] or [L,nS,nA] tables by latent row (pi None: uniform).  Rollout (l, j) draws its actions from
        default_rng(seeds[j]) and runs n_episodes episodes; reseed = "episode" (the reference): episode e resets with default_rng(episode0 +
        e); "none": seed j's own environment stream default_rng(seeds[j]) runs on.  Either way all learners of a seed see the same resets,
        noise and action uniforms, so comparisons are paired.  One launch per tile of seeds (default: all;
        BatchedLatentEnv.eval_td_population), then offsim_td_curves over all seeds.  tie as run_env's.  Returns a TDPopulationResult with
        Q [L,S,nS,nA], tie_mt [L,S,625] whenever a stream ran, td_err with trace_cap.  OFFSIM_ST_KEYERROR does not raise: it is in
        result.status."""
        from .latent_env_drivers import BatchedLatentEnv, LatentEnv
        if not isinstance(env, LatentEnv):
            raise TypeError(f"TDPopulation.run_latent_env: `env` must be a LatentEnv, got {type(env).__name__}")
        seeds, S = self._seeds("run_latent_env", seeds)
        n_episodes = int(n_episodes)
        if n_episodes < 1:
            raise ValueError("TDPopulation.run_latent_env: n_episodes must be positive (an environment never runs dry)")
        for k, x in (("pi", self.pi), ("Q_init", self.Q_init)):
            if x is not None and x.shape[-2:] != (env.nS, env.nA):
                raise ValueError(f"TDPopulation.run_latent_env: {k} [nS,nA] = {(env.nS, env.nA)} expected, got {x.shape}")
        if isinstance(tie, str) and tie not in ("episode", "first"):
            raise ValueError(f"TDPopulation.run_latent_env: tie must be 'episode', 'first' or MT19937 states, got {tie!r}")
        if reseed not in ("episode", "none"):
            raise ValueError(f"TDPopulation.run_latent_env: reseed must be 'episode' or 'none', got {reseed!r}")
        Q0 = np.zeros((env.nS, env.nA)) if self.Q_init is None else self.Q_init

        def launch(b, lo, sd, tie, hp):
            b.set_seeds(sd)
            return b.eval_td_population(pi=self.pi, q=Q0, tie=tie, episode0=episode0, reseed=reseed, **hp)

        return self._run_tiles("run_latent_env", seeds, n_episodes, n_episodes, S if tile is None else tile, lambda n: BatchedLatentEnv(env, n), launch,
                               lambda q: q, tie=tie, tie_out=tie is not None and not (isinstance(tie, str) and tie == "first"), trace_cap=trace_cap)

    def replay(self, log, orders=None, passes=1, td_cap=0, snap_stride=0, snap_cap=0):
        """Every learner on the logged memory itself, no simulator: qlearn(..., memory=...) of offsim4rl/agents/tabular.py:90-104 (and the
        same sweep with the expected-SARSA target) for all L learners in one launch (offsim_replay_td, evaluators/replay.py).
        log: a ReplayLog.  orders: None -- one stream, the log in log order -- or an int32 [S, M] device tensor (replay_orders): stream j
        visits log rows orders[j]; every learner sees every stream, so comparisons are paired.  passes: sweeps over each stream, the
        episode counter (the done flags seen) carrying on.  A callable alpha is tabulated for the episodes passes sweeps can hold.
        td_cap: TD errors of the first td_cap steps; snap_stride / snap_cap: Q after steps 0, stride, 2 stride, ....
        No action is drawn in a replay, so the population's `behaviour` and `epsilon` are ignored.  mode "expsarsa" needs pi.
        pi / Q_init are [nS,nA] or [L,nS,nA] tables by state (Q_init None: zeros).  Returns a TDReplayResult."""
        from .replay import TDReplayResult, replay_td
        if self.mode == L.TD_EXPSARSA and self.pi is None:
            raise ValueError("TDPopulation.replay: mode 'expsarsa' needs pi")
        for k, x in (("pi", self.pi), ("Q_init", self.Q_init)):
            if x is not None and x.shape[-2:] != (log.nS, log.nA):
                raise ValueError(f"TDPopulation.replay: {k} [nS,nA] = {(log.nS, log.nA)} expected, got {x.shape}")
        S = 1 if orders is None else int(orders.shape[0])
        M = log.N if orders is None else int(orders.shape[1])
        a_const, a_tab = np.array([0.0 if callable(a) else float(a) for a in self.alpha]), None
        if any(callable(a) for a in self.alpha):  # the episodes of the longest stream: its done flags, every sweep
            flags = log.done.sum() if orders is None else log.done[orders.clamp(0, log.N - 1).to(torch.int64)].sum(dim=1).max()
            n = int(flags.item()) * int(passes) + 1
            a_tab = np.stack([_schedule(a, n) if callable(a) else np.full(n, float(a)) for a in self.alpha])
        Q0 = np.zeros((log.nS, log.nA)) if self.Q_init is None else self.Q_init
        q0 = torch.from_numpy(np.ascontiguousarray(Q0)).to(log.device)
        q0 = (q0[:, None] if q0.dim() == 3 else q0[None, None]).expand(self.L, S, log.nS, log.nA)
        o = replay_td(log, self.mode, a_const, self.gamma, q0, orders=orders, passes=passes, alpha_ep=a_tab,
                      pi=self.pi if self.mode == L.TD_EXPSARSA else None, td_cap=td_cap, snap_stride=snap_stride, snap_cap=snap_cap)
        td = o.get("td_err")
        return TDReplayResult(Q=o["q"], n_ep=o["n_ep"], steps=o["steps"], status=o["status"], M=M, passes=int(passes),
                              td_err=None if td is None else td.permute(2, 0, 1), q_snap=o.get("q_snap"), learners=self.learners)

    @staticmethod
    def _rows_into(Q0, q, dst_rows, src_rows, n_l, S):
        """q [L,S,rows,nA], the launch's Q, back into copies of Q0 [nS,nA] or [L,nS,nA] on the device: row src_rows[i] of q goes to row
        dst_rows[i] with NumPy's negative-index wrap, the later pair winning a shared row and a row outside [-nS, nS) dropped; rows
        without a source keep Q0's values."""
        nS = Q0.shape[-2]
        q0 = torch.from_numpy(np.ascontiguousarray(Q0, dtype=np.float64)).to(q.device)
        out = (q0[:, None] if q0.dim() == 3 else q0[None, None]).expand(n_l, S, nS, q.shape[-1]).contiguous().clone()
        last = {int(d) % nS: int(s) for d, s in zip(dst_rows, src_rows) if -nS <= d < nS}
        if last:
            rows, src = (torch.tensor(list(v), dtype=torch.int64, device=q.device) for v in (last.keys(), last.values()))
            out[:, :, rows] = q[:, :, src]
        return out
