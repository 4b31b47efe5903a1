"""PSRS_Exo (offsim4rl/evaluators/psrs.py:59-117): PSRS with an exogenous state component.

An observation o splits into (s, x).  Transitions are queued twice: by s (the part the agent controls: action, reward,
next s, done, logging probabilities) and by x (the exogenous part: next x).  Every candidate pops the head of both
queues; the rejection test uses the s-element; the next observation recombines the accepted s' with the popped x'.
Both queue families reuse the ordinary device tables, shuffles and resets; the step is offsim_step_exo.

Whole rollouts -- the reference's drivers evalMC_psrs / qlearn_psrs / expSARSA_psrs on a PSRS_Exo (evaluators/psrs.py hands them here) and
many sampler seeds per launch -- run in offsim_eval_mc_exo (csrc/eval_exo.hpp): BatchedPSRSExo, evalmc_rollouts_exo.  The policy and Q are
indexed by the observation o = o_combine_func(s, x); tabulate_obs lays that map out over the grid of state slots.
BatchedPSRSExo.eval_td_population runs L learners on every seed in one launch (offsim_eval_td_exo_pop), each with any behaviour policy of
the reference on its own Q; TDPopulation.run_exo (td_population.py) is its seed-tile driver.
"""
import ctypes as C
import numbers
import os

import numpy as np
import torch

from .. import _lib as L
from ..table import RolloutState, TransitionTable, seed_streams, seeds_tensor, shuffle_queues
from .rollout_io import (HOST_KEYS, _gamma_pow, _prob_mode, collect_host, episode_bound, host_result, population_result, population_state,
                         rollout_outputs, seed_tiles, td_outputs, td_population_launch)


def tabulate_obs(s_values, x_values, o_combine_func, n_rows):
    """The observation map of offsim_eval_mc_exo for a policy / Q table of `n_rows` rows indexed by o = o_combine_func(s, x):
    (obs_of [len(s_values), len(x_values)] int32, obs_ids [n_obs] int64).  obs_ids are the distinct observations of the grid that have a
    row (ascending): the compact tables are pi[obs_ids] / Q[obs_ids]; obs_of holds the compact row of every pair, -1 where o >= n_rows.
    Observations must be non-negative ints usable as row indices of pi: anything else raises TypeError."""
    ns, nx = len(s_values), len(x_values)
    grid = np.empty((ns, nx), np.int64)
    for i, s in enumerate(s_values):
        for j, x in enumerate(x_values):
            o = o_combine_func(int(s), int(x))
            if isinstance(o, (bool, np.bool_)) or not isinstance(o, (numbers.Integral, np.integer)) or int(o) < 0:
                raise TypeError(f"o_combine_func({int(s)}, {int(x)}) = {o!r}: on the device the observations of a PSRS_Exo must be non-negative "
                                "ints usable as row indices of pi / Q")
            grid[i, j] = int(o)
    ok = grid < int(n_rows)
    obs_ids = np.unique(grid[ok])
    obs_of = np.full((ns, nx), -1, np.int32)
    obs_of[ok] = np.searchsorted(obs_ids, grid[ok]).astype(np.int32)
    return obs_of, obs_ids.astype(np.int64)


_RESEED = {"episode": L.EXO_RESEED_EPISODE, "none": L.EXO_RESEED_NONE, None: L.EXO_RESEED_NONE}


class BatchedPSRSExo:
    """R PSRS_Exo environments on one log: the s-table `ts` and the x-table `tx` (TransitionTables of the same rows, grouped by s and by
    x) with a RolloutState each.  Every method only enqueues kernels on the current stream."""

    def __init__(self, ts, tx, R, rs=None, rx=None):
        assert ts.N == tx.N and ts.N0 == tx.N0, "the two tables hold the same log"
        self.ts, self.tx, self.R = ts, tx, int(R)
        self.rs = RolloutState(ts, R) if rs is None else rs
        self.rx = RolloutState(tx, R) if rx is None else rx

    def reset_sampler(self, seeds, rejection="pcg64"):
        """psrs.py:77-89 for every seed: the init queue and every s- and x-queue shuffled by a fresh default_rng(seed).  The rollouts' own
        rejection streams (reseed="none") start as `rejection` = "pcg64": default_rng(seed), or "philox": rocRAND's Philox4x32-10."""
        dev = self.ts.device
        sd = seeds_tensor(seeds, dev)
        assert sd.numel() == self.R, "one seed per rollout"
        for t, ro in ((self.ts, self.rs), (self.tx, self.rx)):
            perm, init_perm = shuffle_queues(t, sd)
            ro.rewind()
            ro.set_orders(perm, t.N, init_perm, t.N0)
        if rejection == "pcg64":
            seed_streams(sd, self.rs.rng)
            self.rs.rng_kind = L.STREAM_PCG64
        elif rejection == "philox":
            self.rs.rng.zero_()
            self.rs.rng[:, 0] = sd  # seed, draws consumed, 0, 0
            self.rs.rng_kind = L.STREAM_PHILOX
        else:
            raise ValueError(rejection)
        self.rs._refresh()

    def step(self, p_new):
        """PSRS_Exo.step for every rollout (offsim_step_exo): device tensors (row_s, row_x, status, popped)."""
        ts, dev, R = self.ts, self.ts.device, self.R
        p_new = torch.as_tensor(p_new)
        f32 = p_new.dtype == torch.float32 and ts.p_log.dtype == torch.float32
        p = p_new.to(device=dev, dtype=torch.float32 if f32 else torch.float64).reshape(R, ts.nA).contiguous()
        o = [torch.empty(R, dtype=torch.int32, device=dev) for _ in range(4)]
        L.check(L.load().offsim_step_exo(C.byref(ts.c), C.byref(self.tx.c), C.byref(self.rs.c), C.byref(self.rx.c), L.ptr(p),
                                         L.PROB_F32 if f32 else L.PROB_F64, L.ptr(o[0]), L.ptr(o[1]), L.ptr(o[2]), L.ptr(o[3]), L.stream_ptr()))
        return tuple(o)

    def _run(self, pi_obs, obs_of, gamma, n_episodes, reseed, episode0, ep_cap, trace_cap, n_gamma_pow, td):
        ts, tx, dev, R = self.ts, self.tx, self.ts.device, self.R
        if reseed not in _RESEED:
            raise ValueError(f"reseed must be 'episode' or 'none', got {reseed!r}")
        if not isinstance(pi_obs, torch.Tensor):
            pi_obs = torch.from_numpy(np.ascontiguousarray(pi_obs))
        mode = L.PROB_F64 if td is not None else _prob_mode(ts, pi_obs.dtype)
        n_obs = int(pi_obs.shape[0])
        pi_d = pi_obs.to(device=dev, dtype=torch.float32 if mode == L.PROB_F32 else torch.float64).reshape(n_obs, ts.nA).contiguous()
        ob = torch.as_tensor(np.ascontiguousarray(obs_of, dtype=np.int32) if not isinstance(obs_of, torch.Tensor) else obs_of)
        ob = ob.to(device=dev, dtype=torch.int32).reshape(ts.n_slots, tx.n_slots).contiguous()
        n_episodes = episode_bound(n_episodes)
        o, oc = rollout_outputs(R, dev, ep_cap, trace_cap)
        o["last"] = torch.full((R, 3), -1, dtype=torch.int32, device=dev)
        if trace_cap:
            o["trace_row_x"] = torch.full((R, trace_cap), -1, dtype=torch.int32, device=dev)
        tdc, keep = None, ()
        if td is not None:
            q = td["q_obs"]
            q = torch.zeros((R, n_obs, ts.nA), dtype=torch.float64, device=dev) if q is None else \
                torch.as_tensor(q, dtype=torch.float64).to(dev).reshape(R, n_obs, ts.nA).contiguous().clone()
            td_outputs(o, q, trace_cap, td["snap_cap"])
            a_ep = None if td["alpha_ep"] is None else torch.as_tensor(np.ascontiguousarray(td["alpha_ep"], dtype=np.float64)).to(dev)
            tdc = L.TD(mode=td["mode"], alpha=float(td["alpha"]), q=L.ptr(q), td_err=L.ptr(o.get("td_err")), td_cap=trace_cap,
                       behaviour=int(td["behaviour"]), epsilon=0.0, alpha_ep=L.ptr(a_ep), epsilon_ep=None, n_sched=0 if a_ep is None else a_ep.numel(),
                       q_snap=L.ptr(o.get("q_snap")), snap_cap=td["snap_cap"], snap_stride=max(int(td["snap_stride"]), 1), tie_mt=None, beh_arg=None)
            o["q"] = q
            keep = (a_ep,)
        gp = _gamma_pow(gamma, n_gamma_pow, dev, cap=ts.N + 2)
        xo = L.ExoOut(trace_row_x=L.ptr(o.get("trace_row_x")), last=L.ptr(o["last"]))
        L.check(L.load().offsim_eval_mc_exo(C.byref(ts.c), C.byref(tx.c), C.byref(self.rs.c), C.byref(self.rx.c), L.ptr(pi_d), L.ptr(ob), n_obs, mode,
                                            _RESEED[reseed], int(episode0), float(gamma), L.ptr(gp), gp.numel(), int(n_episodes), C.byref(oc),
                                            C.byref(xo), None if tdc is None else C.byref(tdc), L.stream_ptr()))
        o["_keepalive"] = (pi_d, ob, gp) + keep
        o["_kernel"] = "k_eval_mc_exo"
        return o

    def eval_mc(self, pi_obs, obs_of, gamma, n_episodes=None, reseed="episode", episode0=0, ep_cap=0, trace_cap=0, n_gamma_pow=4096):
        """evalMC_psrs (psrs.py:241-271) on every rollout in one launch.  pi_obs [n_obs, nA]: the policy per compact observation row;
        obs_of [ns_slots, nx_slots]: the row of every (s, x) pair, -1 without one (tabulate_obs).  reseed = "episode": episode e draws
        from default_rng(episode0 + e), the reference's protocol; "none": every rollout's own stream runs on.  Returns a dict of device
        tensors: sum_g, n_ep, steps, cand, n_len, status, last [R,3] (+ ep_g, ep_len, trace_row, trace_row_x, trace_pop when asked)."""
        return self._run(pi_obs, obs_of, gamma, n_episodes, reseed, episode0, ep_cap, trace_cap, n_gamma_pow, None)

    def eval_td(self, pi_obs, obs_of, gamma, mode, alpha, q_obs=None, n_episodes=None, reseed="episode", episode0=0, ep_cap=0, trace_cap=0,
                n_gamma_pow=4096, behaviour=L.BEHAVIOUR_FIXED, alpha_ep=None, snap_cap=0, snap_stride=1):
        """qlearn_psrs / expSARSA_psrs (mode: _lib.TD_QLEARN | _lib.TD_EXPSARSA) with the fixed behaviour policy pi_obs, one launch.
        q_obs [R, n_obs, nA] f64 (Q_init in compact rows; zeros if None) comes back updated as out["q"]; out["td_err"] [R, trace_cap];
        alpha_ep: alpha per episode; snap_cap > 0: out["q_snap"] [R, snap_cap, n_obs, nA] = Q after every snap_stride-th step."""
        td = dict(mode=mode, alpha=alpha, q_obs=q_obs, behaviour=behaviour, alpha_ep=alpha_ep, snap_cap=int(snap_cap), snap_stride=snap_stride)
        return self._run(pi_obs, obs_of, gamma, n_episodes, reseed, episode0, ep_cap, trace_cap, n_gamma_pow, td)

    # -- the learner drivers for L learners on this environment's R seeds, any behaviour policy on the learner's own Q, in one launch --
    def eval_td_population(self, mode, alpha, gamma, obs_of, behaviour=L.BEHAVIOUR_FIXED, epsilon=0.0, pi_obs=None, q_obs=None, alpha_ep=None,
                           epsilon_ep=None, n_episodes=None, reseed="episode", episode0=0, ep_cap=0, trace_cap=0, snap_cap=0, tie_mt=None,
                           snap_stride=1, n_gamma_pow=4096):
        """qlearn_psrs / expSARSA_psrs for L learners, each on every one of this environment's S = R rollouts (its seeds): L * S rollouts in
        one launch that share the S queue orders of both families (include/offsim.h, offsim_eval_td_exo_pop).  behaviour (_lib.BEHAVIOUR_*):
        FIXED rejects against pi_obs; EPS_GREEDY (epsilon 0: greedy) and SOFT_GREEDY act on the learner's own Q row of the current
        observation, pi_obs then being only the target of expected SARSA.  alpha, gamma, behaviour and epsilon are each a scalar or [L];
        pi_obs [n_obs,nA] or [L,n_obs,nA] (None: uniform) and q_obs [n_obs,nA], [L,...], [L,S,...] (None: zeros) in the compact rows of
        obs_of [ns_slots, nx_slots] (tabulate_obs), whose largest entry + 1 is n_obs unless pi_obs / q_obs say more; alpha_ep / epsilon_ep
        [n_sched] or [L,n_sched]; tie_mt [L,S,625] NumPy MT19937 states for ties between maxima (None: the first maximum).  L is the
        common length of the per-learner arguments; L = 1 is the single learner.  reseed / episode0: eval_td's.
        Returns eval_td's dict with [L, S, ...] leading dimensions (+ beh_arg, tie_mt where they apply); with BEHAVIOUR_FIXED entry [l, j]
        is, bit for bit, what eval_td gives rollout j under learner l's setting.  It is a query, like BatchedPSRS.eval_td_population: it
        runs on copies of the sampler state of both families (every learner of seed j sees the same queues and, with reseed "none", the
        same stream state), and this environment's own cursors, rejection streams and current slots are left as they were; o["_state"]
        holds where every learner's sampler stands afterwards (rng, cursor, init_cursor, cur_slot of the s family; *_x of the x family)."""
        ts, tx, dev, S = self.ts, self.tx, self.ts.device, self.R
        if reseed not in _RESEED:
            raise ValueError(f"reseed must be 'episode' or 'none', got {reseed!r}")
        ob = torch.as_tensor(np.ascontiguousarray(obs_of, dtype=np.int32) if not isinstance(obs_of, torch.Tensor) else obs_of)
        ob = ob.to(device=dev, dtype=torch.int32).reshape(ts.n_slots, tx.n_slots).contiguous()
        given = next((x for x in (pi_obs, q_obs) if x is not None), None)
        n_obs = int(given.shape[-2]) if given is not None else max(int(ob.max()) + 1, 1)
        n_l, o, oc, pc, keep = td_population_launch("eval_td_population", dev, S, n_obs, ts.nA, ts.N, mode, alpha, gamma, behaviour, epsilon, pi_obs, q_obs,
                                                    alpha_ep, epsilon_ep, tie_mt, n_gamma_pow, ep_cap, trace_cap, snap_cap, snap_stride,
                                                    names=("pi_obs", "q_obs", "n_obs"))
        R = n_l * S
        o["last"] = torch.full((R, 3), -1, dtype=torch.int32, device=dev)
        if trace_cap:
            o["trace_row_x"] = torch.full((R, trace_cap), -1, dtype=torch.int32, device=dev)
        ro_s, cp_s = population_state(self.rs, n_l)
        ro_x, cp_x = population_state(self.rx, n_l)
        xo = L.ExoOut(trace_row_x=L.ptr(o.get("trace_row_x")), last=L.ptr(o["last"]))
        L.check(L.load().offsim_eval_td_exo_pop(C.byref(ts.c), C.byref(tx.c), C.byref(ro_s), C.byref(ro_x), n_l, S, C.byref(pc), L.ptr(ob), n_obs,
                                                _RESEED[reseed], int(episode0), int(episode_bound(n_episodes)), C.byref(oc), C.byref(xo), L.stream_ptr()))
        copies = dict(cp_s, **{k + "_x": v for k, v in cp_x.items() if k != "rng"})
        return population_result(o, n_l, S, copies, keep + (ob, cp_x["rng"]), "k_eval_td_exo_pop", state=True)


def evalmc_rollouts_exo(env_or_tables, seeds, pi, gamma, obs_of=None, reseed="episode", n_episodes=None, tile=None):
    """evalMC_psrs on a PSRS_Exo log for many sampler seeds, one launch per tile of seeds.  `env_or_tables`: a PSRS_Exo -- `pi` [nO, nA] is
    then indexed by the observation -- or a pair (ts, tx) of TransitionTables with `obs_of` given and `pi` in its compact rows.  Returns
    the dictionary of evalmc_rollouts: host arrays sum_g, n_ep, steps, cand, status and value = sum_g / n_ep."""
    seeds = np.asarray(seeds, dtype=np.uint64)
    if isinstance(env_or_tables, PSRS_Exo):
        ts, tx = env_or_tables.ts, env_or_tables.tx
        pi = np.asarray(pi)
        obs_of, ids = env_or_tables.obs_table(pi.shape[0])
        pi = pi[ids]
    else:
        ts, tx = env_or_tables
        if obs_of is None:
            raise ValueError("evalmc_rollouts_exo: a pair of tables needs obs_of")
    tile = len(seeds) if tile is None else int(tile)
    outs = {k: [] for k in HOST_KEYS}
    for _, sd, env in seed_tiles(seeds, max(tile, 1), lambda n: BatchedPSRSExo(ts, tx, n)):
        env.reset_sampler(sd)
        collect_host(outs, env.eval_mc(pi, obs_of, gamma, n_episodes, reseed=reseed))
    return host_result(outs, empty=0)


class PSRS_Exo:
    def __init__(self, buffer, nO=25, nA=5, o_split_func=lambda o: (o, 0), o_combine_func=lambda s, x: s):
        rows = list(buffer)  # (o, a, r, o', done, p, info)
        self.raw_buffer = rows
        self.nS = self.nO = nO
        self.nA = nA
        self.o_split_func, self.o_combine_func = o_split_func, o_combine_func
        n = len(rows)
        sx = [o_split_func(r[0]) for r in rows]
        sx_ = [o_split_func(r[3]) for r in rows]
        s = np.fromiter((int(v[0]) for v in sx), np.int64, n)
        x = np.fromiter((int(v[1]) for v in sx), np.int64, n)
        s_ = np.fromiter((int(v[0]) for v in sx_), np.int64, n)
        x_ = np.fromiter((int(v[1]) for v in sx_), np.int64, n)
        a = np.fromiter((int(r[1]) for r in rows), np.int64, n)
        rew = np.array([r[2] for r in rows], dtype=np.float64) if n else np.zeros(0)
        done = np.fromiter((bool(r[4]) for r in rows), bool, n)
        p_log = np.stack([np.asarray(r[5]) for r in rows]) if n else np.zeros((0, nA))
        t0 = np.fromiter((r[6]["t"] == 0 for r in rows), bool, n)
        self._s, self._x, self._s_next, self._x_next = s, x, s_, x_
        self.ts = TransitionTable(s, a, rew, s_, done, p_log, t0)
        self.tx = TransitionTable(x, np.zeros(n, np.int64), np.zeros(n), x_, np.zeros(n, bool), np.ones((n, 1), np.float32), t0)
        self.rs, self.rx = RolloutState(self.ts, 1), RolloutState(self.tx, 1)
        dev = self.ts.device
        self._o = torch.empty(4, dtype=torch.int32, device=dev)
        self._row = torch.empty(1, dtype=torch.int32, device=dev)
        self.o = None
        self.s = None
        self.reset_sampler()
        self.reset()

    def reset_sampler(self, seed=None):
        """psrs.py:77-89: init queue and every s- and x-queue shuffled by a fresh default_rng(seed)."""
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little")
        sd = seeds_tensor([seed], self.ts.device)
        for t, ro in ((self.ts, self.rs), (self.tx, self.rx)):
            perm, init_perm = shuffle_queues(t, sd)
            ro.rewind()
            ro.set_orders(perm, t.N, init_perm, t.N0)

    def reset(self, seed=None):
        """psrs.py:91-97: the rejection stream restarts from `seed` at EVERY reset."""
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little")
        seed_streams(seeds_tensor([seed], self.ts.device), self.rs.rng)
        lib = L.load()
        L.check(lib.offsim_env_reset(C.byref(self.ts.c), C.byref(self.rs.c), None, L.ptr(self._row), L.stream_ptr()))
        L.check(lib.offsim_env_reset(C.byref(self.tx.c), C.byref(self.rx.c), None, None, L.stream_ptr()))
        row = int(self._row.cpu()[0])
        if row < 0:
            self.s = None
            return None
        self.o = self.raw_buffer[row][0]
        return self.o

    def step(self, p_new):
        """psrs.py:99-117"""
        if isinstance(p_new, torch.Tensor):
            p_new = p_new.detach().cpu().numpy()
        p_new = np.asarray(p_new)
        f32 = p_new.dtype == np.float32 and self.ts.p_log.dtype == torch.float32
        p = torch.from_numpy(np.ascontiguousarray(p_new.reshape(1, -1))).to(self.ts.device, torch.float32 if f32 else torch.float64)
        s_cur, x_cur = self.o_split_func(self.o)
        base = self._o.data_ptr()
        L.check(L.load().offsim_step_exo(C.byref(self.ts.c), C.byref(self.tx.c), C.byref(self.rs.c), C.byref(self.rx.c), L.ptr(p),
                                         L.PROB_F32 if f32 else L.PROB_F64, base, base + 4, base + 8, base + 12, L.stream_ptr()))
        row_s, row_x, status, _ = self._o.cpu().tolist()
        if status == L.ST_KEYERROR:
            raise KeyError((s_cur, x_cur))
        if status != L.ST_OK:
            return None, None, None, None
        rs_ = self.raw_buffer[row_s]
        self.o = self.o_combine_func(int(self._s_next[row_s]), int(self._x_next[row_x]))
        return self.o, rs_[2], bool(rs_[4]), {"s": s_cur, "a": rs_[1], "p": rs_[5]}

    def obs_table(self, n_rows=None):
        """(obs_of, obs_ids) of tabulate_obs over this environment's slot grid, for a pi / Q of n_rows rows (default nO)."""
        return tabulate_obs(self.ts.slot_z, self.tx.slot_z, self.o_combine_func, self.nO if n_rows is None else n_rows)


# ---------------------------------------------------------------------------------------------------
# The reference's drivers on a PSRS_Exo (psrs.py:119-271), one launch each; evaluators/psrs.py hands them here
# ---------------------------------------------------------------------------------------------------
def _launch(env, pi, n_rows, run):
    """One driver call on `env`: the observation map, the launch through a view of the environment's own rollout state, the errors the
    reference raises, and env.o / env.s as its loop leaves them.  Returns (outputs, obs_ids, initial rows served)."""
    obs_of, ids = env.obs_table(n_rows)
    b = BatchedPSRSExo(env.ts, env.tx, 1, env.rs, env.rx)
    ic0 = int(env.rs.init_cursor.cpu()[0])
    o = run(b, obs_of, ids)
    status = int(o["status"].cpu()[0])
    L.check_async_faults()  # (the copy above synchronised the stream)
    ss, xs = int(env.rs.cur_slot.cpu()[0]), int(env.rx.cur_slot.cpu()[0])
    row_s, row_x, row0 = (int(v) for v in o["last"].cpu()[0])
    if row_s >= 0:
        env.o = env.o_combine_func(int(env._s_next[row_s]), int(env._x_next[row_x]))
    elif row0 >= 0:
        env.o = env.raw_buffer[row0][0]
    if status == L.ST_NO_INIT:
        env.s = None
    if status == L.ST_KEYERROR:
        known = 0 <= ss < env.ts.n_slots and 0 <= xs < env.tx.n_slots
        if known and obs_of[ss, xs] < 0:
            raise IndexError(f"observation {env.o} has no row in a table of {n_rows} rows")
        raise KeyError((env.ts.z_of(ss), env.tx.z_of(xs)) if known else env.o)
    ic1 = int(env.rs.init_cursor.cpu()[0])
    order = env.rs.init_perm.cpu().numpy().reshape(-1)[:env.ts.N0].astype(np.int64) if env.rs.init_perm is not None else np.arange(env.ts.N0)
    init_rows = env.ts.init_orig.cpu().numpy()[order[ic0:ic1]]
    return o, ids, init_rows


def evalmc_exo(env, n_episodes, pi, gamma):
    """evalMC_psrs(env, ...) for a PSRS_Exo: (Gs, lengths)."""
    pi = np.asarray(pi)
    if pi.ndim != 2:
        raise ValueError("evalMC_psrs: pi must be a [nO, nA] table")
    n_ep = int(min(n_episodes, env.ts.N0 + 1))
    o, _, _ = _launch(env, pi, pi.shape[0], lambda b, obs_of, ids: b.eval_mc(pi[ids], obs_of, gamma, n_ep, ep_cap=max(n_ep, 1)))
    ne, nl = int(o["n_ep"].cpu()[0]), int(o["n_len"].cpu()[0])
    return o["ep_g"].cpu().numpy()[0, :ne].copy(), o["ep_len"].cpu().numpy()[0, :nl].astype(np.int64)


class _ExoStepMemory:
    """The `memory` list of the learner drivers on a PSRS_Exo: (S, A, R, S', done, p, info) per accepted step, built on first use."""

    def __init__(self, env, rows_s, rows_x, init_rows, pi):
        self._env, self._rows_s, self._rows_x, self._init, self._pi, self._items = env, rows_s, rows_x, init_rows, pi, None

    def _build(self):
        if self._items is None:
            env, items, ep, S = self._env, [], 0, None
            for rs_, rx_ in zip(self._rows_s, self._rows_x):
                if S is None:
                    S = env.raw_buffer[int(self._init[ep])][0]
                    ep += 1
                b = env.raw_buffer[rs_]
                S_ = env.o_combine_func(int(env._s_next[rs_]), int(env._x_next[rx_]))
                items.append((S, b[1], b[2], S_, bool(b[4]), self._pi[S], {"s": int(env._s[rs_]), "a": b[1], "p": b[5]}))
                S = None if b[4] else S_
            self._items = items
        return self._items

    def __len__(self):
        return len(self._rows_s)

    def __iter__(self):
        return iter(self._build())

    def __getitem__(self, i):
        return self._build()[i]


def td_exo(env, what, n_episodes, gamma, alpha, Q_init, save_Q, mode, pi):
    """qlearn_psrs / expSARSA_psrs for a PSRS_Exo with the fixed behaviour policy pi [nO, nA]: (Q, info) as the reference returns them."""
    Q0 = np.zeros((env.nS, env.nA)) if Q_init is None else np.asarray(Q_init).copy().astype(float)
    if pi.shape[0] < Q0.shape[0]:
        raise IndexError(f"{what}: pi has fewer rows than Q")
    n_ep = int(min(n_episodes, env.ts.N0 + 1))
    a_tab = np.array([float(alpha(e)) for e in range(max(n_ep, 1))], dtype=np.float64) if callable(alpha) else None
    cap = env.ts.N + 1
    o, ids, init_rows = _launch(env, pi, Q0.shape[0], lambda b, obs_of, ids: b.eval_td(
        pi[ids], obs_of, gamma, mode, 0.0 if callable(alpha) else alpha, q_obs=Q0[ids][None], n_episodes=n_ep, ep_cap=n_ep + 1, trace_cap=cap,
        alpha_ep=a_tab, snap_cap=cap if save_Q else 0))
    status, ne, steps = int(o["status"].cpu()[0]), int(o["n_ep"].cpu()[0]), int(o["steps"].cpu()[0])
    n_g = ne + (1 if status == L.ST_EXHAUSTED else 0)  # the cut-short episode's return is appended too (psrs.py:177, :232)

    def full(q):  # compact rows back into copies of the [nO, nA] table
        out = np.broadcast_to(Q0, q.shape[:-2] + Q0.shape).copy()
        out[..., ids, :] = q
        return out
    Q = full(o["q"].cpu().numpy()[0])
    Qs = np.array([Q0])
    if save_Q:  # psrs.py:145, :172-173: Q before the first step, then after every step
        Qs = np.concatenate([Q0[None], full(o["q_snap"].cpu().numpy()[0, :steps])], axis=0)
    rows_s, rows_x = o["trace_row"].cpu().numpy()[0, :steps], o["trace_row_x"].cpu().numpy()[0, :steps]
    info = {"Gs": o["ep_g"].cpu().numpy()[0, :n_g].copy(), "Qs": Qs, "memory": _ExoStepMemory(env, rows_s, rows_x, init_rows, pi)}
    if mode == L.TD_QLEARN:
        info["TD_errors"] = o["td_err"].cpu().numpy()[0, :steps].copy()
    return Q, info
