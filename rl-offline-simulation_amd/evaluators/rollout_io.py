"""Host-side plumbing shared by every launch of the rollout kernels (k_eval_mc and its kin) and by the seed-tile drivers above them.

  rollout_outputs     the output dict of a launch and its struct offsim_evalmc_out (the one place that states dtypes, fills, shapes)
  td_outputs          the learner kernels' extras: td_err, beh_arg, q_snap
  tie_stream          a caller's MT19937 states as the int32 tensor the kernels read
  td_env_launch / td_driver_schedules   the learner struct and the schedule / tie preamble of the drivers on a true environment
  td_population_launch   the per-learner arguments of a population of learners as struct offsim_td_pop, with its outputs
  population_state / population_result   a population launch's copies of the sampler state, and its dict as [n, S, ...]
  seed_tiles / collect_host / host_result   the loop over tiles of sampler seeds and the host arrays it returns
  population_host_result   the same for a population of policies on the seeds: [L, S] arrays, mean_value, best
  episode_bound, _gamma_pow, _prob_mode     the episode limit, the discount table and the probability mode of a launch

A leaf: it imports _lib, ctypes, torch and NumPy only, so batched.py, psrs_exo.py and td_population.py all import it at module top.
"""
import ctypes as C
import warnings

import numpy as np
import torch

from .. import _lib as L

_GP_CACHE = {}
_GP_CACHE_BYTES = 256 << 20


def _gamma_pow(gamma, n, device, cap=None):
    """gamma**t exactly as the host computes it for the reference (Python float ** int == libm pow, psrs.py:262), for every
    t an episode can reach: at least `n` entries, then on until the factor is stationary (0, inf or 1: the device clamps t to
    the last entry in that case, csrc/discount.hpp) or `cap` entries (an episode has at most N steps) are there.  Built in
    blocks of 65536 with Python's own `float ** int` (NumPy's array pow is vectorised differently and differs in the last bit for
    some t), so a gamma below 1 stops after the block its factor underflows in; the cache is bounded by bytes (_GP_CACHE_BYTES)."""
    g = float(gamma)
    cap = max(int(n), 2) if cap is None else max(int(cap), int(n), 2)
    key = (g, int(n), cap, str(device))
    if key not in _GP_CACHE:
        stationary = lambda v: len(v) >= 2 and v[-1] == v[-2] and (v[-1] in (0.0, 1.0) or np.isinf(v[-1]))
        blocks, total = [], 0
        while total < max(int(n), 2) or (total < cap and not stationary(blocks[-1])):
            m = min(65536, (max(int(n), 2) if total < max(int(n), 2) else cap) - total)
            blocks.append(np.array([g ** t for t in range(total, total + m)], dtype=np.float64))  # (Python's own pow: NumPy's array pow is not bit-identical)
            total += m
        vals = np.concatenate(blocks)
        keep = len(vals)
        while keep > max(int(n), 2) and vals[keep - 1] == vals[keep - 2] == vals[keep - 3] and (vals[keep - 1] in (0.0, 1.0) or np.isinf(vals[keep - 1])):
            keep -= 1  # (extended in blocks: keep exactly two stationary entries)
        if sum(v.numel() * 8 for v in _GP_CACHE.values()) + keep * 8 > _GP_CACHE_BYTES:
            _GP_CACHE.clear()
        _GP_CACHE[key] = torch.from_numpy(vals[:keep].copy()).to(device)
    return _GP_CACHE[key]


def _prob_mode(table, p_dtype):
    f32 = (p_dtype in (np.float32, torch.float32, np.dtype(np.float32))) and table.p_log.dtype == torch.float32
    return L.PROB_F32 if f32 else L.PROB_F64


def episode_bound(n_episodes):
    """The kernels' episode limit: None (until the log ends) is a bound no log reaches."""
    return 1 << 62 if n_episodes is None else int(n_episodes)


_REQUIRED = (("sum_g", torch.float64), ("n_ep", torch.int64), ("steps", torch.int64), ("cand", torch.int64), ("n_len", torch.int64),
             ("status", torch.int32))


def rollout_outputs(R, device, ep_cap=0, trace_cap=0, out=None, dbg=False):
    """(dict of output tensors, struct offsim_evalmc_out pointing at them) of a launch of R rollouts.  The six required outputs [R]
    are left uninitialised (the kernel writes every entry) and taken from `out` where the caller supplies them; ep_g [R, ep_cap] and
    ep_len [R, ep_cap + 1] (zeros), trace_row (-1) and trace_pop (zeros) [R, trace_cap], and dbg [R, 4] exist only when asked for
    and are always allocated afresh; an absent one is a NULL pointer in the struct."""
    o = out or {}
    for k, dt in _REQUIRED:
        if k not in o:
            o[k] = torch.empty(R, dtype=dt, device=device)
    if ep_cap:
        o["ep_g"] = torch.zeros((R, ep_cap), dtype=torch.float64, device=device)
        o["ep_len"] = torch.zeros((R, ep_cap + 1), dtype=torch.int32, device=device)
    if trace_cap:
        o["trace_row"] = torch.full((R, trace_cap), -1, dtype=torch.int32, device=device)
        o["trace_pop"] = torch.zeros((R, trace_cap), dtype=torch.int32, device=device)
    if dbg:
        o["dbg"] = torch.zeros((R, 4), dtype=torch.int64, device=device)
    oc = L.EvalMCOut(sum_g=L.ptr(o["sum_g"]), n_ep=L.ptr(o["n_ep"]), steps=L.ptr(o["steps"]), cand=L.ptr(o["cand"]), n_len=L.ptr(o["n_len"]),
                     status=L.ptr(o["status"]), ep_g=L.ptr(o.get("ep_g")), ep_len=L.ptr(o.get("ep_len")), ep_cap=ep_cap,
                     trace_row=L.ptr(o.get("trace_row")), trace_pop=L.ptr(o.get("trace_pop")), trace_cap=trace_cap, dbg=L.ptr(o.get("dbg")))
    return o, oc


def td_outputs(o, q, trace_cap, snap_cap, beh_arg=False):
    """The extras of a learner launch on the Q tables q [R, rows, nA], added to `o`: td_err [R, trace_cap] f64 and, for a launch with an
    epsilon-greedy behaviour (`beh_arg`), beh_arg [R, trace_cap] int32 when trace_cap > 0; q_snap [R, snap_cap, rows, nA] f64 when
    snap_cap > 0.  All zeros."""
    R, dev = q.shape[0], q.device
    if trace_cap:
        o["td_err"] = torch.zeros((R, trace_cap), dtype=torch.float64, device=dev)
        if beh_arg:
            o["beh_arg"] = torch.zeros((R, trace_cap), dtype=torch.int32, device=dev)
    if snap_cap:
        o["q_snap"] = torch.zeros((R, snap_cap, *q.shape[1:]), dtype=torch.float64, device=dev)


def tie_stream(tie_mt, device=None):
    """NumPy MT19937 states [..., 625] (int32 / uint32 words, array or tensor) as an int32 tensor on `device` (None: where it is).  A
    tensor that already is one comes back as itself, so a launch advances the caller's states in place."""
    mt = torch.as_tensor(np.ascontiguousarray(tie_mt).view(np.int32) if not isinstance(tie_mt, torch.Tensor) else tie_mt)
    return mt.to(device=device, dtype=torch.int32)


def td_env_launch(td, R, rows, nA, device, o, trace_cap):
    """The learner of a launch on a true environment (BatchedGridWorld.eval_td, BatchedLatentEnv.eval_td), from the dict `td` those methods
    make of their arguments -- mode, alpha, q [R,rows,nA] or None (zeros), behaviour, epsilon, alpha_ep / epsilon_ep, snap_cap, snap_stride,
    tie: None / "first" (the first maximum), "episode" (the stream restarts at every episode: a fresh [R,625] state), or MT19937 states
    advanced in place.  Adds q, tie_mt and the learner extras to `o`; returns (struct offsim_td, what the launch must keep alive, the
    tie_reseed_episode flag)."""
    dev = device
    q = td["q"]
    q = torch.zeros((R, rows, nA), dtype=torch.float64, device=dev) if q is None else \
        torch.as_tensor(q, dtype=torch.float64).to(dev).reshape(R, rows, nA).contiguous().clone()
    behaviour = int(td["behaviour"])
    td_outputs(o, q, trace_cap, td["snap_cap"], beh_arg=behaviour == L.BEHAVIOUR_EPS_GREEDY)
    a_ep, e_ep = (None if x is None else torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).to(dev) for x in (td["alpha_ep"], td["epsilon_ep"]))
    n_sched = max(a_ep.numel() if a_ep is not None else 0, e_ep.numel() if e_ep is not None else 0)
    assert all(x is None or x.numel() == n_sched for x in (a_ep, e_ep)), "alpha_ep and epsilon_ep cover the same episodes"
    tie, mt, reseed = td["tie"], None, 0
    if isinstance(tie, str) and tie == "episode":
        reseed = 1
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
    return tdc, (a_ep, e_ep), reseed


def td_driver_schedules(schedule, alpha, epsilon, kind, n_ep, tie):
    """The preamble of a reference learner driver on a true environment (qlearn_env / expSARSA_env and their latent forms): the behaviour
    code of `kind`, alpha(episode) / epsilon(episode) tabulated for n_ep episodes by `schedule` (the caller's psrs._schedule; each filled with its constant when only the other is a
    schedule; "greedy" is epsilon 0), and tie = "global" turned into NumPy's global MT19937 state as it stands.  Returns (behaviour, a_tab,
    e_tab, epsilon, tie, the global state before the call)."""
    a_tab, e_tab = schedule(alpha, n_ep), schedule(epsilon, n_ep)
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
    return behaviour, a_tab, e_tab, epsilon, tie, st


def td_population_launch(who, device, S, rows, nA, n_log, mode, alpha, gamma, behaviour, epsilon, pi, q, alpha_ep, epsilon_ep, tie_mt, n_gamma_pow,
                         ep_cap, trace_cap, snap_cap, snap_stride, names=("pi_slots", "q_slots", "n_slots")):
    """The arguments of a launch of L learners on S seeds (offsim_eval_td_pop, offsim_eval_td_exo_pop), from what `who` -- a method
    eval_td_population -- was given: alpha, gamma, behaviour (_lib.BEHAVIOUR_*) and epsilon a scalar or [L]; pi [rows,nA] or [L,rows,nA]
    (None: uniform); q [rows,nA], [L,...], [L,S,...] or None (zeros); alpha_ep / epsilon_ep [n_sched] or [L,n_sched]; tie_mt [L,S,625] or
    None.  L is the common length of the per-learner arguments (1 when every one is shared); lengths that disagree raise ValueError.
    `rows`: the rows of pi / Q (state slots, or compact observation rows); n_log: the log's rows (an episode's longest); names: what the
    messages call pi, q and rows.  Returns (L, output dict with q / tie_mt / the learner extras, struct offsim_evalmc_out, struct
    offsim_td_pop, what the launch must keep alive)."""
    dev = device
    pi_name, q_name, rows_name = names
    f64 = lambda x: np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float64)  # noqa: E731
    per = {"alpha": np.atleast_1d(f64(alpha)), "gamma": np.atleast_1d(f64(gamma)), "epsilon": np.atleast_1d(f64(epsilon)),
           "behaviour": np.atleast_1d(np.asarray(behaviour, dtype=np.int64))}
    if any(v.ndim != 1 for v in per.values()):
        raise ValueError(f"{who}: alpha, gamma, behaviour and epsilon are scalars or [L]")
    lens = {k: len(v) for k, v in per.items() if len(v) != 1}
    pi_t = None if pi is None else torch.as_tensor(pi if isinstance(pi, torch.Tensor) else np.ascontiguousarray(pi), dtype=torch.float64)
    if pi_t is not None:
        if pi_t.dim() not in (2, 3) or tuple(pi_t.shape[-2:]) != (rows, nA):
            raise ValueError(f"{who}: {pi_name} [{rows_name},nA] or [L,{rows_name},nA] expected, got {tuple(pi_t.shape)}")
        if pi_t.dim() == 3:
            lens[pi_name] = int(pi_t.shape[0])
    q_t = None if q is None else torch.as_tensor(q if isinstance(q, torch.Tensor) else np.ascontiguousarray(q), dtype=torch.float64)
    if q_t is not None:
        if q_t.dim() not in (2, 3, 4) or tuple(q_t.shape[-2:]) != (rows, nA) or (q_t.dim() == 4 and q_t.shape[1] != S):
            raise ValueError(f"{who}: {q_name} [{rows_name},nA], [L,{rows_name},nA] or [L,S,{rows_name},nA] expected, got {tuple(q_t.shape)}")
        if q_t.dim() > 2:
            lens[q_name] = int(q_t.shape[0])
    sched = {}
    for k, x in (("alpha_ep", alpha_ep), ("epsilon_ep", epsilon_ep)):
        if x is not None:
            sched[k] = np.atleast_1d(f64(x))
            if sched[k].ndim not in (1, 2) or sched[k].shape[-1] < 1:
                raise ValueError(f"{who}: {k} [n_sched] or [L,n_sched] expected")
            if sched[k].ndim == 2:
                lens[k] = sched[k].shape[0]
    mt = None
    if tie_mt is not None:
        mt = tie_stream(tie_mt)
        if mt.dim() != 3 or tuple(mt.shape[1:]) != (S, 625):
            raise ValueError(f"{who}: tie_mt [L,S,625] expected, got {tuple(mt.shape)}")
        lens["tie_mt"] = int(mt.shape[0])
    if len(set(lens.values())) > 1:
        raise ValueError(f"{who}: per-learner arguments of different lengths: {lens}")
    n_l = next(iter(lens.values())) if lens else 1
    if n_l < 1:
        raise ValueError(f"{who}: no learner")
    R = n_l * S
    beh_host = np.ascontiguousarray(np.broadcast_to(per["behaviour"], (n_l,)), dtype=np.int32)
    dev_f64 = lambda a: torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(dev)  # noqa: E731  (a copy: broadcasts are read-only)
    alpha_d, eps_d, gamma_d = (dev_f64(np.broadcast_to(per[k], (n_l,))) for k in ("alpha", "epsilon", "gamma"))
    beh_d = torch.from_numpy(beh_host).to(dev)
    n_sched = max([v.shape[-1] for v in sched.values()], default=0)
    assert all(v.shape[-1] == n_sched for v in sched.values()), "alpha_ep and epsilon_ep cover the same episodes"
    a_ep, e_ep = (dev_f64(np.broadcast_to(sched[k], (n_l, n_sched))) if k in sched else None for k in ("alpha_ep", "epsilon_ep"))
    if pi_t is None:
        pi_t = torch.full((rows, nA), 1.0 / nA, dtype=torch.float64)
    pi_d = pi_t.to(dev).contiguous()
    # the discount tables, one row per learner: each as eval_td builds it, the shorter ones (stationary) padded with their last entry
    gp_rows = [_gamma_pow(g, n_gamma_pow, dev, cap=n_log + 2) for g in np.broadcast_to(per["gamma"], (n_l,)).tolist()]
    n_gp = max(r.numel() for r in gp_rows)
    gp = torch.stack([r if r.numel() == n_gp else torch.cat([r, r[-1:].expand(n_gp - r.numel())]) for r in gp_rows]).contiguous()
    if q_t is None:
        qd = torch.zeros((R, rows, nA), dtype=torch.float64, device=dev)
    else:
        q_t = q_t.to(dev)
        qd = (q_t if q_t.dim() == 4 else q_t.reshape(-1, 1, rows, nA)).expand(n_l, S, rows, nA).reshape(R, rows, nA).contiguous().clone()
    o, oc = rollout_outputs(R, dev, ep_cap, trace_cap)
    td_outputs(o, qd, trace_cap, snap_cap, beh_arg=(beh_host == L.BEHAVIOUR_EPS_GREEDY).any())
    if mt is not None:  # (a copy: the caller's states stay where they were)
        mt = o["tie_mt"] = mt.to(dev).reshape(R, 625).contiguous().clone()
    pc = L.TDPop(mode=int(mode), alpha=L.ptr(alpha_d), epsilon=L.ptr(eps_d), gamma=L.ptr(gamma_d), gamma_pow=L.ptr(gp), n_gamma_pow=n_gp,
                 behaviour=L.ptr(beh_d), behaviour_host=beh_host.ctypes.data_as(C.POINTER(C.c_int32)), alpha_ep=L.ptr(a_ep), epsilon_ep=L.ptr(e_ep),
                 n_sched=n_sched, pi=L.ptr(pi_d), pi_stride=rows * nA if pi_d.dim() == 3 else 0, q=L.ptr(qd), td_err=L.ptr(o.get("td_err")),
                 td_cap=trace_cap, q_snap=L.ptr(o.get("q_snap")), snap_cap=snap_cap, snap_stride=max(int(snap_stride), 1), tie_mt=L.ptr(mt),
                 beh_arg=L.ptr(o.get("beh_arg")))
    o["q"] = qd
    return n_l, o, oc, pc, (pi_d, gp, alpha_d, eps_d, gamma_d, beh_d, a_ep, e_ep, beh_host)


def population_state(st, n_pop):
    """Copies of the sampler state `st` (a RolloutState of S rollouts) for n_pop members that each run all S rollouts: (struct
    offsim_rollouts of n_pop * S rollouts, dict of the repeated rng / cursor / init_cursor / cur_slot).  Member l's rollout j is row
    l * S + j.  The queue orders (perm, init_perm and their strides) are st's own, shared by all members; st itself is not touched."""
    cp = dict(rng=st.rng.repeat(n_pop, 1), cursor=st.cursor.repeat(n_pop, 1), init_cursor=st.init_cursor.repeat(n_pop),
              cur_slot=st.cur_slot.repeat(n_pop))
    ro = L.Rollouts(R=n_pop * st.rng.shape[0], perm=L.ptr(st.perm), perm_stride=st.perm_stride, init_perm=L.ptr(st.init_perm), init_stride=st.init_stride,
                    rng_kind=st.rng_kind, **{k: L.ptr(v) for k, v in cp.items()})
    return ro, cp


def population_result(o, n_pop, S, copies, keep, kernel, state=False):
    """What a population launch returns: every tensor of `o` [n_pop * S, ...] as [n_pop, S, ...], `keep` and the state copies kept
    alive, the kernel's name, and with `state` the copies themselves as o["_state"]: where every member's sampler stands afterwards."""
    split = lambda d: {k: v.reshape(n_pop, S, *v.shape[1:]) for k, v in d.items()}  # noqa: E731
    o = split(o)
    o["_keepalive"] = tuple(keep) + tuple(copies.values())
    if state:
        o["_state"] = split(copies)
    o["_kernel"] = kernel
    return o


def seed_tiles(seeds, tile, make_env):
    """The seed-tile loop of the drivers: yields (offset, the tile's seeds, environment) for tiles of `tile` seeds; make_env(n) builds
    an environment of n rollouts and is called only when the tile length changes (the last, shorter tile)."""
    env = n_env = None
    for b in range(0, len(seeds), tile):
        sd = seeds[b:b + tile]
        if len(sd) != n_env:
            env, n_env = make_env(len(sd)), len(sd)
        yield b, sd, env


HOST_KEYS = ("sum_g", "n_ep", "steps", "cand", "status")


def collect_host(parts, o):
    """Append the launch's outputs named in `parts` as host arrays, then look at the fault word (the copies synchronised the stream)."""
    for k in parts:
        parts[k].append(o[k].cpu().numpy())
    L.check_async_faults()


def host_result(parts, axis=0, empty=None):
    """The drivers' dictionary: every list of `parts` concatenated along `axis` (a driver that accepts no seeds at all gives `empty`, the
    shape of its empty arrays) and value = sum_g / n_ep, NaN where a seed completed no episode."""
    res = {k: np.concatenate(v, axis=axis) if v or empty is None else np.zeros(empty) for k, v in parts.items()}
    with np.errstate(invalid="ignore", divide="ignore"):
        res["value"] = res["sum_g"] / res["n_ep"]
    return res


def population_host_result(parts, n_pop):
    """The dictionary of the population drivers (evalmc_rollouts_population, evalmc_rollouts_queue_population): `parts` holds per seed tile
    the [n_pop, tile] arrays; host_result along the seeds, then mean_value [n_pop], the mean of value over the seeds that have one (NaN
    where none has), and best, the arg-max of mean_value (-1 when every mean is NaN)."""
    res = host_result(parts, axis=1, empty=(n_pop, 0))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (a policy without one completed episode: its mean is NaN, as its values are)
        res["mean_value"] = np.nanmean(res["value"], axis=1)
    res["best"] = -1 if np.isnan(res["mean_value"]).all() else int(np.nanargmax(res["mean_value"]))
    return res
