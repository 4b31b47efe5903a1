"""The argument validation of the six learner entry points, rule by rule: return code and the whole offsim_last_error() text.

offsim_eval_td, offsim_eval_td_pop, offsim_eval_mc_exo, offsim_eval_td_exo_pop, offsim_eval_queue and offsim_eval_queue_pop refuse bad
arguments before any HIP call, so the C ABI is called here without a device (as test_argument_validation_needs_no_device of
test_td_population_host.py does).  Every case starts from an accepted call (R = 0: nothing to run), changes the named arguments and
states what comes back.  A case that breaks two rules pins which check comes first.  The entry points do not agree on every rule (a
negative td_cap, a schedule without n_sched): the differences are pinned as they are.
"""
import ctypes
from types import SimpleNamespace

import pytest

from rl_offline_simulation_amd import _lib as L

OK, EINVAL, EUNSUP = L.OK, L.EINVAL, L.EUNSUPPORTED
P = 8  # any non-NULL pointer: nothing dereferences a device pointer before the launch


def _ref(x):
    return None if x is None else ctypes.byref(x)


def _table(n_slots=4):
    return L.Table(N=0, n_slots=n_slots, nA=2, plog_dtype=L.F32, r_dtype=L.F32)


def _rollouts():
    return L.Rollouts(R=0, rng=P, cursor=P, init_cursor=P, cur_slot=P)


def _out():
    return L.EvalMCOut(sum_g=P, n_ep=P, steps=P, cand=P, n_len=P, status=P)


def _td():
    return L.TD(mode=L.TD_QLEARN, q=P, snap_stride=1)


def _pop(beh):
    return L.TDPop(mode=L.TD_QLEARN, alpha=P, epsilon=P, gamma=P, behaviour=P, behaviour_host=beh, pi=P, q=P, snap_stride=1)


def _beh():
    return (ctypes.c_int32 * 2)(L.BEHAVIOUR_FIXED, L.BEHAVIOUR_FIXED)


def _base(entry):
    """The arguments of an accepted call of `entry`: two learners on three seeds where it is a population, R = 0."""
    a = SimpleNamespace(t=_table(), ro=_rollouts(), out=_out(), gamma_pow=None, n_gamma_pow=0, pi=P, td=_td(), L=2, S=3, beh=_beh(),
                        tx=_table(), rx=_rollouts(), obs_of=P, n_obs=3, prob_mode=L.PROB_F64, reseed=L.EXO_RESEED_NONE, nA_actions=2,
                        tie_reseed=0, episode0=0)
    a.pop = _pop(a.beh)
    return a


def _call(lib, entry, a):
    t, ro, out = _ref(a.t), _ref(a.ro), _ref(a.out)
    if entry == "eval_td":
        return lib.offsim_eval_td(t, ro, a.pi, L.REJECT_DEFAULT, 0.9, a.gamma_pow, a.n_gamma_pow, 1, out, _ref(a.td), None)
    if entry == "eval_td_pop":
        return lib.offsim_eval_td_pop(t, ro, a.L, a.S, _ref(a.pop), L.REJECT_DEFAULT, 1, out, None)
    if entry == "eval_mc_exo":
        return lib.offsim_eval_mc_exo(t, _ref(a.tx), ro, _ref(a.rx), a.pi, a.obs_of, a.n_obs, a.prob_mode, a.reseed, 0, 0.9, a.gamma_pow,
                                      a.n_gamma_pow, 1, out, None, _ref(a.td), None)
    if entry == "eval_td_exo_pop":
        return lib.offsim_eval_td_exo_pop(t, _ref(a.tx), ro, _ref(a.rx), a.L, a.S, _ref(a.pop), a.obs_of, a.n_obs, a.reseed, 0, 1, out, None, None)
    if entry == "eval_queue":
        return lib.offsim_eval_queue(t, ro, a.nA_actions, a.pi, 0.9, a.gamma_pow, a.n_gamma_pow, 1, out, _ref(a.td), a.tie_reseed, a.episode0, None,
                                     None)
    assert entry == "eval_queue_pop"
    return lib.offsim_eval_queue_pop(t, ro, a.nA_actions, a.L, a.S, _ref(a.pop), 1, out, a.tie_reseed, a.episode0, None, None)


def _apply(a, changes):
    """changes: "path=value" pairs as a flat tuple (path, value, path, value, ...); path "td.mode", "beh[1]", "ro" ..."""
    for path, value in zip(changes[::2], changes[1::2]):
        if path.startswith("beh["):
            a.beh[int(path[4:-1])] = value
            continue
        obj, _, name = path.rpartition(".")
        setattr(getattr(a, obj) if obj else a, name, value)


# ---- the rules, as (changes, return code, message) -------------------------------------------------------------------------------------

TABLE = [  # check_table, first in every entry point (behind the NULL pop of the exo / queue populations)
    (("t", None), EINVAL, "table is NULL"),
    (("t.n_slots", 0), EINVAL, "table: bad N / n_slots / nA"),
    (("t.nA", 0), EINVAL, "table: bad N / n_slots / nA"),
    (("t.N", -1), EINVAL, "table: bad N / n_slots / nA"),
    (("t.N", 1), EINVAL, "table: NULL column"),
    (("t.plog_dtype", 9), EINVAL, "table: bad plog_dtype"),
    (("t.r_dtype", 9), EINVAL, "table: bad r_dtype"),
    (("t.r_dtype", 9, "t.plog_dtype", 9), EINVAL, "table: bad plog_dtype"),
]
OUT = [  # check_evalmc_out
    (("out.sum_g", None), EINVAL, "{who}: required output is NULL"),
    (("out.status", None), EINVAL, "{who}: required output is NULL"),
    (("out.status", None, "{gp}n_gamma_pow", 4), EINVAL, "{who}: required output is NULL"),
    (("{gp}n_gamma_pow", 4), EINVAL, "{who}: gamma_pow is NULL"),
]
CAPS = [
    (("out.ep_cap", -1), EINVAL, "{who}: negative ep_cap / trace_cap"),
    (("out.trace_cap", -1), EINVAL, "{who}: negative ep_cap / trace_cap"),
]
SNAP = [
    (("{td}q_snap", P, "{td}snap_stride", 0), EINVAL, "{who}: bad snapshot stride / capacity"),
    (("{td}q_snap", P, "{td}snap_cap", -1), EINVAL, "{who}: bad snapshot stride / capacity"),
    (("{td}q_snap", P), OK, None),
    (("{td}snap_stride", 0), OK, None),
]
TD_MODE = [
    (("{td}mode", 0), EINVAL, "{who}: bad td mode or NULL q"),
    (("{td}mode", 3), EINVAL, "{who}: bad td mode or NULL q"),
    (("{td}mode", L.TD_EXPSARSA), OK, None),
    (("{td}q", None), EINVAL, "{who}: bad td mode or NULL q"),
]
LDS_MC = "{who}: Q table, cursors and policy exceed 160 KiB of LDS"
LDS_EXO = "{who}: obs_of, policy, Q table and cursors exceed 160 KiB of LDS"
LDS_QUEUE = "{who}: cursors, policy and Q table exceed 160 KiB of LDS"
PER_LEARNER = "{who}: a per-learner array is NULL (alpha, epsilon, gamma, behaviour and its host copy, pi)"


def _pop_rules(pi_optional):  # check_td_pop
    return [
        (("L", 0), EINVAL, "{who}: L must be 1..65535 and S >= 1"),
        (("L", 65536), EINVAL, "{who}: L must be 1..65535 and S >= 1"),
        (("S", 0), EINVAL, "{who}: L must be 1..65535 and S >= 1"),
        (("L", 0, "ro.R", 5, "rx.R", 5), EINVAL, "{who}: L must be 1..65535 and S >= 1"),
        (("ro.R", 5, "rx.R", 5), EINVAL, "{who}: ro->R must be L * S"),
        (("ro.R", 5, "rx.R", 5, "pop.alpha", None), EINVAL, "{who}: ro->R must be L * S"),
        (("pop.alpha", None), EINVAL, PER_LEARNER),
        (("pop.epsilon", None), EINVAL, PER_LEARNER),
        (("pop.gamma", None), EINVAL, PER_LEARNER),
        (("pop.behaviour", None), EINVAL, PER_LEARNER),
        (("pop.behaviour_host", None), EINVAL, PER_LEARNER),
        (("pop.pi_stride", -1), EINVAL, PER_LEARNER),
        (("pop.n_gamma_pow", -1), EINVAL, PER_LEARNER),
        (("pop.gamma", None, "beh[0]", 5), EINVAL, PER_LEARNER),
        (("beh[1]", 5), EINVAL, "{who}: bad behaviour"),
        (("beh[0]", -1), EINVAL, "{who}: bad behaviour"),
        (("beh[1]", 5, "pop.alpha_ep", P), EINVAL, "{who}: bad behaviour"),
        (("beh[0]", L.BEHAVIOUR_EPS_GREEDY, "beh[1]", L.BEHAVIOUR_SOFT_GREEDY), OK, None),
        (("pop.alpha_ep", P), EINVAL, "{who}: schedules need n_sched > 0"),
        (("pop.epsilon_ep", P), EINVAL, "{who}: schedules need n_sched > 0"),
        (("pop.epsilon_ep", P, "pop.n_sched", 1), OK, None),
    ] + ([] if pi_optional else [(("pop.pi", None), EINVAL, PER_LEARNER)])


EXO_COMMON = [  # exo_check_common behind the two tables
    (("tx", None), EINVAL, "table is NULL"),
    (("tx.r_dtype", 9), EINVAL, "table: bad r_dtype"),
    (("t.N0", 1), EINVAL, "{who}: the s-table and the x-table hold different logs (N / N0 differ)"),
    (("t.N0", 1, "ro", None), EINVAL, "{who}: the s-table and the x-table hold different logs (N / N0 differ)"),
    (("t.N0", 1, "tx.N0", 1), EINVAL, "{who}: table without its init rows"),
    (("t.N0", 1, "tx.N0", 1, "t.init_slot", P, "tx.init_slot", P), EINVAL, "{who}: table without its init rows"),
    (("t.N0", 1, "tx.N0", 1, "t.init_slot", P, "tx.init_slot", P, "t.init_orig", P), OK, None),
    (("ro", None), EINVAL, "{who}: rs / rx NULL or of different R"),
    (("rx", None), EINVAL, "{who}: rs / rx NULL or of different R"),
    (("rx.R", 1), EINVAL, "{who}: rs / rx NULL or of different R"),
    (("ro.R", -1, "rx.R", -1), EINVAL, "{who}: rs / rx NULL or of different R"),
    (("n_obs", 0), EINVAL, "{who}: bad n_obs, or obs_of / pi is NULL"),
    (("obs_of", None), EINVAL, "{who}: bad n_obs, or obs_of / pi is NULL"),
    (("obs_of", None, "reseed", 2), EINVAL, "{who}: bad n_obs, or obs_of / pi is NULL"),
    (("reseed", 2), EINVAL, "{who}: bad reseed mode"),
    (("reseed", 2, "ro.rng_kind", 7), EINVAL, "{who}: bad reseed mode"),
    (("ro.rng_kind", 7), EINVAL, "{who}: unknown stream provider"),
    (("ro.rng_kind", L.STREAM_PHILOX), OK, None),
    (("reseed", L.EXO_RESEED_EPISODE), OK, None),
    (("reseed", L.EXO_RESEED_EPISODE, "ro.rng_kind", L.STREAM_PHILOX), EUNSUP,
     "{who}: OFFSIM_EXO_RESEED_EPISODE seeds default_rng(episode): the stream must be OFFSIM_STREAM_PCG64"),
    (("out", None), EINVAL, "{who}: out is NULL"),
] + OUT + CAPS + [
    (("out.ep_cap", -1, "{gp}n_gamma_pow", 4), EINVAL, "{who}: gamma_pow is NULL"),
]
EXO_SHAPE = [  # exo_launch_shape: the two products, then the carve with one rollout per workgroup
    (("t.n_slots", 300, "tx.n_slots", 300), EUNSUP, LDS_EXO),
    (("n_obs", 30000), EUNSUP, LDS_EXO),
    (("n_obs", 8000), EUNSUP, LDS_EXO),
    (("n_obs", 2000), OK, None),
]

QUEUE_COMMON = [  # queue_check behind the table
    (("t.N0", 1), EINVAL, "{who}: table without its init rows"),
    (("t.N0", 1, "t.init_slot", P), EINVAL, "{who}: table without its init rows"),
    (("t.N0", 1, "t.init_slot", P, "t.init_orig", P), OK, None),
    (("ro", None), EINVAL, "{who}: ro is NULL or R < 0"),
    (("ro.R", -1), EINVAL, "{who}: ro is NULL or R < 0"),
    (("ro.R", 6, "ro.rng", None), EINVAL, "{who}: NULL rollout state"),
    (("ro.R", 6, "ro.cursor", None), EINVAL, "{who}: NULL rollout state"),
    (("ro.R", 6, "ro.init_cursor", None), EINVAL, "{who}: NULL rollout state"),
    (("ro.R", 6, "ro.cur_slot", None, "nA_actions", 3), EINVAL, "{who}: NULL rollout state"),
    (("ro.rng", None), OK, None),
    (("nA_actions", 0), EINVAL, "{who}: nA_actions is not the table's nA"),
    (("nA_actions", 3), EINVAL, "{who}: nA_actions is not the table's nA"),
    (("t.n_slots", 5), EINVAL, "{who}: n_slots is no multiple of nA (the table is not keyed by z * nA + a)"),
    (("t.n_slots", 5, "ro.rng_kind", L.STREAM_PHILOX), EINVAL, "{who}: n_slots is no multiple of nA (the table is not keyed by z * nA + a)"),
    (("ro.rng_kind", L.STREAM_PHILOX), EUNSUP,
     "{who}: the action stream must be OFFSIM_STREAM_PCG64 (a Philox double lies in (0, 1]: u = 1.0 selects action nA)"),
    (("ro.rng_kind", 7), EINVAL, "{who}: unknown stream provider"),
    (("ro.rng_kind", 7, "out", None), EINVAL, "{who}: unknown stream provider"),
    (("out", None), EINVAL, "{who}: out is NULL"),
] + OUT + CAPS + [
    (("out.trace_cap", -1, "tie_reseed", 2), EINVAL, "{who}: negative ep_cap / trace_cap"),
    (("tie_reseed", 2), EINVAL, "{who}: tie_reseed_episode is 0 or 1"),
    (("tie_reseed", -1, "{td}mode", 0), EINVAL, "{who}: tie_reseed_episode is 0 or 1"),
] + TD_MODE + [
    (("{td}td_cap", -1), EINVAL, "{who}: negative td_cap"),
    (("{td}td_cap", -1, "{td}q_snap", P, "{td}snap_stride", 0), EINVAL, "{who}: negative td_cap"),
] + SNAP + [
    (("tie_reseed", 1), EINVAL, "{who}: tie_reseed_episode needs td->tie_mt (the stream is written back there) and episode0 >= 0"),
    (("tie_reseed", 1, "{td}tie_mt", P, "episode0", -1), EINVAL,
     "{who}: tie_reseed_episode needs td->tie_mt (the stream is written back there) and episode0 >= 0"),
    (("tie_reseed", 1, "{td}tie_mt", P), OK, None),
    (("tie_reseed", 1, "{td}q_snap", P, "{td}snap_cap", -1), EINVAL, "{who}: bad snapshot stride / capacity"),
]
QUEUE_SHAPE = [  # queue_launch_shape: the slot count, then the carve with one rollout per workgroup
    (("t.n_slots", 40962), EUNSUP, LDS_QUEUE),
    (("t.n_slots", 8000), EUNSUP, LDS_QUEUE),
    (("t.n_slots", 4000), OK, None),
]

RULES = {
    "eval_td": TABLE + [
        (("ro", None), EINVAL, "{who}: bad argument"),
        (("ro.R", -1), EINVAL, "{who}: bad argument"),
        (("pi", None), EINVAL, "{who}: bad argument"),
        (("out", None), EINVAL, "{who}: bad argument"),
        (("td", None), EINVAL, "{who}: bad argument"),
        (("t.r_dtype", 9, "ro", None), EINVAL, "table: bad r_dtype"),
        (("pi", None, "out.status", None), EINVAL, "{who}: bad argument"),
    ] + OUT + TD_MODE + [
        (("out.n_ep", None, "td.mode", 0), EINVAL, "{who}: required output is NULL"),
        (("n_gamma_pow", 4, "td.q", None), EINVAL, "{who}: gamma_pow is NULL"),
        (("td.mode", 0, "td.behaviour", 3), EINVAL, "{who}: bad td mode or NULL q"),
        (("td.behaviour", 3), EINVAL, "{who}: bad behaviour"),
        (("td.behaviour", -1), EINVAL, "{who}: bad behaviour"),
        (("td.behaviour", L.BEHAVIOUR_EPS_GREEDY), OK, None),
        (("td.behaviour", L.BEHAVIOUR_SOFT_GREEDY, "td.tie_mt", P), OK, None),
        (("td.behaviour", 3, "td.alpha_ep", P), EINVAL, "{who}: bad behaviour"),
        (("td.alpha_ep", P), EINVAL, "{who}: schedules need n_sched > 0"),
        (("td.epsilon_ep", P), EINVAL, "{who}: schedules need n_sched > 0"),
        (("td.alpha_ep", P, "td.epsilon_ep", P, "td.n_sched", 2), OK, None),
        (("td.alpha_ep", P, "td.q_snap", P, "td.snap_stride", 0), EINVAL, "{who}: schedules need n_sched > 0"),
    ] + SNAP + [
        (("td.td_cap", -1), OK, None),  # not checked here (the queue and exo entry points refuse it)
        (("td.td_cap", -1, "td.td_err", P), OK, None),
        (("ro.R", 1, "t.n_slots", 30000), EUNSUP, LDS_MC),
        (("ro.R", 1, "t.n_slots", 30000, "td.mode", 0), EINVAL, "{who}: bad td mode or NULL q"),
    ],
    "eval_td_pop": TABLE + [
        (("ro", None), EINVAL, "{who}: bad argument"),
        (("ro.R", -1), EINVAL, "{who}: bad argument"),
        (("pop", None), EINVAL, "{who}: bad argument"),
        (("out", None), EINVAL, "{who}: bad argument"),
        (("t.plog_dtype", -1, "pop", None), EINVAL, "table: bad plog_dtype"),
        (("out", None, "L", 0), EINVAL, "{who}: bad argument"),
    ] + OUT + [
        (("out.cand", None, "L", 0), EINVAL, "{who}: required output is NULL"),
        (("pop.n_gamma_pow", 4, "S", 0), EINVAL, "{who}: gamma_pow is NULL"),
    ] + _pop_rules(False) + [
        (("ro.R", 5, "pop.mode", 0), EINVAL, "{who}: ro->R must be L * S"),
        (("pop.mode", 0, "pop.alpha", None), EINVAL, "{who}: bad td mode or NULL q"),
        (("pop.alpha_ep", P, "pop.q_snap", P, "pop.snap_stride", 0), EINVAL, "{who}: schedules need n_sched > 0"),
    ] + TD_MODE + SNAP + [
        (("pop.td_cap", -1), OK, None),  # not checked here (the queue and exo populations refuse it)
        (("ro.R", 6, "t.n_slots", 30000), EUNSUP, LDS_MC),
        (("ro.R", 6, "t.n_slots", 30000, "pop.q_snap", P, "pop.snap_cap", -1), EINVAL, "{who}: bad snapshot stride / capacity"),
    ],
    "eval_mc_exo": TABLE + EXO_COMMON + [
        (("pi", None), EINVAL, "{who}: bad n_obs, or obs_of / pi is NULL"),
        (("pi", None, "prob_mode", 5), EINVAL, "{who}: bad n_obs, or obs_of / pi is NULL"),
        (("out.ep_cap", -1, "pi", None), EINVAL, "{who}: negative ep_cap / trace_cap"),
        (("prob_mode", 5), EINVAL, "{who}: bad prob_mode"),
        (("prob_mode", 5, "td.mode", 0), EINVAL, "{who}: bad prob_mode"),
        (("prob_mode", L.PROB_F32, "t.plog_dtype", L.F64), EINVAL, "{who}: OFFSIM_PROB_F32 needs an f32 p_log"),
        (("prob_mode", L.PROB_F32, "td", None), OK, None),  # evalMC in float
        (("td", None), OK, None),
    ] + TD_MODE + [
        (("td.mode", 0, "prob_mode", L.PROB_F32), EINVAL, "{who}: bad td mode or NULL q"),
        (("prob_mode", L.PROB_F32), EINVAL, "{who}: the learner drivers take an f64 pi (OFFSIM_PROB_F64)"),
        (("prob_mode", L.PROB_F32, "td.behaviour", 3), EINVAL, "{who}: the learner drivers take an f64 pi (OFFSIM_PROB_F64)"),
        (("td.behaviour", 3), EINVAL, "{who}: bad behaviour"),
        (("td.behaviour", 3, "td.tie_mt", P), EINVAL, "{who}: bad behaviour"),
        (("td.behaviour", L.BEHAVIOUR_EPS_GREEDY), EUNSUP,
         "{who}: only OFFSIM_BEHAVIOUR_FIXED (no greedy behaviour on the learner's own Q, no tie stream)"),
        (("td.behaviour", L.BEHAVIOUR_SOFT_GREEDY, "td.alpha_ep", P), EUNSUP,
         "{who}: only OFFSIM_BEHAVIOUR_FIXED (no greedy behaviour on the learner's own Q, no tie stream)"),
        (("td.tie_mt", P), EUNSUP, "{who}: only OFFSIM_BEHAVIOUR_FIXED (no greedy behaviour on the learner's own Q, no tie stream)"),
        (("td.alpha_ep", P), EINVAL, "{who}: schedules need n_sched > 0"),
        (("td.alpha_ep", P, "td.td_cap", -1), EINVAL, "{who}: schedules need n_sched > 0"),
        (("td.epsilon_ep", P), OK, None),  # only alpha_ep is in this entry point's schedule rule (the others refuse it)
        (("td.td_cap", -1), EINVAL, "{who}: negative td_cap"),
        (("td.td_cap", -1, "td.q_snap", P, "td.snap_stride", 0), EINVAL, "{who}: negative td_cap"),
    ] + SNAP + EXO_SHAPE + [
        (("n_obs", 30000, "td.q_snap", P, "td.snap_cap", -1), EINVAL, "{who}: bad snapshot stride / capacity"),
        (("n_obs", 8000, "td", None), OK, None),  # without the Q table the same carve fits
    ],
    "eval_td_exo_pop": [
        (("pop", None), EINVAL, "{who}: pop is NULL"),
        (("pop", None, "t", None), EINVAL, "{who}: pop is NULL"),
    ] + TABLE + EXO_COMMON + _pop_rules(False) + [
        (("out.trace_cap", -1, "L", 0), EINVAL, "{who}: negative ep_cap / trace_cap"),
        (("pop.mode", 0, "pop.alpha", None), EINVAL, "{who}: bad td mode or NULL q"),
    ] + TD_MODE + SNAP + [
        (("pop.td_cap", -1), EINVAL, "{who}: negative td_cap"),
        (("pop.td_cap", -1, "L", 0), EINVAL, "{who}: L must be 1..65535 and S >= 1"),
        (("pop.td_cap", -1, "pop.q_snap", P, "pop.snap_stride", 0), EINVAL, "{who}: bad snapshot stride / capacity"),
        (("pop.td_cap", -1, "n_obs", 30000), EINVAL, "{who}: negative td_cap"),
    ] + EXO_SHAPE,
    "eval_queue": TABLE + QUEUE_COMMON + [
        (("td.behaviour", 3), EINVAL, "{who}: bad behaviour"),
        (("td.mode", 0, "td.behaviour", 3), EINVAL, "{who}: bad td mode or NULL q"),
        (("td.behaviour", 3, "td.alpha_ep", P), EINVAL, "{who}: bad behaviour"),
        (("td.alpha_ep", P), EINVAL, "{who}: schedules need n_sched > 0"),
        (("td.epsilon_ep", P), EINVAL, "{who}: schedules need n_sched > 0"),
        (("td.epsilon_ep", P, "td.td_cap", -1), EINVAL, "{who}: schedules need n_sched > 0"),
        (("td", None), OK, None),
        (("td", None, "tie_reseed", 1), EINVAL, "{who}: tie_reseed_episode without a learner"),
        (("pi", None), EINVAL, "{who}: pi is NULL (only Q-learning with a behaviour on the learner's own Q runs without one)"),
        (("pi", None, "td", None), EINVAL, "{who}: pi is NULL (only Q-learning with a behaviour on the learner's own Q runs without one)"),
        (("pi", None, "td.behaviour", L.BEHAVIOUR_EPS_GREEDY, "td.mode", L.TD_EXPSARSA), EINVAL,
         "{who}: pi is NULL (only Q-learning with a behaviour on the learner's own Q runs without one)"),
        (("pi", None, "td.behaviour", L.BEHAVIOUR_SOFT_GREEDY), OK, None),
        (("pi", None, "tie_reseed", 1), EINVAL, "{who}: tie_reseed_episode needs td->tie_mt (the stream is written back there) and episode0 >= 0"),
        (("pi", None, "t.n_slots", 40962), EINVAL, "{who}: pi is NULL (only Q-learning with a behaviour on the learner's own Q runs without one)"),
    ] + QUEUE_SHAPE + [
        (("t.n_slots", 8000, "td", None), OK, None),  # without the Q table the same carve fits
    ],
    "eval_queue_pop": [
        (("pop", None), EINVAL, "{who}: pop is NULL"),
        (("pop", None, "t", None), EINVAL, "{who}: pop is NULL"),
    ] + TABLE + QUEUE_COMMON + _pop_rules(True) + [
        (("pop.td_cap", -1, "L", 0), EINVAL, "{who}: negative td_cap"),  # the learner rules of offsim_eval_queue come before L and S
        (("pop.mode", 0, "L", 0), EINVAL, "{who}: bad td mode or NULL q"),
        (("tie_reseed", 1, "L", 0), EINVAL, "{who}: tie_reseed_episode needs td->tie_mt (the stream is written back there) and episode0 >= 0"),
        (("pop.alpha_ep", P, "L", 0), EINVAL, "{who}: L must be 1..65535 and S >= 1"),
        (("pop.pi", None), EINVAL, "{who}: pi is NULL (only Q-learning with a behaviour on every learner's own Q runs without one)"),
        (("pop.pi", None, "beh[0]", L.BEHAVIOUR_EPS_GREEDY), EINVAL,
         "{who}: pi is NULL (only Q-learning with a behaviour on every learner's own Q runs without one)"),
        (("pop.pi", None, "beh[0]", L.BEHAVIOUR_EPS_GREEDY, "beh[1]", L.BEHAVIOUR_SOFT_GREEDY, "pop.mode", L.TD_EXPSARSA), EINVAL,
         "{who}: pi is NULL (only Q-learning with a behaviour on every learner's own Q runs without one)"),
        (("pop.pi", None, "beh[0]", L.BEHAVIOUR_EPS_GREEDY, "beh[1]", L.BEHAVIOUR_SOFT_GREEDY), OK, None),
        (("pop.pi", None, "beh[1]", 5), EINVAL, "{who}: bad behaviour"),
        (("pop.pi", None, "t.n_slots", 40962), EINVAL,
         "{who}: pi is NULL (only Q-learning with a behaviour on every learner's own Q runs without one)"),
    ] + QUEUE_SHAPE,
}


def _cases():
    for entry, rules in RULES.items():
        pop = entry.endswith("_pop")
        sub = {"who": entry, "td": "pop." if pop else "td.", "gp": "pop." if pop else ""}
        for i, (changes, rc, msg) in enumerate(rules):
            changes = tuple(c.format(**sub) if isinstance(c, str) else c for c in changes)
            name = ",".join(f"{p}={v}" for p, v in zip(changes[::2], changes[1::2]))
            yield pytest.param(entry, changes, rc, None if msg is None else msg.format(**sub).encode(), id=f"{entry}-{i}-{name}")


@pytest.fixture(scope="module")
def lib():
    return L.load()


def test_the_unchanged_call_of_every_entry_point_is_accepted(lib):
    for entry in RULES:
        assert _call(lib, entry, _base(entry)) == OK, (entry, lib.offsim_last_error())


@pytest.mark.parametrize("entry,changes,rc,msg", list(_cases()))
def test_rule(lib, entry, changes, rc, msg):
    a = _base(entry)
    _apply(a, changes)
    got = _call(lib, entry, a)
    assert got == rc, (got, lib.offsim_last_error())
    if msg is not None:
        assert lib.offsim_last_error() == msg
