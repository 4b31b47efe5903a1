"""The argument validation of offsim_replay_td and the LPW chooser offsim_replay_lpw, rule by rule: both decide before any HIP call, so the
C ABI is called here without a device (as tests/test_td_validation_host.py does for the learner entry points).  Every case starts from a
call that passes validation up to the LDS refusal and changes the named arguments."""
import ctypes
import os
import sys

import pytest

from rl_offline_simulation_amd import _lib as L

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import replay_host as H  # noqa: E402

P = 8  # any non-NULL pointer: nothing dereferences a device pointer before the launch
HUGE = dict(nS=20481, nA=1)  # one entry past the LDS limit: a valid call ends in OFFSIM_EUNSUPPORTED, with no device


def _call(log_over=None, rp_over=None, n_l=2, S=1, log=True, rp=True):
    lg = dict(N=10, s=P, a=P, r=P, s_next=P, done=P, **HUGE)
    lg.update(log_over or {})
    r = dict(mode=L.TD_QLEARN, order=None, M=0, passes=1, alpha=P, gamma=P, q=P, n_ep=P, steps=P, status=P)
    r.update(rp_over or {})
    lib = L.load()
    rc = lib.offsim_replay_td(ctypes.byref(L.ReplayLog(**lg)) if log else None, n_l, S, ctypes.byref(L.Replay(**r)) if rp else None, None)
    return rc, lib.offsim_last_error().decode()


def test_symbols_exist():
    lib = L.load()
    assert lib.offsim_replay_td and lib.offsim_replay_lpw


def test_a_valid_call_reaches_the_lds_refusal():
    rc, msg = _call()
    assert rc == L.EUNSUPPORTED and msg == "replay_td: one learner's Q table exceeds 160 KiB of LDS"
    rc, msg = _call(rp_over=dict(order=P, M=5), S=3)
    assert rc == L.EUNSUPPORTED
    rc, msg = _call(rp_over=dict(mode=L.TD_EXPSARSA, pi=P, alpha_ep=P, n_sched=4, q_snap=P, snap_stride=1, td_err=P, td_cap=3, passes=7))
    assert rc == L.EUNSUPPORTED


EINVAL_CASES = [
    ("NULL log", dict(log=False), "replay_td: bad argument"),
    ("NULL rp", dict(rp=False), "replay_td: bad argument"),
    ("NULL s", dict(log_over=dict(s=None)), "replay_td: NULL log column"),
    ("NULL a", dict(log_over=dict(a=None)), "replay_td: NULL log column"),
    ("NULL r", dict(log_over=dict(r=None)), "replay_td: NULL log column"),
    ("NULL s_next", dict(log_over=dict(s_next=None)), "replay_td: NULL log column"),
    ("NULL done", dict(log_over=dict(done=None)), "replay_td: NULL log column"),
    ("N = 0", dict(log_over=dict(N=0)), "replay_td: bad N / nS / nA"),
    ("nS = 0", dict(log_over=dict(nS=0)), "replay_td: bad N / nS / nA"),
    ("nA = 0", dict(log_over=dict(nA=0)), "replay_td: bad N / nS / nA"),
    ("L = 0", dict(n_l=0), "replay_td: L must be 1..65535 and S >= 1"),
    ("L = 65536", dict(n_l=65536), "replay_td: L must be 1..65535 and S >= 1"),
    ("S = 0", dict(S=0), "replay_td: L must be 1..65535 and S >= 1"),
    ("S = 2 without an order", dict(S=2), "replay_td: S streams need an order (without one the stream is the log: S = 1)"),
    ("an order with M = 0", dict(rp_over=dict(order=P, M=0)), "replay_td: an order needs M >= 1"),
    ("passes = 0", dict(rp_over=dict(passes=0)), "replay_td: passes must be >= 1"),
    ("bad mode", dict(rp_over=dict(mode=0)), "replay_td: bad td mode or NULL q"),
    ("NULL q", dict(rp_over=dict(q=None)), "replay_td: bad td mode or NULL q"),
    ("NULL alpha", dict(rp_over=dict(alpha=None)), "replay_td: a per-learner array is NULL (alpha, gamma)"),
    ("NULL gamma", dict(rp_over=dict(gamma=None)), "replay_td: a per-learner array is NULL (alpha, gamma)"),
    ("expected SARSA without pi", dict(rp_over=dict(mode=L.TD_EXPSARSA)), "replay_td: expected SARSA needs pi"),
    ("alpha_ep without n_sched", dict(rp_over=dict(alpha_ep=P)), "replay_td: schedules need n_sched > 0"),
    ("snapshot stride 0", dict(rp_over=dict(q_snap=P, snap_stride=0)), "replay_td: bad snapshot stride / capacity"),
    ("negative snapshot capacity", dict(rp_over=dict(q_snap=P, snap_stride=1, snap_cap=-1)), "replay_td: bad snapshot stride / capacity"),
    ("negative td_cap", dict(rp_over=dict(td_err=P, td_cap=-1)), "replay_td: negative td_cap"),
    ("NULL n_ep", dict(rp_over=dict(n_ep=None)), "replay_td: required output is NULL"),
    ("NULL steps", dict(rp_over=dict(steps=None)), "replay_td: required output is NULL"),
    ("NULL status", dict(rp_over=dict(status=None)), "replay_td: required output is NULL"),
]


@pytest.mark.parametrize("what,kw,msg", EINVAL_CASES, ids=[c[0] for c in EINVAL_CASES])
def test_einval(what, kw, msg):
    assert _call(**kw) == (L.EINVAL, msg)


def test_sizes_past_int32_are_refused():
    assert _call(log_over=dict(N=2 ** 31))[0] == L.EUNSUPPORTED
    assert _call(rp_over=dict(order=P, M=2 ** 31))[0] == L.EUNSUPPORTED
    assert _call(rp_over=dict(order=P, M=2 ** 31 - 1, passes=2 ** 33))[0] == L.EUNSUPPORTED


def test_lpw_is_the_budget_formula():
    lib = L.load()
    for nS, nA in ((1, 1), (25, 5), (64, 5), (65, 5), (320, 1), (321, 1), (128, 5), (129, 5), (512, 5), (513, 5), (4096, 5), (20480, 1), (20481, 1), (6827, 3)):
        for n_l in (1, 2, 3, 4, 5, 31, 32, 33, 64, 65, 130, 65535):
            assert lib.offsim_replay_lpw(nS, nA, n_l) == H.lpw(nS, nA, n_l), (nS, nA, n_l)
    assert lib.offsim_replay_lpw(20480, 1, 64) == 1 and lib.offsim_replay_lpw(20481, 1, 64) == 0  # exactly at the limit, one entry past it
    for bad in ((0, 5, 1), (5, 0, 1), (5, 5, 0), (5, 5, 65536)):
        assert lib.offsim_replay_lpw(*bad) == L.EINVAL
