"""tests/replay_host.py, the plain loop the replay kernel is held to, against the reference's own qlearn(..., memory=...) as recorded in
tests/golden/replay/*.npz (tests/golden/make_golden_replay.py) -- bit for bit -- and its own rules: orders, passes, the schedule's last
entry, snapshots, the KeyError stop, the LPW chooser."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import replay_host as H  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("queue_iid_2k", "queue_grid_300x15")
ALPHA_SCHED = lambda e: 0.5 / (1.0 + 0.1 * e)  # noqa: E731


def golden_log(name):
    """(log, recorded reference) of a fixture: the in_* columns as the generator fed them to the reference"""
    inp, d = np.load(os.path.join(GOLDEN, name + ".npz")), np.load(os.path.join(GOLDEN, "replay", name + ".npz"))
    log = (inp["in_z"].astype(np.int32), inp["in_a"].astype(np.int32), inp["in_r"].astype(np.float64), inp["in_z_next"].astype(np.int32),
           inp["in_done"] != 0, int(d["nS"]), int(d["nA"]))
    return log, d


@pytest.mark.parametrize("name", FIXTURES)
def test_host_loop_is_the_reference(name):
    log, d = golden_log(name)
    N, nS, nA = len(log[0]), log[5], log[6]
    sched = np.array([ALPHA_SCHED(e) for e in range(int(d["n_ep"]) + 1)])
    runs = {"c": dict(alpha=[float(d["alpha"])], q=np.zeros((1, nS, nA))), "s": dict(alpha=[0.0], q=d["q_init"][None], alpha_ep=sched[None])}
    for tag, kw in runs.items():
        o = H.stream(log, H.QLEARN, gamma=[float(d["gamma"])], td_cap=N, snap_stride=1, snap_cap=N, **kw)
        assert (o["steps"], o["status"], o["n_ep"]) == (N, H.ST_OK, int(d["n_ep"]))
        assert np.array_equal(o["q"][0], d[tag + "_Q"]) and np.array_equal(o["td_err"][:, 0], d[tag + "_td"]), (name, tag)
        Qs = np.concatenate([kw["q"], o["q_snap"][0]])
        assert Qs.shape == tuple(d[tag + "_Qs_shape"]) and np.array_equal(Qs[:9], d[tag + "_Qs9"]) and np.array_equal(Qs[::500], d[tag + "_Qs500"]), (name, tag)


def test_rules_of_the_loop():
    log = H.synth_log(150, 7, 3, seed=3)
    N = 150
    alpha, gamma, q = H.learners(4, 7, 3, seed=4)
    base = H.stream(log, H.QLEARN, alpha, gamma, q, td_cap=N)
    # the identity order is the log; two passes are the order written twice; the episode counter carries on
    ident = H.stream(log, H.QLEARN, alpha, gamma, q, order=np.arange(N), td_cap=N)
    assert all(np.array_equal(base[k], ident[k]) for k in ("q", "td_err")) and base["n_ep"] == int(log[4].sum())
    sched = np.random.default_rng(5).uniform(0.01, 0.9, (4, 6))  # shorter than the episodes: the last entry serves the rest
    assert base["n_ep"] > 6
    two = H.stream(log, H.EXPSARSA, alpha, gamma, q, passes=2, alpha_ep=sched, pi=np.full((7, 3), 1 / 3), td_cap=2 * N)
    twice = H.stream(log, H.EXPSARSA, alpha, gamma, q, order=np.tile(np.arange(N), 2), alpha_ep=sched, pi=np.full((7, 3), 1 / 3), td_cap=2 * N)
    assert np.array_equal(two["q"], twice["q"]) and np.array_equal(two["td_err"], twice["td_err"]) and two["n_ep"] == 2 * base["n_ep"] == twice["n_ep"]
    # learners never interact
    one = H.stream(log, H.QLEARN, alpha[2:3], gamma[2:3], q[2:3], td_cap=N)
    assert np.array_equal(one["q"][0], base["q"][2]) and np.array_equal(one["td_err"][:, 0], base["td_err"][:, 2])
    # snapshots: Q after steps 0, 7, 14, ...; the stop before a step outside the tables
    snap = H.stream(log, H.QLEARN, alpha, gamma, q, snap_stride=7, snap_cap=5)
    for i in range(5):
        part = H.stream((*(c[:7 * i + 1] for c in log[:5]), 7, 3), H.QLEARN, alpha, gamma, q)
        assert np.array_equal(snap["q_snap"][:, i], part["q"])
    bad = tuple(c.copy() for c in log[:5]) + (7, 3)
    bad[3][40] = 7
    o = H.stream(bad, H.QLEARN, alpha, gamma, q)
    part = H.stream((*(c[:40] for c in log[:5]), 7, 3), H.QLEARN, alpha, gamma, q)
    assert (o["steps"], o["status"]) == (40, H.ST_KEYERROR) and np.array_equal(o["q"], part["q"]) and o["n_ep"] == part["n_ep"]


def test_nan_in_a_row_maximum():
    """The rule of offsim_eval_td: a NaN in the first entry of Q[s'] stays, a NaN in a later entry is passed over."""
    log = (np.array([0, 0], np.int32), np.array([0, 0], np.int32), np.array([1.0, 1.0]), np.array([1, 2], np.int32), np.array([False, False]), 3, 3)
    q = np.zeros((1, 3, 3))
    q[0, 1] = [np.nan, 5.0, 1.0]
    q[0, 2] = [2.0, np.nan, 1.0]
    o = H.stream(log, H.QLEARN, [0.5], [1.0], q, td_cap=2)
    assert np.isnan(o["td_err"][0, 0]) and np.isnan(o["q"][0, 0, 0])
    o = H.stream((*(c[1:] for c in log[:5]), 3, 3), H.QLEARN, [0.5], [1.0], q, td_cap=1)
    assert o["td_err"][0, 0] == 3.0 and o["q"][0, 0, 0] == 1.5


def test_lpw_formula():
    assert [H.lpw(25, 5, n) for n in (1, 2, 3, 5, 33, 64, 65, 1000)] == [1, 2, 4, 8, 64, 64, 64, 64]
    assert [H.lpw(n, 1, 64) for n in (320, 321, 640, 641, 1280, 1281, 2560, 2561, 5120, 5121, 10240, 10241, 20480, 20481)] == \
        [64, 32, 32, 16, 16, 8, 8, 4, 4, 2, 2, 1, 1, 0]
    assert H.lpw(4096, 5, 3) == 1 and H.lpw(6827, 3, 1) == 0
