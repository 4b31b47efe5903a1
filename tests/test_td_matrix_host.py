"""What the learner-kernel matrix (tests/test_gpu_td_matrix.py) rests on, checked without a device: the plain Python loop of
tests/td_host.py reproduces the reference's recorded qlearn_psrs / expSARSA_psrs runs, the case list of tests/td_cases.py covers what the
matrix is meant to cover and no case is vacuous, and the restated LDS arithmetic gives each case the launch it is named for."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import td_cases as K  # noqa: E402
import td_host as H  # noqa: E402
from common import load  # noqa: E402

sched_alpha = lambda ep: 0.5 / (1.0 + 0.1 * ep)   # noqa: E731  (tests/golden/make_golden.py, section 11b)
sched_eps = lambda ep: max(0.05, 0.9 ** ep)       # noqa: E731


def _golden_log(d):
    log = H.Log(d["in_z"], d["in_a"], d["in_r"], d["in_z_next"], d["in_done"], d["in_p_log"], d["in_t0"])
    assert log.z_base == 0 and log.n_slots <= d["Q_init"].shape[0]
    return log


def _replay(log, seed, q_init, tie=None, keep_p=False, **kw):
    cap = log.N + 1
    lr = H.Learner(log, seed, np.zeros((log.n_slots, log.nA)) if q_init is None else q_init[:log.n_slots], tie)
    o = H.run(lr, trace_cap=cap, ep_cap=cap, keep_p=keep_p, **kw)
    o["Gs"] = o["ep_g"][:o["n_ep"] + (o["status"] == H.ST_EXHAUSTED)]  # the cut-short episode's return is appended too (psrs.py:177, :232)
    return o


def _mt_of_seed(np_seed):
    st = np.random.RandomState(int(np_seed)).get_state()
    return np.concatenate([np.asarray(st[1], np.uint32), np.array([st[2]], np.uint32)])


@pytest.mark.parametrize("name", ["td_iid_2k", "td_grid_300x15"])
def test_host_loop_replays_the_recorded_drivers(name):
    d = load(name)
    log = _golden_log(d)
    n, gam, al, Qi = log.n_slots, float(d["gamma"]), float(d["alpha"]), d["Q_init"]
    uniform = np.full((n, 5), 0.2)
    for s in (int(x) for x in d["seeds"]):
        runs = {"ql": dict(mode=H.QLEARN, pi=uniform, behaviour=H.FIXED),
                "qe1": dict(mode=H.QLEARN, pi=uniform, behaviour=H.EPS_GREEDY, epsilon=0.1),
                "qe5": dict(mode=H.QLEARN, pi=uniform, behaviour=H.EPS_GREEDY, epsilon=0.5)}
        for tag, kw in runs.items():
            o = _replay(log, s, Qi, gamma=gam, alpha=al, **kw)
            k, m = f"s{s}_{tag}", o["steps"]
            assert np.array_equal(o["q"], d[k + "_Q"][:n]) and np.array_equal(o["td_err"][:m], d[k + "_td"]), k
            assert np.array_equal(o["Gs"], d[k + "_Gs"]) and np.array_equal(o["trace_row"][:m], d[k + "_rows"]), k
        o = _replay(log, s, None, mode=H.EXPSARSA, pi=d["pi"][:n], gamma=gam, alpha=al)
        assert np.abs(o["q"] - d[f"s{s}_es_Q"][:n]).max() <= 1e-12  # (the reference's `@` is BLAS: its order of summation is not ours)
        assert np.array_equal(o["Gs"], d[f"s{s}_es_Gs"]) and np.array_equal(o["trace_row"][:o["steps"]], d[f"s{s}_es_rows"])


def test_host_loop_replays_schedules_ties_snapshots_and_the_tie_stream():
    d = load("td2_iid_2k")
    log = _golden_log(d)
    n, gam, Qi, pi = log.n_slots, float(d["gamma"]), d["Q_init"], d["pi"]
    N0 = int(np.sum(d["in_t0"])) + 1
    a_tab, e_tab = np.array([sched_alpha(e) for e in range(N0)]), np.array([sched_eps(e) for e in range(N0)])
    uniform = np.full((n, 5), 0.2)
    E, S = H.EPS_GREEDY, H.SOFT_GREEDY
    runs = {
        "sched": dict(mode=H.QLEARN, behaviour=E, alpha_ep=a_tab, epsilon_ep=e_tab, alpha=0.0, q0=Qi, pi=uniform),
        "ties": dict(mode=H.QLEARN, behaviour=E, alpha=0.1, epsilon=0.3, q0=None, pi=uniform),
        "ties_sched": dict(mode=H.QLEARN, behaviour=E, alpha_ep=a_tab, epsilon_ep=e_tab, alpha=0.0, q0=None, pi=uniform),
        "greedy": dict(mode=H.QLEARN, behaviour=E, alpha=0.1, epsilon=0.0, q0=None, pi=uniform),
        "soft": dict(mode=H.QLEARN, behaviour=S, alpha=0.1, q0=None, pi=uniform),
        "saveq": dict(mode=H.QLEARN, behaviour=E, alpha=0.1, epsilon=0.2, q0=None, pi=uniform, n_episodes=12, snap_cap=log.N + 1),
        "es_sched": dict(mode=H.EXPSARSA, behaviour=H.FIXED, alpha_ep=a_tab, alpha=0.0, q0=None, pi=pi[:n], n_episodes=12, snap_cap=log.N + 1),
    }
    for s in (int(x) for x in d["seeds"]):
        for tag, kw in runs.items():
            kw = dict(kw)
            k = f"s{s}_{tag}"
            o = _replay(log, s, kw.pop("q0"), tie=_mt_of_seed(d[k + "_np_seed"]), keep_p=True, gamma=gam, **kw)
            m = o["steps"]
            assert np.array_equal(o["trace_row"][:m], d[k + "_rows"]) and np.array_equal(o["Gs"], d[k + "_Gs"]), k
            assert np.array_equal(np.array(o["beh_p"]), d[k + "_p"]), (k, "behaviour distributions")
            rs = np.random.RandomState()
            rs.set_state(("MT19937", o["tie_mt"][:624], int(o["tie_mt"][624])))
            assert np.array_equal(rs.random_sample(3), d[k + "_after"]), (k, "the tie stream stands where the reference leaves the global one")
            q0 = np.zeros((n, 5)) if tag not in ("sched",) else Qi[:n]
            Qs = np.concatenate([q0[None], o["q_snap"][:m]]) if "snap_cap" in kw else None
            if tag == "es_sched":
                assert np.abs(o["q"] - d[k + "_Q"][:n]).max() <= 1e-12 and np.abs(Qs - d[k + "_Qs"][:, :n]).max() <= 1e-12
            else:
                assert np.array_equal(o["q"], d[k + "_Q"][:n]) and np.array_equal(o["td_err"][:m], d[k + "_td"]), k
                if tag == "saveq":
                    assert np.array_equal(Qs, d[k + "_Qs"][:, :n])


# ---------------------------------------------------------------------------------------------------------------------------------
RUN = [c for c in K.CASES if not c.refused]


def _total(case, key):
    return sum(o[key] for o in K.host(case))


def test_the_restated_lds_formula_gives_each_case_its_launch():
    shape = lambda name: K.BY_NAME[name].shape  # noqa: E731
    assert K.lds_bytes(4, 25, 5) == 4 * 65 * 32 + 4 * 1000 + 1000 + 104 + 400 + 8 + 160 + 4 * 2496 == 23976
    assert shape("pl-f64-qlearn-eps-R4") == (4, 23976, False)
    assert shape("nA2-R7")[0] == 4
    assert shape("waves2-R3") == (2, 41100, False) and K.lds_bytes(4, 80, 16) > 65536
    assert shape("nA80-eps-R3") == (2, 58744, False) and K.lds_bytes(4, 25, 80) > 65536
    assert shape("waves1-R3") == (1, 54876, False) and K.lds_bytes(2, 190, 16) > 65536
    assert shape("lds-above-64k-R3") == (1, 79108, False)
    assert shape("lds-160k-last-that-fits-R2") == (1, 163644, False) and 163644 <= 160 * 1024
    assert shape("lds-160k-first-refused") == (1, 163908, True)  # one more state: 264 bytes more, 68 past the limit
    for c in K.CASES:  # a case named for a launch gets it
        w, b, refused = c.shape
        assert refused == c.refused
        if c.name.startswith(("waves2", "waves1")):
            assert w == int(c.name[5]) and b <= 65536
        if c.name.startswith("lds-"):
            assert w == 1 and b > 65536


def test_the_case_list_covers_the_kernel():
    by = lambda f: [c for c in RUN if f(c)]  # noqa: E731
    for pl in ("f64", "f32", "f16"):
        assert {c.mode for c in RUN if c.table.pl == pl} == {H.QLEARN, H.EXPSARSA}, pl
    assert {c.table.rd for c in RUN} == {"f32", "f64"}
    # launch shapes: each at R = 1 and at an R that is no multiple of its waves; waves = 4 also at R = 4 and R = 9
    shapes = {"w4": lambda c: c.shape[0] == 4, "w2": lambda c: c.shape[0] == 2, "w1": lambda c: c.shape[0] == 1 and c.shape[1] <= 65536,
              "big": lambda c: c.shape[1] > 65536}
    for tag, f in shapes.items():
        Rs = {c.R for c in by(f)}
        w = {"w4": 4, "w2": 2}.get(tag, 1)
        assert 1 in Rs and any(R > 1 and (w == 1 or R % w) for R in Rs), (tag, Rs)
    assert {4, 9} <= {c.R for c in by(shapes["w4"])}
    assert any(c.refused for c in K.CASES) and any(c.shape[1] > 160 * 1024 - 512 for c in RUN)
    nAs = {c.table.nA for c in RUN}
    assert {2, 5, 16} <= nAs and any(a > 64 for a in nAs)
    assert any(c.table.nA > 64 and c.behaviour == b for c in RUN for b in (H.EPS_GREEDY,)) and any(c.table.nA > 64 and c.behaviour == H.SOFT_GREEDY for c in RUN)
    # behaviours x modes
    assert {(c.behaviour, c.mode) for c in RUN} == {(b, m) for b in (H.FIXED, H.EPS_GREEDY, H.SOFT_GREEDY) for m in (H.QLEARN, H.EXPSARSA)}
    eg = by(lambda c: c.behaviour == H.EPS_GREEDY)
    assert any(c.mt == "none" for c in eg) and any(c.mt != "none" for c in eg)
    assert any(c.epsilon == 0.0 and c.epsilon_ep is None and c.mt != "none" for c in eg)
    for c in by(lambda c: c.alpha_ep is not None and "constants" not in c.name):  # schedules shorter than the run: the clamp is used
        assert int(_total(c, "n_ep").max()) > len(c.alpha_ep) + 1, c.name
    assert any(c.epsilon_ep is not None and c.behaviour == H.EPS_GREEDY and len(set(c.epsilon_ep)) > 1 for c in RUN)
    assert any(c.alpha_ep is not None and c.mode == H.EXPSARSA and len(set(c.alpha_ep)) > 1 for c in RUN)
    # tie stream
    assert any(int(_total(c, "mt_words").max()) >= 1300 for c in RUN)
    mid = by(lambda c: c.mt == "mid")
    assert mid and all(0 < int(w) < 624 for c in mid for w in K.mt_of(c)[:, 624])
    assert all(int(w) == 624 for c in RUN if c.mt == "fresh" for w in K.mt_of(c)[:, 624])
    for c in by(lambda c: c.mt != "none" and c.R > 1):
        assert len({K.mt_of(c)[i].tobytes() for i in range(c.R)}) == c.R, c.name
    # sampler
    assert {c.stream for c in RUN} == {"pcg64", "philox"} and {c.reject for c in RUN} == {K.REJECT_DEFAULT, K.REJECT_NEVER}
    assert any(c.stream == "philox" and c.reject == K.REJECT_NEVER for c in RUN) and any(c.stream == "philox" and c.behaviour == H.EPS_GREEDY for c in RUN)
    assert {c.reset for c in RUN} == {"plain", "keyed", "shared"}
    # ends
    ends = {c.name: set(K.host(c)[-1]["status"].tolist()) for c in RUN}
    for st in (H.ST_EXHAUSTED, H.ST_NO_INIT, H.ST_KEYERROR, H.ST_OK):
        assert any(st in v for v in ends.values()), st
    assert any(len(v) >= 2 and H.ST_KEYERROR in v for v in ends.values())
    few = by(lambda c: c.n_episodes not in (None, 0))
    assert few and all((K.host(c)[0]["n_ep"] == c.n_episodes).all() and (K.host(c)[0]["status"] == H.ST_OK).all() for c in few)
    assert any(c.n_episodes == 0 for c in RUN)
    # caps smaller than the run, with neighbours on both sides of a row
    capped = by(lambda c: c.trace_cap is not None)
    assert {c.snap_stride for c in capped} == {1, 3}
    for c in capped:
        o = K.host(c)[0]
        assert c.R >= 3 and (o["steps"] > c.trace_cap).all() and (o["n_ep"] > c.ep_cap).all() and (o["steps"] > c.snap_cap * c.snap_stride).all(), c.name
    # discount
    assert {0.0, 1.0, 0.97} <= {c.gamma for c in RUN}
    short = by(lambda c: c.n_gamma_pow < 4096)
    assert {c.gamma for c in short} == {0.0, 1.0}
    assert all(int(K.host(c)[0]["ep_len"].max()) > c.n_gamma_pow for c in short)
    assert all(int(K.host(c)[0]["ep_len"].max()) < 4096 for c in RUN if c.n_gamma_pow == 4096)
    # resume
    res = by(lambda c: c.resume_k is not None)
    assert any(c.mt != "none" for c in res) and any(c.stream == "philox" for c in res)


def test_no_case_is_vacuous():
    for c in RUN:
        steps, n_ep = _total(c, "steps"), _total(c, "n_ep")
        if not c.edge:
            assert np.median(steps) >= 200 and n_ep.max() >= 3, (c.name, steps, n_ep)
        if c.behaviour == H.EPS_GREEDY and c.mt != "none" and c.n_episodes != 0:
            assert _total(c, "mt_words").max() >= 1, c.name
        if c.q_init == "randn":  # no ties by construction: the first-maximum and the drawn maximum agree
            assert _total(c, "mt_words").max() == 0
    # the launches whose learners differ from each other: a shared Q table or tie stream could not pass
    for c in RUN:
        if c.R > 1 and c.n_episodes != 0 and c.alpha != 0.0:
            o = K.host(c)[-1]
            assert len({o["q"][i].tobytes() for i in range(c.R)}) == c.R, c.name


def test_constant_schedules_equal_the_constants():
    a, b = K.host(K.BY_NAME["constants-R3"])[0], K.host(K.BY_NAME["constants-as-schedules-R3"])[0]
    for k in a:
        assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("name", [c.name for c in K.CASES if c.resume_k is not None])
def test_two_calls_equal_one(name):
    """k episodes and then the rest: every output, laid end to end, and the final state equal the one-call run's."""
    c = K.BY_NAME[name]
    first, second = K.host(c)
    one = K.host(K.replace(c, resume_k=None))[0]
    assert (first["n_ep"] == c.resume_k).all() and (first["status"] == H.ST_OK).all() and (second["steps"] > 0).all()
    for k in ("q", "tie_mt", "cursor", "init_cursor", "cur_slot", "status", "after"):
        assert (one[k] is None and second[k] is None) or np.array_equal(one[k], second[k]), k
    for k in ("steps", "cand", "n_ep", "n_len", "mt_words"):
        assert np.array_equal(first[k] + second[k], one[k]), k
    for i in range(c.R):
        m1, m2, e1, e2 = int(first["steps"][i]), int(second["steps"][i]), int(first["n_ep"][i]), int(second["n_len"][i])
        for k in ("trace_row", "trace_pop", "td_err") + (("beh_arg",) if c.behaviour == H.EPS_GREEDY else ()):
            assert np.array_equal(np.concatenate([first[k][i, :m1], second[k][i, :m2]]), one[k][i, :m1 + m2]), (k, i)
        assert np.array_equal(np.concatenate([first["ep_g"][i, :e1], second["ep_g"][i, :e2]]), one["ep_g"][i, :e1 + e2]), i
        assert np.array_equal(np.concatenate([first["ep_len"][i, :e1], second["ep_len"][i, :e2]]), one["ep_len"][i, :e1 + e2]), i
        if c.snap_cap:
            k1 = min(m1, c.snap_cap)  # (the second call's snapshots count its own steps from 0)
            assert c.snap_stride == 1 and np.array_equal(first["q_snap"][i, :k1], one["q_snap"][i, :k1])
            k2 = min(m2, c.snap_cap)
            assert np.array_equal(second["q_snap"][i, :k2][:max(c.snap_cap - m1, 0)], one["q_snap"][i, m1:m1 + k2])
        # sum_g adds the returns in episode order: the one-call sum continues the first call's
        s = float(first["sum_g"][i])
        for g in second["ep_g"][i, :int(second["n_ep"][i])]:
            s = s + float(g)
        assert s == float(one["sum_g"][i])
