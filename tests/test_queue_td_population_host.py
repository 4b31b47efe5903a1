"""What the queue learner-population tests (tests/test_gpu_queue_td_population.py) rest on, checked without a device: the C ABI of
offsim_eval_queue_pop is exported, bound and documented and refuses every bad argument before any HIP call (the pointers are fake
addresses: a launch would fault) while offsim_eval_queue answers its own test's inputs as before; the restated LDS formula gives each case
its launch shape; the case list of tests/queue_td_population_host.py is not vacuous; and the mirror at L = 1 replays what the reference's
own qlearn / expSARSA returned on its own QueueEvaluator_impl (tests/golden/queue_drivers/*.npz)."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import queue_host as Q  # noqa: E402
import queue_td_population_host as H  # noqa: E402
from test_queue_drivers_host import ALPHA_SCHED, EPS_SCHED, FIXTURES, RUNS, golden_log  # noqa: E402
from test_queue_drivers_host import _call as single_call  # noqa: E402

F = 0x1000
TD_RUNS = ("qu", "qe", "qs", "qg", "qf", "es")


# ---- the C ABI ----
def test_symbol_exported_bound_and_documented():
    from rl_offline_simulation_amd import _lib
    src = open(os.path.join(ROOT, "include", "offsim.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    n = "offsim_eval_queue_pop"
    assert "int " + n + "(" in src and hasattr(lib, n) and n in _lib.SIGNATURES
    doc = src[src.index("/* " + n + ":"):src.index("int " + n + "(")]
    for word in ("rgument validation happens before any HIP call", "OFFSIM_STREAM_PHILOX", "(0, 1]", "OFFSIM_EUNSUPPORTED", "160 KiB", "learner-major",
                 "Identity", "nZ * nA in the place of n_slots * nA", "tie_reseed_episode", "EVERY behaviour", "pop->pi may be NULL only"):
        assert word in doc, word
    from rl_offline_simulation_amd.evaluators import BatchedQueueEvaluator, TDPopulation
    assert callable(BatchedQueueEvaluator.eval_td_population) and callable(TDPopulation.run_queue)


def _call(L=3, S=5, R=None, t=None, ro=True, nA=2, kind=0, out=True, pop=True, beh=None, reseed=0, episode0=0, rng=F, outkw=None, **popkw):
    """offsim_eval_queue_pop on fake pointers; t: table fields to change (False: NULL); popkw: fields of struct offsim_td_pop to change."""
    from rl_offline_simulation_amd import _lib as Lb
    tc = Lb.Table(N=10, n_slots=6, nA=2, plog_dtype=Lb.F32, r_dtype=Lb.F32, seg_off=F, p_log=F, a=F, r=F, z_next=F, done=F, orig_idx=F, N0=2,
                  init_slot=F, init_orig=F)
    for k, v in (t or {}).items():
        setattr(tc, k, v)
    roc = Lb.Rollouts(R=L * S if R is None else R, rng=rng, cursor=F, init_cursor=F, cur_slot=F, rng_kind=kind)
    okw = dict(sum_g=F, n_ep=F, steps=F, cand=F, n_len=F, status=F)
    okw.update(outkw or {})
    oc = Lb.EvalMCOut(**okw)
    bh = (ctypes.c_int32 * max(L, 1))(*([Lb.BEHAVIOUR_EPS_GREEDY] * max(L, 1) if beh is None else beh))
    kw = dict(mode=Lb.TD_QLEARN, alpha=F, epsilon=F, gamma=F, gamma_pow=F, n_gamma_pow=4, behaviour=F, behaviour_host=bh, pi=F, pi_stride=0, q=F, snap_stride=1)
    kw.update(popkw)
    pc = Lb.TDPop(**kw)
    return Lb.load().offsim_eval_queue_pop(None if t is False else ctypes.byref(tc), ctypes.byref(roc) if ro else None, nA, L, S,
                                           ctypes.byref(pc) if pop else None, 10, ctypes.byref(oc) if out else None, reseed, episode0, None, None)


def test_eval_queue_pop_validation_before_any_hip_call():
    from rl_offline_simulation_amd import _lib as L
    err = L.load().offsim_last_error
    assert _call(R=0) == L.OK, err()  # R = 0 validates and launches nothing
    assert _call(R=0, tie_mt=F, beh_arg=F, td_err=F, reseed=1) == L.OK and _call(R=0, tie_mt=F, reseed=1, episode0=(1 << 32) - 2) == L.OK
    assert _call(R=0, beh=[L.BEHAVIOUR_FIXED, L.BEHAVIOUR_EPS_GREEDY, L.BEHAVIOUR_SOFT_GREEDY]) == L.OK
    # ---- what offsim_eval_queue checks.  The action stream: Philox is refused, nothing is stepped
    assert _call(kind=L.STREAM_PHILOX) == L.EUNSUPPORTED and b"(0, 1]" in err() and err().startswith(b"eval_queue_pop")
    assert _call(kind=5) == L.EINVAL
    # the table and its key
    assert _call(t=False) == L.EINVAL and _call(t=dict(seg_off=None)) == L.EINVAL and _call(t=dict(init_slot=None)) == L.EINVAL
    assert _call(t=dict(n_slots=7)) == L.EINVAL and b"multiple of nA" in err()
    assert _call(nA=3) == L.EINVAL and b"table's nA" in err()
    assert _call(nA=0) == L.EINVAL
    # the rollout state, the outputs, the capacities
    assert _call(ro=False) == L.EINVAL and _call(R=-1) == L.EINVAL and _call(rng=None) == L.EINVAL
    assert _call(out=False) == L.EINVAL and _call(outkw=dict(status=None)) == L.EINVAL and _call(outkw=dict(sum_g=None)) == L.EINVAL
    assert _call(gamma_pow=None) == L.EINVAL and b"gamma_pow" in err()
    assert _call(outkw=dict(ep_cap=-1)) == L.EINVAL and _call(outkw=dict(trace_cap=-1)) == L.EINVAL and _call(td_cap=-1) == L.EINVAL
    # the tie modes
    assert _call(reseed=2) == L.EINVAL and _call(reseed=-1) == L.EINVAL
    assert _call(reseed=1) == L.EINVAL and b"tie_mt" in err()
    assert _call(tie_mt=F, reseed=1, episode0=-1) == L.EINVAL
    # ---- what offsim_eval_td_pop checks: L, S, R = L * S
    assert _call(pop=False) == L.EINVAL
    for kw in (dict(L=0), dict(L=65536), dict(L=-1), dict(S=0), dict(S=-2)):
        assert _call(R=15, **kw) == L.EINVAL and b"1..65535" in err(), kw
    assert _call(L=65535, S=1, R=0) == L.OK
    assert _call(R=14) == L.EINVAL and b"L * S" in err() and _call(R=16) == L.EINVAL
    # the mode, the per-learner arrays, the host copy of the behaviours, the schedules, the snapshots
    assert _call(mode=0) == L.EINVAL and _call(mode=3) == L.EINVAL and _call(q=None) == L.EINVAL
    for k in ("alpha", "epsilon", "gamma", "behaviour"):
        assert _call(**{k: None}) == L.EINVAL and b"per-learner array" in err(), k
    assert _call(behaviour_host=None) == L.EINVAL and _call(pi_stride=-1) == L.EINVAL and _call(n_gamma_pow=-1) == L.EINVAL
    assert _call(beh=[0, 1, 7]) == L.EINVAL and b"bad behaviour" in err() and _call(beh=[-1, 0, 0]) == L.EINVAL
    assert _call(alpha_ep=F, n_sched=0) == L.EINVAL and _call(epsilon_ep=F, n_sched=0) == L.EINVAL and _call(R=0, alpha_ep=F, epsilon_ep=F, n_sched=3) == L.OK
    assert _call(q_snap=F, snap_stride=0) == L.EINVAL and _call(q_snap=F, snap_cap=-1) == L.EINVAL
    # pi may be NULL only for Q-learning with no fixed-behaviour learner
    assert _call(R=0, pi=None) == L.OK and _call(R=0, pi=None, beh=[L.BEHAVIOUR_SOFT_GREEDY, L.BEHAVIOUR_EPS_GREEDY, L.BEHAVIOUR_SOFT_GREEDY]) == L.OK
    assert _call(pi=None, beh=[L.BEHAVIOUR_EPS_GREEDY, L.BEHAVIOUR_FIXED, L.BEHAVIOUR_EPS_GREEDY]) == L.EINVAL and b"pi is NULL" in err()
    assert _call(pi=None, mode=L.TD_EXPSARSA) == L.EINVAL and b"pi is NULL" in err()
    # ---- the LDS size: refused when one rollout does not fit 160 KiB (queue_host.lds_bytes restates the carve), before any launch
    S = Q.LDS_SLOTS
    big = lambda n, **kw: _call(t=dict(n_slots=n, nA=5), nA=5, **kw)  # noqa: E731
    assert big(S["big-last"], R=0) == L.OK and big(S["refused"]) == L.EUNSUPPORTED and b"160 KiB" in err() and err().startswith(b"eval_queue_pop")
    assert big(S["refused"], R=0) == L.EUNSUPPORTED and big(5 << 20) == L.EUNSUPPORTED
    n_nopi = next(n for n in range(5, 1 << 20, 5) if Q.launch_shape(n, 5, False, True)[2])
    assert n_nopi > S["refused"] and big(n_nopi - 5, R=0, pi=None) == L.OK and big(n_nopi, pi=None) == L.EUNSUPPORTED


def test_eval_queue_answers_its_own_tests_inputs_as_before():
    """offsim_eval_queue's checks moved into a helper both entry points call: the inputs of test_eval_queue_validation_before_any_hip_call, with
    the codes that test asserts (the test itself is part of the suite and runs as it is), and the order in which two faults are reported."""
    from rl_offline_simulation_amd import _lib as L
    err = L.load().offsim_last_error
    assert single_call(R=0) == L.OK and single_call(R=0, td={}) == L.OK and single_call(R=0, td=dict(tie_mt=F), reseed=1) == L.OK
    assert single_call(kind=L.STREAM_PHILOX) == L.EUNSUPPORTED and b"(0, 1]" in err() and err().startswith(b"eval_queue:")
    assert single_call(t=dict(n_slots=7)) == L.EINVAL and single_call(nA=3) == L.EINVAL and single_call(rng=None) == L.EINVAL
    assert single_call(pi=None) == L.EINVAL and b"pi is NULL" in err()
    assert single_call(pi=None, td=dict(behaviour=L.BEHAVIOUR_EPS_GREEDY), R=0) == L.OK
    assert single_call(td=dict(td_cap=-1)) == L.EINVAL and single_call(reseed=1) == L.EINVAL and single_call(td={}, reseed=1) == L.EINVAL
    # a Philox stream on a table that is also too large: the provider is looked at first; a NULL pi on one: the NULL pi
    assert single_call(t=dict(n_slots=Q.LDS_SLOTS["refused"], nA=5), nA=5, td={}, kind=L.STREAM_PHILOX) == L.EUNSUPPORTED and b"(0, 1]" in err()
    assert single_call(t=dict(n_slots=Q.LDS_SLOTS["refused"], nA=5), nA=5, td={}, pi=None) == L.EINVAL
    assert single_call(t=dict(n_slots=Q.LDS_SLOTS["refused"], nA=5), nA=5, td={}) == L.EUNSUPPORTED and b"160 KiB" in err()


# ---- the carve and the case list ----
def test_the_restated_lds_formula_gives_each_case_its_launch():
    want = {"lds-waves4": (4, False, 3 * 1), "lds-waves2": (2, False, 3 * 2), "lds-waves1": (1, False, 3 * 3), "lds-big": (1, True, 3 * 3)}
    for name, (w, big, groups) in want.items():
        c = H.BY_NAME[name]
        assert (c.log.N, c.S, c.L) == (2000, 3, 3) and c.log.n_slots == c.n_slots and c.log.nA == 5
        got = c.shape
        assert (got[0], got[1] > 65536, got[2], got[3]) == (w, big, False, groups), name
        comp = np.concatenate([(c.log.z - c.log.z_lo) * c.log.nA + c.log.a, (c.log.z_next - c.log.z_lo) * c.log.nA])
        assert c.log.n_slots <= max(1024, 4 * len(np.unique(comp))), name  # (TransitionTable keeps such ids dense)
    assert sorted(H.BY_NAME[n].n_slots for n in want) == [Q.LDS_SLOTS[k] for k in ("waves4", "waves2", "waves1", "big")]
    base = H.BY_NAME["qlearn-eps-first"]
    assert base.shape[0] == 4 and base.shape[3] == 3 * 2  # 5 seeds: a full and a partly filled workgroup per learner
    assert H.BY_NAME["qlearn-eps-L1-S1"].shape[3] == 1 and H.BY_NAME["qlearn-every-behaviour-L2-S9"].shape[3] == 2 * 3
    assert H.launch_shape(Q.LDS_SLOTS["refused"], 5, 3, 5)[2] and not H.launch_shape(Q.LDS_SLOTS["big-last"], 5, 3, 5)[2]


def test_the_case_list_covers_what_the_issue_names():
    C = H.CASES
    by = lambda f: [c for c in C if f(c)]  # noqa: E731
    assert all(len(set(v)) == c.L for c in C if c.name != "qlearn-greedy-fresh" for v in (c.alpha, c.epsilon, c.gamma))
    assert all(len(set(v)) == 3 for v in (H.BY_NAME["qlearn-greedy-fresh"].alpha, H.BY_NAME["qlearn-greedy-fresh"].gamma))
    assert by(lambda c: (c.L, c.S, c.N, c.nZ, c.nA) == (3, 5, 600, 5, 5)) and by(lambda c: (c.L, c.S) == (1, 1)) and by(lambda c: (c.L, c.S) == (2, 9))
    for beh in ((H.F,) * 3, (H.E,) * 3, (H.SOFT,) * 3):
        assert by(lambda c: c.mode == H.QLEARN and c.behaviour == beh), beh
    assert by(lambda c: c.behaviour == (H.E,) * 3 and set(c.epsilon) == {0.0})  # greedy
    assert by(lambda c: {H.F, H.E, H.SOFT} <= set(c.behaviour) and 0.0 in [e for e, b in zip(c.epsilon, c.behaviour) if b == H.E])
    assert by(lambda c: c.mode == H.EXPSARSA and c.pi_per_learner) and by(lambda c: c.mode == H.EXPSARSA and not c.pi_per_learner)
    assert by(lambda c: c.sched) and {c.tie for c in C} == {"first", "fresh", "mid", "episode"}
    assert by(lambda c: c.tie == "episode" and c.episode0 == 2 ** 32 - 2) and {c.q0 for c in C} == {"zero", "rand"}
    assert by(lambda c: c.log.nA == 70) and by(lambda c: c.neg_state and c.log.z_lo == -1) and by(lambda c: c.holes) and by(lambda c: c.n_episodes == 2)
    assert by(lambda c: c.r32 and c.log.r.dtype == np.float32) and by(lambda c: c.snap)
    a, e = H.schedules(H.BY_NAME["qlearn-eps-schedules-episode"])
    assert len(set(a[0])) > 1 and len(set(e[0])) > 1 and all(len(set(a[l])) == 1 and len(set(e[l])) == 1 for l in (1, 2))


@pytest.mark.parametrize("name", [c.name for c in H.CASES])
def test_no_case_is_vacuous(name):
    c = H.BY_NAME[name]
    o = H.host(c)
    assert tuple(o["q"].shape) == (c.L, c.S, c.log.nZ, c.log.nA)
    if c.n_episodes is not None:
        assert (o["status"] == H.ST_OK).all() and (o["n_ep"] == c.n_episodes).all()
    elif c.holes:
        assert (o["status"] == H.ST_KEYERROR).all() and (o["steps"] > 0).any()
    else:
        assert np.isin(o["status"], (H.ST_EXHAUSTED, H.ST_NO_INIT)).all() and (o["steps"] > 0).all()
    if c.L > 1:  # on every seed at least two learners end with different Q
        assert all(any(not np.array_equal(o["q"][a, j], o["q"][b, j]) for a in range(c.L) for b in range(a)) for j in range(c.S)), name
    if c in H.TIE_CASES:  # every epsilon-greedy rollout met two or more maxima after its first step
        m = H.run_population(c, snap_all=True)
        assert np.array_equal(m["q"], o["q"])
        assert all(H.ties_after_the_first_step(c, l, j, m) >= 1 for l in range(c.L) if c.behaviour[l] == H.E for j in range(c.S)), name
    if c.streams():
        mt0 = H.mt_of(c)
        eps = [l for l in range(c.L) if c.behaviour[l] == H.E]
        if not c.holes and c.q0 == "zero":  # every such learner drew from its stream
            assert all(not np.array_equal(o["tie_mt"][l, j], mt0[l, j]) for l in eps for j in range(c.S)), name
        if c.tie == "mid":  # position 600 of 624, and some rollout crossed the block: the words changed, not only the position
            assert (mt0[..., 624] == 600).all()
            assert any(not np.array_equal(o["tie_mt"][l, j, :624], mt0[l, j, :624]) for l in eps for j in range(c.S)), name
        others = [l for l in range(c.L) if c.behaviour[l] != H.E]  # the other behaviours leave their streams alone
        assert all(np.array_equal(o["tie_mt"][l, j], mt0[l, j]) for l in others for j in range(c.S)), name


def test_the_case_list_ends_in_every_status_and_every_tie_mode_has_a_tie_case():
    seen = set()
    for c in H.CASES:
        seen |= set(H.host(c)["status"].ravel().tolist())
    assert {H.ST_OK, H.ST_EXHAUSTED, H.ST_KEYERROR} <= seen
    assert {c.tie for c in H.TIE_CASES} == {"first", "fresh", "mid", "episode"}
    assert all(c in H.TIE_CASES for c in H.CASES if c.tie == "mid" or c.episode0)
    # ragged curves: some episode that some but not all seeds completed
    o = H.host(H.BY_NAME["qlearn-every-behaviour-fresh"])
    n, mean, _ = H.curves(o["ep_g"], o["n_ep"])
    assert ((n > 0) & (n < 5)).any() and np.isfinite(mean[n > 0]).all()


# ---- the mirror at one learner replays the reference's recorded drivers ----
def recorded_settings(d, tag, n):
    """(mode, behaviour, alpha, epsilon, alpha_ep, epsilon_ep, Q_init given) of run `tag` of n episodes"""
    mode, beh, eps, q_given, sched = RUNS[tag]
    return (mode, beh, float(d["alpha"]), eps, np.array([ALPHA_SCHED(e) for e in range(n)]) if sched else None,
            np.array([EPS_SCHED(e) for e in range(n)]) if sched else None, q_given)


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(f)[:-4] for f in FIXTURES])
def test_mirror_at_one_learner_replays_the_recorded_drivers(path):
    d, log = np.load(path), golden_log(path)
    nS, gam = int(d["nS"]), float(d["gamma"])
    assert (log.z_lo, log.nZ) == (0, nS)
    for s in (int(v) for v in d["seeds"]):
        for tag in TD_RUNS:
            k = f"s{s}_{tag}_"
            n = int(d[k + "n"])
            mode, beh, alpha, eps, a_ep, e_ep, q_given = recorded_settings(d, tag, n)
            pi = d["pi"] if tag == "es" else np.full((nS, log.nA), 1.0 / log.nA)
            q0 = d["q_init"].copy() if q_given else np.zeros((nS, log.nA))
            o = Q.run(Q.Sampler(log, s), np.random.default_rng(1000 + s), mode, pi, gam, alpha=alpha, q=q0, behaviour=beh, epsilon=eps, alpha_ep=a_ep,
                      epsilon_ep=e_ep, tie="episode", n_episodes=n, trace_cap=log.N + 1, ep_cap=log.N + 1)
            m = o["steps"]
            assert o["status"] == H.ST_OK and o["n_ep"] == n and np.array_equal(o["tie_mt"], d[k + "mt"]) and np.array_equal(o["ep_g"][:n], d[k + "Gs"]), k
            if tag == "es":  # (the reference's `@` is BLAS: its order of summation is not ours)
                assert np.abs(o["q"] - d[k + "Q"]).max() <= 1e-12 and np.abs(o["td_err"][:m] - d[k + "td"]).max() <= 1e-12, k
            else:
                assert np.array_equal(o["q"], d[k + "Q"]) and np.array_equal(o["td_err"][:m], d[k + "td"]), k
