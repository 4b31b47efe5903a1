"""What the PSRS_Exo learner-population tests (tests/test_gpu_exo_td_population.py) rest on, checked without a device: the plain Python loop
of tests/exo_td_population_host.py at L = 1 reproduces what the reference's own qlearn_psrs returned on its own PSRS_Exo under the behaviour
policies that look at Q (tests/golden/exo_td_pop/*.npz) -- Q, returns, TD errors, the final observation and the final state of NumPy's
global MT19937 stream, bit for bit --, the C ABI of offsim_eval_td_exo_pop refuses every bad argument before any HIP call (the pointers
are fake addresses: a launch would fault), and the case list covers what the kernel matrix is meant to cover."""
import ctypes
import glob
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import exo_host as X  # noqa: E402
import exo_td_population_host as H  # noqa: E402
from test_exo_drivers_host import golden_log, obs_after  # noqa: E402
from rl_offline_simulation_amd import _lib as _L  # noqa: E402

_SIGNATURE = _L.SIGNATURES["offsim_eval_td_exo_pop"]  # everything below is about this entry point: without it nothing here has a subject

FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "exo_td_pop", "*.npz")))
RUNS = {"greedy": dict(behaviour=H.EPS_GREEDY, epsilon=0.0), "eps": dict(behaviour=H.EPS_GREEDY), "sched": dict(behaviour=H.EPS_GREEDY, sched=True),
        "soft": dict(behaviour=H.SOFT_GREEDY)}
F = 0x1000


def run_settings(d, run):
    """(alpha, epsilon, alpha_ep, epsilon_ep, behaviour) of a recorded run"""
    s = RUNS[run]
    sched = s.get("sched", False)
    return (0.0 if sched else float(d["alpha"]), 0.0 if sched else s.get("epsilon", float(d["epsilon"])), d["alpha_ep"] if sched else None,
            d["epsilon_ep"] if sched else None, s["behaviour"])


def test_two_fixtures_of_four_runs_each():
    assert [os.path.basename(f) for f in FIXTURES] == ["exo_a_mod4.npz", "exo_c_skewed.npz"]
    for f in FIXTURES:
        d = np.load(f)
        assert d["seeds"].tolist() == [0, 5] and os.path.getsize(f) < 256 * 1024
        fresh = np.random.RandomState(int(d["np_seed"])).get_state()
        for s in (0, 5):
            for run in RUNS:
                mt = d[f"s{s}_{run}_mt"]
                moved = int(mt[624]) != fresh[2] or not np.array_equal(mt[:624], fresh[1])
                assert moved == (run != "soft"), (f, s, run)  # every greedy run tied at least once (from Q = 0: at its first step)


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(f)[:-4] for f in FIXTURES])
def test_host_loop_at_one_learner_replays_the_reference(path):
    d = np.load(path)
    log, combine, nO = golden_log(d)
    obs_of, ids = log.obs_of(combine, nO)
    cap, open_episode = log.N + 1, False
    uniform = np.full((len(ids), log.nA), 1.0 / log.nA)
    for s in (int(v) for v in d["seeds"]):
        for run in RUNS:
            k = f"s{s}_{run}_"
            alpha, eps, a_ep, e_ep, beh = run_settings(d, run)
            rs = np.random.RandomState(int(d["np_seed"]))
            q = np.zeros((len(ids), log.nA))
            o = H.run(X.Sampler(log, s), H.QLEARN, uniform, obs_of, float(d["gamma"]), alpha, q, behaviour=beh, epsilon=eps, alpha_ep=a_ep, epsilon_ep=e_ep,
                      rs=rs, trace_cap=cap, ep_cap=cap)
            full = np.zeros((nO, log.nA))
            full[ids] = o["q"]
            Gs = o["ep_g"][:o["n_ep"] + (o["status"] == X.ST_EXHAUSTED)]  # the cut-short episode's return is appended too (psrs.py:177)
            open_episode |= o["status"] == X.ST_EXHAUSTED
            assert np.array_equal(full, d[k + "Q"]) and np.array_equal(Gs, d[k + "Gs"]) and np.array_equal(o["td_err"][:o["steps"]], d[k + "td"]), k
            assert obs_after(log, combine, d, o) == int(d[k + "o"]) and np.array_equal(o["tie_mt"], d[k + "mt"]), k
    assert open_episode


# ---- the C ABI ----
def test_symbol_exported_bound_and_documented():
    from rl_offline_simulation_amd import _lib
    src = open(os.path.join(ROOT, "include", "offsim.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    n = "offsim_eval_td_exo_pop"
    assert "int " + n + "(" in src and hasattr(lib, n) and n in _lib.SIGNATURES
    doc = src[src.index("/* " + n + ":"):src.index("int " + n + "(")]
    for word in ("rgument validation happens before any HIP call", "OFFSIM_EXO_RESEED_EPISODE", "OFFSIM_EXO_RESEED_NONE", "OFFSIM_EUNSUPPORTED", "obs_of",
                 "160 KiB", "learner-major", "Identity", "n_obs in the place of n_slots"):
        assert word in doc, word


def _call(L=3, S=5, R=None, ts=None, tx=None, rs=True, rx=True, Rx=None, obs_of=F, n_obs=6, reseed=1, kind=0, out=True, pop=True, beh=None, xout=True,
          outkw=None, **popkw):
    """offsim_eval_td_exo_pop on fake pointers; ts / tx: dicts of table fields to change; popkw: fields of struct offsim_td_pop to change."""
    from rl_offline_simulation_amd import _lib as Lb

    def table(n_slots, ch):
        t = Lb.Table(N=10, n_slots=n_slots, nA=2, plog_dtype=Lb.F32, r_dtype=Lb.F32, seg_off=F, p_log=F, a=F, r=F, z_next=F, done=F, orig_idx=F, N0=2,
                     init_slot=F, init_orig=F)
        for k, v in (ch or {}).items():
            setattr(t, k, v)
        return t
    t_s, t_x = table(3, ts), table(2, tx)
    R = L * S if R is None else R
    ro_s = Lb.Rollouts(R=R, rng=F, cursor=F, init_cursor=F, cur_slot=F, rng_kind=kind)
    ro_x = Lb.Rollouts(R=R if Rx is None else Rx, rng=F, cursor=F, init_cursor=F, cur_slot=F)
    okw = dict(sum_g=F, n_ep=F, steps=F, cand=F, n_len=F, status=F)
    okw.update(outkw or {})
    oc, xo = Lb.EvalMCOut(**okw), Lb.ExoOut(trace_row_x=None, last=F)
    bh = (ctypes.c_int32 * max(L, 1))(*([Lb.BEHAVIOUR_EPS_GREEDY] * max(L, 1) if beh is None else beh))
    kw = dict(mode=Lb.TD_QLEARN, alpha=F, epsilon=F, gamma=F, gamma_pow=F, n_gamma_pow=4, behaviour=F, behaviour_host=bh, pi=F, pi_stride=0, q=F, snap_stride=1)
    kw.update(popkw)
    pc = Lb.TDPop(**kw)
    return Lb.load().offsim_eval_td_exo_pop(None if ts is False else ctypes.byref(t_s), None if tx is False else ctypes.byref(t_x),
                                            ctypes.byref(ro_s) if rs else None, ctypes.byref(ro_x) if rx else None, L, S, ctypes.byref(pc) if pop else None,
                                            obs_of, n_obs, reseed, 0, 10, ctypes.byref(oc) if out else None, ctypes.byref(xo) if xout else None, None)


def test_eval_td_exo_pop_validation_before_any_hip_call():
    from rl_offline_simulation_amd import _lib as L
    err = L.load().offsim_last_error
    assert _call(R=0) == L.OK, err()  # R = 0 validates and launches nothing
    assert _call(R=0, xout=False) == L.OK and _call(R=0, reseed=0, kind=L.STREAM_PHILOX) == L.OK and _call(R=0, tie_mt=F, beh_arg=F, td_err=F) == L.OK
    assert _call(R=0, beh=[L.BEHAVIOUR_FIXED, L.BEHAVIOUR_EPS_GREEDY, L.BEHAVIOUR_SOFT_GREEDY]) == L.OK
    # what offsim_eval_mc_exo checks: the two tables
    assert _call(ts=False) == L.EINVAL and _call(tx=False) == L.EINVAL
    assert _call(ts=dict(n_slots=0)) == L.EINVAL and _call(tx=dict(seg_off=None)) == L.EINVAL and _call(ts=dict(plog_dtype=9)) == L.EINVAL
    assert _call(tx=dict(N=11)) == L.EINVAL and b"different logs" in err()
    assert _call(tx=dict(N0=3)) == L.EINVAL and b"different logs" in err()
    assert _call(tx=dict(init_slot=None)) == L.EINVAL and b"init rows" in err()
    # ... the rollouts
    assert _call(rs=False) == L.EINVAL and _call(rx=False) == L.EINVAL and _call(R=-1) == L.EINVAL
    assert _call(Rx=4) == L.EINVAL and b"different R" in err()
    # ... n_obs and obs_of
    for kw in (dict(n_obs=0), dict(n_obs=-3), dict(obs_of=None)):
        assert _call(**kw) == L.EINVAL and err().startswith(b"eval_td_exo_pop"), kw
    # ... the reseed / provider pair
    assert _call(reseed=2) == L.EINVAL and _call(reseed=-1) == L.EINVAL and _call(kind=5) == L.EINVAL
    assert _call(reseed=L.EXO_RESEED_EPISODE, kind=L.STREAM_PHILOX) == L.EUNSUPPORTED and b"PCG64" in err()
    # ... the outputs and capacities
    assert _call(out=False) == L.EINVAL and _call(outkw=dict(status=None)) == L.EINVAL and _call(outkw=dict(sum_g=None)) == L.EINVAL
    assert _call(gamma_pow=None) == L.EINVAL and b"gamma_pow" in err()
    assert _call(outkw=dict(ep_cap=-1)) == L.EINVAL and _call(outkw=dict(trace_cap=-1)) == L.EINVAL and _call(td_cap=-1) == L.EINVAL
    # what offsim_eval_td_pop checks: L, S, R = L * S
    assert _call(pop=False) == L.EINVAL
    for kw in (dict(L=0), dict(L=65536), dict(L=-1), dict(S=0), dict(S=-2)):
        assert _call(R=15, **kw) == L.EINVAL and b"1..65535" in err(), kw
    assert _call(L=65535, S=1, R=0) == L.OK
    assert _call(R=14) == L.EINVAL and b"L * S" in err() and _call(R=16) == L.EINVAL
    # ... the mode, the per-learner arrays, the host copy of the behaviours, the schedules, the snapshots
    assert _call(mode=0) == L.EINVAL and _call(mode=3) == L.EINVAL and _call(q=None) == L.EINVAL
    for k in ("alpha", "epsilon", "gamma", "behaviour", "pi"):
        assert _call(**{k: None}) == L.EINVAL and b"per-learner array" in err(), k
    assert _call(behaviour_host=None) == L.EINVAL and _call(pi_stride=-1) == L.EINVAL and _call(n_gamma_pow=-1) == L.EINVAL
    assert _call(beh=[0, 1, 7]) == L.EINVAL and b"bad behaviour" in err() and _call(beh=[-1, 0, 0]) == L.EINVAL
    assert _call(alpha_ep=F, n_sched=0) == L.EINVAL and _call(epsilon_ep=F, n_sched=0) == L.EINVAL and _call(R=0, alpha_ep=F, epsilon_ep=F, n_sched=3) == L.OK
    assert _call(q_snap=F, snap_stride=0) == L.EINVAL and _call(q_snap=F, snap_cap=-1) == L.EINVAL
    # the LDS size: refused when one rollout does not fit 160 KiB -- the edge found with the restated carve (here ns = 3, nx = 2, nA = 2)
    n_edge = next(n for n in range(1, 1 << 20) if H.launch_shape(3, 2, n, 2)[2])
    assert H.lds_bytes(1, 3, 2, n_edge - 1, 2) <= 160 * 1024 < H.lds_bytes(1, 3, 2, n_edge, 2)
    assert n_edge < next(n for n in range(1, 1 << 20) if X.launch_shape(3, 2, n, 2, 8, True)[2])  # (the tie stream and beh_lds take their place)
    assert _call(R=0, n_obs=n_edge - 1) == L.OK and _call(R=0, n_obs=n_edge) == L.EUNSUPPORTED and b"160 KiB" in err() and err().startswith(b"eval_td_exo_pop")
    assert _call(n_obs=n_edge) == L.EUNSUPPORTED and _call(n_obs=1 << 30) == L.EUNSUPPORTED
    assert _call(ts=dict(n_slots=1 << 20), tx=dict(n_slots=1 << 20)) == L.EUNSUPPORTED


def test_eval_mc_exo_still_refuses_the_greedy_behaviours():
    from rl_offline_simulation_amd import _lib as L
    from test_exo_drivers_host import _call as mc_call
    for b in (L.BEHAVIOUR_EPS_GREEDY, L.BEHAVIOUR_SOFT_GREEDY):
        assert mc_call(td=dict(behaviour=b)) == L.EUNSUPPORTED and b"OFFSIM_BEHAVIOUR_FIXED" in L.load().offsim_last_error()
    assert mc_call(td=dict(tie_mt=F)) == L.EUNSUPPORTED


def test_population_methods_exist():
    from rl_offline_simulation_amd.evaluators import BatchedPSRSExo, TDPopulation, TDPopulationResult
    assert callable(BatchedPSRSExo.eval_td_population) and callable(TDPopulation.run_exo) and "tie_mt" in TDPopulationResult.__dataclass_fields__


# ---- the carve and the case list ----
def test_the_restated_carve_gives_each_case_its_launch():
    assert H.lds_bytes(4, 5, 2, 10, 3) == X.lds_bytes(4, 5, 2, 10, 3, 8, True) + 8 + 4 * 3 * 8 + 4 * 624 * 4
    shapes = {c.name: c.shape for c in H.CASES}
    assert shapes["qlearn-eps-mt-mid"][0] == 4 and shapes["qlearn-eps-mt-mid"][3] == 3 * 2  # 5 seeds: a full and a partly filled workgroup per learner
    assert shapes["lds-waves2"][0] == 2 and shapes["lds-waves2"][3] == 3 * 3
    assert shapes["lds-waves1"][0] == 1 and shapes["lds-waves1"][1] <= 65536 and shapes["lds-waves1"][3] == 15
    assert shapes["lds-above-64k"][0] == 1 and shapes["lds-above-64k"][1] > 65536 and not shapes["lds-above-64k"][2]
    for name, waves, big in (("lds-waves2", 2, False), ("lds-waves1", 1, False), ("lds-above-64k", 1, True)):
        n = H.BY_NAME[name].n_obs_pad
        w, b, refused, _ = H.launch_shape(5, 2, n - 1, 3)
        assert not refused and (w, b > 65536) != (waves, big)  # the first n_obs of its shape


def test_the_case_list_covers_the_kernel():
    C = H.CASES
    by = lambda f: [c for c in C if f(c)]  # noqa: E731
    assert all((c.log.N, c.log.ns, c.log.nx, c.log.nA) == (500, 5, 2, 3) for c in C) and (H.N_L, H.N_S) == (3, 5)
    assert all(len(set(v)) == 3 for c in C for v in (c.alpha, c.epsilon, c.gamma))  # learners that agree in no hyper-parameter
    assert {b for c in C for b in c.behaviour} == {H.F, H.E, H.SOFT} and by(lambda c: len(set(c.behaviour)) == 3)
    assert {c.mode for c in C} == {H.QLEARN, H.EXPSARSA} and {c.reseed for c in C} == {"episode", "none"} and {c.mt for c in C} == {"none", "fresh", "mid"}
    assert by(lambda c: c.pi_per_learner and c.mode == H.EXPSARSA) and by(lambda c: not c.pi_per_learner and c.mode == H.EXPSARSA)
    assert by(lambda c: c.alpha_ep and c.epsilon_ep) and by(lambda c: c.episode0 > (1 << 32)) and by(lambda c: c.stream == "philox" and c.reseed == "none")
    assert not by(lambda c: c.stream == "philox" and c.reseed == "episode")
    assert by(lambda c: c.trace_cap and c.ep_cap) and by(lambda c: c.resume_k == 2) and by(lambda c: c.snap_cap)
    assert {c.shape[0] for c in C} == {4, 2, 1} and by(lambda c: c.shape[1] > 65536)


@pytest.mark.parametrize("name", [c.name for c in H.CASES])
def test_no_case_is_vacuous(name):
    c = H.BY_NAME[name]
    calls = H.host(c)
    o = calls[-1]
    assert np.isin(o["status"], (X.ST_EXHAUSTED, X.ST_NO_INIT)).all() and (calls[0]["steps"] > 0).all()
    assert (np.abs(o["q"]).max(axis=(2, 3)) > 0).all()
    if c.resume_k:
        assert (calls[0]["n_ep"] == c.resume_k).all() and (calls[0]["status"] == X.ST_OK).all() and (o["steps"] > 0).all()
    if c.trace_cap:
        assert (o["steps"] > c.trace_cap).all() and (o["n_ep"] > c.ep_cap).any()
    eps_learners = [l for l in range(H.N_L) if c.behaviour[l] == H.E]
    if c.mt != "none" and eps_learners:
        mt0 = H.mt_of(c)
        assert all(not np.array_equal(o["tie_mt"][l, j], mt0[l, j]) for l in eps_learners for j in range(H.N_S))  # every such learner tied
        if c.mt == "mid":  # ... and some rollout twisted inside the run: the words changed, not only the position
            assert any(not np.array_equal(o["tie_mt"][l, j, :624], mt0[l, j, :624]) for l in eps_learners for j in range(H.N_S))
    # learners differ: no two learners of a seed end with the same Q
    assert all(not np.array_equal(o["q"][a, j], o["q"][b, j]) for a in range(H.N_L) for b in range(a) for j in range(H.N_S))
    if c.curve:
        n, mean, _ = H.curves(o["ep_g"], o["n_ep"])
        assert ((n > 0) & (n < H.N_S)).any() and np.isfinite(mean[n > 0]).all()  # ragged over the seeds
