"""What the grid-world driver tests (tests/test_gpu_env_drivers.py) rest on, checked without a device: the host mirror's integers(n) is
NumPy's, the plain Python loop of tests/env_drivers_host.py over the host mirror reproduces what the reference's own drivers returned on
its own grid worlds (tests/golden/env_drivers/*.npz), the C ABI of offsim_eval_env / offsim_eval_env_pop refuses every bad argument before
any HIP call (the pointers are fake addresses: a launch would fault), and so do the Python drivers."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import env_drivers_host as H  # noqa: E402
from rl_offline_simulation_amd.evaluators import true_env_drivers as T  # noqa: E402

F = 0x1000


def test_integers_on_the_buffered_halves_is_numpys():
    for n in range(1, 8):
        for e in range(200):
            g, s = np.random.default_rng(e), T.ExoStream(e)
            assert [int(g.integers(n)) for _ in range(40)] == [s.integers(n) for _ in range(40)], (n, e)


def test_four_fixtures_with_every_run():
    for name in H.WORLDS:
        f = H.Fixture(name)
        assert len(f.runs) == 2 * 2 * 2 * len(H.DRIVERS) and {r.split("|")[0] for r in f.runs} == set(H.DRIVERS)
        assert os.path.getsize(os.path.join(H.GOLDEN, name + ".npz")) < 64 * 1024
        assert (f.d["R"] == 1.0).any() and (f.d["mt_pos"] < 624).any()  # goals are reached, ties are drawn


@pytest.mark.parametrize("name", list(H.WORLDS))
def test_host_loop_replays_the_recorded_drivers(name):
    f = H.Fixture(name)
    d, n, gam, al = f.d, int(f.d["n_episodes"]), float(f.d["gamma"]), float(f.d["alpha"])
    for i in range(len(f.runs)):
        drv, goal, num_steps, seed = f.settings(i)
        mode, beh, eps = H.DRIVERS[drv]
        w = T.GridWorld(5, num_steps, goal, f.kind, f.factor)
        pi = d["pi"] if drv in ("evalMC", "rollout", "expSARSA") else H.uniform(w.nS)
        mem = []
        o = H.run(w, np.random.default_rng(seed), mode, pi, gam, alpha=al, q=None if mode == H.EVALMC else np.zeros((w.nS, 5)), behaviour=beh,
                  epsilon=0.0 if eps is None else eps, epsilon_ep=np.array([H.EPS_SCHED(e) for e in range(n)]) if eps is None else None,
                  tie=None if drv == "evalMC" else "episode", n_episodes=n, trace_cap=n * num_steps, ep_cap=n, snap_cap=n * num_steps, memory=mem)
        m = o["steps"]
        assert o["status"] == H.ST_OK and o["n_ep"] == n and np.array_equal(o["ep_g"], d["Gs"][i]), f.runs[i]
        if drv == "evalMC":
            assert np.array_equal(o["ep_len"][:n], d["lengths"][i]), f.runs[i]
            continue
        got, want = H.memory_arrays(mem), f.memory(i)
        assert all(np.array_equal(got[k], want[k]) for k in want), f.runs[i]
        if drv == "rollout":
            continue
        assert np.array_equal(o["tie_mt"], f.mt(i)), f.runs[i]  # np.random.seed(last episode), advanced by that episode's ties
        Qs = np.concatenate([np.zeros((1, w.nS, 5)), o["q_snap"][:m]])
        if mode == H.EXPSARSA:  # (the reference's `@` is BLAS: its order of summation is not ours)
            assert np.abs(o["q"] - d["Q"][i]).max() <= 1e-12 and np.abs(o["td_err"][:m] - f.td(i)).max() <= 1e-12, f.runs[i]
            assert np.abs(Qs - f.Qs(i)).max() <= 1e-12, f.runs[i]
        else:
            assert np.array_equal(o["q"], d["Q"][i]) and np.array_equal(o["td_err"][:m], f.td(i)) and np.array_equal(Qs, f.Qs(i)), f.runs[i]


def test_single_steps_on_the_host_mirror():
    w = T.GridWorld(3, 4, (1, 1), "counter", 4)
    assert (w.nS, w.nA, w.s) == (36, 5, None)
    s0 = w.reset(seed=2)
    c = int(np.random.default_rng(2).integers(4))
    assert s0 == 9 * c
    s1, r, done, info = w.step(2)
    assert (s1, r, done) == (1 + 9 * ((c + 1) % 4), -0.1, False) and (info["z"], info["z_next"], info["t"], info["task_id"]) == (0, 1, 0, 4)
    s2, r, done, _ = w.step(1)
    assert (s2 % 9, r, done, w.s) == (4, 1.0, True, s2)
    with pytest.raises(ValueError):
        w.step(5)


# ---- the Python drivers refuse before they touch the device ----
def test_python_refusals():
    with pytest.raises(ValueError, match="factor"):
        T.GridWorld(kind="noise", factor=0)
    with pytest.raises(ValueError, match="factor"):
        T.GridWorld(kind="plain", factor=2)
    with pytest.raises(ValueError, match="off the"):
        T.GridWorld(num_cells=3, goal=(3, 0))
    with pytest.raises(ValueError, match="kind"):
        T.GridWorld(kind="history")
    with pytest.raises(ValueError, match="positive"):
        T.GridWorld(num_steps=0)
    w = T.GridWorld(kind="noise", factor=2)
    bad = np.full((25, 5), 0.2)
    for call in (lambda: T.evalMC_env(w, 3, bad, 0.9, seed=0), lambda: T.rollout_env(w, 3, bad, 0.9, seed=0), lambda: T.expSARSA_env(w, 3, bad, 0.9, seed=0),
                 lambda: T.evalmc_rollouts_env(w, [0, 1], bad, 0.9, 3), lambda: T.evalmc_rollouts_env(w, [0], np.full((2, 3, 50, 5), 0.2), 0.9, 3)):
        with pytest.raises(ValueError, match="pi must be"):
            call()
    with pytest.raises(NotImplementedError):
        T.qlearn_env(w, 3, lambda Q, args: np.abs(Q) / np.abs(Q).sum(axis=1, keepdims=True), 0.9, seed=0)
    uniform_beh = lambda Q, args: np.ones_like(Q) / Q.shape[1]  # noqa: E731
    with pytest.raises(ValueError, match="Q_init"):
        T.qlearn_env(w, 3, uniform_beh, 0.9, Q_init=np.zeros((25, 5)), seed=0)
    with pytest.raises(ValueError, match="tie"):
        T.qlearn_env(w, 3, uniform_beh, 0.9, seed=0, tie="last")
    with pytest.raises(TypeError):
        T.evalMC_env(object(), 3, bad, 0.9)
    from rl_offline_simulation_amd.evaluators import TDPopulation
    with pytest.raises(TypeError):
        TDPopulation("qlearn", 0.1, 0.9).run_env(object(), [0], 3)
    with pytest.raises(ValueError, match="n_episodes"):
        TDPopulation("qlearn", 0.1, 0.9).run_env(w, [0], 0)
    with pytest.raises(ValueError, match="expected"):
        TDPopulation("expsarsa", 0.1, 0.9, pi=bad).run_env(w, [0], 3)
    with pytest.raises(ValueError, match="tie"):
        TDPopulation("qlearn", 0.1, 0.9).run_env(w, [0], 3, tie="last")
    # n_episodes = 0 is the reference's empty result, no launch
    Gs, lengths = T.evalMC_env(w, 0, np.full((50, 5), 0.2), 0.9, seed=0)
    assert len(Gs) == 0 and len(lengths) == 0


# ---- the C ABI ----
def test_symbols_exported_bound_and_documented():
    from rl_offline_simulation_amd import _lib
    src = open(os.path.join(ROOT, "include", "offsim.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("offsim_eval_env", "offsim_eval_env_pop"):
        assert "int " + n + "(" in src and hasattr(lib, n) and n in _lib.SIGNATURES
        doc = src[src.index("/* " + n + ":"):src.index("int " + n + "(")]
        for word in ("rgument validation happens before any HIP call", "OFFSIM_EUNSUPPORTED", "launches nothing"):
            assert word in doc, (n, word)
    doc = src[src.index("/* offsim_eval_env:"):src.index("int offsim_eval_env(")]
    for word in ("OFFSIM_STREAM_PHILOX", "(0, 1]", "160 KiB", "64 KiB", "tabular.py:", "gridworld.py:", "tie_reseed_episode", "cdf_k", "integers", "Lemire"):
        assert word in doc, word


def _call(R=5, env=None, ro=True, pi=F, kind=0, out=True, td=None, gp=None, n_gp=0, reseed=0, episode0=0, rng=F, n_ep=10, pop=None, LS=None, **outkw):
    """offsim_eval_env (LS None) or offsim_eval_env_pop (LS = (L, S); pop: offsim_td_pop fields, None: the evalMC stack) on fake pointers;
    env: world fields to change (False: NULL)."""
    from rl_offline_simulation_amd import _lib as L
    ec = L.GridEnv(kind=L.GRID_NOISE, num_cells=5, num_steps=15, goal_x=4, goal_y=4, factor=2)
    for k, v in (env or {}).items():
        setattr(ec, k, v)
    roc = L.EnvRollouts(R=R, rng_kind=kind, rng=rng)
    okw = dict(sum_g=F, n_ep=F, steps=F, cand=F, n_len=F, status=F)
    okw.update(outkw)
    oc = L.EvalMCOut(**okw)
    e, r, o = None if env is False else ctypes.byref(ec), ctypes.byref(roc) if ro else None, ctypes.byref(oc) if out else None
    if LS is not None:
        pc = None
        if pop is not None:
            beh = (ctypes.c_int32 * LS[0])(*([pop.pop("beh", L.BEHAVIOUR_FIXED)] * LS[0]))
            kw = dict(mode=L.TD_QLEARN, alpha=F, epsilon=F, gamma=F, gamma_pow=gp, n_gamma_pow=n_gp, behaviour=F,
                      behaviour_host=ctypes.cast(beh, ctypes.POINTER(ctypes.c_int32)), pi=F, q=F, snap_stride=1)
            kw.update(pop)
            pc = ctypes.byref(L.TDPop(**kw))
        return L.load().offsim_eval_env_pop(e, r, LS[0], LS[1], pc, pi, 0.9, gp, n_gp, n_ep, o, reseed, episode0, None)
    tdc = None
    if td is not None:
        kw = dict(mode=L.TD_QLEARN, alpha=0.1, q=F, behaviour=L.BEHAVIOUR_FIXED, snap_stride=1)
        kw.update(td)
        tdc = L.TD(**kw)
    return L.load().offsim_eval_env(e, r, pi, 0.9, gp, n_gp, n_ep, o, None if tdc is None else ctypes.byref(tdc), reseed, episode0, None)


def test_eval_env_validation_before_any_hip_call():
    from rl_offline_simulation_amd import _lib as L
    err = L.load().offsim_last_error
    assert _call(R=0) == L.OK, err()  # R = 0 validates and launches nothing
    assert _call(R=0, td={}) == L.OK and _call(R=0, td=dict(behaviour=L.BEHAVIOUR_EPS_GREEDY), pi=None) == L.OK
    assert _call(R=0, td=dict(tie_mt=F), reseed=1) == L.OK
    # the world
    assert _call(env=False) == L.EINVAL
    assert _call(env=dict(kind=3)) == L.EINVAL and _call(env=dict(kind=-1)) == L.EINVAL and b"kind" in err()
    assert _call(env=dict(num_cells=0)) == L.EINVAL and _call(env=dict(num_steps=0)) == L.EINVAL
    assert _call(env=dict(goal_x=5)) == L.EINVAL and _call(env=dict(goal_y=-1)) == L.EINVAL and b"off the grid" in err()
    assert _call(env=dict(factor=0)) == L.EINVAL and _call(env=dict(kind=L.GRID_PLAIN)) == L.EINVAL and b"factor" in err()
    assert _call(R=0, env=dict(kind=L.GRID_PLAIN, factor=1)) == L.OK and _call(R=0, env=dict(kind=L.GRID_COUNTER, factor=1)) == L.OK
    # the action stream: Philox is refused, nothing is stepped
    assert _call(kind=L.STREAM_PHILOX) == L.EUNSUPPORTED and b"(0, 1]" in err()
    assert _call(kind=5) == L.EINVAL
    # NULLs
    assert _call(ro=False) == L.EINVAL and _call(R=-1) == L.EINVAL and _call(rng=None) == L.EINVAL
    assert _call(out=False) == L.EINVAL and _call(status=None) == L.EINVAL and _call(sum_g=None) == L.EINVAL
    assert _call(pi=None) == L.EINVAL and b"pi is NULL" in err()
    assert _call(pi=None, td={}) == L.EINVAL and _call(pi=None, td=dict(mode=L.TD_EXPSARSA, behaviour=L.BEHAVIOUR_SOFT_GREEDY)) == L.EINVAL
    assert _call(n_gp=4) == L.EINVAL and b"gamma_pow" in err()
    assert _call(ep_cap=-1) == L.EINVAL and _call(trace_cap=-1) == L.EINVAL
    # an environment never runs dry
    assert _call(n_ep=0) == L.EINVAL and _call(n_ep=-3) == L.EINVAL and b"max_episodes" in err()
    assert _call(episode0=-1) == L.EINVAL
    # the learner
    assert _call(td=dict(mode=0)) == L.EINVAL and _call(td=dict(mode=3)) == L.EINVAL and _call(td=dict(q=None)) == L.EINVAL
    assert _call(td=dict(behaviour=7)) == L.EINVAL
    assert _call(td=dict(alpha_ep=F, n_sched=0)) == L.EINVAL and _call(td=dict(epsilon_ep=F, n_sched=0)) == L.EINVAL and _call(td=dict(td_cap=-1)) == L.EINVAL
    assert _call(td=dict(q_snap=F, snap_stride=0)) == L.EINVAL and _call(td=dict(q_snap=F, snap_cap=-1)) == L.EINVAL
    # the tie modes
    assert _call(reseed=2) == L.EINVAL and _call(reseed=1) == L.EINVAL and _call(td={}, reseed=1) == L.EINVAL and b"tie_mt" in err()
    # the LDS rule of the learner shape (env_drivers_host.lds_bytes restates the carve): one rollout past 160 KiB is refused
    last = max(f for f in range(1, 400) if not H.launch_shape(125 * f)[2])
    big = lambda f, **kw: _call(env=dict(factor=f), **kw)  # noqa: E731
    assert big(last, R=0, td={}) == L.OK and big(last + 1, td={}) == L.EUNSUPPORTED and b"160 KiB" in err()
    assert _call(env=dict(num_cells=203, goal_x=0, goal_y=0), td={}) == L.EUNSUPPORTED
    # evalMC reads a policy that does not fit LDS from global memory: no refusal until nS * 5 > 2^24
    assert big(last + 1, R=0) == L.OK and big(1 << 18, R=0) == L.EUNSUPPORTED and b"2^24" in err()


def test_eval_env_pop_validation_before_any_hip_call():
    from rl_offline_simulation_amd import _lib as L
    err = L.load().offsim_last_error
    # the evalMC stack
    assert _call(R=0, LS=(3, 2)) == L.OK, err()
    assert _call(R=6, LS=(3, 2), pi=None) == L.EINVAL and b"pi_stack" in err()
    assert _call(R=5, LS=(3, 2)) == L.EINVAL and b"L * S" in err()
    assert _call(R=0, LS=(0, 2)) == L.EINVAL and _call(R=0, LS=(65536, 1)) == L.EINVAL and _call(R=0, LS=(1, 0)) == L.EINVAL
    assert _call(R=6, LS=(3, 2), reseed=1) == L.EINVAL and _call(R=6, LS=(3, 2), n_ep=0) == L.EINVAL
    assert _call(R=6, LS=(3, 2), env=dict(factor=0)) == L.EINVAL and _call(R=6, LS=(3, 2), kind=L.STREAM_PHILOX) == L.EUNSUPPORTED
    assert _call(R=6, LS=(3, 2), env=dict(factor=1 << 18)) == L.EUNSUPPORTED
    # learners
    assert _call(R=0, LS=(3, 2), pop={}) == L.OK, err()
    assert _call(R=0, LS=(3, 2), pop=dict(tie_mt=F), reseed=1) == L.OK
    assert _call(R=5, LS=(3, 2), pop={}) == L.EINVAL and _call(R=0, LS=(0, 2), pop={}) == L.EINVAL
    assert _call(R=6, LS=(3, 2), pop=dict(alpha=None)) == L.EINVAL and _call(R=6, LS=(3, 2), pop=dict(behaviour_host=None)) == L.EINVAL
    assert _call(R=6, LS=(3, 2), pop=dict(beh=9)) == L.EINVAL and _call(R=6, LS=(3, 2), pop=dict(mode=0)) == L.EINVAL
    assert _call(R=6, LS=(3, 2), pop=dict(q=None)) == L.EINVAL
    assert _call(R=6, LS=(3, 2), pop=dict(pi=None)) == L.EINVAL and b"pi is NULL" in err()
    assert _call(R=0, LS=(3, 2), pop=dict(pi=None, beh=L.BEHAVIOUR_EPS_GREEDY)) == L.OK
    assert _call(R=6, LS=(3, 2), pop=dict(pi=None, beh=L.BEHAVIOUR_EPS_GREEDY, mode=L.TD_EXPSARSA)) == L.EINVAL
    assert _call(R=6, LS=(3, 2), pop=dict(alpha_ep=F, n_sched=0)) == L.EINVAL and _call(R=6, LS=(3, 2), pop=dict(q_snap=F, snap_stride=0)) == L.EINVAL
    assert _call(R=6, LS=(3, 2), pop=dict(td_cap=-1)) == L.EINVAL
    assert _call(R=6, LS=(3, 2), pop={}, reseed=1) == L.EINVAL and b"tie_mt" in err()
    assert _call(R=6, LS=(3, 2), pop={}, n_ep=0) == L.EINVAL and _call(R=6, LS=(3, 2), pop={}, env=dict(goal_x=7)) == L.EINVAL
    last = max(f for f in range(1, 400) if not H.launch_shape(125 * f)[2])
    assert _call(R=0, LS=(3, 2), pop={}, env=dict(factor=last)) == L.OK and _call(R=6, LS=(3, 2), pop={}, env=dict(factor=last + 1)) == L.EUNSUPPORTED


def test_the_restated_lds_rule_gives_the_matrix_its_launch_shapes():
    assert [H.launch_shape(125 * f, False)[0] for f in (1, 13, H.factor_for_waves(2), H.factor_for_waves(1))] == [4, 4, 2, 1]
    assert H.factor_for_waves(2) == 14 and H.factor_for_waves(1) == 31
    assert 3 * 25 * 22 * 40 > 65536 >= 3 * 25 * 21 * 40  # the evalMC stack of L = 3 leaves LDS at factor 22
