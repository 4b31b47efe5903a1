"""What the latent-state driver tests (tests/test_gpu_latent_env.py) rest on, checked without a device: the plain Python loop of
tests/latent_env_host.py reproduces what the reference's own z_expSARSA, evalMC and qlearn returned on its own MyGridNaviCoords behind a
seeded MLP encoder (tests/golden/latent_env/coords_mlp.npz); the host box encoder is the oracle's at the thresholds, their f32 neighbours
and out of bounds; the -1 wrap reads the last row; the package's host mirror (LatentEnv.reset / step) agrees with that loop; and the C ABI
of offsim_eval_env_latent / offsim_eval_env_latent_pop and the Python entries refuse every bad argument before any HIP call (the pointers
are fake addresses: a launch would fault)."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import latent_env_host as H  # noqa: E402
from oracle import oracle as O  # noqa: E402
from rl_offline_simulation_amd.evaluators import latent_env_drivers as T  # noqa: E402

F = 0x1000


# ---- the fixtures ----
def test_fixture_holds_every_run_and_a_clear_gap():
    f = H.Fixture()
    assert len(f.runs) == 2 * 2 * 2 * len(H.DRIVERS) and {r.split("|")[0] for r in f.runs} == set(H.DRIVERS)
    assert float(f.d["min_gap"]) > 1e-3 and int(f.d["n_latent"]) >= 4 and os.path.getsize(os.path.join(H.GOLDEN, "coords_mlp.npz")) < 256 * 1024
    assert f.weights[0].shape == (16, 2) and f.weights[2].shape == (25, 16) and all(w.dtype == np.float32 for w in f.weights)
    assert (f.d["Gs"] > 0).any() and (f.d["mt_pos"] < 624).any()  # goals are reached, ties are drawn


def test_host_loop_replays_the_recorded_drivers():
    f = H.Fixture()
    d, n, gam, al = f.d, int(f.d["n_episodes"]), float(f.d["gamma"]), float(f.d["alpha"])
    enc = H.MlpEncoder(f.weights)
    for i in range(len(f.runs)):
        drv, goal, num_steps, seed = f.settings(i)
        mode, beh, eps = H.DRIVERS[drv]
        w = H.LiveWorld("coords", enc, reseed=True, num_steps=num_steps, goal=goal)
        for rec_max in ((True, False) if drv == "z_expSARSA" else (False,)):
            o = H.run(w, 25, 5, H.chooser(np.random.default_rng(seed), 5), mode, d["pi"], gam, alpha=al, q=None if mode == H.EVALMC else np.zeros((25, 5)),
                      behaviour=beh, epsilon=0.0 if eps is None else eps, epsilon_ep=np.array([H.EPS_SCHED(e) for e in range(n)]) if eps is None else None,
                      tie=None if drv == "evalMC" else "episode", n_episodes=n, trace_cap=n * num_steps, ep_cap=n, snap_cap=n * num_steps, rec_max=rec_max)
            m = o["steps"]
            assert o["status"] == H.ST_OK and o["n_ep"] == n and np.array_equal(o["ep_g"], d["Gs"][i]), f.runs[i]
            if drv == "evalMC":
                assert np.array_equal(o["ep_len"][:n], d["lengths"][i]), f.runs[i]
                continue
            assert np.array_equal(o["tie_mt"], f.mt(i)), f.runs[i]  # np.random.seed(last episode), advanced by that episode's ties
            Qs = np.concatenate([np.zeros((1, 25, 5)), o["q_snap"][:m]])
            if drv == "qlearn_eps" or drv == "qlearn_eps_sched":
                assert np.array_equal(o["q"], d["Q"][i]) and np.array_equal(o["td_err"][:m], f.td(i)) and np.array_equal(Qs, f.Qs(i)), f.runs[i]
            else:  # the reference's `@` is BLAS: its order of summation is not ours
                assert np.abs(o["q"] - d["Q"][i]).max() <= 1e-12 and np.abs(Qs - f.Qs(i)).max() <= 1e-12, f.runs[i]
                if rec_max:  # the recorded error: R + gamma * max Q[z'] - Q[z, A], a plain expression on a Q that agrees to 1e-12
                    assert np.abs(o["td_err"][:m] - f.td(i)).max() <= 1e-12, f.runs[i]
                else:
                    assert len(f.td(i)) == m
    assert min(enc.gaps) > 1e-3 and abs(min(enc.gaps) - float(d["min_gap"])) < 1e-12


def test_z_expsarsa_recorded_error_is_bit_exact_where_the_update_is():
    """with a one-hot pi the sum Q[z_] @ pi[z_] has one non-zero term: the update is order-free, so z_expSARSA matches bit for bit -- checked on
    a loop of its own against the plain expressions of tabular.py:229 / :232"""
    w = H.LiveWorld("coords", H.MlpEncoder(H.Fixture().weights), reseed=True, num_steps=6, goal=(1, 1))
    pi = np.eye(5)[np.random.default_rng(2).integers(0, 5, 25)]
    q = np.random.default_rng(3).standard_normal((25, 5))
    q0 = q.copy()
    o = H.run(w, 25, 5, H.chooser(np.random.default_rng(4), 5), H.EXPSARSA, pi, 0.9, alpha=0.5, q=q, n_episodes=3, trace_cap=18, rec_max=True)
    Q = q0
    for k in range(o["steps"]):
        z, a, r, z_ = (o[key][k] for key in ("trace_z", "trace_pop", "trace_reward", "trace_z_next"))
        assert o["td_err"][k] == r + 0.9 * Q[z_].max() - Q[z, a]
        Q[z, a] = Q[z, a] + 0.5 * (r + 0.9 * (Q[z_] @ pi[z_]) - Q[z, a])
    assert np.array_equal(Q, o["q"])


# ---- the box encoder ----
def _box_cases():
    f = np.float32
    th = [f(v) for v in (-2.4, 2.4, -0.8, 0.8, -0.5, 0.5, 0.0174532, -0.0174532, 0.1047192, -0.1047192, 0.2094384, -0.2094384, 0.87266, -0.87266, 0.0)]
    vals = sorted({float(v) for t in th for v in (t, np.nextafter(t, f(np.inf)), np.nextafter(t, f(-np.inf)))})
    rows = []
    for k in range(4):
        for v in vals:
            row = [0.01, 0.02, 0.003, 0.04]
            row[k] = v
            rows.append(row)
    g = np.random.default_rng(0)
    rows += (g.uniform(-1, 1, (400, 4)) * [2.6, 1.0, 0.23, 1.5]).tolist()
    rows += [[3.0, 0, 0, 0], [0, 0, 0.3, 0], [-2.5, 9, 0, 9], [0, 0, -0.21, 0], [np.nan, 0, 0, 0]]
    return np.array(rows, np.float32)


def test_host_box_encoder_is_the_oracles_at_thresholds_neighbours_and_out_of_bounds():
    x = _box_cases()
    want = O.cartpole_encode(x)
    assert (want == -1).sum() >= 10 and want.max() > 100
    assert [T.box_of(r) for r in x] == want.tolist()
    assert [H.BoxEncoder()(r) for r in x] == want.tolist()


def test_the_minus_one_wrap_reads_the_last_row():
    """CartPole falls over: the terminal step's z' is -1, and Q[-1] is the last row -- a Q_init whose last row is distinct shows up in
    the first terminal TD error"""
    q = np.zeros((163, 2))
    q[162] = [7.0, 5.0]
    w = H.LiveWorld("cartpole", H.BoxEncoder(), reseed=True, cap=500)
    o = H.run(w, 163, 2, H.chooser(np.random.default_rng(0), 2), H.QLEARN, np.tile([1.0, 0.0], (163, 1)), 0.9, alpha=0.0, q=q, n_episodes=1, trace_cap=500)
    m = o["steps"]
    assert m < 500 and o["trace_z_next"][m - 1] == -1 and o["trace_done"][m - 1] == 1  # always pushing left: out of bounds
    assert o["td_err"][m - 1] == 1.0 + 0.9 * 7.0 - 0.0 and (o["trace_z_next"][:m - 1] >= 0).all()
    env = T.LatentEnv("cartpole", _box(), 163)
    assert env.row(-1) == 162 and env.row(5) == 5 and T.LatentEnv("cartpole", _box(), 162).row(-1) == 161


# ---- the package's host mirror ----
def _box():
    from rl_offline_simulation_amd.encoders import CartpoleBoxEncoder
    return CartpoleBoxEncoder()


def _homer(dO, Hd, nZ, seed=1, scale=1.0):
    from rl_offline_simulation_amd.encoders import HOMEREncoder
    from rl_offline_simulation_amd.encoders.homer import ENC_KEYS
    return HOMEREncoder(dO, 5 if dO == 2 else 2, nZ, Hd, state_dict=dict(zip(ENC_KEYS, H.mlp_weights(dO, Hd, nZ, seed, scale))), device="cpu")


def test_host_mirror_agrees_with_the_host_loop():
    f = H.Fixture()
    from rl_offline_simulation_amd.encoders import HOMEREncoder
    from rl_offline_simulation_amd.encoders.homer import ENC_KEYS
    enc = HOMEREncoder(2, 5, 25, 16, state_dict=dict(zip(ENC_KEYS, f.weights)), device="cpu")
    env = T.LatentEnv("grid_coords", enc, 25, num_steps=7, goal=(1, 1))
    assert (env.nS, env.nA, env.bound, env.s) == (25, 5, 7, None)
    w = H.LiveWorld("coords", H.MlpEncoder(f.weights), reseed=True, num_steps=7, goal=(1, 1))
    g = np.random.default_rng(3)
    for e in range(4):
        z, zw, done = env.reset(seed=e), w.reset(e), False
        assert z == zw
        while not done:
            a = int(g.integers(5))
            (z, r, done, _), (zw, rw, dw) = env.step(a), w.step(a)
            assert (z, r, done) == (zw, rw, dw) and np.array_equal(env.state_row(), w.state_row())
    box = T.LatentEnv("cartpole", _box(), 163, max_episode_steps=30)
    wb = H.LiveWorld("cartpole", H.BoxEncoder(), reseed=True, cap=30)
    z, zw, done, n = box.reset(seed=5), wb.reset(5), False, 0
    assert z == zw and np.array_equal(box.state_row(), np.random.default_rng(5).uniform(-0.05, 0.05, 4))
    while not done:
        (z, r, done, _), (zw, rw, dw) = box.step(n % 2), wb.step(n % 2)
        n += 1
        assert (z, r, done) == (zw, rw, dw) and np.array_equal(box.state_row(), wb.state_row())
    assert n <= 30
    with pytest.raises(ValueError):
        box.step(2)


def test_cartpole_mlp_weights_keep_the_skipped_steps_within_one_percent():
    """the 4-8-10 encoder of the GPU test: on the host loop alone, the steps whose f64 top-2 gap is below encoder_host's tolerance for the
    shape (where an in-tolerance f32 forward may choose the other state) are at most 1 % of all steps"""
    enc = H.MlpEncoder(H.mlp_weights(4, 8, 10, H.CARTPOLE_MLP_WEIGHT_SEED))
    for seed in H.CARTPOLE_MLP_SEEDS:
        w = H.LiveWorld("cartpole", enc, reseed=True, cap=40)
        H.run(w, 10, 2, H.chooser(np.random.default_rng(seed), 2), H.EVALMC, np.full((10, 2), 0.5), 0.9, n_episodes=4)
    clear, _ = H.clear_rows(enc.weights, np.stack(enc.obs))
    assert len(clear) > 100 and (~clear).sum() <= 0.01 * len(clear), ((~clear).sum(), len(clear))


# ---- the Python entries refuse before they touch the device ----
def test_python_refusals(monkeypatch):
    from rl_offline_simulation_amd import _lib as L
    from rl_offline_simulation_amd.evaluators import TDPopulation

    def no_device():
        raise AssertionError("a refusal must come before any device is asked for")

    monkeypatch.setattr(L, "require_device", no_device)
    monkeypatch.setattr(L, "stream_ptr", no_device)
    with pytest.raises(ValueError, match="kind"):
        T.LatentEnv("grid", _box(), 163)
    with pytest.raises(ValueError, match="box encoder reads CartPole"):
        T.LatentEnv("grid_coords", _box(), 163)
    with pytest.raises(ValueError, match="at least 162"):
        T.LatentEnv("cartpole", _box(), 161)
    with pytest.raises(ValueError, match="input width"):
        T.LatentEnv("cartpole", _homer(2, 8, 10), 10)
    with pytest.raises(ValueError, match="latent states but num_states"):
        T.LatentEnv("grid_coords", _homer(2, 8, 10), 9)
    with pytest.raises(ValueError, match="at most 4096"):
        T.LatentEnv("grid_coords", _homer(2, 4097, 3), 9)
    with pytest.raises(TypeError):
        T.LatentEnv("cartpole", object(), 163)
    with pytest.raises(ValueError, match="max_episode_steps"):
        T.LatentEnv("cartpole", _box(), 163, max_episode_steps=0)
    with pytest.raises(ValueError, match="off the"):
        T.LatentEnv("grid_coords", _homer(2, 8, 10), 10, num_cells=3, goal=(3, 0))
    from rl_offline_simulation_amd.encoders import HOMEREncoder
    with pytest.raises(ValueError, match="no weights"):
        T.LatentEnv("grid_coords", HOMEREncoder(2, 5, 10, 8, device="cpu"), 10)
    w = T.LatentEnv("cartpole", _box(), 163)
    assert w.max_episode_steps == 500 and w.bound == 500
    bad = np.full((162, 2), 0.5)
    for call in (lambda: T.evalMC_latent_env(w, 3, bad, 0.9, seed=0), lambda: T.expSARSA_latent_env(w, 3, bad, 0.9, seed=0),
                 lambda: T.z_expSARSA_env(w, 3, bad, 0.9, seed=0), lambda: T.evalmc_rollouts_latent_env(w, [0, 1], bad, 0.9, 3),
                 lambda: T.evalmc_rollouts_latent_env(w, [0], np.full((2, 3, 163, 2), 0.5), 0.9, 3)):
        with pytest.raises(ValueError, match="pi must be"):
            call()
    ok = np.full((163, 2), 0.5)
    with pytest.raises(ValueError, match="reseed"):
        T.evalmc_rollouts_latent_env(w, [0, 1], ok, 0.9, 3, reseed="step")
    with pytest.raises(ValueError, match="action seed"):
        T.evalmc_rollouts_latent_env(w, [0, 1], ok, 0.9, 3, action_seeds=[1])
    with pytest.raises(ValueError, match="n_episodes"):
        T.evalmc_rollouts_latent_env(w, [0, 1], ok, 0.9, 0)
    with pytest.raises(NotImplementedError):
        T.qlearn_latent_env(w, 3, lambda Q, args: np.abs(Q) / np.abs(Q).sum(axis=1, keepdims=True), 0.9, seed=0)
    uniform_beh = lambda Q, args: np.ones_like(Q) / Q.shape[1]  # noqa: E731
    with pytest.raises(ValueError, match="Q_init"):
        T.qlearn_latent_env(w, 3, uniform_beh, 0.9, Q_init=np.zeros((162, 2)), seed=0)
    with pytest.raises(ValueError, match="tie"):
        T.qlearn_latent_env(w, 3, uniform_beh, 0.9, seed=0, tie="last")
    with pytest.raises(TypeError):
        T.evalMC_latent_env(object(), 3, ok, 0.9)
    with pytest.raises(TypeError):
        TDPopulation("qlearn", 0.1, 0.9).run_latent_env(object(), [0], 3)
    with pytest.raises(ValueError, match="n_episodes"):
        TDPopulation("qlearn", 0.1, 0.9).run_latent_env(w, [0], 0)
    with pytest.raises(ValueError, match="expected"):
        TDPopulation("expsarsa", 0.1, 0.9, pi=bad).run_latent_env(w, [0], 3)
    with pytest.raises(ValueError, match="tie"):
        TDPopulation("qlearn", 0.1, 0.9).run_latent_env(w, [0], 3, tie="last")
    with pytest.raises(ValueError, match="reseed"):
        TDPopulation("qlearn", 0.1, 0.9).run_latent_env(w, [0], 3, reseed="step")
    # n_episodes = 0 is the reference's empty result, no launch; no seeds, no launch
    Gs, lengths = T.evalMC_latent_env(w, 0, ok, 0.9, seed=0)
    assert len(Gs) == 0 and len(lengths) == 0
    Q, info = T.z_expSARSA_env(w, 0, ok, 0.9, seed=0)
    assert Q.shape == (163, 2) and info["memory"] == []
    r = T.evalmc_rollouts_latent_env(w, [], np.stack([ok, ok]), 0.9, 3)
    assert r["value"].shape == (2, 0) and r["best"] == -1


# ---- the C ABI ----
def test_symbols_exported_bound_and_documented():
    from rl_offline_simulation_amd import _lib
    src = open(os.path.join(ROOT, "include", "offsim.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("offsim_eval_env_latent", "offsim_eval_env_latent_pop"):
        assert "int " + n + "(" in src and hasattr(lib, n) and n in _lib.SIGNATURES
    doc = src[src.index("* offsim_eval_env_latent:"):src.index("int offsim_eval_env_latent(")]
    for word in ("rgument validation happens before any HIP call", "OFFSIM_EUNSUPPORTED", "launches nothing", "160 KiB", "64 KiB", "4096", "tabular.py:",
                 "z + nS", "rec_max", "reseed", "OFFSIM_LATENT_BOX", "OFFSIM_LATENT_MLP", "L * S"):
        assert word in doc, word


def _call(S=5, env=None, enc=None, run=None, ro=True, pi=F, out=True, td=None, gp=None, n_gp=0, n_ep=10, pop=None, LS=None, **outkw):
    """offsim_eval_env_latent (LS None) or offsim_eval_env_latent_pop (LS = (L, S); pop: offsim_td_pop fields, None: the evalMC stack) on fake
    pointers; env / enc / run: fields to change (False: NULL).  The default is CartPole with the box encoder, nS = 163, cap 500."""
    from rl_offline_simulation_amd import _lib as L
    ec = L.EnvEval(kind=L.ENV_CARTPOLE, S=S, num_cells=5, num_steps=15, goal_x=4, goal_y=4, rng_env=F, rng_act=F)
    nc = L.LatentEncoder(kind=L.LATENT_BOX, nS=163, dO=4, H=8, nZ=10, W1=F, b1=F, W2=F, b2=F)
    rc = L.LatentRun(reseed=1, max_episode_steps=500)
    for st, kw in ((ec, env), (nc, enc), (rc, run)):
        for k, v in (kw or {}).items():
            setattr(st, k, v)
    okw = dict(sum_g=F, n_ep=F, steps=F, cand=F, n_len=F, status=F)
    okw.update(outkw)
    oc = L.EvalMCOut(**okw)
    e, n, r, o = (None if x is False else ctypes.byref(s) for x, s in ((env, ec), (enc, nc), (run, rc), (out, oc)))
    if LS is not None:
        pc = None
        if pop is not None:
            pop = dict(pop)
            beh = (ctypes.c_int32 * LS[0])(*([pop.pop("beh", L.BEHAVIOUR_FIXED)] * LS[0]))
            kw = dict(mode=L.TD_QLEARN, alpha=F, epsilon=F, gamma=F, gamma_pow=gp, n_gamma_pow=n_gp, behaviour=F,
                      behaviour_host=ctypes.cast(beh, ctypes.POINTER(ctypes.c_int32)), pi=F, q=F, snap_stride=1)
            kw.update(pop)
            pc = ctypes.byref(L.TDPop(**kw))
        return L.load().offsim_eval_env_latent_pop(e, n, LS[0], LS[1], pc, pi, 0.9, gp, n_gp, n_ep, o, r, None)
    tdc = None
    if td is not None:
        kw = dict(mode=L.TD_QLEARN, alpha=0.1, q=F, behaviour=L.BEHAVIOUR_FIXED, snap_stride=1)
        kw.update(td)
        tdc = L.TD(**kw)
    return L.load().offsim_eval_env_latent(e, n, pi, 0.9, gp, n_gp, n_ep, o, None if tdc is None else ctypes.byref(tdc), r, None)


MLP4 = dict(kind=1, nS=10)                                   # CartPole's 4-8-10
COORDS, MLP2 = dict(kind=1), dict(kind=1, nS=25, dO=2, H=16, nZ=25)  # the coordinate grid's 2-16-25


def test_eval_env_latent_validation_before_any_hip_call():
    from rl_offline_simulation_amd import _lib as L
    err = L.load().offsim_last_error
    assert _call(S=0) == L.OK, err()  # S = 0 validates and launches nothing
    assert _call(S=0, td={}) == L.OK and _call(S=0, td=dict(behaviour=L.BEHAVIOUR_EPS_GREEDY), pi=None) == L.OK
    assert _call(S=0, td=dict(tie_mt=F), run=dict(tie_reseed_episode=1)) == L.OK
    assert _call(S=0, enc=MLP4) == L.OK and _call(S=0, env=COORDS, enc=MLP2, run=dict(max_episode_steps=0)) == L.OK, err()
    assert _call(S=0, td=dict(mode=L.TD_EXPSARSA), run=dict(rec_max=1)) == L.OK
    # the world and its pairing with the encoder
    assert _call(env=False) == L.EINVAL and _call(enc=False) == L.EINVAL and _call(run=False) == L.EINVAL
    assert _call(env=dict(kind=L.ENV_GRID)) == L.EUNSUPPORTED and b"discrete grid" in err()
    assert _call(env=dict(kind=3)) == L.EINVAL and _call(env=dict(kind=-1)) == L.EINVAL and b"kind" in err()
    assert _call(env=COORDS) == L.EUNSUPPORTED and b"OFFSIM_LATENT_BOX" in err()  # the box encoder on the grid
    assert _call(env=dict(kind=1, num_cells=0), enc=MLP2) == L.EINVAL and _call(env=dict(kind=1, num_steps=0), enc=MLP2) == L.EINVAL
    assert _call(env=dict(kind=1, goal_x=5), enc=MLP2) == L.EINVAL and b"off the grid" in err()
    assert _call(env=COORDS, enc=MLP4) == L.EINVAL and b"input width" in err()  # a 4-wide encoder on the grid's 2-wide observation
    assert _call(enc=dict(kind=2)) == L.EINVAL and _call(enc=dict(nS=0)) == L.EINVAL and _call(enc=dict(nS=161)) == L.EINVAL and b"162" in err()
    assert _call(S=0, enc=dict(nS=162)) == L.OK
    assert _call(enc=dict(kind=1, nS=10, W1=None)) == L.EINVAL and _call(enc=dict(kind=1, nS=10, b2=None)) == L.EINVAL
    assert _call(enc=dict(kind=1, nS=9)) == L.EINVAL and b"nZ" in err()
    assert _call(enc=dict(kind=1, nS=10, H=0)) == L.EINVAL and _call(enc=dict(kind=1, nS=10, nZ=0)) == L.EINVAL
    # H / nZ beyond the limits and beyond the carve
    assert _call(enc=dict(kind=1, nS=10, H=4097)) == L.EUNSUPPORTED and b"4096" in err()
    assert _call(enc=dict(kind=1, nS=5000, nZ=4097)) == L.EUNSUPPORTED
    mlp = lambda Hd: (4, Hd, 10)  # noqa: E731
    last = max(h for h in range(1, 4097) if not H.launch_shape(10, 2, True, False, mlp(h))[2])
    assert last < 4096 and _call(S=0, enc=dict(kind=1, nS=10, H=last)) == L.OK
    assert _call(enc=dict(kind=1, nS=10, H=last + 1)) == L.EUNSUPPORTED and b"160 KiB" in err()
    # the table: nS * nA beyond the one-rollout carve
    big = max(s for s in range(163, 20481) if not H.launch_shape(s, 2, True, True)[2])
    assert _call(S=0, enc=dict(nS=big), td={}) == L.OK and _call(enc=dict(nS=big + 1), td={}) == L.EUNSUPPORTED and b"160 KiB" in err()
    assert _call(enc=dict(nS=20481)) == L.EUNSUPPORTED
    # the run
    assert _call(run=dict(reseed=2)) == L.EINVAL and _call(run=dict(max_episode_steps=-1)) == L.EINVAL
    assert _call(run=dict(max_episode_steps=0)) == L.EINVAL and b"CartPole needs max_episode_steps" in err()
    assert _call(run=dict(episode0=-1)) == L.EINVAL and _call(run=dict(rec_max=2)) == L.EINVAL and _call(run=dict(trace_cap=-1)) == L.EINVAL
    assert _call(run=dict(rec_max=1)) == L.EINVAL and _call(run=dict(rec_max=1), td={}) == L.EINVAL and b"OFFSIM_TD_EXPSARSA" in err()
    # the streams
    assert _call(env=dict(rng_act=None)) == L.EINVAL and _call(env=dict(rng_env=None), run=dict(reseed=0)) == L.EINVAL
    assert _call(S=0, env=dict(rng_env=None)) == L.OK and _call(S=-1) == L.EINVAL
    # NULLs
    assert _call(out=False) == L.EINVAL and _call(status=None) == L.EINVAL and _call(sum_g=None) == L.EINVAL
    assert _call(pi=None) == L.EINVAL and b"pi is NULL" in err()
    assert _call(pi=None, td={}) == L.EINVAL and _call(pi=None, td=dict(mode=L.TD_EXPSARSA, behaviour=L.BEHAVIOUR_SOFT_GREEDY)) == L.EINVAL
    assert _call(n_gp=4) == L.EINVAL and b"gamma_pow" in err()
    assert _call(ep_cap=-1) == L.EINVAL and _call(trace_cap=-1) == L.EINVAL
    assert _call(n_ep=0) == L.EINVAL and _call(n_ep=-3) == L.EINVAL and b"n_episodes" in err()
    # the learner
    assert _call(td=dict(mode=0)) == L.EINVAL and _call(td=dict(mode=3)) == L.EINVAL and _call(td=dict(q=None)) == L.EINVAL
    assert _call(td=dict(behaviour=7)) == L.EINVAL
    assert _call(td=dict(alpha_ep=F, n_sched=0)) == L.EINVAL and _call(td=dict(epsilon_ep=F, n_sched=0)) == L.EINVAL and _call(td=dict(td_cap=-1)) == L.EINVAL
    assert _call(td=dict(q_snap=F, snap_stride=0)) == L.EINVAL and _call(td=dict(q_snap=F, snap_cap=-1)) == L.EINVAL
    assert _call(run=dict(tie_reseed_episode=2)) == L.EINVAL and _call(run=dict(tie_reseed_episode=1)) == L.EINVAL
    assert _call(td={}, run=dict(tie_reseed_episode=1)) == L.EINVAL and b"tie_mt" in err()


def test_eval_env_latent_pop_validation_before_any_hip_call():
    from rl_offline_simulation_amd import _lib as L
    err = L.load().offsim_last_error
    # the evalMC stack
    assert _call(S=0, LS=(3, 2)) == L.OK, err()
    assert _call(S=6, LS=(3, 2), pi=None) == L.EINVAL and b"pi_stack" in err()
    assert _call(S=5, LS=(3, 2)) == L.EINVAL and b"L * S" in err()
    assert _call(S=0, LS=(0, 2)) == L.EINVAL and _call(S=0, LS=(65536, 1)) == L.EINVAL and _call(S=0, LS=(1, 0)) == L.EINVAL
    assert _call(S=6, LS=(3, 2), run=dict(tie_reseed_episode=1)) == L.EINVAL and _call(S=6, LS=(3, 2), run=dict(rec_max=1)) == L.EINVAL
    assert _call(S=6, LS=(3, 2), n_ep=0) == L.EINVAL and _call(S=6, LS=(3, 2), env=COORDS) == L.EUNSUPPORTED
    assert _call(S=6, LS=(3, 2), run=dict(max_episode_steps=0)) == L.EINVAL and _call(S=6, LS=(3, 2), enc=dict(nS=20481)) == L.EUNSUPPORTED
    # learners
    assert _call(S=0, LS=(3, 2), pop={}) == L.OK, err()
    assert _call(S=0, LS=(3, 2), pop=dict(tie_mt=F), run=dict(tie_reseed_episode=1)) == L.OK
    assert _call(S=0, LS=(3, 2), pop=dict(mode=L.TD_EXPSARSA), run=dict(rec_max=1)) == L.OK
    assert _call(S=5, LS=(3, 2), pop={}) == L.EINVAL and b"L * S" in err() and _call(S=0, LS=(0, 2), pop={}) == L.EINVAL
    assert _call(S=6, LS=(3, 2), pop=dict(alpha=None)) == L.EINVAL and _call(S=6, LS=(3, 2), pop=dict(behaviour_host=None)) == L.EINVAL
    assert _call(S=6, LS=(3, 2), pop=dict(beh=9)) == L.EINVAL and _call(S=6, LS=(3, 2), pop=dict(mode=0)) == L.EINVAL
    assert _call(S=6, LS=(3, 2), pop=dict(q=None)) == L.EINVAL
    assert _call(S=6, LS=(3, 2), pop=dict(pi=None)) == L.EINVAL and b"pi is NULL" in err()
    assert _call(S=0, LS=(3, 2), pop=dict(pi=None, beh=L.BEHAVIOUR_EPS_GREEDY)) == L.OK
    assert _call(S=6, LS=(3, 2), pop=dict(pi=None, beh=L.BEHAVIOUR_EPS_GREEDY, mode=L.TD_EXPSARSA)) == L.EINVAL
    assert _call(S=6, LS=(3, 2), pop=dict(alpha_ep=F, n_sched=0)) == L.EINVAL and _call(S=6, LS=(3, 2), pop=dict(q_snap=F, snap_stride=0)) == L.EINVAL
    assert _call(S=6, LS=(3, 2), pop=dict(td_cap=-1)) == L.EINVAL
    assert _call(S=6, LS=(3, 2), pop={}, run=dict(tie_reseed_episode=1)) == L.EINVAL and b"tie_mt" in err()
    assert _call(S=6, LS=(3, 2), pop={}, run=dict(rec_max=1)) == L.EINVAL
    assert _call(S=6, LS=(3, 2), pop={}, env=COORDS) == L.EUNSUPPORTED and _call(S=6, LS=(3, 2), pop={}, enc=dict(kind=1, nS=10, H=4097)) == L.EUNSUPPORTED
    big = max(s for s in range(163, 20481) if not H.launch_shape(s, 2, True, True)[2])
    assert _call(S=0, LS=(3, 2), pop={}, enc=dict(nS=big)) == L.OK and _call(S=6, LS=(3, 2), pop={}, enc=dict(nS=big + 1)) == L.EUNSUPPORTED


def test_the_restated_lds_rule_gives_the_matrix_its_launch_shapes():
    assert [H.launch_shape(s, 2, False)[0] for s in (163, H.nS_for_waves(2, 2, 163), H.nS_for_waves(1, 2, 163))] == [4, 2, 1]
    assert H.launch_shape(25, 5, True, True, (2, 16, 25))[0] == 4
