"""CPU-only: the host helper that cuts a collect record into episodes (tests/true_env_population_host.py), and the refusals of
offsim_eval_env_obs and evalmc_rollouts_true_env, every one of which comes before any HIP call."""
import ctypes as C

import numpy as np
import pytest

import true_env_population_host as P

SERVED, TERM, TRUNC, RESET, ALIVE = 1, 2, 4, 8, 16
LIVE = SERVED | ALIVE


# ---- episodes_from_records on hand-built records ----
def test_episodes_terminated_truncated_and_open_tail():
    # episode 0: three steps, terminated; episode 1: two steps, truncated; episode 2: terminated and truncated at once; then an open tail
    flags = [LIVE, LIVE, LIVE | TERM | RESET, LIVE, LIVE | TRUNC | RESET, LIVE | TERM | TRUNC | RESET, LIVE, LIVE]
    reward = np.array([1.0, -0.1, 0.5, 1.0, 1.0, 2.0, 7.0, 7.0], np.float32)
    Gs, lengths, ended = P.episodes_from_records(flags, reward, np.zeros(8, np.int32), 0.9)
    assert lengths.tolist() == [3, 2, 1] and ended.tolist() == [TERM, TRUNC, TERM | TRUNC]
    r = [float(v) for v in reward]  # the f32 rewards widened: -0.1f is not the double -0.1
    assert Gs.tolist() == [(0.0 + 0.9 ** 0 * r[0]) + 0.9 ** 1 * r[1] + 0.9 ** 2 * r[2], (0.0 + r[3]) + 0.9 ** 1 * r[4], 0.0 + r[5]]
    assert Gs.dtype == np.float64 and lengths.dtype == np.int32 and ended.dtype == np.uint8


def test_episode_that_ends_at_the_last_step():
    flags = [LIVE, LIVE | TERM | RESET, LIVE, LIVE | TRUNC | RESET]
    Gs, lengths, ended = P.episodes_from_records(flags, np.ones(4, np.float32), np.zeros(4, np.int32), 0.5)
    assert lengths.tolist() == [2, 2] and ended.tolist() == [TERM, TRUNC] and Gs.tolist() == [1.5, 1.5]


def test_open_tail_alone_and_empty():
    Gs, lengths, ended = P.episodes_from_records([LIVE, LIVE], np.ones(2, np.float32), np.zeros(2, np.int32), 0.9)
    assert len(Gs) == len(lengths) == len(ended) == 0
    Gs, lengths, ended = P.episodes_from_records([], np.zeros(0, np.float32), np.zeros(0, np.int32), 0.9)
    assert len(Gs) == 0 and np.isnan(P.sequential_mean(Gs))


def test_gamma_one_is_the_plain_f64_sum_in_step_order():
    reward = np.array([-0.1] * 7 + [1.0], np.float32)
    flags = [LIVE] * 7 + [LIVE | TERM | RESET]
    Gs, lengths, _ = P.episodes_from_records(flags, reward, np.ones(8, np.int32), 1.0)
    want = 0.0
    for v in reward:
        want = want + float(v)
    assert Gs.tolist() == [want] and lengths.tolist() == [8]
    assert P.sequential_mean([1.0, 2.0, 4.0]) == (1.0 + 2.0 + 4.0) / 3.0


def test_a_stopped_environment_ends_the_record():
    # the third step could not be served (no action drawn): flags 0, and nothing after it counts
    flags = [LIVE, LIVE | TERM | RESET, 0, 0]
    Gs, lengths, _ = P.episodes_from_records(flags, np.array([1, 1, 0, 0], np.float32), np.array([0, 1, 2, -1], np.int32), 0.9)
    assert lengths.tolist() == [2] and Gs.tolist() == [1.0 + 0.9]


# ---- the C ABI's argument checks (before any HIP call) ----
def _capi():
    from rl_offline_simulation_amd import _lib as L
    lib = L.load()
    bufs = [(C.c_uint64 * 1024)() for _ in range(3)]
    p = [C.cast(b, C.c_void_p).value for b in bufs]

    def env(kind, S=2, num_cells=5, num_steps=15):
        return L.EnvEval(kind=kind, S=S, num_cells=num_cells, num_steps=num_steps, goal_x=4, goal_y=4, rng_env=p[0], rng_act=p[1])

    def mlp(widths, form=L.COLLECT_MLP, x_dtype=L.F32):
        arr = (L.MLPLayer * (len(widths) - 1))()
        for i, (a, b) in enumerate(zip(widths, widths[1:])):
            arr[i].W, arr[i].b, arr[i].out = p[0], p[1], b
            setattr(arr[i], "in", a)
        c = L.CollectPolicy(form=form, n_layers=len(arr), layers_host=C.cast(arr, C.POINTER(L.MLPLayer)), activation=L.ACT_TANH, x_dtype=x_dtype,
                            dO=widths[0])
        c._keep = arr
        return c

    out = L.EnvEvalOut(**{k: p[2] for k in ("Gs", "lengths", "ended", "n_ep", "steps", "status", "value")})

    def call(e, pol, L_=1, n_ep=3, cap=500, gp=p[2], n_gp=1024, o=out):
        return lib.offsim_eval_env_obs(None if e is None else C.byref(e), None if pol is None else C.byref(pol), L_, n_ep, cap, gp, n_gp,
                                       None if o is None else C.byref(o), None)

    return L, lib, env, mlp, out, call


def _err(lib):
    return lib.offsim_last_error().decode()


def test_capi_refusals():
    L, lib, env, mlp, out, call = _capi()
    cp, gr, co = env(L.ENV_CARTPOLE), env(L.ENV_GRID), env(L.ENV_GRID_COORDS)
    ok = mlp((4, 8, 8, 2))
    assert call(None, ok) == L.EINVAL and "env is NULL" in _err(lib)
    assert call(cp, None) == L.EINVAL and call(cp, ok, o=None) == L.EINVAL
    assert call(env(7), ok) == L.EINVAL and "kind" in _err(lib)
    assert call(env(L.ENV_CARTPOLE, S=-1), ok) == L.EINVAL
    no_streams = env(L.ENV_CARTPOLE)
    no_streams.rng_act = None
    assert call(no_streams, ok) == L.EINVAL and "rng_act" in _err(lib)
    assert call(env(L.ENV_GRID, num_cells=0), mlp((1, 8, 5))) == L.EINVAL and call(env(L.ENV_GRID, num_steps=0), mlp((1, 8, 5))) == L.EINVAL
    assert call(cp, ok, n_ep=-1) == L.EINVAL and call(cp, ok, cap=-1) == L.EINVAL
    # the network against the kind: the observation's width, then the actions
    for e, widths in ((cp, (2, 8, 2)), (gr, (2, 8, 5)), (co, (1, 8, 5)), (co, (4, 8, 5))):
        assert call(e, mlp(widths)) == L.EINVAL and "input width" in _err(lib), widths
    for e, widths in ((cp, (4, 8, 5)), (gr, (1, 8, 2)), (co, (2, 8, 4))):
        assert call(e, mlp(widths)) == L.EINVAL and "nA" in _err(lib), widths
    assert call(cp, mlp((4, 8, 17))) == L.EINVAL
    # the observations are the environment's own f32
    assert call(cp, mlp((4, 8, 2), x_dtype=L.F16)) == L.EINVAL and "f32" in _err(lib)
    # no logged rows, and tabular policies are another entry's
    for form in (L.COLLECT_TABULAR, L.COLLECT_ROWS):
        assert call(gr, L.CollectPolicy(form=form, x_dtype=L.F64, pi=1)) == L.EUNSUPPORTED and "OFFSIM_COLLECT_MLP" in _err(lib)
    # the population
    for n in (0, -1, 65536):
        assert call(cp, ok, L_=n) == L.EINVAL and "1..65535" in _err(lib)
    assert call(env(L.ENV_CARTPOLE, S=0), ok, L_=65535) == L.OK
    # CartPole needs a cap; the grids do not
    assert call(cp, ok, cap=0) == L.EINVAL and "max_episode_steps" in _err(lib)
    assert call(env(L.ENV_GRID, S=0), mlp((1, 8, 5)), cap=0) == L.OK
    # gamma_pow covers the longest episode: the cap, on the grids num_steps or a cap below it
    assert call(cp, ok, cap=500, n_gp=499) == L.EINVAL and "gamma_pow" in _err(lib)
    assert call(cp, ok, gp=None) == L.EINVAL
    assert call(env(L.ENV_GRID, S=0), mlp((1, 8, 5)), cap=0, n_gp=14) == L.EINVAL
    assert call(env(L.ENV_GRID, S=0), mlp((1, 8, 5)), cap=0, n_gp=15) == L.OK
    assert call(env(L.ENV_GRID, S=0), mlp((1, 8, 5)), cap=7, n_gp=7) == L.OK
    assert call(env(L.ENV_GRID, S=0), mlp((1, 8, 5)), cap=100, n_gp=15) == L.OK
    # the trace
    assert call(cp, ok, o=L.EnvEvalOut(trace_cap=-1)) == L.EINVAL and "trace_cap" in _err(lib)
    # the workgroup's LDS: 4-256-256-2 is 67 586 floats, 264 KiB; 4-128-256-2 (134 KiB of weights and 8 rollouts' rows) still fits
    assert call(cp, mlp((4, 256, 256, 2))) == L.EUNSUPPORTED and "160 KiB" in _err(lib)
    assert call(env(L.ENV_CARTPOLE, S=0), mlp((4, 128, 256, 2))) == L.OK
    # with rollouts to run, the outputs must be there
    assert call(cp, ok, o=L.EnvEvalOut()) == L.EINVAL and "out->Gs" in _err(lib)
    # S = 0 and n_episodes = 0 launch nothing and need no outputs
    assert call(env(L.ENV_CARTPOLE, S=0), ok, o=L.EnvEvalOut()) == L.OK
    assert call(cp, ok, n_ep=0, o=L.EnvEvalOut()) == L.OK


# ---- the Python entry: every refusal before a device is asked for ----
def _nets(widths, n=1, activation="tanh"):
    from rl_offline_simulation_amd.evaluators import MLPPolicy
    g = np.random.default_rng(3)
    return [MLPPolicy([(g.standard_normal((b, a)).astype(np.float32), np.zeros(b, np.float32)) for a, b in zip(widths, widths[1:])], activation)
            for _ in range(n)]


def test_python_refusals(monkeypatch):
    from rl_offline_simulation_amd import _lib as L
    from rl_offline_simulation_amd.evaluators import CallablePolicy, PolicyPopulation, RowPolicy, evalmc_rollouts_true_env as run

    def no_device():
        raise AssertionError("a refusal must come before any device is asked for")

    monkeypatch.setattr(L, "require_device", no_device)
    monkeypatch.setattr(L, "stream_ptr", no_device)
    ok = _nets((4, 8, 2))
    rows = RowPolicy(np.ones((3, 2)), np.ones((3, 2)))
    with pytest.raises(ValueError, match="width"):
        run("cartpole", [1, 2], _nets((2, 8, 2)), 0.9, 3)
    with pytest.raises(ValueError, match="actions"):
        run("grid_coords", [1, 2], _nets((2, 8, 2)), 0.9, 3)
    with pytest.raises(ValueError, match="width"):
        run("grid", [1, 2], _nets((2, 8, 5)), 0.9, 3, num_cells=4)
    with pytest.raises(NotImplementedError):
        run("cartpole", [1, 2], [ok[0], rows], 0.9, 3)
    with pytest.raises(NotImplementedError):
        run("cartpole", [1, 2], PolicyPopulation.from_rows([rows]), 0.9, 3)
    with pytest.raises(NotImplementedError):
        run("cartpole", [1, 2], CallablePolicy(lambda x: x), 0.9, 3)
    with pytest.raises(ValueError, match="no policies"):
        run("cartpole", [1, 2], [], 0.9, 3)
    with pytest.raises(TypeError):
        run("cartpole", [1, 2], [np.ones((25, 5))], 0.9, 3)
    with pytest.raises(ValueError, match="max_episode_steps"):
        run("cartpole", [1, 2], ok, 0.9, 3, max_episode_steps=0)
    with pytest.raises(ValueError, match="max_episode_steps"):
        run("grid", [1, 2], _nets((1, 8, 5)), 0.9, 3, max_episode_steps=-1)
    with pytest.raises(ValueError, match="n_episodes"):
        run("cartpole", [1, 2], ok, 0.9, -1)
    with pytest.raises(ValueError, match="environment is one of"):
        run("pendulum", [1, 2], ok, 0.9, 3)
    with pytest.raises(TypeError):
        run("cartpole", [1, 2], ok, 0.9, 3, num_cells=5)
    with pytest.raises(TypeError):
        run("grid", [1, 2], _nets((1, 8, 5)), 0.9, 3, cells=5)
    with pytest.raises(ValueError, match="action seed"):
        run("cartpole", [1, 2], ok, 0.9, 3, action_seeds=[1])
    with pytest.raises(ValueError, match="tile"):
        run("cartpole", [1, 2], ok, 0.9, 3, tile=0)
    # the library's own limit, found through its checks: the workgroup's LDS
    with pytest.raises(L.OffsimError, match="160 KiB"):
        run("cartpole", [1, 2], _nets((4, 256, 256, 2)), 0.9, 3)


def test_python_empty_results_need_no_device(monkeypatch):
    from rl_offline_simulation_amd import _lib as L
    from rl_offline_simulation_amd.evaluators import evalmc_rollouts_true_env as run
    monkeypatch.setattr(L, "require_device", lambda: (_ for _ in ()).throw(AssertionError("no launch expected")))
    nets = _nets((4, 8, 2), n=3)
    r = run("cartpole", [], nets, 0.9, 3)
    assert r["value"].shape == (3, 0) and r["Gs"].shape == (3, 0, 3) and r["best"] == -1 and np.isnan(r["mean_value"]).all()
    r = run("cartpole", [1, 2], nets, 0.9, 0, trace_cap=4)
    assert r["value"].shape == (3, 2) and np.isnan(r["value"]).all() and r["Gs"].shape == (3, 2, 0) and (r["n_ep"] == 0).all()
    assert r["trace_action"].shape == (3, 2, 4) and (r["trace_action"] == -1).all() and (r["status"] == L.ST_OK).all()
