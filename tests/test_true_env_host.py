"""CPU-only: the host loop of the logged environments (tests/true_env_host.py) against fixtures recorded from the reference's own
MyGridNavi / MyGridNaviCoords (tests/golden/true_env, made by tests/golden/make_golden_true_env.py), bit for bit; the layout of the host
record function; and the argument checks of the offsim_env_* entry points, which run before any HIP call."""
import ctypes as C
import os

import numpy as np
import pytest

import true_env_host as H

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "true_env")


@pytest.mark.parametrize("kind,name", [("grid", "grid.npz"), ("coords", "grid_coords.npz")])
def test_host_grid_equals_reference(kind, name):
    d = np.load(os.path.join(GOLDEN, name))
    assert len(d["seed"]) == 12 and d["actions"].shape == (60,)
    assert sorted(set(d["seed"])) == [0, 4, 9] and sorted(set(d["num_steps"])) == [3, 15]
    assert sorted(set(map(tuple, d["goal"]))) == [(1, 1), (4, 4)]
    for c in range(len(d["seed"])):
        env = H.HostEnv(kind, int(d["seed"][c]), num_cells=5, num_steps=int(d["num_steps"][c]), goal=tuple(d["goal"][c]))
        for i, a in enumerate(d["actions"]):
            o64, o32, z = env.obs64(), env.obs(), env.z
            t = env.step_count
            r, done = env.step(int(a))
            # the observation as the f64 the reference returned, and as its f32 rounding
            assert np.array_equal(np.asarray(o64), d["obs_before"][c, i]), (c, i)
            assert np.array_equal(np.asarray(env.obs64()), d["obs_after"][c, i]), (c, i)
            if kind == "coords":
                assert np.array_equal(o32, d["obs_before"][c, i].astype(np.float32)) and o32.dtype == np.float32
                assert np.array_equal(env.obs(), d["obs_after"][c, i].astype(np.float32))
            assert r == d["reward"][c, i] and done == bool(d["done"][c, i]), (c, i)
            assert (z, env.z, t) == (int(d["z"][c, i]), int(d["z_next"][c, i]), int(d["t"][c, i])), (c, i)
            if done:
                env.reset()


def test_uniform_is_low_plus_range_times_double():
    """What the device computes for a draw: lo + (hi - lo) * next_double, with hi - lo = 0.2 / 0.1 exactly"""
    a, b = np.random.default_rng(5), np.random.default_rng(5)
    assert np.array_equal(a.uniform(-0.1, 0.1, 64), -0.1 + 0.2 * b.random(64))
    assert np.array_equal(a.uniform(-0.05, 0.05, 64), -0.05 + 0.1 * b.random(64))


def test_cartpole_host_equals_synth():
    """The host CartPole is synth.cartpole_log's: same seed stream, same states (its one rng serves resets and actions in turn)."""
    from rl_offline_simulation_amd import synth
    e = synth.cartpole_log(400, seed=3, n_envs=1)
    g = np.random.default_rng(3)
    s = g.uniform(-0.05, 0.05, (1, 4))[0]
    for i in range(400):
        assert np.array_equal(s.astype(np.float32), e["observations"][i])
        a = int(g.random(1)[0] >= 0.5)
        assert a == e["actions"][i]
        s = H.cartpole_step(s, a)
        assert np.array_equal(s.astype(np.float32), e["next_observations"][i])
        assert H.cartpole_done(s) == bool(e["terminals"][i])
        if e["terminals"][i] or e["truncateds"][i]:
            s = g.uniform(-0.05, 0.05, (1, 4))[0]


@pytest.mark.parametrize("kind", ["grid", "coords", "cartpole"])
def test_host_record_layout(kind):
    """record's dataset: the key list of the reference's record_dataset_in_memory (offsim4rl/utils/dataset_utils.py:103-113) plus
    truncateds and the grids' infos/z, infos/z_next; env-major rows cut to N; episode_ids = cumsum(steps == 0) - 1."""
    nA = H.N_ACTIONS[kind]
    p = np.full(nA, 1.0 / nA, np.float32)
    v = H.HostVectorEnv(kind, [3, 5, 8], [11, 12, 13], **({} if kind == "cartpole" else dict(num_steps=4)))
    exp = v.record(lambda e, i, obs: p, 17, max_episode_steps=6)
    ref_keys = {"episode_ids", "steps", "observations", "actions", "action_distributions", "rewards", "next_observations", "terminals"}
    extra = {"truncateds"} | (set() if kind == "cartpole" else {"infos/z", "infos/z_next"})
    assert set(exp) == ref_keys | extra
    assert all(len(x) == 17 for x in exp.values())
    assert np.array_equal(exp["episode_ids"], np.cumsum(exp["steps"] == 0) - 1)
    assert exp["action_distributions"].dtype == np.float32 and exp["action_distributions"].shape == (17, nA)
    # env-major: the first T = 6 rows are environment 0's consecutive steps, and a row's successor in its episode starts where it ended
    ends = exp["terminals"] | exp["truncateds"]
    for i in range(5):
        if not ends[i]:
            assert exp["steps"][i + 1] == exp["steps"][i] + 1
            assert np.array_equal(exp["observations"][i + 1], exp["next_observations"][i])
        else:
            assert exp["steps"][i + 1] == 0
    # a second vector environment on the same seeds gives the same record: the loop is a function of the seeds alone
    exp2 = H.HostVectorEnv(kind, [3, 5, 8], [11, 12, 13], **({} if kind == "cartpole" else dict(num_steps=4))).record(lambda e, i, obs: p, 17, 6)
    assert all(np.array_equal(exp[k], exp2[k]) for k in exp)
    from rl_offline_simulation_amd.data import OfflineDataset, ProbDistribution
    OfflineDataset(None, None, ProbDistribution.Discrete, **exp)


# ---- the C ABI's argument checks (before any HIP call) ----
def _capi():
    from rl_offline_simulation_amd import _lib as L
    lib = L.load()
    bufs = [(C.c_uint64 * 64)() for _ in range(5)]
    p = [C.cast(b, C.c_void_p).value for b in bufs]

    def env(kind, R=2, num_cells=5):
        return L.Env(kind=kind, R=R, num_cells=num_cells, num_steps=15, goal_x=4, goal_y=4, rng_env=p[0], rng_act=p[1], state=p[2], step_count=p[3],
                     ep_t=p[4])

    def mlp(cls, form, widths):
        arr = (L.MLPLayer * (len(widths) - 1))()
        for i, (a, b) in enumerate(zip(widths, widths[1:])):
            arr[i].W, arr[i].b, arr[i].out = p[0], p[1], b
            setattr(arr[i], "in", a)
        c = cls(form=form, n_layers=len(arr), layers_host=C.cast(arr, C.POINTER(L.MLPLayer)), activation=L.ACT_TANH, x_dtype=L.F32, dO=widths[0])
        c._keep = arr
        return c

    out = L.EnvOut(action=p[0], reward=p[1], flags=p[2], ep_step=p[3])
    ppo = L.CollectPPOOut(value=p[0], logp=p[1], final_value=p[2])
    return L, lib, bufs, env, mlp, out, ppo


def _err(lib):
    return lib.offsim_last_error().decode()


def test_capi_null_pointers():
    L, lib, bufs, env, mlp, out, ppo = _capi()
    pol = mlp(L.CollectPolicy, L.COLLECT_MLP, (2, 8, 5))
    val = mlp(L.CollectValue, L.VALUE_MLP, (2, 8, 1))
    e = env(L.ENV_GRID_COORDS)
    assert lib.offsim_env_collect(None, C.byref(pol), 4, 0, C.byref(out), None) == L.EINVAL and "env is NULL" in _err(lib)
    assert lib.offsim_env_collect(C.byref(e), None, 4, 0, C.byref(out), None) == L.EINVAL
    assert lib.offsim_env_collect(C.byref(e), C.byref(pol), 4, 0, None, None) == L.EINVAL
    assert lib.offsim_env_collect(C.byref(e), C.byref(pol), 4, 0, C.byref(L.EnvOut()), None) == L.EINVAL and "out->flags" in _err(lib)
    assert lib.offsim_env_collect(C.byref(e), C.byref(pol), -1, 0, C.byref(out), None) == L.EINVAL
    bad = env(L.ENV_GRID_COORDS)
    bad.state = None
    assert lib.offsim_env_collect(C.byref(bad), C.byref(pol), 4, 0, C.byref(out), None) == L.EINVAL and "env->rng_env" in _err(lib)
    assert lib.offsim_env_collect_reset(C.byref(bad), None, None) == L.EINVAL
    assert lib.offsim_env_collect_reset(None, None, None) == L.EINVAL
    bad = env(7)
    assert lib.offsim_env_collect(C.byref(bad), C.byref(pol), 4, 0, C.byref(out), None) == L.EINVAL and "kind" in _err(lib)
    assert lib.offsim_env_collect_ppo(C.byref(e), C.byref(pol), None, 4, 0, C.byref(out), C.byref(ppo), None) == L.EINVAL
    assert lib.offsim_env_collect_ppo(C.byref(e), C.byref(pol), C.byref(val), 4, 0, C.byref(out), None, None) == L.EINVAL
    assert lib.offsim_env_collect_ppo(C.byref(e), C.byref(pol), C.byref(val), 4, 0, C.byref(out), C.byref(L.CollectPPOOut()), None) == L.EINVAL
    tab = L.CollectPolicy(form=L.COLLECT_TABULAR, x_dtype=L.F64)
    assert lib.offsim_env_collect(C.byref(e), C.byref(tab), 4, 0, C.byref(out), None) == L.EINVAL and "pi is NULL" in _err(lib)
    # a network that does not fit the environment's observation or actions
    assert lib.offsim_env_collect(C.byref(e), C.byref(mlp(L.CollectPolicy, L.COLLECT_MLP, (4, 8, 5))), 4, 0, C.byref(out), None) == L.EINVAL
    assert "input width" in _err(lib)
    assert lib.offsim_env_collect(C.byref(e), C.byref(mlp(L.CollectPolicy, L.COLLECT_MLP, (2, 8, 2))), 4, 0, C.byref(out), None) == L.EINVAL
    # T = 0 and R = 0 launch nothing and need no records
    assert lib.offsim_env_collect(C.byref(e), C.byref(pol), 0, 0, C.byref(L.EnvOut()), None) == L.OK
    assert lib.offsim_env_collect(C.byref(env(L.ENV_CARTPOLE, R=0)), C.byref(mlp(L.CollectPolicy, L.COLLECT_MLP, (4, 8, 2))), 4, 0, C.byref(out), None) == L.OK
    assert lib.offsim_env_collect_ppo(C.byref(e), C.byref(pol), C.byref(val), 0, 0, C.byref(L.EnvOut()), C.byref(L.CollectPPOOut()), None) == L.OK
    assert lib.offsim_env_collect_reset(C.byref(env(L.ENV_GRID, R=0)), None, None) == L.OK


def test_capi_population_shape():
    L, lib, bufs, env, mlp, out, ppo = _capi()
    pol, val = mlp(L.CollectPolicy, L.COLLECT_MLP, (2, 8, 5)), mlp(L.CollectValue, L.VALUE_MLP, (2, 8, 1))
    e = env(L.ENV_GRID_COORDS, R=6)
    call = lambda nl, ne, p=pol: lib.offsim_env_collect_ppo_pop(C.byref(e), C.byref(p), C.byref(val), nl, ne, 4, 0, C.byref(out), C.byref(ppo), None)
    assert call(3, 3) == L.EINVAL and "L * E" in _err(lib)
    assert call(0, 6) == L.EINVAL and call(65536, 1) == L.EINVAL and call(6, 0) == L.EINVAL
    tab = L.CollectPolicy(form=L.COLLECT_TABULAR, x_dtype=L.F64, pi=C.cast(bufs[0], C.c_void_p).value)
    assert call(3, 2, tab) == L.EUNSUPPORTED
    assert lib.offsim_env_collect_ppo_pop(C.byref(e), C.byref(pol), C.byref(val), 3, 2, 0, 0, C.byref(out), C.byref(ppo), None) == L.OK


def test_capi_limits():
    L, lib, bufs, env, mlp, out, ppo = _capi()
    e = env(L.ENV_GRID_COORDS)
    # more than 16 actions
    assert lib.offsim_env_collect(C.byref(e), C.byref(mlp(L.CollectPolicy, L.COLLECT_MLP, (2, 8, 17))), 4, 0, C.byref(out), None) == L.EINVAL
    assert "16 actions" in _err(lib)
    # the workgroup's LDS over 160 KiB: pi of a 70 x 70 grid as f64 (4900 * 5 * 8 bytes)
    tab = L.CollectPolicy(form=L.COLLECT_TABULAR, x_dtype=L.F64, pi=C.cast(bufs[0], C.c_void_p).value)
    assert lib.offsim_env_collect(C.byref(env(L.ENV_GRID, num_cells=70)), C.byref(tab), 4, 0, C.byref(out), None) == L.EUNSUPPORTED
    assert "160 KiB" in _err(lib)
    # the networks' floats over OFFSIM_COLLECT_MLP_MAX_FLOATS
    big = mlp(L.CollectPolicy, L.COLLECT_MLP, (2, 256, 256, 5))
    assert lib.offsim_env_collect(C.byref(e), C.byref(big), 4, 0, C.byref(out), None) == L.EUNSUPPORTED
    # TABULAR on CartPole, and the ROWS form anywhere
    assert lib.offsim_env_collect(C.byref(env(L.ENV_CARTPOLE)), C.byref(tab), 4, 0, C.byref(out), None) == L.EUNSUPPORTED
    assert "grid" in _err(lib)
    rows = L.CollectPolicy(form=L.COLLECT_ROWS)
    assert lib.offsim_env_collect(C.byref(e), C.byref(rows), 4, 0, C.byref(out), None) == L.EUNSUPPORTED
    # a critic of per-row tables has no rows to read
    val = L.CollectValue(form=L.VALUE_ROWS)
    pol = mlp(L.CollectPolicy, L.COLLECT_MLP, (2, 8, 5))
    assert lib.offsim_env_collect_ppo(C.byref(e), C.byref(pol), C.byref(val), 4, 0, C.byref(out), C.byref(ppo), None) == L.EUNSUPPORTED
