"""evalmc_rollouts_true_env / PPOPopulation.evaluate_env (offsim_eval_env_obs, csrc/eval_env_obs.hpp) on the device.

Held bit for bit to the collect kernel of the same environments (VectorX.collect cut into episodes by tests/true_env_population_host.py)
and, on the grids, to the plain Python loop of tests/true_env_host.py in closed loop with MLPPolicy.forward; CartPole's dynamics
independently of collect through the traced states, within the suite's tolerance for that step (4 eps: 8 times the deviation
tools/true_env_error_table.py measured, profiles/true_env_error.jsonl).  Then the population against single calls, pairing, tiles, the
undrawable row, the query property and the empty calls.

Shapes: L = 3 policies (grid.y > 1), S = 9 seeds (a second workgroup with one live wavefront), 3 episodes."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import true_env_host as H  # noqa: E402
import true_env_population_host as P  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NL, S, NEP = 3, 9, 3
SEEDS, ACTION_SEEDS = 40 + np.arange(S), 900 + 7 * np.arange(S)
GRID = dict(num_cells=3, num_steps=6, goal=(2, 2))
HOST_KIND = {"cartpole": "cartpole", "grid": "grid", "grid_coords": "coords"}
WIDTH = {"cartpole": (4, 2), "grid": (1, 5), "grid_coords": (2, 5)}
# (environment, hidden widths, activation, gamma, max_episode_steps): every network shape -- 8-8 tanh, 5 ReLU (widths off the lane
# multiples), 64-64 tanh -- and both gammas on every environment; CartPole with a cap that truncates every episode and with CartPole-v1's
CASES = [("cartpole", (8, 8), "tanh", 0.9, 8), ("cartpole", (5,), "relu", 1.0, 8), ("cartpole", (64, 64), "tanh", 0.9, 500),
         ("cartpole", (8, 8), "tanh", 1.0, 500), ("grid", (8, 8), "tanh", 0.9, None), ("grid", (5,), "relu", 1.0, None),
         ("grid", (64, 64), "tanh", 0.9, 4), ("grid_coords", (8, 8), "tanh", 0.9, None), ("grid_coords", (5,), "relu", 1.0, None),
         ("grid_coords", (64, 64), "tanh", 1.0, None)]
IDS = [f"{k}-{'x'.join(map(str, h))}-{a}-g{g}-cap{c}" for k, h, a, g, c in CASES]


@pytest.fixture(scope="module")
def gpu():
    from rl_offline_simulation_amd import _lib
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    _lib.load()
    return torch.device("cuda", 0)


def _nets(kind, hidden, activation, n=NL, seed=11):
    """n MLPPolicy's of one architecture with weights large enough that the policies differ from uniform and from each other"""
    from rl_offline_simulation_amd.evaluators import MLPPolicy
    g = np.random.default_rng(seed)
    dO, nA = WIDTH[kind]
    widths = (dO,) + tuple(hidden) + (nA,)
    nets = []
    for _ in range(n):
        ws = [((g.standard_normal((b, a)) * 2.0 / np.sqrt(a)).astype(np.float32), (0.3 * g.standard_normal(b)).astype(np.float32))
              for a, b in zip(widths, widths[1:])]
        if kind == "grid":  # a cell id is a large input: keep the logits apart but finite
            ws[0] = (ws[0][0] * 0.2, ws[0][1])
        nets.append(MLPPolicy(ws, activation))
    return nets


def _kw(kind):
    return {} if kind == "cartpole" else dict(GRID)


def _vector_env(kind, gpu, n=S):
    from rl_offline_simulation_amd.evaluators import VectorCartPole, VectorGridNavi
    if kind == "cartpole":
        return VectorCartPole(n, device=gpu)
    return VectorGridNavi(n, coords=kind == "grid_coords", device=gpu, **GRID)


def _bound(kind, cap):
    return cap if kind == "cartpole" else (min(cap, GRID["num_steps"]) if cap else GRID["num_steps"])


def _run(kind, nets, gamma, cap, **kw):
    from rl_offline_simulation_amd.evaluators import evalmc_rollouts_true_env
    return evalmc_rollouts_true_env(kind, SEEDS, nets, gamma, NEP, max_episode_steps=cap, action_seeds=ACTION_SEEDS, **kw, **_kw(kind))


_RESULTS = {}


def _result(case):
    """the population call of a case with a full trace, computed once and shared (read only)"""
    if case not in _RESULTS:
        kind, hidden, act, gamma, cap = case
        nets = _nets(kind, hidden, act)
        _RESULTS[case] = (nets, _run(kind, nets, gamma, cap, trace_cap=NEP * _bound(kind, cap)))
    return _RESULTS[case]


def _same(a, b, keys=None):
    for k in keys or a:
        if isinstance(a[k], np.ndarray):
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
        else:
            assert a[k] == b[k], k


def _check_against_records(res, l, j, flags, reward, action, gamma, who):
    """row (l, j) of a result against one environment's [T] collect records"""
    Gs, lengths, ended = P.episodes_from_records(flags, reward, action, gamma)
    assert len(Gs) >= NEP, who
    Gs, lengths, ended = Gs[:NEP], lengths[:NEP], ended[:NEP]
    n = int(lengths.sum())
    assert np.array_equal(res["lengths"][l, j], lengths) and np.array_equal(res["ended"][l, j], ended), who
    assert np.array_equal(res["trace_action"][l, j, :n], action[:n]) and (res["trace_action"][l, j, n:] == -1).all(), who
    assert np.array_equal(res["Gs"][l, j].view(np.uint64), Gs.view(np.uint64)), (who, res["Gs"][l, j], Gs)
    assert res["value"][l, j] == P.sequential_mean(Gs) and res["sum_g"][l, j] == sum_in_order(Gs), who
    assert res["n_ep"][l, j] == NEP and res["steps"][l, j] == n == res["cand"][l, j] and res["status"][l, j] == 0, who


def sum_in_order(Gs):
    s = 0.0
    for g in Gs.tolist():
        s = s + g
    return s


# ---- 1. against the collect kernel, bit for bit ----
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_equals_collect_records(gpu, case):
    kind, hidden, act, gamma, cap = case
    nets, res = _result(case)
    T = NEP * _bound(kind, cap)
    assert res["Gs"].shape == (NL, S, NEP) and res["value"].shape == (NL, S) and res["mean_value"].shape == (NL,)
    for l, net in enumerate(nets):
        env = _vector_env(kind, gpu)
        env.seed(SEEDS)
        env.set_action_seeds(ACTION_SEEDS)
        env.reset()
        col = env.collect(net, T, cap, record_obs=False, record_probs=False)
        flags, reward, action = env.records.flags.cpu().numpy(), col.reward.cpu().numpy(), env.drawn_action.cpu().numpy()
        for j in range(S):
            _check_against_records(res, l, j, flags[:, j], reward[:, j], action[:, j], gamma, (l, j))
    if cap == 8:  # hardly a pole falls within eight steps: episodes are truncated
        assert (res["ended"] & P.TRUNCATED).any() and (res["lengths"] <= 8).all()
    if kind == "cartpole" and cap == 500:
        assert (res["ended"] & P.TERMINATED).any()
    with np.errstate(invalid="ignore"):
        assert np.array_equal(res["mean_value"], np.nanmean(res["value"], axis=1)) and res["best"] == int(np.argmax(res["mean_value"]))


# ---- 2. the grids against the plain Python loop, in closed loop with MLPPolicy.forward ----
@pytest.mark.parametrize("case", [c for c in CASES if c[0] != "cartpole"], ids=[i for c, i in zip(CASES, IDS) if c[0] != "cartpole"])
def test_grids_equal_host_loop(gpu, case):
    from rl_offline_simulation_amd.evaluators.obs_policy import obs_tensor
    kind, hidden, act, gamma, cap = case
    nets, res = _result(case)
    T = NEP * _bound(kind, cap)
    dO = WIDTH[kind][0]
    for l, net in enumerate(nets):
        host = H.HostVectorEnv(HOST_KIND[kind], SEEDS, ACTION_SEEDS, **GRID)
        host.reset()  # seed()'s reset is the constructor's; this is the first episode's

        def policy(e, i, obs):
            return net.forward(obs_tensor(np.asarray(obs).reshape(1, dO), gpu)).cpu().numpy()[0]

        if kind == "grid":  # the observation is one of nine cell ids: one forward for all of them
            table = net.forward(obs_tensor(np.arange(GRID["num_cells"] ** 2).reshape(-1, 1), gpu)).cpu().numpy()
            policy = lambda e, i, obs: table[int(obs)]  # noqa: E731
        want = host.collect(policy, T, cap)
        for j in range(S):
            _check_against_records(res, l, j, want["flags"][:, j], want["reward"][:, j], want["action"][:, j], gamma, (l, j))


# ---- 3. CartPole's dynamics, independently of collect ----
def _tolerance():
    rows = [json.loads(x) for x in open(os.path.join(ROOT, "profiles", "true_env_error.jsonl")) if x.strip()]
    worst = max(r["max_dev_eps"] for r in rows if r["what"] == "cartpole next_state")
    return min(8.0 * worst * H.EPS, 1e-12)


@pytest.mark.parametrize("cap", [8, 500])
def test_cartpole_dynamics_from_the_trace(gpu, cap):
    nets = _nets("cartpole", (8, 8), "tanh")
    res = _run("cartpole", nets, 0.9, cap, trace_cap=64)
    st, nst, act = res["trace_state"], res["trace_next_state"], res["trace_action"]
    assert st.shape == (NL, S, 64, 4) and act.shape == (NL, S, 64)
    worst = 0.0
    for l in range(NL):
        for j in range(S):
            n = min(64, int(res["steps"][l, j]))
            assert n > 0 and (act[l, j, :n] >= 0).all() and (act[l, j, n:] == -1).all() and np.isnan(st[l, j, n:]).all()
            worst = max(worst, H.cartpole_deviation(st[l, j, :n, None], act[l, j, :n, None], nst[l, j, :n, None]))
            # the episodes of the trace: the first state of each in [-0.05, 0.05)^4, the end where the traced next state or the cap says
            i = 0
            for e in range(NEP):
                ln = int(res["lengths"][l, j, e])
                if i >= n:
                    break
                assert (st[l, j, i] >= -0.05).all() and (st[l, j, i] < 0.05).all(), (l, j, e)
                for t in range(min(ln, n - i)):
                    done, trunc = H.cartpole_done(nst[l, j, i + t]), t + 1 >= cap
                    assert (done or trunc) == (t == ln - 1), (l, j, e, t)
                    if t == ln - 1:
                        assert res["ended"][l, j, e] == (P.TERMINATED if done else 0) | (P.TRUNCATED if trunc else 0)
                    elif t + 1 < min(ln, n - i):
                        assert np.array_equal(st[l, j, i + t + 1], nst[l, j, i + t])
                i += ln
            # reward 1 per step: the return is the discount table's partial sum
            for e in range(NEP):
                assert res["Gs"][l, j, e] == sum_in_order(np.array([0.9 ** t * 1.0 for t in range(int(res["lengths"][l, j, e]))]))
    tol = _tolerance()
    print(f"cartpole trace, cap {cap}: max deviation {worst:.3f} eps, allowed {tol / H.EPS:.3f} eps")
    assert worst * H.EPS <= tol


# ---- 4. the population equals single calls; from_ppo equals from_policies; evaluate_env equals the function ----
@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[5], CASES[9]], ids=[IDS[0], IDS[2], IDS[5], IDS[9]])
def test_population_equals_singles(gpu, case):
    kind, hidden, act, gamma, cap = case
    nets, res = _result(case)
    tc = NEP * _bound(kind, cap)
    for l, net in enumerate(nets):
        one = _run(kind, net, gamma, cap, trace_cap=tc)
        assert one["value"].shape == (1, S) and one["best"] == 0
        for k in one:
            if isinstance(one[k], np.ndarray) and k != "mean_value":
                assert np.array_equal(one[k][0].view(np.uint8), res[k][l].view(np.uint8)), (k, l)
        assert one["mean_value"][0] == res["mean_value"][l]


def test_from_ppo_and_evaluate_env(gpu):
    from rl_offline_simulation_amd.evaluators import MLPValue, PolicyPopulation, PPOPopulation
    kind, hidden, act, gamma, cap = CASES[0]
    nets = _nets(kind, hidden, act)
    g = np.random.default_rng(2)
    critics = [MLPValue([(g.standard_normal((8, 4)).astype(np.float32), np.zeros(8, np.float32)),
                         (g.standard_normal((1, 8)).astype(np.float32), np.zeros(1, np.float32))]) for _ in range(NL)]
    pop = PPOPopulation(nets, critics)
    a = _run(kind, PolicyPopulation.from_ppo(pop), gamma, cap)
    b = _run(kind, PolicyPopulation.from_policies([pop.actor(l) for l in range(NL)]), gamma, cap)
    c = pop.evaluate_env(kind, SEEDS, gamma, NEP, max_episode_steps=cap, action_seeds=ACTION_SEEDS)
    _same(a, b)
    _same(a, c)
    _same(a, _result(CASES[0])[1], keys=a.keys())
    # a VectorCartPole in the place of the name: the same call
    _same(a, pop.evaluate_env(_vector_env(kind, gpu, 2), SEEDS, gamma, NEP, max_episode_steps=cap, action_seeds=ACTION_SEEDS))


# ---- 5. pairing ----
@pytest.mark.parametrize("kind", ["cartpole", "grid_coords"])
def test_pairing(gpu, kind):
    nets = _nets(kind, (8, 8), "tanh")
    cap = 8 if kind == "cartpole" else None
    res = _run(kind, [nets[0], nets[1], nets[0]], 0.9, cap, trace_cap=8)
    for k in ("Gs", "lengths", "ended", "value", "steps", "trace_action", "trace_state", "trace_next_state"):
        assert np.array_equal(res[k][0].view(np.uint8), res[k][2].view(np.uint8)), k
    assert not np.array_equal(res["trace_action"][0], res["trace_action"][1])  # (different policies do act differently)
    # every policy of a seed starts its first episode in the same state: the same reset draws
    first = res["trace_state"][:, :, 0]
    assert np.array_equal(first[0], first[1]) and not np.isnan(first).any()
    assert len({first[0, j].tobytes() for j in range(S)}) == S  # (and the seeds differ)
    # the default action streams are the seeds' own
    from rl_offline_simulation_amd.evaluators import evalmc_rollouts_true_env
    d = evalmc_rollouts_true_env(kind, SEEDS, nets, 0.9, NEP, max_episode_steps=cap, **_kw(kind))
    e = evalmc_rollouts_true_env(kind, SEEDS, nets, 0.9, NEP, max_episode_steps=cap, action_seeds=SEEDS, **_kw(kind))
    _same(d, e)


# ---- 6. tiles change no bit ----
@pytest.mark.parametrize("case", [CASES[1], CASES[7]], ids=[IDS[1], IDS[7]])
def test_tiles(gpu, case):
    kind, hidden, act, gamma, cap = case
    nets, res = _result(case)
    tc = NEP * _bound(kind, cap)
    _same(res, _run(kind, nets, gamma, cap, trace_cap=tc, tile=4))
    _same(res, _run(kind, nets, gamma, cap, trace_cap=tc, policy_tile=2))
    _same(res, _run(kind, nets, gamma, cap, trace_cap=tc, tile=4, policy_tile=2))


# ---- 7. a row from which no action can be drawn ----
def test_undrawable_row(gpu):
    from rl_offline_simulation_amd import _lib as L
    from rl_offline_simulation_amd.evaluators import MLPPolicy, PolicyPopulation
    from rl_offline_simulation_amd.evaluators import true_env_population as TP
    from rl_offline_simulation_amd.evaluators.rollout_io import _gamma_pow
    kind, hidden, act, gamma, cap = CASES[0]
    nets, res = _result(CASES[0])
    ws = [(W.clone(), b.clone()) for W, b in nets[1].weights]
    ws[1][0][3, 2] = float("nan")
    bad = [nets[0], MLPPolicy(ws, act), nets[2]]
    with pytest.raises(ValueError, match="policy 1"):
        _run(kind, bad, gamma, cap)
    # the C entry: policy 1's rollouts stop at their first step, the others are what they are without it
    env = _vector_env(kind, gpu)
    env.seed(SEEDS)
    env.set_action_seeds(ACTION_SEEDS)
    st = PolicyPopulation.from_policies(bad)._stack
    wd, arr = st._device_weights(gpu)
    o = TP._launch(TP._c_env(L.ENV_CARTPOLE, {}, S, env.rng_env, env.rng_act), st, arr, len(wd), NL, S, NEP, cap, _gamma_pow(gamma, cap, gpu, cap=cap), 4, gpu)
    o = {k: v.cpu().numpy() for k, v in o.items()}
    assert (o["status"][1] == L.ST_KEYERROR).all() and (o["n_ep"][1] == 0).all() and (o["steps"][1] == 0).all() and np.isnan(o["value"][1]).all()
    assert (o["Gs"][1] == 0).all() and (o["lengths"][1] == 0).all() and (o["ended"][1] == 0).all()
    assert (o["trace_action"][1, :, 0] == 2).all() and (o["trace_action"][1, :, 1:] == -1).all() and np.isnan(o["trace_state"][1]).all()
    for l in (0, 2):
        assert (o["status"][l] == L.ST_OK).all()
        for k in ("Gs", "lengths", "ended", "n_ep", "steps", "value"):
            assert np.array_equal(o[k][l].view(np.uint8), res[k][l].view(np.uint8)), (k, l)


# ---- 8. a query: the environment passed in is left as it was ----
def test_environment_untouched(gpu):
    from rl_offline_simulation_amd.evaluators import evalmc_rollouts_true_env
    nets = _nets("cartpole", (8, 8), "tanh")
    env = _vector_env("cartpole", gpu, 5)
    env.seed([3, 4, 5, 6, 7])
    env.collect(nets[0], 6, 4)  # an open episode, both streams advanced
    keep = {k: getattr(env, k).clone() for k in ("state", "rng_env", "rng_act", "step_count", "_ep_t")}
    res = evalmc_rollouts_true_env(env, SEEDS, nets, 0.9, NEP, max_episode_steps=8, action_seeds=ACTION_SEEDS)
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(getattr(env, k), v), k
    _same(res, _run("cartpole", nets, 0.9, 8))
    # a grid's parameters are taken from the environment
    g = _vector_env("grid_coords", gpu, 2)
    gn = _nets("grid_coords", (8, 8), "tanh")
    _same(evalmc_rollouts_true_env(g, SEEDS, gn, 0.9, NEP, action_seeds=ACTION_SEEDS), _run("grid_coords", gn, 0.9, None))
    with pytest.raises(TypeError):
        evalmc_rollouts_true_env(g, SEEDS, gn, 0.9, NEP, num_cells=3)


# ---- 9. nothing to run ----
def test_empty_calls(gpu):
    from rl_offline_simulation_amd.evaluators import evalmc_rollouts_true_env
    nets = _nets("cartpole", (8, 8), "tanh")
    r = evalmc_rollouts_true_env("cartpole", [], nets, 0.9, NEP)
    assert r["value"].shape == (NL, 0) and r["Gs"].shape == (NL, 0, NEP) and r["mean_value"].shape == (NL,) and r["best"] == -1
    r = evalmc_rollouts_true_env("cartpole", SEEDS, nets, 0.9, 0)
    assert r["Gs"].shape == (NL, S, 0) and (r["n_ep"] == 0).all() and (r["steps"] == 0).all() and np.isnan(r["value"]).all() and r["best"] == -1
