"""The tabular drivers on the true grid worlds in one launch (offsim_eval_env / offsim_eval_env_pop, csrc/eval_env.hpp): both launch shapes
against the plain Python loop of tests/env_drivers_host.py over the host mirror -- every output and the action stream left behind, bit for
bit --, the population and the stack against the single forms, continuation across calls, the reference's recorded drivers through
evalMC_env / qlearn_env / expSARSA_env / rollout_env (tests/golden/env_drivers/*.npz), and a PSRS_Exo built from rollout_env's memory."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import env_drivers_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
ALPHA = 0.2
ALPHA_EP = np.array([0.5 / (1.0 + 0.1 * e) for e in range(7)])
EPS_EP = np.array([0.9 / (1.0 + 0.2 * e) for e in range(7)])


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch.device("cuda", 0)


def world(kind="plain", factor=1, num_cells=5, num_steps=15, goal=(4, 4)):
    from rl_offline_simulation_amd.evaluators import GridWorld
    return GridWorld(num_cells, num_steps, goal, kind, factor)


def batched(w, seeds, gpu):
    from rl_offline_simulation_amd.evaluators import BatchedGridWorld
    b = BatchedGridWorld(w, len(seeds), device=gpu)
    b.set_action_seeds(seeds)
    return b


def host(w, seeds, mode, pi, gamma, q0=None, ties=None, **kw):
    """the host loop per seed; ties: None / "episode" / a list of RandomStates"""
    return [H.run(w, np.random.default_rng(s), mode, pi, gamma, q=None if q0 is None else q0[i].copy(),
                  tie=ties[i] if isinstance(ties, list) else ties, **kw) for i, s in enumerate(seeds)]


SCALARS = ("sum_g", "n_ep", "steps", "cand", "n_len", "status")


def assert_rows(o, mine, tag, td=False, beh_arg=False, snap=False, rng=None, rows=None):
    """outputs [R, ...] (or the rows `rows` of them) against the host's per-rollout dicts"""
    pick = (lambda v: v) if rows is None else (lambda v: v[rows])
    for k in SCALARS:
        assert pick(o[k].cpu().numpy()).tolist() == [m[k] for m in mine], (tag, k)
    for k in ("ep_g", "ep_len", "trace_pop") + (("q", "td_err") if td else ()) + (("beh_arg",) if beh_arg else ()) + (("q_snap",) if snap else ()):
        a, b = pick(o[k].cpu().numpy()), np.stack([m[k] for m in mine])
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (tag, k)  # (expected SARSA under a NaN policy row writes NaN into Q)
    if td and "tie_mt" in o:
        assert np.array_equal(pick(o["tie_mt"].cpu().numpy().view(np.uint32)), np.stack([m["tie_mt"] for m in mine])), (tag, "tie_mt")
    if rng is not None:
        assert np.array_equal(pick(rng.cpu().numpy().view(np.uint64)), np.stack([m["rng"] for m in mine])), (tag, "the action stream")


# (num_cells, goal, num_steps, gamma, n_episodes)
GRIDS = [(2, (1, 1), 1, 1.0, 1), (2, (1, 1), 3, 0.9, 7), (3, (2, 1), 3, 1.0, 7), (3, (1, 2), 15, 0.9, 1), (5, (4, 4), 15, 0.9, 7), (5, (1, 1), 15, 1.0, 7)]
KINDS = [("plain", 1), ("noise", 1), ("noise", 2), ("noise", 3), ("counter", 1), ("counter", 4)]
# driver -> (mode, behaviour, epsilon)
DRIVERS = {"evalMC": (H.EVALMC, H.FIXED, 0.0), "qlearn-uniform": (H.QLEARN, H.FIXED, 0.0), "qlearn-eps": (H.QLEARN, H.EPS_GREEDY, 0.3),
           "qlearn-greedy": (H.QLEARN, H.EPS_GREEDY, 0.0), "qlearn-soft": (H.QLEARN, H.SOFT_GREEDY, 0.0), "expSARSA": (H.EXPSARSA, H.FIXED, 0.0)}
SEEDS3 = [3, 10, 17]


def policies(w, drv):
    if drv in ("evalMC", "expSARSA"):
        return {"uniform": H.uniform(w.nS), "shortest": H.shortest_path(w), "gapped": H.gapped(w.nS), "nan": H.nan_second_step(w)}
    if drv == "qlearn-uniform":
        return {"uniform": H.uniform(w.nS), "nan": H.nan_second_step(w)}
    return {"own-Q": None}


@pytest.mark.parametrize("drv", list(DRIVERS))
@pytest.mark.parametrize("kind,factor", KINDS, ids=[f"{k}{f}" for k, f in KINDS])
def test_kinds_and_drivers_against_the_host_loop(kind, factor, drv, gpu):
    from rl_offline_simulation_amd import _lib as L
    mode, beh, eps = DRIVERS[drv]
    saw_goal = saw_key = False
    for nc, goal, ns, gamma, n_ep in GRIDS:
        w = world(kind, factor, nc, ns, goal)
        cap = n_ep * ns + 1
        for pname, pi in policies(w, drv).items():
            tag = (kind, factor, drv, nc, ns, pname)
            b = batched(w, SEEDS3, gpu)
            if mode == H.EVALMC:
                mine = host(w, SEEDS3, mode, pi, gamma, n_episodes=n_ep, trace_cap=cap, ep_cap=n_ep)
                o = b.eval_mc(pi, gamma, n_ep, ep_cap=n_ep, trace_cap=cap)
                assert o["_kernel"] == "k_eval_env_mc"
                assert_rows(o, mine, tag, rng=b.rng)
            else:
                q0 = np.zeros((3, w.nS, 5)) if beh == H.EPS_GREEDY else np.random.default_rng(7).standard_normal((3, w.nS, 5)) * 0.1
                kw = dict(alpha=ALPHA, behaviour=beh, epsilon=eps, n_episodes=n_ep, trace_cap=cap, ep_cap=n_ep)
                mine = host(w, SEEDS3, mode, pi, gamma, q0=q0, ties="episode", **kw)
                o = b.eval_td(pi, gamma, mode, q=q0, tie="episode", **kw)
                assert o["_kernel"] == "k_eval_env"
                assert_rows(o, mine, tag, td=True, beh_arg=beh == H.EPS_GREEDY, rng=b.rng)
            if pname == "nan" and nc > 1 and ns > 1:  # the second step meets a NaN row: the draw is consumed, the environment has not stepped
                assert all(m["status"] == L.ST_KEYERROR and m["steps"] == 1 and m["trace_pop"][1] == 5 for m in mine), tag
                saw_key = True
            else:
                assert all(m["status"] == L.ST_OK and m["n_ep"] == n_ep for m in mine) or pname == "nan", tag
            saw_goal = saw_goal or (pname == "shortest" and all(m["ep_g"][0] > 0 for m in mine))
    if drv in ("evalMC", "expSARSA"):
        assert saw_goal and saw_key


# ---- the evalMC instance: the rollout is the lane ----
@pytest.mark.parametrize("S", [1, 5, 63, 65, 257])
def test_evalmc_lanes_waves_and_workgroups(S, gpu):
    w = world("noise", 2, 5, 15, (2, 1))
    seeds = [11 + 3 * i for i in range(S)]
    pi = H.gapped(w.nS, seed=5) * 0.5 + H.uniform(w.nS) * 0.5
    mine = host(w, seeds, H.EVALMC, pi, 0.9, n_episodes=3, trace_cap=46, ep_cap=3)
    b = batched(w, seeds, gpu)
    o = b.eval_mc(pi, 0.9, 3, ep_cap=3, trace_cap=46)
    assert_rows(o, mine, S, rng=b.rng)
    assert len({m["steps"] for m in mine}) > 1 or S == 1  # lanes of a wave finish at different times


@pytest.mark.parametrize("factor", [2, 22], ids=["lds", "global"])
def test_evalmc_stack_equals_the_single_policies(factor, gpu):
    """L = 3 policies whose episodes differ in length; at factor 22 the stack (3 * 550 * 40 bytes) is read from global memory"""
    w = world("counter", factor, 5, 15, (2, 2))
    S = 65 if factor == 2 else 5
    seeds = [5 + 2 * i for i in range(S)]
    stack = np.stack([H.uniform(w.nS), H.shortest_path(w), H.gapped(w.nS)])
    assert (3 * w.nS * 40 > 65536) == (factor == 22)
    b = batched(w, seeds, gpu)
    rng0 = b.rng.clone()
    o = b.eval_mc_population(stack, 0.9, 4, ep_cap=4, trace_cap=61, state=True)
    assert torch.equal(b.rng, rng0)  # a query
    for l in range(3):
        b1 = batched(w, seeds, gpu)
        o1 = b1.eval_mc(stack[l], 0.9, 4, ep_cap=4, trace_cap=61)
        for k in SCALARS + ("ep_g", "ep_len", "trace_pop"):
            assert torch.equal(o[k][l], o1[k]), (factor, l, k)
        assert torch.equal(o["_state"]["rng"][l], b1.rng)
        mine = host(w, seeds[:3], H.EVALMC, stack[l], 0.9, n_episodes=4, trace_cap=61, ep_cap=4)
        assert_rows({k: v[l] for k, v in o.items() if isinstance(v, torch.Tensor)}, mine, (factor, l), rows=slice(0, 3))
    steps = o["steps"].cpu().numpy()
    assert (steps[1] == 16).all() and (steps[0] > 16).any()  # the shortest path ends its episodes early: 4 steps each


def test_evalmc_rollouts_env_and_its_stack(gpu):
    from rl_offline_simulation_amd.evaluators import evalmc_rollouts_env
    w = world("noise", 3)
    seeds, stack = list(range(6)), None
    stack = np.stack([H.uniform(w.nS), H.shortest_path(w)])
    one = evalmc_rollouts_env(w, seeds, stack[0], 0.9, 5, episode0=2)
    mine = host(w, seeds, H.EVALMC, stack[0], 0.9, n_episodes=5, episode0=2)
    assert one["sum_g"].tolist() == [m["sum_g"] for m in mine] and one["n_ep"].tolist() == [5] * 6
    assert np.array_equal(one["value"], one["sum_g"] / 5)
    both = evalmc_rollouts_env(w, seeds, stack, 0.9, 5, episode0=2)
    assert both["sum_g"].shape == (2, 6) and np.array_equal(both["sum_g"][0], one["sum_g"]) and both["best"] == 1
    assert np.array_equal(both["mean_value"], both["value"].mean(axis=1))


# ---- the learner instance: one wavefront per rollout ----
@pytest.mark.parametrize("S", [1, 3, 5])
@pytest.mark.parametrize("tie", ["first", "episode", "states"])
def test_learner_ties_schedules_and_snapshots(S, tie, gpu):
    w = world("counter", 4, 3, 15, (2, 2))
    seeds = [2 + 5 * i for i in range(S)]
    stride = 1 if S != 3 else 3
    kw = dict(alpha=0.0, behaviour=H.EPS_GREEDY, epsilon=0.0, alpha_ep=ALPHA_EP, epsilon_ep=EPS_EP, n_episodes=7, trace_cap=106, ep_cap=7, snap_cap=40,
              snap_stride=stride)
    q0 = np.zeros((S, w.nS, 5))
    ties_h = {"first": None, "episode": "episode", "states": [np.random.RandomState(500 + i) for i in range(S)]}[tie]
    ties_d = {"first": None, "episode": "episode", "states": np.stack([H.mt_words(np.random.RandomState(500 + i)) for i in range(S)])}[tie]
    mine = host(w, seeds, H.QLEARN, None, 0.9, q0=q0, ties=ties_h, **kw)
    b = batched(w, seeds, gpu)
    o = b.eval_td(None, 0.9, H.QLEARN, q=q0, tie=ties_d, **kw)
    assert ("tie_mt" in o) == (tie != "first")
    assert_rows(o, mine, (S, tie), td=True, beh_arg=True, snap=True, rng=b.rng)  # (tie_mt: the state afterwards)


@pytest.mark.parametrize("waves", [2, 1])
def test_learner_launch_shapes(waves, gpu):
    """an nS that leaves room for 2 rollouts and for 1 rollout per workgroup (the 64 KiB rule of include/offsim.h)"""
    factor = H.factor_for_waves(waves)
    w = world("noise", factor, 5, 15, (1, 1))
    seeds = [4, 9, 14, 19, 24]
    kw = dict(alpha=ALPHA, behaviour=H.EPS_GREEDY, epsilon=0.4, n_episodes=3, trace_cap=46, ep_cap=3)
    q0 = np.zeros((5, w.nS, 5))
    mine = host(w, seeds, H.QLEARN, None, 0.9, q0=q0, ties="episode", **kw)
    b = batched(w, seeds, gpu)
    o = b.eval_td(None, 0.9, H.QLEARN, q=q0, tie="episode", **kw)
    assert_rows(o, mine, waves, td=True, beh_arg=True, rng=b.rng)


@pytest.mark.parametrize("short", [0, 1])
def test_traces_at_their_capacity_and_one_short(short, gpu):
    w = world("plain", 1, 3, 4, (2, 2))
    seeds = [1, 2, 3]
    pi = H.uniform(w.nS)
    full = host(w, seeds, H.EXPSARSA, pi, 0.9, q0=np.zeros((3, w.nS, 5)), alpha=ALPHA, n_episodes=2, trace_cap=9, ep_cap=2)
    n = min(m["steps"] for m in full)
    cap = n - short
    kw = dict(alpha=ALPHA, n_episodes=2, trace_cap=cap, ep_cap=2 - short, snap_cap=cap)
    mine = host(w, seeds, H.EXPSARSA, pi, 0.9, q0=np.zeros((3, w.nS, 5)), **kw)
    b = batched(w, seeds, gpu)
    o = b.eval_td(pi, 0.9, H.EXPSARSA, **kw)
    assert_rows(o, mine, short, td=True, snap=True, rng=b.rng)
    assert all(m["steps"] >= cap for m in mine) and (short == 0 or all(m["steps"] > cap for m in mine))


# ---- continuation ----
@pytest.mark.parametrize("drv", ["evalMC", "qlearn-eps", "expSARSA"])
def test_two_calls_equal_one(drv, gpu):
    mode, beh, eps = DRIVERS[drv]
    w = world("noise", 2, 5, 15, (3, 1))
    seeds = [6, 7, 8]
    pi = None if beh != H.FIXED else H.gapped(w.nS) * 0.5 + 0.1
    if mode == H.EVALMC:
        mine = host(w, seeds, mode, pi, 0.9, n_episodes=7, ep_cap=7)
    else:
        mine = host(w, seeds, mode, pi, 0.9, q0=np.zeros((3, w.nS, 5)), ties="episode", alpha=ALPHA, behaviour=beh, epsilon=eps, alpha_ep=ALPHA_EP,
                    n_episodes=7, ep_cap=7)
    b = batched(w, seeds, gpu)
    q, parts, done = None, [], 0
    for n in (3, 4):
        if mode == H.EVALMC:
            o = b.eval_mc(pi, 0.9, n, ep_cap=n, episode0=done)
        else:
            o = b.eval_td(pi, 0.9, mode, ALPHA, q=q, behaviour=beh, epsilon=eps, alpha_ep=ALPHA_EP[done:], n_episodes=n, ep_cap=n, tie="episode", episode0=done)
            q = o["q"]
        parts.append(o)
        done += n
    assert np.array_equal(torch.cat([p["ep_g"] for p in parts], dim=1).cpu().numpy(), np.stack([m["ep_g"] for m in mine]))
    assert np.array_equal(b.rng.cpu().numpy().view(np.uint64), np.stack([m["rng"] for m in mine]))
    if mode != H.EVALMC:
        assert np.array_equal(q.cpu().numpy(), np.stack([m["q"] for m in mine]))
        assert np.array_equal(parts[-1]["tie_mt"].cpu().numpy().view(np.uint32), np.stack([m["tie_mt"] for m in mine]))


# ---- the reference's policies, as tabular.py writes them ----
def _random_argmax(x):
    return np.random.choice(np.where(x == np.max(x))[0])


def uniformly_random_policy(Q, args):
    return np.ones_like(Q) / Q.shape[1]


def greedy_policy(Q, args):
    pi = np.zeros_like(Q)
    for s in range(len(Q)):
        pi[s, _random_argmax(Q[s])] = 1
    return pi


def soft_greedy_policy(Q, args):
    pi = np.zeros_like(Q)
    for s in range(len(Q)):
        pi[s, np.where(np.isclose(Q[s], np.max(Q[s])))[0]] = 1
    return pi / pi.sum(axis=1, keepdims=True)


def epsilon_greedy_policy(Q, args):
    epsilon = args["epsilon"]
    pi = np.ones_like(Q) * epsilon / (Q.shape[1])
    for s in range(len(Q)):
        pi[s, _random_argmax(Q[s])] = 1 - epsilon + epsilon / (Q.shape[1])
    return pi


BEHAVIOURS = {"qlearn_uniform": uniformly_random_policy, "qlearn_eps": epsilon_greedy_policy, "qlearn_eps_sched": epsilon_greedy_policy,
              "qlearn_greedy": greedy_policy, "qlearn_soft": soft_greedy_policy}


# ---- the population ----
@pytest.mark.parametrize("n_l,S", [(1, 1), (1, 5), (3, 1), (3, 5)])
def test_run_env_rows_equal_the_single_drivers(n_l, S, gpu):
    from rl_offline_simulation_amd.evaluators import TDPopulation, qlearn_env, expSARSA_env
    w = world("noise", 2, 5, 15, (2, 2))
    seeds = [21 + i for i in range(S)]
    beh = ["eps_greedy", "fixed", "soft_greedy"][:n_l]
    gammas, alphas = [0.9, 1.0, 0.8][:n_l], [0.2, (lambda e: 0.5 / (1 + e)), 0.1][:n_l]
    res = TDPopulation("qlearn", alphas, gammas, epsilon=[0.3, 1.0, 1.0][:n_l], behaviour=beh).run_env(w, seeds, 6, trace_cap=91)
    fn = {"eps_greedy": epsilon_greedy_policy, "fixed": uniformly_random_policy, "soft_greedy": soft_greedy_policy}
    assert tuple(res.Q.shape) == (n_l, S, w.nS, 5) and (res.status == 0).all() and (res.n_ep == 6).all()
    for l in range(n_l):
        for j, s in enumerate(seeds):
            Q, info = qlearn_env(w, 6, fn[beh[l]], gammas[l], alpha=alphas[l], epsilon=0.3, seed=s)
            assert np.array_equal(res.Q[l, j].cpu().numpy(), Q) and np.array_equal(res.Gs[l, j].cpu().numpy(), info["Gs"]), (l, j)
            assert np.array_equal(res.td_err[l, j, :len(info["TD_errors"])].cpu().numpy(), info["TD_errors"]), (l, j)
    Gs = res.Gs.cpu().numpy()
    mean = np.array([[sum(Gs[l, :, e].tolist()) / S for e in range(6)] for l in range(n_l)])
    assert np.array_equal(res.curve_mean.cpu().numpy(), mean) and (res.curve_n == S).all()
    var = np.array([[sum([(Gs[l, j, e] - mean[l, e]) * (Gs[l, j, e] - mean[l, e]) for j in range(S)]) / S for e in range(6)] for l in range(n_l)])
    assert np.array_equal(res.curve_var.cpu().numpy(), var)
    assert res.best(last=2) == int(np.argmax(mean[:, -2:].mean(axis=1)))
    pis = np.stack([H.uniform(w.nS), H.gapped(w.nS) * 0.5 + 0.1, H.shortest_path(w) * 0.5 + 0.1][:n_l])
    res = TDPopulation("expsarsa", 0.1, gammas, pi=pis).run_env(w, seeds, 4, tie="first")
    for l in range(n_l):
        for j, s in enumerate(seeds):
            Q, info = expSARSA_env(w, 4, pis[l], gammas[l], alpha=0.1, seed=s, tie="first")
            assert np.array_equal(res.Q[l, j].cpu().numpy(), Q) and np.array_equal(res.Gs[l, j].cpu().numpy(), info["Gs"]), (l, j)


# ---- the reference's recorded drivers through the drop-ins ----
@pytest.mark.parametrize("name", list(H.WORLDS))
def test_drivers_reproduce_the_reference(name, gpu):
    from rl_offline_simulation_amd.evaluators import evalMC_env, qlearn_env, expSARSA_env, rollout_env
    f = H.Fixture(name)
    d, n, gam, al = f.d, int(f.d["n_episodes"]), float(f.d["gamma"]), float(f.d["alpha"])
    for i in range(len(f.runs)):
        drv, goal, num_steps, seed = f.settings(i)
        w = world(f.kind, f.factor, 5, num_steps, goal)
        np.random.seed(12345)
        if drv == "evalMC":
            Gs, lengths = evalMC_env(w, n, d["pi"], gam, seed=seed)
            assert np.array_equal(Gs, d["Gs"][i]) and np.array_equal(lengths, d["lengths"][i]), f.runs[i]
            info = None
        elif drv == "rollout":
            info = rollout_env(w, n, d["pi"], gam, seed=seed)
        elif drv == "expSARSA":
            Q, info = expSARSA_env(w, n, d["pi"], gam, alpha=al, save_Q=1, seed=seed)
            assert np.abs(Q - d["Q"][i]).max() <= 1e-12 and np.abs(info["TD_errors"] - f.td(i)).max() <= 1e-12, f.runs[i]
            assert np.abs(info["Qs"] - f.Qs(i)).max() <= 1e-12, f.runs[i]
        else:
            Q, info = qlearn_env(w, n, BEHAVIOURS[drv], gam, alpha=al, epsilon=H.EPS_SCHED if drv == "qlearn_eps_sched" else 0.3, save_Q=1, seed=seed)
            assert np.array_equal(Q, d["Q"][i]) and np.array_equal(info["TD_errors"], f.td(i)) and np.array_equal(info["Qs"], f.Qs(i)), f.runs[i]
        assert np.array_equal(H.mt_words(np.random.mtrand._rand), f.mt(i)), f.runs[i]  # the global stream, as the reference leaves it
        if info is not None:
            assert np.array_equal(info["Gs"], d["Gs"][i]), f.runs[i]
            got, want = H.memory_arrays(info["memory"]), f.memory(i)
            assert all(np.array_equal(got[k], want[k]) for k in want), f.runs[i]
            assert w.s == int(want["S_"][-1])


# ---- end to end: the true world's memory builds the simulator it is compared with ----
def test_rollout_memory_builds_a_psrs_exo(gpu):
    from rl_offline_simulation_amd.evaluators import PSRS_Exo, evalMC_psrs, evalMC_env, rollout_env
    """Seeds and gamma are fixed so that the host loops alone satisfy the bound (tests/exo_host.py on the host loop's memory: 0.34 standard
    errors apart at gamma = 1).  gamma = 1 because the time limit is not part of the simulator's state: its episodes end where the popped
    row says, so their lengths are spread around the true world's 15 and a discounted return is biased (4.8 standard errors at
    gamma = 0.9 with these seeds) -- the kind of finding this ground truth exists for, not what this test is about."""
    w = world("noise", 2)
    pi = H.uniform(w.nS)
    mem = rollout_env(w, 120, pi, 1.0, seed=1)["memory"]
    sim = PSRS_Exo(mem, nO=w.nS, nA=5, o_split_func=lambda o: (o % 25, o // 25), o_combine_func=lambda s, x: s + 25 * x)
    sim.reset_sampler(3)
    Gs_sim, _ = evalMC_psrs(sim, 10 ** 6, pi, 1.0)
    Gs_true, _ = evalMC_env(w, 400, pi, 1.0, seed=2)
    assert len(Gs_sim) >= 30 and len(Gs_true) == 400
    se = np.sqrt(Gs_sim.var(ddof=1) / len(Gs_sim) + Gs_true.var(ddof=1) / len(Gs_true))
    print("PSRS_Exo", Gs_sim.mean(), len(Gs_sim), "true", Gs_true.mean(), "se", se)
    assert abs(Gs_sim.mean() - Gs_true.mean()) <= 4 * se
