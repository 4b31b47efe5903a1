"""The tabular drivers on latent states in one launch (offsim_eval_env_latent / offsim_eval_env_latent_pop, csrc/eval_env_latent.hpp).

  grid_coords + MLP   against the plain Python loop of tests/latent_env_host.py, every output, the tie stream and both streams' end
                      positions bit for bit (expected SARSA to 1e-12); the reference's recorded drivers through the drop-ins
  CartPole + BOX      checked from the trace: the rollout is closed-loop and the device's sin / cos may differ from the host's by an ulp,
                      so the rollout may leave a host rollout -- z is the host box of the traced state, next_state is within DESIGN section
                      28's rule (8 times the largest measured line of profiles/true_env_error.jsonl) of the host's f64 step from the traced state, the resets are default_rng(e)'s bits, and Q, td_err, Gs and
                      the tie stream are the host learner replayed on the traced (z, A, r, z', done)
  CartPole + MLP      the traced z is the f64 arg max wherever tests/encoder_host.py's rule calls the row clear
  population          entry [l, j] equals the single call; tiles change no bit; the call is a query
  shapes / statuses   the 4 / 2 / 1 carve, a carve above 64 KiB, the MLP's weights behind a learner's Q at 2 and 1 rollouts per workgroup,
                      an undrawable row, the empty calls
Shapes: L = 3, S = 5 (4 rollouts per workgroup + 1: a partial workgroup and a workgroup boundary), 3 to 4 episodes."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import latent_env_host as H  # noqa: E402
from true_env_host import EPS, cartpole_deviation  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [3, 10, 17, 24, 31]
GAMMA, ALPHA, N_EP = 0.9, 0.2, 4
ALPHA_EP = np.array([0.5 / (1.0 + 0.1 * e) for e in range(N_EP)])
EPS_EP = np.array([0.9 / (1.0 + 0.2 * e) for e in range(N_EP)])
SCALARS = ("sum_g", "n_ep", "steps", "cand", "n_len", "status")
TRACE = ("trace_z", "trace_z_next", "trace_reward", "trace_done", "trace_state", "trace_next_state")
# driver -> (mode, behaviour, epsilon, rec_max)
DRIVERS = {"evalMC": (H.EVALMC, H.FIXED, 0.0, False), "qlearn-fixed": (H.QLEARN, H.FIXED, 0.0, False), "qlearn-eps": (H.QLEARN, H.EPS_GREEDY, 0.3, False),
           "qlearn-greedy": (H.QLEARN, H.EPS_GREEDY, 0.0, False), "qlearn-soft": (H.QLEARN, H.SOFT_GREEDY, 0.0, False),
           "expSARSA": (H.EXPSARSA, H.FIXED, 0.0, False), "z_expSARSA": (H.EXPSARSA, H.FIXED, 0.0, True)}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def fx():
    return H.Fixture()


def homer(weights, gpu):
    from rl_offline_simulation_amd.encoders import HOMEREncoder
    from rl_offline_simulation_amd.encoders.homer import ENC_KEYS
    (Hd, dO), nZ = weights[0].shape, weights[2].shape[0]
    return HOMEREncoder(dO, 5 if dO == 2 else 2, nZ, Hd, state_dict=dict(zip(ENC_KEYS, weights)), device=gpu)


def coords(weights, gpu, num_steps=6, goal=(1, 1), nS=25):
    from rl_offline_simulation_amd.evaluators import LatentEnv
    return LatentEnv("grid_coords", homer(weights, gpu), nS, num_steps=num_steps, goal=goal)


def cartpole(gpu, cap, weights=None, nS=163):
    from rl_offline_simulation_amd.encoders import CartpoleBoxEncoder
    from rl_offline_simulation_amd.evaluators import LatentEnv
    return LatentEnv("cartpole", CartpoleBoxEncoder() if weights is None else homer(weights, gpu), nS, max_episode_steps=cap)


def batched(env, seeds, gpu):
    from rl_offline_simulation_amd.evaluators import BatchedLatentEnv
    b = BatchedLatentEnv(env, len(seeds), device=gpu)
    b.set_seeds(seeds)
    return b


def host(env, weights, seeds, mode, pi, gamma, reseed="episode", q0=None, ties=None, **kw):
    """the host loop per seed (the action stream and, under reseed = 'none', the environment stream are default_rng(seed));
    ties: None / "episode" / a list of RandomStates"""
    rows = []
    for i, s in enumerate(seeds):
        enc = H.BoxEncoder() if weights is None else H.MlpEncoder(weights)
        kind = "cartpole" if env.kind == "cartpole" else "coords"
        wkw = {} if kind == "cartpole" else dict(num_steps=env.num_steps, goal=env.goal, num_cells=env.num_cells)
        w = H.LiveWorld(kind, enc, seed=s, reseed=reseed == "episode", cap=env.max_episode_steps, **wkw)
        gen = np.random.default_rng(s)
        m = H.run(w, env.nS, env.nA, H.chooser(gen, env.nA), mode, pi, gamma, q=None if q0 is None else q0[i].copy(),
                  tie=ties[i] if isinstance(ties, list) else ties, **kw)
        m["rng_act_end"], m["rng_env_end"] = H.rng_words(gen), w.env_words()
        if weights is not None:
            assert min(enc.gaps) > 1e-3, "the case's weights leave a top-2 logit gap an f32 summation order could close"
        rows.append(m)
    return rows


def assert_rows(o, mine, tag, td=False, beh_arg=False, snap=False, trace=True, tol=0.0, rows=None):
    """outputs [R, ...] (or the rows `rows` of them) against the host's per-rollout dicts; tol: for q, td_err, q_snap, ep_g, sum_g"""
    pick = (lambda v: v) if rows is None else (lambda v: v[rows])
    loose = ("q", "td_err", "q_snap", "ep_g", "sum_g") if tol else ()
    for k in SCALARS + ("ep_g", "ep_len", "trace_pop") + (TRACE if trace else ()) + (("q", "td_err") if td else ()) + (("beh_arg",) if beh_arg else ()) + \
            (("q_snap",) if snap else ()):
        a, b = pick(o[k].cpu().numpy()), np.stack([np.asarray(m[k]) for m in mine])
        if k in loose:
            assert np.abs(a - b).max() <= tol, (tag, k, np.abs(a - b).max())
        else:
            assert np.array_equal(a, b.astype(a.dtype)), (tag, k)
    if td and "tie_mt" in o:
        assert np.array_equal(pick(o["tie_mt"].cpu().numpy().view(np.uint32)), np.stack([m["tie_mt"] for m in mine])), (tag, "tie_mt")
    for k in ("rng_act_end", "rng_env_end"):
        assert np.array_equal(pick(o[k].cpu().numpy().view(np.uint64)), np.stack([m[k] for m in mine])), (tag, k)


def policy(nS, nA, seed=5):
    return np.random.default_rng(seed).dirichlet(np.full(nA, 1.5), nS)


# ---- 1. grid_coords + MLP against the host loop ----
@pytest.mark.parametrize("reseed", ["episode", "none"])
@pytest.mark.parametrize("drv", list(DRIVERS))
def test_coords_mlp_against_the_host_loop(drv, reseed, gpu, fx):
    mode, beh, eps, rec_max = DRIVERS[drv]
    env = coords(fx.weights, gpu)
    pi = policy(25, 5) if drv != "qlearn-fixed" else np.full((25, 5), 0.2)
    cap = N_EP * env.bound + 1
    b = batched(env, SEEDS, gpu)
    if mode == H.EVALMC:
        mine = host(env, fx.weights, SEEDS, mode, pi, GAMMA, reseed, n_episodes=N_EP, trace_cap=cap, ep_cap=N_EP)
        o = b.eval_mc(pi, GAMMA, N_EP, ep_cap=N_EP, trace_cap=cap, reseed=reseed)
        assert_rows(o, mine, (drv, reseed))
    else:
        q0 = np.zeros((5, 25, 5)) if beh == H.EPS_GREEDY else np.random.default_rng(7).standard_normal((5, 25, 5)) * 0.1
        kw = dict(alpha=ALPHA, behaviour=beh, epsilon=eps, n_episodes=N_EP, trace_cap=cap, ep_cap=N_EP, alpha_ep=ALPHA_EP,
                  epsilon_ep=EPS_EP if drv == "qlearn-eps" else None, snap_cap=5, snap_stride=3, rec_max=rec_max)
        mine = host(env, fx.weights, SEEDS, mode, None if pi is None else pi, GAMMA, reseed, q0=q0, ties="episode", **kw)
        o = b.eval_td(None if beh != H.FIXED else pi, GAMMA, mode, q=q0, tie="episode", reseed=reseed, **kw)
        assert_rows(o, mine, (drv, reseed), td=True, beh_arg=beh == H.EPS_GREEDY, snap=True, tol=1e-12 if mode == H.EXPSARSA else 0.0)
    assert all(m["status"] == H.ST_OK and m["n_ep"] == N_EP for m in mine)
    assert any((m["trace_reward"] == 1.0).any() for m in mine) or drv in ("qlearn-greedy", "qlearn-soft")  # the goal (1, 1) is reached
    assert np.array_equal(b.rng_act.cpu().numpy(), o["rng_act_end"].cpu().numpy())


def test_tie_modes_and_continuation(gpu, fx):
    from rl_offline_simulation_amd import _lib as L
    env = coords(fx.weights, gpu)
    cap = N_EP * env.bound + 1
    kw = dict(alpha=ALPHA, behaviour=H.EPS_GREEDY, epsilon=0.3, trace_cap=cap, ep_cap=N_EP)
    q0 = np.zeros((5, 25, 5))
    for reseed in ("episode", "none"):
        # "first": the first maximum; given states: each rollout's own MT19937 stream runs on
        mine = host(env, fx.weights, SEEDS, H.QLEARN, None, GAMMA, reseed, q0=q0, ties=None, n_episodes=N_EP, **kw)
        o = batched(env, SEEDS, gpu).eval_td(None, GAMMA, L.TD_QLEARN, q=q0, tie="first", reseed=reseed, n_episodes=N_EP, **kw)
        assert_rows(o, mine, ("first", reseed), td=True, beh_arg=True)
        rs = [np.random.RandomState(100 + s) for s in SEEDS]
        states = np.stack([H.mt_words(r) for r in rs])
        mine = host(env, fx.weights, SEEDS, H.QLEARN, None, GAMMA, reseed, q0=q0, ties=rs, n_episodes=N_EP, **kw)
        o = batched(env, SEEDS, gpu).eval_td(None, GAMMA, L.TD_QLEARN, q=q0, tie=states, reseed=reseed, n_episodes=N_EP, **kw)
        assert_rows(o, mine, ("states", reseed), td=True, beh_arg=True)
        # one call of 4 episodes equals 1 + 3 with episode0 moved on, Q and the streams handed on
        whole = batched(env, SEEDS, gpu).eval_td(None, GAMMA, L.TD_QLEARN, q=q0, tie="episode", reseed=reseed, n_episodes=N_EP, **kw)
        b = batched(env, SEEDS, gpu)
        first = b.eval_td(None, GAMMA, L.TD_QLEARN, q=q0, tie="episode", reseed=reseed, n_episodes=1, **kw)
        rest = b.eval_td(None, GAMMA, L.TD_QLEARN, q=first["q"], tie="episode", reseed=reseed, n_episodes=N_EP - 1, episode0=1, **kw)
        for k in ("q", "tie_mt", "rng_act_end", "rng_env_end"):
            assert torch.equal(whole[k], rest[k]), (reseed, k)
        assert torch.equal(whole["ep_g"][:, 1:], rest["ep_g"][:, :N_EP - 1]) and torch.equal(whole["ep_g"][:, 0], first["ep_g"][:, 0])
        assert torch.equal(whole["steps"], first["steps"] + rest["steps"])


def test_the_reference_fixture_through_the_drop_ins(gpu, fx):
    from rl_offline_simulation_amd.evaluators import evalMC_latent_env, qlearn_latent_env, z_expSARSA_env, expSARSA_latent_env
    d, n, gam, al = fx.d, int(fx.d["n_episodes"]), float(fx.d["gamma"]), float(fx.d["alpha"])

    def eps_greedy(Q, args):  # the reference's epsilon_greedy_policy, as _behaviour_kind probes it
        pi = np.ones_like(Q) * args["epsilon"] / Q.shape[1]
        for s in range(len(Q)):
            pi[s, np.random.choice(np.where(Q[s] == np.max(Q[s]))[0])] = 1 - args["epsilon"] + args["epsilon"] / Q.shape[1]
        return pi

    for i in range(len(fx.runs)):
        drv, goal, num_steps, seed = fx.settings(i)
        env = coords(fx.weights, gpu, num_steps, goal)
        np.random.seed(12345)
        if drv == "evalMC":
            Gs, lengths = evalMC_latent_env(env, n, d["pi"], gam, seed=seed)
            assert np.array_equal(Gs, d["Gs"][i]) and np.array_equal(lengths, d["lengths"][i]), fx.runs[i]
            continue
        if drv == "z_expSARSA":
            Q, info = z_expSARSA_env(env, n, d["pi"], gam, alpha=al, save_Q=1, seed=seed)
            tol = 1e-12
        else:
            Q, info = qlearn_latent_env(env, n, eps_greedy, gam, alpha=al, epsilon=H.EPS_SCHED if drv == "qlearn_eps_sched" else 0.3, save_Q=1, seed=seed)
            tol = 0.0
        st = np.random.get_state()
        assert np.array_equal(np.concatenate([st[1], [st[2]]]).astype(np.uint32), fx.mt(i)), fx.runs[i]
        assert np.array_equal(info["Gs"], d["Gs"][i]) and len(info["memory"]) == len(fx.td(i)), fx.runs[i]
        for a, b in ((Q, d["Q"][i]), (info["TD_errors"], fx.td(i)), (info["Qs"], fx.Qs(i))):
            assert np.abs(a - b).max() <= tol, (fx.runs[i], np.abs(a - b).max())
        z, A, R, z_, done, p, t = info["memory"][0]
        assert t == {"t": 0} and 0 <= z < 25 and np.array_equal(p, d["pi"][z]) if drv == "z_expSARSA" else abs(p.sum() - 1) < 1e-12
    env = coords(fx.weights, gpu, 15, (4, 4))
    Q, info = expSARSA_latent_env(env, 2, d["pi"], gam, alpha=al, seed=0)
    Qz, infoz = z_expSARSA_env(env, 2, d["pi"], gam, alpha=al, seed=0)
    assert np.array_equal(Q, Qz) and not np.array_equal(info["TD_errors"], infoz["TD_errors"])  # the flag changes the record, not the update


# ---- 2. CartPole + BOX, from the trace ----
CARTPOLE_BOX_CAPS = (8, 40)


def _tolerance_eps():
    """DESIGN section 28's rule, from the measured lines: 8 times the largest deviation profiles/true_env_error.jsonl holds for env_step's
    CartPole (tools/true_env_error_table.py's lines and tools/latent_env_error_table.py's for this kernel), never more than 1e-12"""
    rows = [json.loads(x) for x in open(os.path.join(ROOT, "profiles", "true_env_error.jsonl")) if x.strip()]
    worst = max(r["max_dev_eps"] for r in rows if r["what"] == "cartpole next_state")
    assert any(r.get("kernel") == "k_eval_env_latent" for r in rows), "no measured line of this kernel in profiles/true_env_error.jsonl"
    return min(8.0 * worst, 1e-12 / EPS)


def run_cartpole_box_case(gpu, cap):
    """the device's outputs of one traced case (also tools/latent_env_error_table.py's): (host arrays of every output, q0, the call's keywords)"""
    from rl_offline_simulation_amd import _lib as L
    env = cartpole(gpu, cap)
    n_ep, tc = 4, 4 * cap + 1
    q0 = np.zeros((5, 163, 2))
    q0[:, 162] = [7.0, 5.0]  # the row a terminal step's error reads
    kw = dict(alpha=ALPHA, behaviour=H.EPS_GREEDY, epsilon=0.3, n_episodes=n_ep, trace_cap=tc, ep_cap=n_ep)
    o = batched(env, SEEDS, gpu).eval_td(None, GAMMA, L.TD_QLEARN, q=q0, tie="episode", **kw)
    return {k: v.cpu().numpy() for k, v in o.items() if isinstance(v, torch.Tensor)}, q0, kw


def case_deviation(host_o, i):
    """largest deviation of rollout i's traced next_state from the host's f64 step of the traced state and action, in eps * max(1, |value|)"""
    m = int(host_o["steps"][i])
    return cartpole_deviation(host_o["trace_state"][i, :m, None], host_o["trace_pop"][i, :m, None], host_o["trace_next_state"][i, :m, None])


@pytest.mark.parametrize("cap", CARTPOLE_BOX_CAPS)
def test_cartpole_box_from_the_trace(cap, gpu):
    from rl_offline_simulation_amd import _lib as L
    n_ep = 4
    host_o, q0, kw = run_cartpole_box_case(gpu, cap)
    worst, saw_out = 0.0, False
    for i, s in enumerate(SEEDS):
        m = int(host_o["steps"][i])
        z, z_, r, dn, A = (host_o[k][i, :m] for k in ("trace_z", "trace_z_next", "trace_reward", "trace_done", "trace_pop"))
        st, nx = host_o["trace_state"][i, :m], host_o["trace_next_state"][i, :m]
        assert host_o["status"][i] == L.ST_OK and host_o["n_ep"][i] == n_ep and (r == 1.0).all()
        # z and z' are the host box of the traced f32 state, exactly
        assert [H.BoxEncoder()(x) for x in st.astype(np.float32)] == z.tolist() and [H.BoxEncoder()(x) for x in nx.astype(np.float32)] == z_.tolist()
        # next_state within DESIGN section 28's rule of the host f64 step from the traced state and action
        dev = case_deviation(host_o, i)
        print(f"cartpole latent: cap {cap} seed {s}: max deviation {dev:.3f} eps over {m} steps")
        worst = max(worst, dev)
        # the reset rows under reseed = "episode", and the chain within an episode
        starts = np.flatnonzero(np.concatenate([[True], dn[:-1] != 0]))
        assert len(starts) == n_ep
        for e, k in enumerate(starts):
            assert np.array_equal(st[k], np.random.default_rng(e).uniform(-0.05, 0.05, 4)), (cap, s, e)
        assert all(np.array_equal(st[k], nx[k - 1]) and z[k] == z_[k - 1] for k in range(1, m) if not dn[k - 1])
        ends = np.flatnonzero(dn)
        assert all((k + 1 - starts[e]) <= cap for e, k in enumerate(ends))
        # the learner replayed on the traced (z, A, r, z', done)
        w = H.TraceWorld(z, z_, r, dn)
        mine = H.run(w, 163, 2, H.replayer(A), H.QLEARN, None, GAMMA, q=q0[i].copy(), tie="episode", **kw)
        for k in ("q", "td_err", "ep_g", "ep_len", "beh_arg"):
            assert np.array_equal(host_o[k][i], mine[k]), (cap, s, k)
        assert host_o["sum_g"][i] == mine["sum_g"] and np.array_equal(host_o["tie_mt"][i].view(np.uint32), mine["tie_mt"])
        out = np.flatnonzero(z_ == -1)
        saw_out = saw_out or len(out) > 0
        assert all(dn[k] for k in out)
    assert worst <= _tolerance_eps(), (worst, _tolerance_eps())
    assert saw_out or cap == 8  # a pole falls within 40 steps: the terminal error read row nS - 1 = 162 (replayed above through NumPy's Q[-1])


# ---- 3. CartPole + MLP ----
def test_cartpole_mlp_trace_is_the_f64_arg_max_where_clear(gpu):
    weights = H.mlp_weights(4, 8, 10, H.CARTPOLE_MLP_WEIGHT_SEED)
    env = cartpole(gpu, 40, weights, nS=10)
    seeds = list(H.CARTPOLE_MLP_SEEDS)
    o = batched(env, seeds, gpu).eval_mc(np.full((10, 2), 0.5), GAMMA, 4, ep_cap=4, trace_cap=161)
    obs, zs = [], []
    for i in range(len(seeds)):
        m = int(o["steps"][i])
        for a, b in (("trace_state", "trace_z"), ("trace_next_state", "trace_z_next")):
            obs.append(o[a][i, :m].cpu().numpy().astype(np.float32))
            zs.append(o[b][i, :m].cpu().numpy())
    obs, zs = np.concatenate(obs), np.concatenate(zs)
    clear, want = H.clear_rows(weights, obs)
    assert len(zs) > 100 and (~clear).sum() <= 0.01 * len(zs), ((~clear).sum(), len(zs))
    assert np.array_equal(zs[clear], want[clear])
    assert (zs >= 0).all() and (zs < 10).all() and len(np.unique(zs)) > 1


# ---- 4. population ----
def test_population_equals_the_single_calls_and_is_a_query(gpu, fx):
    from rl_offline_simulation_amd import _lib as L
    from rl_offline_simulation_amd.evaluators import TDPopulation, evalmc_rollouts_latent_env
    env = coords(fx.weights, gpu)
    alphas, epss, gammas = [0.1, 0.3, 0.5], [0.3, 0.1, 0.0], [0.9, 0.8, 1.0]
    for reseed in ("episode", "none"):
        pop = TDPopulation("qlearn", alphas, gammas, epsilon=epss, behaviour="eps_greedy")
        res = pop.run_latent_env(env, SEEDS, N_EP, reseed=reseed, trace_cap=12)
        tiled = pop.run_latent_env(env, SEEDS, N_EP, reseed=reseed, trace_cap=12, tile=2)
        for k in ("Q", "Gs", "n_ep", "steps", "status", "td_err", "tie_mt", "curve_mean"):
            assert torch.equal(getattr(res, k), getattr(tiled, k)), (reseed, "seed tiles", k)
        for l in range(3):
            one = batched(env, SEEDS, gpu).eval_td(None, gammas[l], L.TD_QLEARN, alphas[l], behaviour=L.BEHAVIOUR_EPS_GREEDY, epsilon=epss[l], tie="episode",
                                                   n_episodes=N_EP, ep_cap=N_EP, trace_cap=12, reseed=reseed)
            assert torch.equal(res.Q[l], one["q"]) and torch.equal(res.Gs[l], one["ep_g"]) and torch.equal(res.td_err[l], one["td_err"]), (reseed, l)
            assert torch.equal(res.tie_mt[l], one["tie_mt"]) and torch.equal(res.steps[l], one["steps"])
        # learner tiles: a population of the last two learners alone
        part = TDPopulation("qlearn", alphas[1:], gammas[1:], epsilon=epss[1:], behaviour="eps_greedy").run_latent_env(env, SEEDS, N_EP, reseed=reseed)
        assert torch.equal(part.Q, res.Q[1:]) and torch.equal(part.Gs, res.Gs[1:])
        # a query: the streams handed in are untouched, all members of a seed see the same resets
        b = batched(env, SEEDS, gpu)
        act, envs = b.rng_act.clone(), b.rng_env.clone()
        o = b.eval_td_population(L.TD_QLEARN, alphas, gammas, behaviour=L.BEHAVIOUR_EPS_GREEDY, epsilon=epss, tie="episode", n_episodes=N_EP, ep_cap=N_EP,
                                 trace_cap=12, reseed=reseed, state=True)
        assert torch.equal(b.rng_act, act) and torch.equal(b.rng_env, envs) and o["trace_state"].shape == (3, 5, 12, 4)
        assert torch.equal(o["trace_state"][0, :, 0], o["trace_state"][1, :, 0]) and torch.equal(o["trace_state"][0, :, 0], o["trace_state"][2, :, 0])
        # the policy stack
        stack = np.stack([policy(25, 5, s) for s in (1, 2, 3)])
        r = evalmc_rollouts_latent_env(env, SEEDS, stack, GAMMA, N_EP, reseed=reseed)
        assert r["value"].shape == (3, 5) and r["best"] == int(np.argmax(r["mean_value"]))
        for l in range(3):
            one = evalmc_rollouts_latent_env(env, SEEDS, stack[l], GAMMA, N_EP, reseed=reseed)
            for k in ("sum_g", "n_ep", "steps", "status", "value"):
                assert np.array_equal(r[k][l], one[k]), (reseed, l, k)


# ---- 5. launch shapes and statuses ----
def test_undrawable_row_and_the_carve(gpu, fx):
    from rl_offline_simulation_amd import _lib as L
    env = coords(fx.weights, gpu)
    pi = policy(25, 5)
    mine0 = host(env, fx.weights, SEEDS, H.EVALMC, pi, GAMMA, n_episodes=1, trace_cap=8, ep_cap=1)
    bad = np.full_like(pi, np.nan)  # only the first episode's first latent state has a row to draw from
    bad[[int(m["trace_z"][0]) for m in mine0]] = pi[0]
    mine = host(env, fx.weights, SEEDS, H.EVALMC, bad, GAMMA, n_episodes=N_EP, trace_cap=8, ep_cap=N_EP)
    o = batched(env, SEEDS, gpu).eval_mc(bad, GAMMA, N_EP, ep_cap=N_EP, trace_cap=8)
    assert_rows(o, mine, "undrawable")
    assert any(m["status"] == L.ST_KEYERROR and m["trace_pop"][m["steps"]] == 5 for m in mine)  # the draw consumed: rng_act_end compared above
    # the 4 / 2 / 1 rollouts-per-workgroup carve, nS chosen to force each (CartPole + BOX, learners)
    big = 5000  # one rollout per workgroup whose carve (Q 80 000 bytes + the tie stream) lies above 64 KiB: the big-LDS launch
    assert H.launch_shape(big, 2, False)[:2] == (1, 80000 + 16 + 2496) and not H.launch_shape(big, 2, False)[2]
    for waves, nS in ((4, H.nS_for_waves(4, 2, 163)), (2, H.nS_for_waves(2, 2, 163)), (1, H.nS_for_waves(1, 2, 163)), (1, big)):
        envc = cartpole(gpu, 8, nS=nS)
        q0 = np.random.default_rng(waves).standard_normal((5, nS, 2)) * 0.01
        kw = dict(alpha=ALPHA, behaviour=H.SOFT_GREEDY, n_episodes=3, trace_cap=25, ep_cap=3)
        oc = batched(envc, SEEDS, gpu).eval_td(None, GAMMA, L.TD_QLEARN, q=q0, **kw)
        ho = {k: v.cpu().numpy() for k, v in oc.items() if isinstance(v, torch.Tensor)}
        for i in range(5):
            m = int(ho["steps"][i])
            w = H.TraceWorld(*(ho[k][i, :m] for k in ("trace_z", "trace_z_next", "trace_reward", "trace_done")))
            mm = H.run(w, nS, 2, H.replayer(ho["trace_pop"][i, :m]), H.QLEARN, None, GAMMA, q=q0[i].copy(), **kw)
            assert np.array_equal(ho["q"][i], mm["q"]) and np.array_equal(ho["td_err"][i], mm["td_err"]) and np.array_equal(ho["ep_g"][i], mm["ep_g"]), (waves, i)
            assert (ho["trace_z"][i, :m] >= 0).all() and ho["n_ep"][i] == 3


def test_mlp_weights_share_the_carve_with_a_learners_q_below_four_rollouts(gpu, fx):
    """the coordinate grid with nS padded until the learner's carve holds 2 rollouts per workgroup and then 1 above 64 KiB: the encoder's
    weights sit behind Q, pi and the tie streams, and the rollouts equal the host loop as at 4 rollouts per workgroup"""
    from rl_offline_simulation_amd import _lib as L
    mlp = (2, 16, 25)
    for waves, nS in ((2, H.nS_for_waves(2, 5, 25, True, mlp)), (1, 1700)):
        shape = H.launch_shape(nS, 5, True, True, mlp)
        assert shape[0] == waves and not shape[2] and (waves == 2 or shape[1] > 65536)
        env = coords(fx.weights, gpu, nS=nS)
        pi = policy(nS, 5)
        q0 = np.random.default_rng(waves).standard_normal((5, nS, 5)) * 0.1
        kw = dict(alpha=ALPHA, behaviour=H.FIXED, n_episodes=3, trace_cap=19, ep_cap=3)
        mine = host(env, fx.weights, SEEDS, H.EXPSARSA, pi, GAMMA, q0=q0, ties="episode", **kw)
        o = batched(env, SEEDS, gpu).eval_td(pi, GAMMA, L.TD_EXPSARSA, q=q0, tie="episode", **kw)
        assert_rows(o, mine, ("mlp carve", waves), td=True, tol=1e-12)


def test_empty_calls(gpu, fx):
    from rl_offline_simulation_amd.evaluators import (BatchedLatentEnv, TDPopulation, evalMC_latent_env, evalmc_rollouts_latent_env, qlearn_latent_env,
                                                      z_expSARSA_env)
    from rl_offline_simulation_amd import _lib as L
    env, box = coords(fx.weights, gpu), cartpole(gpu, 8)
    pi, pib = policy(25, 5), np.full((163, 2), 0.5)
    # no rollouts: the C entries validate and launch nothing -- real one-row buffers, filled beforehand, come back as they were
    import ctypes as C
    for e, p in ((env, pi), (box, pib)):
        b = BatchedLatentEnv(e, 1, device=gpu)
        pi_d = torch.as_tensor(p).to(gpu).contiguous()
        gp = torch.ones(e.bound + 2, dtype=torch.float64, device=gpu)
        for pop in (False, True):
            o = {k: torch.full((1,), -7, dtype=dt, device=gpu) for k, dt in (("sum_g", torch.float64), ("n_ep", torch.int64), ("steps", torch.int64),
                                                                             ("cand", torch.int64), ("n_len", torch.int64), ("status", torch.int32))}
            oc = L.EvalMCOut(**{k: L.ptr(v) for k, v in o.items()})
            ec, enc, run = b._structs(b.rng_act, b.rng_env, {}, 1, 0, 0)
            ec.S = 0
            ends = torch.full((1, 4), -7, dtype=torch.int64, device=gpu)
            run.rng_act_end = run.rng_env_end = L.ptr(ends)
            if pop:
                rc = L.load().offsim_eval_env_latent_pop(C.byref(ec), C.byref(enc), 3, 2, None, L.ptr(pi_d), GAMMA, L.ptr(gp), gp.numel(), 3, C.byref(oc),
                                                         C.byref(run), L.stream_ptr())
            else:
                rc = L.load().offsim_eval_env_latent(C.byref(ec), C.byref(enc), L.ptr(pi_d), GAMMA, L.ptr(gp), gp.numel(), 3, C.byref(oc), None, C.byref(run),
                                                     L.stream_ptr())
            torch.cuda.synchronize()
            assert rc == L.OK and all((v == -7).all() for v in o.values()) and (ends == -7).all(), (e.kind, pop)
    L.check_async_faults()
    # no seeds through the many-seed driver
    r = evalmc_rollouts_latent_env(env, [], pi, GAMMA, 3)
    assert r["value"].shape == (0,) and r["sum_g"].shape == (0,)
    r = evalmc_rollouts_latent_env(box, [], np.stack([pib, pib, pib]), GAMMA, 3)
    assert r["value"].shape == (3, 0) and r["best"] == -1 and np.isnan(r["mean_value"]).all()
    with pytest.raises(ValueError, match="seed"):
        TDPopulation("qlearn", 0.1, 0.9).run_latent_env(env, [], 3)
    # no episodes through the drop-ins: the reference's empty results
    Gs, lengths = evalMC_latent_env(env, 0, pi, GAMMA, seed=0)
    assert len(Gs) == 0 and len(lengths) == 0
    eps_greedy = lambda Q, args: np.ones_like(Q) / Q.shape[1]  # noqa: E731
    for Q, info in (qlearn_latent_env(box, 0, eps_greedy, GAMMA, seed=0), z_expSARSA_env(env, 0, pi, GAMMA, seed=0)):
        assert not Q.any() and info["memory"] == [] and len(info["Gs"]) == 0 and info["Qs"].shape[0] == 1
