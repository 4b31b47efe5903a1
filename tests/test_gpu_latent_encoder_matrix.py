"""The in-kernel MLP encoder of k_eval_env_latent (latent_encode<ENV, OFFSIM_LATENT_MLP>, csrc/eval_env_latent.hpp) held to the oracle's f32
encoder on EVERY observation, over the case table of tests/latent_encoder_cases.py: more than one lane round in H and in nZ, both staging
transposes, exact ties out of lane order and inside one lane, all-equal / NaN / infinite logits, H = 4096 and nZ = 4096, and encoders whose
size alone sets the launch to 4, 2 and 1 rollouts per workgroup.  No top-2 gap is asserted and no row is left out.

  grid, every case, evalMC      the whole output set equals the host loop (LiveWorld behind the oracle's encoder) bit for bit
  grid, lane / tie / carve      Q-learning eps-greedy with the per-episode tie stream (bit for bit) and expected SARSA (1e-12, the existing
                                tests' bound for its sum): q, td_err, tie_mt and q_snap too, so a wrong z is a wrong row written
  CartPole, lane / tie / limit  from the trace (the rollout is closed-loop): trace_z / trace_z_next are the oracle's z of the traced state
                                rounded to f32 on every row, next_state is within DESIGN section 28's rule of the host's f64 step, and the
                                learner replayed on the trace matches
  population                    entry [l, j] equals the single call and the host loop at L = 3, S = 5 (a partial last workgroup per member)
  the box encoder's wrap        nS = 200: a pole that falls reads row 199
Runs: R = 5 rollouts, 3 episodes, num_steps = 6 on the grid, CartPole's cap 12 (the case table's constants)."""
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import latent_encoder_cases as K  # noqa: E402
import latent_env_host as H  # noqa: E402
from test_gpu_latent_env import _tolerance_eps, assert_rows, batched, cartpole, gpu, homer  # noqa: E402,F401
from true_env_host import cartpole_deviation  # noqa: E402

pytestmark = pytest.mark.gpu
SEEDS, N_EP, GAMMA, ALPHA = K.SEEDS, K.N_EP, K.GAMMA, K.ALPHA
# learner -> (mode, behaviour, epsilon, tolerance on q / td_err / q_snap / ep_g / sum_g)
LEARNERS = {"qlearn-eps": (H.QLEARN, H.EPS_GREEDY, 0.3, 0.0), "expSARSA": (H.EXPSARSA, H.FIXED, 0.0, 1e-12)}


def latent_env(case, gpu):
    from rl_offline_simulation_amd.evaluators import LatentEnv
    w = K.weights(case)
    if case["env"] == "grid_coords":
        return LatentEnv("grid_coords", homer(w, gpu), case["nS"], num_steps=K.GRID_STEPS, goal=K.GRID_GOAL), w
    return LatentEnv("cartpole", homer(w, gpu), case["nS"], max_episode_steps=K.CARTPOLE_CAP), w


def host_arrays(o):
    return {k: v.cpu().numpy() for k, v in o.items() if isinstance(v, torch.Tensor)}


# ---- 1. the grid, every case, evalMC against the host loop ----
@pytest.mark.parametrize("name", K.names(env="grid_coords"))
def test_grid_evalmc_equals_the_host_loop_behind_the_oracle(name, gpu):
    case = K.BY_NAME[name]
    env, w = latent_env(case, gpu)
    waves, lds, refused = K.shape(case)
    assert not refused and (case["group"] != "limit" or (waves == 1 and lds > 65536))
    pi = K.policy(case["nS"], 5)
    cap = N_EP * env.bound + 1
    mine, enc = K.host_rows(case, w, H.EVALMC, pi, trace_cap=cap, ep_cap=N_EP)
    b = batched(env, SEEDS, gpu)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    o = b.eval_mc(pi, GAMMA, N_EP, ep_cap=N_EP, trace_cap=cap)
    torch.cuda.synchronize()
    print(f"latent encoder matrix: {name}: eval_mc of {len(SEEDS)} rollouts x {N_EP} episodes, {waves} per workgroup, {lds} B of LDS: "
          f"{1e3 * (time.perf_counter() - t0):.1f} ms")
    assert_rows(o, mine, name)
    assert all(m["status"] == H.ST_OK and m["n_ep"] == N_EP for m in mine) and len(enc.z) == sum(m["steps"] for m in mine) + N_EP * len(SEEDS)


# ---- 2. the grid, the lane-round, tie and carve cases with a learner ----
@pytest.mark.parametrize("drv", list(LEARNERS))
@pytest.mark.parametrize("name", K.names(("lane", "tie", "carve"), env="grid_coords"))
def test_grid_learner_equals_the_host_loop_behind_the_oracle(name, drv, gpu):
    case = K.BY_NAME[name]
    assert drv in case["learners"]
    mode, beh, eps, tol = LEARNERS[drv]
    env, w = latent_env(case, gpu)
    nS = case["nS"]
    if case["group"] == "carve" and drv == "expSARSA":  # the shape the case is in the table for
        assert K.shape(case, have_pi=True, td=True)[::2] == (case["waves"], False)
    pi = K.policy(nS, 5) if beh == H.FIXED else None
    q0 = np.zeros((len(SEEDS), nS, 5)) if beh == H.EPS_GREEDY else np.random.default_rng(7).standard_normal((len(SEEDS), nS, 5)) * 0.1
    kw = dict(alpha=ALPHA, behaviour=beh, epsilon=eps, n_episodes=N_EP, trace_cap=N_EP * env.bound + 1, ep_cap=N_EP, snap_cap=5, snap_stride=3)
    mine, _ = K.host_rows(case, w, mode, pi, q0=q0, tie="episode", **kw)
    o = batched(env, SEEDS, gpu).eval_td(pi, GAMMA, mode, q=q0, tie="episode", **kw)
    assert_rows(o, mine, (name, drv), td=True, beh_arg=beh == H.EPS_GREEDY, snap=True, tol=tol)
    assert all(m["status"] == H.ST_OK and m["n_ep"] == N_EP for m in mine)


# ---- 3. CartPole, from the trace ----
@pytest.mark.parametrize("name", K.names(env="cartpole"))
def test_cartpole_trace_is_the_oracles_z_on_every_row(name, gpu):
    from rl_offline_simulation_amd import _lib as L
    case = K.BY_NAME[name]
    env, w = latent_env(case, gpu)
    nS, cap = case["nS"], K.CARTPOLE_CAP
    tc = N_EP * cap + 1
    learner = bool(case["learners"])
    b = batched(env, SEEDS, gpu)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if learner:
        q0 = np.zeros((len(SEEDS), nS, 2))
        kw = dict(alpha=ALPHA, behaviour=H.EPS_GREEDY, epsilon=0.3, n_episodes=N_EP, trace_cap=tc, ep_cap=N_EP)
        o = b.eval_td(None, GAMMA, L.TD_QLEARN, q=q0, tie="episode", **kw)
    else:
        waves, lds, refused = K.shape(case)
        assert waves == 1 and lds > 65536 and not refused
        pi = np.full((nS, 2), 0.5)
        o = b.eval_mc(pi, GAMMA, N_EP, ep_cap=N_EP, trace_cap=tc)
    torch.cuda.synchronize()
    print(f"latent encoder matrix: {name}: {len(SEEDS)} rollouts x {N_EP} episodes: {1e3 * (time.perf_counter() - t0):.1f} ms")
    ho = host_arrays(o)
    worst = 0.0
    for i, s in enumerate(SEEDS):
        m = int(ho["steps"][i])
        z, z_, r, dn, A = (ho[k][i, :m] for k in ("trace_z", "trace_z_next", "trace_reward", "trace_done", "trace_pop"))
        st, nx = ho["trace_state"][i, :m], ho["trace_next_state"][i, :m]
        assert ho["status"][i] == L.ST_OK and ho["n_ep"][i] == N_EP and (r == 1.0).all() and m >= N_EP
        # z and z' are the oracle's z of the traced state rounded to f32: every row
        assert np.array_equal(K.oracle_z(w, st.astype(np.float32)), z), (name, s, "trace_z")
        assert np.array_equal(K.oracle_z(w, nx.astype(np.float32)), z_), (name, s, "trace_z_next")
        worst = max(worst, cartpole_deviation(st[:, None], A[:, None], nx[:, None]))
        starts = np.flatnonzero(np.concatenate([[True], dn[:-1] != 0]))
        assert len(starts) == N_EP
        for e, k in enumerate(starts):
            assert np.array_equal(st[k], np.random.default_rng(e).uniform(-0.05, 0.05, 4)), (name, s, e)
        assert all(np.array_equal(st[k], nx[k - 1]) and z[k] == z_[k - 1] for k in range(1, m) if not dn[k - 1])
        assert all((k + 1 - starts[e]) <= cap for e, k in enumerate(np.flatnonzero(dn)))
        # the learner (or the returns) replayed on the traced (z, A, r, z', done)
        tw = H.TraceWorld(z, z_, r, dn)
        if learner:
            mine = H.run(tw, nS, 2, H.replayer(A), H.QLEARN, None, GAMMA, q=q0[i].copy(), tie="episode", **kw)
            for k in ("q", "td_err", "ep_g", "ep_len", "beh_arg"):
                assert np.array_equal(ho[k][i], mine[k]), (name, s, k)
            assert np.array_equal(ho["tie_mt"][i].view(np.uint32), mine["tie_mt"])
        else:
            mine = H.run(tw, nS, 2, H.replayer(A), H.EVALMC, pi, GAMMA, n_episodes=N_EP, trace_cap=tc, ep_cap=N_EP)
            for k in ("ep_g", "ep_len"):
                assert np.array_equal(ho[k][i], mine[k]), (name, s, k)
        assert ho["sum_g"][i] == mine["sum_g"]
    assert worst <= _tolerance_eps(), (worst, _tolerance_eps())


# ---- 4. population: a lane-round case and the out-of-order tie at L = 3, S = 5 ----
@pytest.mark.parametrize("name", ["lane-65x65-grid", "tie-out-of-lane-order-grid"])
def test_population_entries_equal_the_single_calls_and_the_host_loop(name, gpu):
    from rl_offline_simulation_amd import _lib as L
    from rl_offline_simulation_amd.evaluators import TDPopulation, evalmc_rollouts_latent_env
    case = K.BY_NAME[name]
    env, w = latent_env(case, gpu)
    nS = case["nS"]
    alphas, epss, gammas = [0.1, 0.3, 0.5], [0.3, 0.1, 0.0], [0.9, 0.8, 1.0]
    res = TDPopulation("qlearn", alphas, gammas, epsilon=epss, behaviour="eps_greedy").run_latent_env(env, SEEDS, N_EP, trace_cap=12)
    for l in range(3):
        one = batched(env, SEEDS, gpu).eval_td(None, gammas[l], L.TD_QLEARN, alphas[l], behaviour=L.BEHAVIOUR_EPS_GREEDY, epsilon=epss[l], tie="episode",
                                               n_episodes=N_EP, ep_cap=N_EP, trace_cap=12)
        for a, k in ((res.Q, "q"), (res.Gs, "ep_g"), (res.td_err, "td_err"), (res.tie_mt, "tie_mt"), (res.steps, "steps")):
            assert torch.equal(a[l], one[k]), (name, l, k)
    # learner 0 against the host loop itself (gamma 0.9 is the table's)
    kw = dict(alpha=alphas[0], behaviour=H.EPS_GREEDY, epsilon=epss[0], n_episodes=N_EP, trace_cap=12, ep_cap=N_EP)
    mine, _ = K.host_rows(case, w, H.QLEARN, None, q0=np.zeros((len(SEEDS), nS, 5)), tie="episode", **kw)
    assert np.array_equal(res.Q[0].cpu().numpy(), np.stack([m["q"] for m in mine]))
    assert np.array_equal(res.tie_mt[0].cpu().numpy().view(np.uint32), np.stack([m["tie_mt"] for m in mine]))
    # the policy stack
    stack = np.stack([K.policy(nS, 5, s) for s in (1, 2, 3)])
    r = evalmc_rollouts_latent_env(env, SEEDS, stack, GAMMA, N_EP)
    assert r["value"].shape == (3, 5)
    for l in range(3):
        one = evalmc_rollouts_latent_env(env, SEEDS, stack[l], GAMMA, N_EP)
        for k in ("sum_g", "n_ep", "steps", "status", "value"):
            assert np.array_equal(r[k][l], one[k]), (name, l, k)
        mine, _ = K.host_rows(case, w, H.EVALMC, stack[l])
        assert np.array_equal(r["sum_g"][l], [m["sum_g"] for m in mine]) and np.array_equal(r["steps"][l], [m["steps"] for m in mine]), (name, l)


# ---- 5. the box encoder's wrap above 163 rows ----
def test_box_out_of_bounds_reads_the_last_row_at_200_rows(gpu):
    from rl_offline_simulation_amd import _lib as L
    nS, cap, n_ep = 200, 40, 4
    env = cartpole(gpu, cap, nS=nS)
    q0 = np.zeros((len(SEEDS), nS, 2))
    q0[:, nS - 1] = [7.0, 5.0]  # the row a terminal step's error reads: -1 wraps to nS - 1
    kw = dict(alpha=ALPHA, behaviour=H.EPS_GREEDY, epsilon=0.3, n_episodes=n_ep, trace_cap=n_ep * cap + 1, ep_cap=n_ep)
    ho = host_arrays(batched(env, SEEDS, gpu).eval_td(None, GAMMA, L.TD_QLEARN, q=q0, tie="episode", **kw))
    saw_out = False
    for i, s in enumerate(SEEDS):
        m = int(ho["steps"][i])
        z, z_, r, dn, A = (ho[k][i, :m] for k in ("trace_z", "trace_z_next", "trace_reward", "trace_done", "trace_pop"))
        assert ho["status"][i] == L.ST_OK and ho["n_ep"][i] == n_ep
        box = H.BoxEncoder()
        assert [box(x) for x in ho["trace_state"][i, :m].astype(np.float32)] == z.tolist()
        assert [box(x) for x in ho["trace_next_state"][i, :m].astype(np.float32)] == z_.tolist()
        mine = H.run(H.TraceWorld(z, z_, r, dn), nS, 2, H.replayer(A), H.QLEARN, None, GAMMA, q=q0[i].copy(), tie="episode", **kw)
        for k in ("q", "td_err", "ep_g", "ep_len", "beh_arg"):
            assert np.array_equal(ho[k][i], mine[k]), (s, k)
        assert ho["sum_g"][i] == mine["sum_g"] and np.array_equal(ho["tie_mt"][i].view(np.uint32), mine["tie_mt"])
        out = np.flatnonzero(z_ == -1)
        assert all(dn[k] for k in out)
        saw_out = saw_out or len(out) > 0
    assert saw_out  # a pole falls within 40 steps: its terminal error read row 199 (replayed above through NumPy's Q[-1] of a 200-row table)

