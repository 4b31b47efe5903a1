"""VectorGridNavi / VectorCartPole (offsim_env_collect*, csrc/collect_env.hpp) on the device.

The grids are held bit for bit to the plain Python loop of tests/true_env_host.py, teacher-forced on the recorded probs: observations, cell
ids, actions, rewards, flags, ep_step and where both streams stand; probs to MLPPolicy.forward at the recorded observation and value to
MLPValue.forward, bit for bit; logp by tests/test_gpu_ppo.py's rule (exp(logp) against probs[a] within 1e-6, the MLP form against torch's
log_softmax within 2e-6: no function of the package returns the logits).  CartPole is teacher-forced per step: the host's f64 step from the
device's own recorded state and action against the device's next_state, within 8 times the largest deviation
tools/true_env_error_table.py measured over these cases (profiles/true_env_error.jsonl, in eps * max(1, |value|)) and never above
1e-12 * max(1, |value|); flags, f32 roundings, reset draws, ep_step and the action draws exactly.  Then carry-over, masked reset, the
population against single learners, PPOLearner.fit against the loop written by hand, and record."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import true_env_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVES = 8  # COLLECT_WAVES
# (E, T, max_episode_steps, num_cells, goal, num_steps)
GRID_CASES = [(1, 40, None, 2, (1, 1), 3), (5, 40, 2, 5, (4, 4), 3), (2 * WAVES + 1, 40, 500, 2, (1, 1), 3), (2 * WAVES + 1, 1, None, 5, (4, 4), 3),
              (5, 0, None, 5, (4, 4), 3), (2 * WAVES + 1, 40, None, 5, (4, 4), 15)]
GRID_IDS = ["E1", "E5-cap2", "E17-cap500", "T1", "T0", "goal44-15steps"]


@pytest.fixture(scope="module")
def gpu():
    from rl_offline_simulation_amd import _lib
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    _lib.load()
    return torch.device("cuda", 0)


def _nets(dO, nA, seed):
    from rl_offline_simulation_amd.evaluators import MLPPolicy, MLPValue
    torch.manual_seed(seed)
    pi = torch.nn.Sequential(torch.nn.Linear(dO, 8), torch.nn.Tanh(), torch.nn.Linear(8, nA))
    v = torch.nn.Sequential(torch.nn.Linear(dO, 8), torch.nn.Tanh(), torch.nn.Linear(8, 1))
    with torch.no_grad():
        pi[0].weight.mul_(3.0)
        pi[2].weight.mul_(3.0)
    return MLPPolicy.from_torch(pi), MLPValue.from_torch(v)


def _tab(nS, dtype, seed=5):
    """pi [nS, 5] that leans up and right, so that episodes reach a far goal"""
    p = np.random.default_rng(seed).dirichlet(np.ones(5), nS) * 0.5 + np.array([0.0, 0.25, 0.25, 0.0, 0.0])
    return (p / p.sum(1, keepdims=True)).astype(dtype)


def _grid(gpu, E, coords, num_cells, goal, num_steps, seed0=100):
    from rl_offline_simulation_amd.evaluators import VectorGridNavi
    env = VectorGridNavi(E, num_cells=num_cells, num_steps=num_steps, goal=goal, coords=coords, device=gpu)
    es, as_ = seed0 + np.arange(E), 7000 + seed0 + np.arange(E)
    env.seed(es)
    env.set_action_seeds(as_)
    host = H.HostVectorEnv("coords" if coords else "grid", es, as_, num_cells=num_cells, num_steps=num_steps, goal=goal)
    return env, host


def _np(x):
    return x.cpu().numpy()


def _check_grid(env, host, col, T, cap):
    """the device's records of one call against the host loop teacher-forced on the recorded probs, and the streams' end positions"""
    probs = _np(col.probs)
    want = host.collect(lambda e, i, obs: probs[i, e], T, cap)
    rec = env.records
    got = dict(obs=col.obs, next_obs=col.next_obs, state=rec.state, next_state=rec.next_state, action=env.drawn_action, reward=col.reward,
               flags=rec.flags, ep_step=rec.ep_step)
    for k, v in got.items():
        g = _np(v)
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, k
        assert np.array_equal(g.view(np.uint8), want[k].view(np.uint8)), k
    fl = want["flags"]
    assert np.array_equal(_np(col.terminated), fl & H.TERMINATED != 0) and np.array_equal(_np(col.truncated), fl & H.TRUNCATED != 0)
    assert np.array_equal(_np(col.reset), fl & H.RESET != 0) and bool(col.alive.all()) and bool((col.status == 0).all())
    E = len(host.envs)
    assert np.array_equal(_np(col.row), (np.arange(E)[None, :] * T + np.arange(T)[:, None]).astype(np.int32))
    assert np.array_equal(_np(col.action), want["action"].astype(np.int64))
    we, wa = host.streams()
    assert np.array_equal(_np(env.rng_env), we) and np.array_equal(_np(env.rng_act), wa)
    assert np.array_equal(_np(env._ep_t), np.array(host.ep_t, np.int32))
    assert np.array_equal(_np(env.step_count), np.array([e.step_count for e in host.envs], np.int32))
    assert np.array_equal(_np(col.final_obs), np.stack([e.obs() for e in host.envs]).reshape(_np(col.final_obs).shape))
    return want


def _check_ppo_records(batch, actor, critic, env, dO):
    """value / final_value to MLPValue.forward bit for bit; logp by the suite's rule"""
    from rl_offline_simulation_amd.evaluators.obs_policy import obs_tensor
    T, E = batch.valid.shape
    dev = batch.val.device
    assert bool(batch.valid.all())
    x = obs_tensor(batch.obs.reshape(T * E, dO), dev)
    assert torch.equal(batch.val, critic.forward(x).reshape(T, E))
    assert torch.equal(batch.final_value, critic.forward(obs_tensor(env.obs.reshape(E, dO), dev)))
    act = batch.act.long()
    pa = batch.collected.probs.gather(2, act.unsqueeze(-1))[..., 0]
    assert float((batch.logp.exp() - pa).abs().max()) <= 1e-6
    if actor is not None:
        h = x.float()
        for i, (W, b) in enumerate(actor.weights):
            h = h @ W.to(dev).T + b.to(dev)
            if i < len(actor.weights) - 1:
                h = torch.tanh(h)
        ls = torch.log_softmax(h.reshape(T, E, -1), -1).gather(2, act.unsqueeze(-1))[..., 0]
        assert float((batch.logp - ls).abs().max()) <= 2e-6


@pytest.mark.parametrize("coords", [True, False], ids=["coords", "cells"])
@pytest.mark.parametrize("case", GRID_CASES, ids=GRID_IDS)
def test_grid_mlp_equals_host_loop(gpu, case, coords):
    from rl_offline_simulation_amd.evaluators.obs_policy import obs_tensor
    E, T, cap, nc, goal, ns = case
    env, host = _grid(gpu, E, coords, nc, goal, ns)
    dO = 2 if coords else 1
    actor, critic = _nets(dO, 5, 1)
    if not coords:  # a cell id is a large input: keep the logits apart but finite
        actor.weights[0] = (actor.weights[0][0] * 0.2, actor.weights[0][1])
    col = env.collect(actor, T, cap)
    assert col.obs.shape[:2] == (T, E) and col.probs.shape == (T, E, 5)
    want = _check_grid(env, host, col, T, cap)
    if T:
        assert torch.equal(col.probs, actor.forward(obs_tensor(col.obs.reshape(T * E, dO), gpu)).reshape(T, E, 5))
        if T > 1:
            assert (want["flags"] & H.RESET).any()
    if cap == 2:
        assert (want["flags"] & H.TRUNCATED).any() and (want["ep_step"] <= 1).all()
    # the PPO form from where the first call left off: the same trajectory rules, the critic's records, and both bootstraps
    for boot in ("reference", "spinup"):
        batch = env.collect_ppo(actor, critic, T, cap, bootstrap=boot)
        _check_grid(env, host, batch.collected, T, cap)
        if T:
            _check_ppo_records(batch, actor, critic, env, dO)
            tr = batch.collected.truncated & ~batch.collected.terminated
            if boot == "spinup":
                vt = critic.forward(obs_tensor(batch.collected.next_obs.reshape(T * E, dO), gpu)).reshape(T, E)
                assert torch.equal(batch.v_trunc[tr], vt[tr]) and bool((batch.v_trunc[~tr] == 0).all())
                assert bool(tr.any()) == (cap == 2)


@pytest.mark.parametrize("coords", [True, False], ids=["coords", "cells"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", [GRID_CASES[1], GRID_CASES[2], GRID_CASES[5]], ids=[GRID_IDS[1], GRID_IDS[2], GRID_IDS[5]])
def test_grid_tabular_equals_host_loop(gpu, case, dtype, coords):
    E, T, cap, nc, goal, ns = case
    env, host = _grid(gpu, E, coords, nc, goal, ns, seed0=300)
    pi = _tab(nc * nc, dtype)
    col = env.collect(pi, T, cap)
    want = _check_grid(env, host, col, T, cap)
    # probs is the f32 value of pi's row at the cell
    assert np.array_equal(_np(col.probs), pi[want["state"]].astype(np.float32))
    if ns == 15:  # the far goal is reached: reward 1 and an episode that ends before num_steps
        assert (want["reward"] == 1.0).any() and ((want["flags"] & H.TERMINATED != 0) & (want["ep_step"] < ns - 1)).any()
    _, critic = _nets(2 if coords else 1, 5, 2)
    batch = env.collect_ppo(pi, critic, T, cap)
    _check_grid(env, host, batch.collected, T, cap)
    _check_ppo_records(batch, None, critic, env, 2 if coords else 1)


def test_grid_carry_over_and_masked_reset(gpu):
    """two calls of T against one call of 2T; reset(mask) between calls"""
    E, T = 2 * WAVES + 1, 20
    actor, _ = _nets(2, 5, 3)
    a, _ = _grid(gpu, E, True, 5, (4, 4), 3)
    b, host = _grid(gpu, E, True, 5, (4, 4), 3)
    one = a.collect(actor, 2 * T, 2)
    first, st1 = b.collect(actor, T, 2), b.records
    second, st2 = b.collect(actor, T, 2), b.records
    for k in ("obs", "probs", "action", "reward", "next_obs", "terminated", "truncated", "reset"):
        assert torch.equal(getattr(one, k), torch.cat([getattr(first, k), getattr(second, k)])), k
    assert torch.equal(a.records.ep_step, torch.cat([st1.ep_step, st2.ep_step])) and torch.equal(a.records.state, torch.cat([st1.state, st2.state]))
    for k in ("rng_env", "rng_act", "state", "step_count", "_ep_t"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    # masked reset: the masked environments start over with two draws of their env stream, the others are untouched
    both = _np(torch.cat([first.probs, second.probs]))
    host.collect(lambda e, i, obs: both[i, e], 2 * T, 2)
    mask = np.arange(E) % 3 == 0
    before = [x.clone() for x in (b.state, b.rng_env, b.step_count, b._ep_t, b.rng_act)]
    obs, alive = b.reset(torch.as_tensor(mask))
    host.reset(mask)
    keep = torch.as_tensor(~mask, device=gpu)
    for x, y in zip(before[:4], (b.state, b.rng_env, b.step_count, b._ep_t)):
        assert torch.equal(x[keep], y[keep])
    assert torch.equal(before[4], b.rng_act) and bool(alive.all())
    assert np.array_equal(_np(obs), np.stack([e.obs() for e in host.envs]))
    col = b.collect(actor, 7, 2)
    _check_grid(b, host, col, 7, 2)


# ---- CartPole ----
def _tolerance():
    rows = [json.loads(x) for x in open(os.path.join(ROOT, "profiles", "true_env_error.jsonl")) if x.strip()]
    worst = max(r["max_dev_eps"] for r in rows if r["what"] == "cartpole next_state")
    return min(8.0 * worst * H.EPS, 1e-12)


def run_cartpole_case(gpu, case, ppo=False):
    """the device's records of one case (also tools/true_env_error_table.py's): (env, actor, critic, collected or batch, seeds)"""
    from rl_offline_simulation_amd.evaluators import VectorCartPole
    E, T, cap, s0 = case
    env = VectorCartPole(E, device=gpu)
    es, as_ = s0 + np.arange(E), 9000 + s0 + np.arange(E)
    env.seed(es)
    env.set_action_seeds(as_)
    actor, critic = _nets(4, 2, 4)
    out = env.collect_ppo(actor, critic, T, cap) if ppo else env.collect(actor, T, cap)
    return env, actor, critic, out, es, as_


@pytest.mark.parametrize("ppo", [False, True], ids=["collect", "collect_ppo"])
@pytest.mark.parametrize("case", H.CARTPOLE_CASES, ids=[f"E{c[0]}-T{c[1]}-cap{c[2]}" for c in H.CARTPOLE_CASES])
def test_cartpole_teacher_forced(gpu, case, ppo):
    from rl_offline_simulation_amd.evaluators.obs_policy import obs_tensor
    E, T, cap, _ = case
    env, actor, critic, out, es, as_ = run_cartpole_case(gpu, case, ppo)
    col = out.collected if ppo else out
    st, nst, act = _np(env.records.state), _np(env.records.next_state), _np(env.drawn_action)
    fl, ep = _np(env.records.flags), _np(env.records.ep_step)
    # the dynamics: the host's f64 step from the device's own state and action
    tol = _tolerance()
    dev = H.cartpole_deviation(st, act, nst)
    print(f"cartpole case {case}: max deviation {dev:.3f} eps, allowed {tol / H.EPS:.3f} eps")
    assert dev * H.EPS <= tol
    # exact, on the device's own records
    assert np.array_equal(_np(col.obs), st.astype(np.float32)) and np.array_equal(_np(col.next_obs), nst.astype(np.float32))
    assert torch.equal(col.probs, actor.forward(obs_tensor(col.obs.reshape(T * E, 4), gpu)).reshape(T, E, 2))
    assert bool((col.reward == 1.0).all()) and bool((col.status == 0).all())
    probs = _np(col.probs)
    capn = 0 if cap is None else cap
    for k in range(E):
        g, ag = np.random.default_rng(int(es[k])), np.random.default_rng(int(as_[k]))
        s, t = -0.05 + 0.1 * g.random(4), 0  # seed()'s reset
        for i in range(T):
            assert np.array_equal(st[i, k], s) and ep[i, k] == t
            assert act[i, k] == H.draw(probs[i, k], ag.random())
            term = H.cartpole_done(nst[i, k])
            t += 1
            trunc = capn > 0 and t >= capn
            want = H.SERVED | H.ALIVE | (H.TERMINATED if term else 0) | (H.TRUNCATED if trunc else 0) | (H.RESET if term or trunc else 0)
            assert fl[i, k] == want, (i, k)
            if term or trunc:
                s, t = -0.05 + 0.1 * g.random(4), 0
            else:
                s = nst[i, k]
        assert np.array_equal(_np(env.state)[k], s) and int(env._ep_t[k]) == t
        assert np.array_equal(_np(env.rng_env)[k], H.stream_words(g)) and np.array_equal(_np(env.rng_act)[k], H.stream_words(ag))
    if T > 1:
        assert (fl & H.RESET).any()
    if ppo:
        _check_ppo_records(out, actor, critic, env, 4)


def test_cartpole_carry_over(gpu):
    from rl_offline_simulation_amd.evaluators import VectorCartPole
    actor, critic = _nets(4, 2, 4)
    envs = []
    for _ in range(2):
        e = VectorCartPole(5, device=gpu)
        e.seed(60 + np.arange(5))
        envs.append(e)
    one = envs[0].collect_ppo(actor, critic, 40, 9)
    st = envs[0].records.state
    halves = [(envs[1].collect_ppo(actor, critic, 20, 9), envs[1].records.state) for _ in range(2)]
    for k in ("obs", "act", "rew", "val", "logp", "valid"):
        assert torch.equal(getattr(one, k), torch.cat([h[0]._asdict()[k] for h in halves])), k
    assert torch.equal(st, torch.cat([h[1] for h in halves])) and torch.equal(one.final_value, halves[1][0].final_value)
    for k in ("rng_env", "rng_act", "state", "_ep_t"):
        assert torch.equal(getattr(envs[0], k), getattr(envs[1], k)), k


# ---- population and fit ----
@pytest.mark.parametrize("kind", ["coords", "cartpole"])
def test_population_equals_single_learners(gpu, kind):
    from rl_offline_simulation_amd.evaluators import PPOPopulation, VectorCartPole, VectorGridNavi
    nl, E, T, cap = 3, 2, 24, 5
    dO, nA = (2, 5) if kind == "coords" else (4, 2)
    nets = [_nets(dO, nA, 40 + l) for l in range(nl)]
    mk = (lambda n: VectorGridNavi(n, num_steps=3, device=gpu)) if kind == "coords" else (lambda n: VectorCartPole(n, device=gpu))
    env = mk(nl * E)
    es, as_ = 500 + np.arange(nl * E), 800 + np.arange(nl * E)
    env.seed(es)
    env.set_action_seeds(as_)
    pop = PPOPopulation([n[0] for n in nets], [n[1] for n in nets])
    for boot in ("reference", "spinup"):
        batch = env.collect_ppo_population(pop, T, cap, bootstrap=boot)
        rec = env.records
        for l in range(nl):
            sl = slice(l * E, (l + 1) * E)
            one = mk(E)
            one.seed(es[sl])
            one.set_action_seeds(as_[sl])
            if boot == "spinup":  # the second call goes on from the first one's state
                one.collect_ppo(nets[l][0], nets[l][1], T, cap, bootstrap="reference")
            b = one.collect_ppo(nets[l][0], nets[l][1], T, cap, bootstrap=boot)
            for f in ("obs", "act", "rew", "val", "logp", "adv", "adv_raw", "ret", "valid", "v_trunc"):
                x, y = getattr(batch, f), getattr(b, f)
                assert (x is None and y is None) or torch.equal(x[:, sl], y), (f, l)
            assert torch.equal(batch.final_value[sl], b.final_value)
            assert torch.equal(rec.state[:, sl], one.records.state) and torch.equal(rec.flags[:, sl], one.records.flags)
            for f in ("rng_env", "rng_act", "state", "_ep_t", "step_count"):
                assert torch.equal(getattr(env, f)[sl], getattr(one, f)), (f, l)


def test_fit_equals_the_hand_written_loop(gpu):
    from rl_offline_simulation_amd.evaluators import EpisodeTracker, PPOLearner, VectorGridNavi, ppo_epoch_log
    E, T = 4, 16
    runs = []
    for hand in (False, True):
        actor, critic = _nets(2, 5, 9)
        env = VectorGridNavi(E, num_steps=5, goal=(1, 1), device=gpu)
        env.seed(40 + np.arange(E))
        learner = PPOLearner(actor, critic, train_pi_iters=4, train_v_iters=4)
        if not hand:
            log = learner.fit(env, epochs=2, T=T)
            runs.append((log, actor, critic, env))
            continue
        tracker = EpisodeTracker(E, gpu)
        logs, infos = [], []
        for _ in range(2):
            b = env.collect_ppo(actor, critic, T)
            logs.append(ppo_epoch_log(b, tracker))
            infos.append(learner.update(b))
        runs.append(((logs, infos), actor, critic, env))
    (log, a0, c0, e0), ((logs, infos), a1, c1, e1) = runs
    for rows in (logs, infos):
        for k in rows[0]._fields:
            x, y = getattr(log, k), torch.stack([getattr(z, k) for z in rows])
            assert x.dtype == y.dtype and x.shape == y.shape, k
            assert torch.equal(x, y) or (x.is_floating_point() and torch.equal(x.nan_to_num(nan=-7.0), y.nan_to_num(nan=-7.0))), k
    assert int(log.StepsServed.sum()) == 2 * T * E
    for n0, n1 in ((a0, a1), (c0, c1)):
        for (W0, b0), (W1, b1) in zip(n0._device_weights(gpu)[0], n1._device_weights(gpu)[0]):
            assert torch.equal(W0, W1) and torch.equal(b0, b1)
    assert torch.equal(e0.state, e1.state) and torch.equal(e0.rng_act, e1.rng_act)


# ---- record ----
@pytest.mark.parametrize("coords", [True, False], ids=["coords", "cells"])
def test_record_equals_host_record_and_builds_a_psrs(gpu, coords):
    from rl_offline_simulation_amd.evaluators import VectorPSRS
    E, N, cap = 5, 183, 6
    env, host = _grid(gpu, E, coords, 5, (1, 1), 4, seed0=900)
    pi = _tab(25, np.float32, seed=8)
    ds = env.record(pi, N, cap)
    want = host.record(lambda e, i, obs: pi[int(host.envs[e].z)], N, cap)
    assert set(ds.experience) == set(want) and len(ds) == N
    for k, v in want.items():
        g = ds.experience[k]
        assert g.dtype == v.dtype and g.shape == v.shape and np.array_equal(g, v), k
    # the dataset goes straight into a simulator that serves rows
    if coords:
        class Cells:
            def encode(self, x):
                x = np.asarray(x, np.float64)
                return (np.floor(x[:, 0] * 5 + 1e-6).clip(0, 4) + 5 * np.floor(x[:, 1] * 5 + 1e-6).clip(0, 4)).astype(np.int64)
        sim = VectorPSRS(ds, num_envs=3, num_states=25, encoder=Cells(), device=gpu)
        policy = _nets(2, 5, 11)[0]
    else:
        sim = VectorPSRS(ds, num_envs=3, device=gpu)
        policy = _tab(25, np.float64, seed=8)
    sim.reset_sampler([1, 2, 3])
    sim.reset()
    col = sim.collect(policy, 10, cap)
    assert int((col.row >= 0).sum()) > 0


def test_record_cartpole_with_a_network(gpu):
    """record logs any policy collect takes: a CartPole log from an MLP actor, its rows chained and its probs the actor's"""
    from rl_offline_simulation_amd.evaluators import VectorCartPole
    from rl_offline_simulation_amd.evaluators.obs_policy import obs_tensor
    env = VectorCartPole(7, device=gpu)
    env.seed(70 + np.arange(7))
    actor, _ = _nets(4, 2, 4)
    ds = env.record(actor, 300, 30)
    e = ds.experience
    assert len(ds) == 300 and e["observations"].dtype == np.float32 and e["observations"].shape == (300, 4)
    assert np.array_equal(e["episode_ids"], np.cumsum(e["steps"] == 0) - 1) and e["steps"][0] == 0
    p = actor.forward(obs_tensor(e["observations"], gpu)).cpu().numpy()
    assert np.array_equal(p, e["action_distributions"])
    ends = e["terminals"] | e["truncateds"]
    T = -(-300 // 7)
    for i in range(299):
        if (i + 1) % T == 0:
            continue  # the next row is another environment's
        if ends[i]:
            assert e["steps"][i + 1] == 0
        else:
            assert e["steps"][i + 1] == e["steps"][i] + 1 and np.array_equal(e["observations"][i + 1], e["next_observations"][i])
    assert ends.any() and (e["steps"] < 30).all()
