"""VectorPSRS.collect_ppo (offsim_vector_collect_ppo + offsim_ppo_advantages) and MLPValue (offsim_value_mlp): the critic forward against torch,
the in-kernel critic against MLPValue.forward bit for bit, the trajectory against collect's, logp against torch, the buffer against the
reference's PPO agent (tests/golden/ppo/*.npz) and its NumPy restatement (tests/ppo_host.py), and the edges."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_host as H  # noqa: E402
from test_gpu_collect import _cartpole, _env, _grid, _mlp, _state, _twins  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ppo", "*.npz")))
TOL = 1e-4


@pytest.fixture(scope="module")
def gpu():
    from rl_offline_simulation_amd import _lib
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    _lib.load()
    return torch.device("cuda", 0)


def _critic(dO, depth, act, seed=0, hidden=32):
    from rl_offline_simulation_amd.evaluators import MLPValue
    torch.manual_seed(100 + seed)
    kind = {"tanh": torch.nn.Tanh, "relu": torch.nn.ReLU, "leaky_relu": lambda: torch.nn.LeakyReLU(0.05)}[act]
    mods, w = [], dO
    for _ in range(depth - 1):
        mods += [torch.nn.Linear(w, hidden), kind()]
        w = hidden
    mods += [torch.nn.Linear(w, 1), torch.nn.Identity()]
    return torch.nn.Sequential(*mods), MLPValue.from_torch(torch.nn.Sequential(*mods))


def _close(got, want, tol=TOL):
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    return bool(((got - want).abs() <= tol * want.abs().clamp(min=1.0)).all())


# ---- 1. the critic forward ----
@pytest.mark.parametrize("depth,hidden,act,xdt", [(1, 8, "tanh", torch.float32), (2, 256, "relu", torch.float32), (3, 64, "tanh", torch.float16),
                                                  (4, 100, "leaky_relu", torch.float32), (4, 17, "tanh", torch.float16)])
def test_value_forward_matches_torch(gpu, depth, hidden, act, xdt):
    from rl_offline_simulation_amd.evaluators import MLPValue
    net, _ = _critic(9, depth, act, hidden=hidden)
    v = MLPValue.from_torch(net)
    x = (torch.randn(1000, 9, generator=torch.Generator().manual_seed(depth)) * 2).to(xdt)
    rows = torch.randint(0, 1000, (777,), generator=torch.Generator().manual_seed(1), dtype=torch.int32)
    got = v.forward(x.to(gpu), rows.to(gpu))
    with torch.no_grad():
        ref = net.double()(x.double())[:, 0][rows.long()]
    scale = float(ref.abs().max()) + 1.0
    assert got.shape == (777,) and got.dtype == torch.float32
    assert float((got.double().cpu() - ref).abs().max()) <= 1e-5 * scale
    assert v.forward(x[:0].to(gpu)).shape == (0,)


# ---- 2. collect_ppo against collect ----
def _spinup_pair(dO, nA, seed=0, hidden=16):
    """spinup-shaped actor and critic (mlp() with its trailing Identity), tanh"""
    from rl_offline_simulation_amd.evaluators import MLPPolicy, MLPValue
    torch.manual_seed(seed)
    pi = torch.nn.Sequential(torch.nn.Linear(dO, hidden), torch.nn.Tanh(), torch.nn.Linear(hidden, hidden), torch.nn.Tanh(),
                             torch.nn.Linear(hidden, nA), torch.nn.Identity())
    v = torch.nn.Sequential(torch.nn.Linear(dO, hidden), torch.nn.Tanh(), torch.nn.Linear(hidden, hidden), torch.nn.Tanh(),
                            torch.nn.Linear(hidden, 1), torch.nn.Identity())
    with torch.no_grad():
        pi[0].weight.mul_(3.0)
    return MLPPolicy.from_torch(pi), MLPValue.from_torch(v), pi, v


CASES = [  # (rejection, p_log dtype, actor form, critic form, cap)
    ("pcg64", np.float32, "mlp", "mlp", 20),
    ("philox", np.float64, "mlp", "rows", 7),
    ("pcg64", np.float64, "rows", "mlp", 11),
    ("philox", np.float32, "rows", "rows", None),
    ("philox", np.float32, "mlp", "mlp", 9),
    ("pcg64", np.float64, "tabular", "mlp", 6),
    ("pcg64", np.float32, "tabular", "rows", 6),
]


@pytest.mark.parametrize("rejection,plog,actor_form,critic_form,cap", CASES)
def test_collect_ppo_keeps_collects_trajectory_and_records_the_critic(gpu, rejection, plog, actor_form, critic_form, cap):
    from rl_offline_simulation_amd.evaluators import RowPolicy, RowValue
    from rl_offline_simulation_amd.evaluators.obs_policy import obs_tensor
    E, T = 37, 200
    if actor_form == "tabular":  # observations are states
        g = _grid()
        d = dict(g, obs=g["z"], next_obs=g["z_next"], p_log=g["p_log"].astype(plog))
        a, b = _twins(d, E, np.arange(E) % 11, rejection, discrete=True)
        actor = np.random.default_rng(0).dirichlet(np.ones(5), size=int(max(d["z"].max(), d["z_next"].max())) + 1)
        _, critic, _, vnet = _spinup_pair(1, 5, seed=4)
        dO, nA = 1, 5
    else:
        d = _cartpole(3000, 4, plog)
        a, b = _twins(d, E, np.arange(E) % 11, rejection)
        actor, critic, _, vnet = _spinup_pair(4, 2, seed=1)
        dO, nA = 4, 2
    xn, x0 = obs_tensor(a._next_obs, gpu), obs_tensor(a._obs, gpu)
    if actor_form == "rows":
        actor = RowPolicy(actor.forward(xn), actor.forward(x0))
    if critic_form == "rows":
        crit = RowValue(critic.forward(xn), critic.forward(x0))
    else:
        crit = critic
    boot = "spinup" if cap and cap < 10 else "reference"
    p = a.collect_ppo(actor, crit, T, max_episode_steps=cap, bootstrap=boot)
    c = b.collect(actor, T, max_episode_steps=cap)
    for f in ("row", "obs", "probs", "terminated", "truncated", "reset", "alive", "final_obs", "status"):
        assert torch.equal(getattr(p.collected, f), getattr(c, f)), f
    for x, y in zip(_state(a), _state(b)):
        assert torch.equal(x, y)
    assert torch.equal(a._ep_t, b._ep_t)
    v = p.valid
    assert int(v.sum()) > E * T // 10
    # the in-kernel critic is MLPValue.forward, bit for bit, at the observations asked at / held at the end / next_obs of truncating rows
    want = critic.forward(obs_tensor(p.obs.reshape(T * E, dO), gpu)).reshape(T, E)
    assert torch.equal(p.val[v], want[v]) and bool((p.val[~v] == 0).all())
    assert torch.equal(p.final_value, critic.forward(obs_tensor(a.obs, gpu)))
    if boot == "spinup":
        tr = p.collected.truncated & ~p.collected.terminated
        assert bool(tr.any())
        vt = critic.forward(xn)[p.collected.row.clamp(min=0).long()]
        assert torch.equal(p.v_trunc[tr], vt[tr]) and bool((p.v_trunc[~tr] == 0).all())
    # logp of the served action
    act = p.act.long()
    pa = p.collected.probs.gather(2, act.unsqueeze(-1))[..., 0]
    assert float((p.logp.exp() - pa)[v].abs().max()) <= 1e-6
    if actor_form == "mlp":
        logits = _logits(actor, obs_tensor(p.obs.reshape(T * E, dO), gpu)).reshape(T, E, nA)
        ls = torch.log_softmax(logits, -1).gather(2, act.unsqueeze(-1))[..., 0]
        assert float((p.logp - ls)[v].abs().max()) <= 2e-6
    # the buffer is ppo_host's over the records
    host_check(p, 0.99, 0.97, boot)


def _logits(mlp, x):
    """the actor's logits in torch (f32) from its weights"""
    h = x.float()
    for k, (W, b) in enumerate(mlp.weights):
        h = h @ W.to(h.device).t() + (0 if b is None else b.to(h.device))
        if k < len(mlp.weights) - 1:
            h = torch.tanh(h) if mlp.activation == "tanh" else torch.relu(h)
    return h


def host_check(p, gamma, lam, boot):
    t = lambda x: x.cpu().numpy()
    col = p.collected
    adv, ret, norm, mean, std = H.batch(t(p.rew).astype(np.float64), t(p.val).astype(np.float64), t(col.terminated), t(col.truncated), t(p.valid),
                                        t(p.final_value).astype(np.float64), gamma, lam, boot,
                                        None if p.v_trunc is None else t(p.v_trunc).astype(np.float64))
    assert _close(p.adv_raw, adv) and _close(p.ret, ret)
    assert _close(p.adv_mean, mean) and _close(p.adv_std, std)
    assert _close(p.adv, norm)


# ---- 3. the reference's PPO agent ----
def _fixture_env(f, E):
    d = {k: f[k] for k in ("obs", "next_obs", "z", "z_next", "a", "r", "done", "p_log", "t0")}
    return _env(**d, E=E)


def _nets(f):
    from rl_offline_simulation_amd.evaluators import MLPPolicy, MLPValue
    n = len([k for k in f.files if k.startswith("pi_W")])
    return (MLPPolicy([(f[f"pi_W{k}"], f[f"pi_b{k}"]) for k in range(n)], "tanh"),
            MLPValue([(f[f"v_W{k}"], f[f"v_b{k}"]) for k in range(n)], "tanh"))


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_reference_agent_one_environment_per_seed(gpu, path):
    f = np.load(path)
    T, cap, gamma, lam = int(f["T"]), int(f["cap"]), float(f["gamma"]), float(f["lam"])
    actor, critic = _nets(f)
    for s in f["seeds"]:
        env = _fixture_env(f, 1)
        env.reset_sampler([int(s)])
        env.reset()
        for j in range(2):
            p = env.collect_ppo(actor, critic, T, max_episode_steps=cap, gamma=gamma, lam=lam)
            sl = slice(j * T, (j + 1) * T)
            assert np.array_equal(p.collected.row[:, 0].cpu().numpy(), f[f"rows_{s}"][sl]), (s, j)
            for k, mine in (("val", p.val), ("logp", p.logp), ("adv_raw", p.adv_raw), ("ret", p.ret), ("adv", p.adv)):
                assert _close(mine[:, 0], f[f"{k}_{s}_{j}"]), (s, j, k)
            assert _close(p.adv_mean, f[f"adv_mean_{s}_{j}"]) and _close(p.adv_std, f[f"adv_std_{s}_{j}"])
            lv = float(f[f"last_val_{s}_{j}"])
            if not np.isnan(lv):  # the epoch cut an episode: its bootstrap is final_value
                assert _close(p.final_value[0], lv)


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_reference_agent_all_seeds_at_once(gpu, path):
    f = np.load(path)
    T, cap, gamma, lam = int(f["T"]), int(f["cap"]), float(f["gamma"]), float(f["lam"])
    actor, critic = _nets(f)
    seeds = [int(s) for s in f["seeds"]]
    env = _fixture_env(f, len(seeds))
    env.reset_sampler(seeds)
    env.reset()
    for j in range(2):
        p = env.collect_ppo(actor, critic, T, max_episode_steps=cap, gamma=gamma, lam=lam)
        for e, s in enumerate(seeds):
            assert np.array_equal(p.collected.row[:, e].cpu().numpy(), f[f"rows_{s}"][j * T:(j + 1) * T]), (s, j)
            for k, mine in (("val", p.val), ("logp", p.logp), ("adv_raw", p.adv_raw), ("ret", p.ret)):
                assert _close(mine[:, e], f[f"{k}_{s}_{j}"]), (s, j, k)
        host_check(p, gamma, lam, "reference")  # the normalisation is global over all environments
        fl = p.flat()
        assert fl["adv"].shape == (T * len(seeds),) and torch.equal(fl["adv"][:T], p.adv[:, 0]) and torch.equal(fl["obs"][T:2 * T], p.obs[:, 1])


# ---- 4. the buffer kernels on their own ----
@pytest.mark.parametrize("T,E,boot", [(1, 1, "reference"), (1, 300, "spinup"), (57, 513, "reference"), (200, 256, "spinup"), (33, 7, "reference")])
def test_ppo_advantages_matches_host(gpu, T, E, boot):
    from rl_offline_simulation_amd.evaluators import ppo_advantages
    g = np.random.default_rng(T * 1000 + E)
    rew, val = g.standard_normal((T, E)).astype(np.float32), g.standard_normal((T, E)).astype(np.float32)
    term, trunc = g.random((T, E)) < 0.1, g.random((T, E)) < 0.05
    valid = np.ones((T, E), bool)
    stop = g.integers(0, T + 1, E)  # environments stop after `stop` valid steps
    valid &= np.arange(T)[:, None] < stop[None, :]
    valid[:, : min(3, E)] = False if E > 3 else valid[:, : min(3, E)]  # all-invalid columns
    fv, vt = g.standard_normal(E).astype(np.float32), g.standard_normal((T, E)).astype(np.float32)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(gpu)
    out = ppo_advantages(dev(rew), dev(val), dev(term), dev(trunc), dev(valid), dev(fv), dev(vt) if boot == "spinup" else None, gamma=0.97,
                         lam=0.9, bootstrap=boot)
    adv, ret, norm, mean, std = H.batch(rew.astype(np.float64), val.astype(np.float64), term, trunc, valid, fv.astype(np.float64), 0.97, 0.9, boot,
                                        vt.astype(np.float64))
    assert _close(out.adv_raw, adv) and _close(out.ret, ret) and _close(out.mean, mean) and _close(out.std, std)
    if valid.sum() > 1:
        assert _close(out.adv, norm)
    assert bool((out.adv_raw[~dev(valid)] == 0).all())
    again = ppo_advantages(dev(rew), dev(val), dev(term), dev(trunc), dev(valid), dev(fv), dev(vt) if boot == "spinup" else None, gamma=0.97,
                           lam=0.9, bootstrap=boot)
    assert torch.equal(again.adv, out.adv) and torch.equal(again.std, out.std)  # fixed reduction order
    # nothing valid: unnormalised, std 0
    none = ppo_advantages(dev(rew), dev(val), dev(term), dev(trunc), dev(np.zeros((T, E), bool)), dev(fv), dev(vt), bootstrap=boot)
    assert float(none.std) == 0.0 and bool((none.adv == 0).all())


# ---- 5. determinism and the edges ----
def test_two_runs_are_bit_identical(gpu):
    d = _cartpole(3000, 4, np.float32)
    actor, critic, _, _ = _spinup_pair(4, 2, seed=3)
    outs = []
    for _ in range(2):
        env = _twins(d, 300, np.arange(300))[0]
        outs.append(env.collect_ppo(actor, critic, 64, max_episode_steps=13))
    for k in ("val", "logp", "adv", "adv_raw", "ret", "final_value", "adv_mean", "adv_std"):
        assert torch.equal(getattr(outs[0], k), getattr(outs[1], k)), k


def test_zero_steps_and_split_calls(gpu):
    from rl_offline_simulation_amd.evaluators.obs_policy import obs_tensor
    d = _cartpole(3000, 4, np.float32)
    actor, critic, _, _ = _spinup_pair(4, 2, seed=5)
    a, b = _twins(d, 19, np.arange(19) + 2)
    before = _state(a)
    p0 = a.collect_ppo(actor, critic, 0)
    assert p0.val.shape == (0, 19) and p0.adv.shape == (0, 19) and float(p0.adv_std) == 0.0
    for x, y in zip(before, _state(a)):
        assert torch.equal(x, y)
    # collect_ppo, step_and_reset, collect, collect_ppo == collect of the whole length (rows), state carried over
    r1 = a.collect_ppo(actor, critic, 30, max_episode_steps=None).collected.row
    rs = []
    for _ in range(5):
        a.step_and_reset(actor.forward(obs_tensor(a.obs, gpu)))
        rs.append(torch.where(a.env._status == 0, a.env._row, torch.full_like(a.env._row, -1)))
    r3 = a.collect(actor, 20).row
    r4 = a.collect_ppo(actor, critic, 25, max_episode_steps=None).collected.row
    c = b.collect(actor, 80)
    assert torch.equal(torch.cat([r1, torch.stack(rs), r3, r4]), c.row)
    for x, y in zip(_state(a), _state(b)):
        assert torch.equal(x, y)


def test_exhaustion_empty_init_and_keyerror(gpu):
    from rl_offline_simulation_amd import _lib as L
    _, critic, _, _ = _spinup_pair(2, 5, seed=6)
    actor = _mlp(2, 5, 2, "tanh", seed=1)
    for d, cap in ((_grid(every_row_initial=True), None), (_grid(), 3), (_grid(keyerror=True), None)):
        E, T = 8, 400
        a, b = _twins(d, E, np.arange(E))
        p = a.collect_ppo(actor, critic, T, max_episode_steps=cap)
        c = b.collect(actor, T, max_episode_steps=cap)
        assert torch.equal(p.collected.row, c.row) and torch.equal(p.collected.status, c.status)
        st = p.collected.status.cpu().numpy()
        assert set(st) <= {L.ST_EXHAUSTED, L.ST_NO_INIT, L.ST_KEYERROR}
        # every environment stopped: its open path bootstraps with v at the observation it stopped at (obs buffer, unchanged since)
        from rl_offline_simulation_amd.evaluators.obs_policy import obs_tensor
        assert torch.equal(p.final_value, critic.forward(obs_tensor(a.obs, gpu)))
        host_check(p, 0.99, 0.97, "reference")
    strict = _twins(_grid(keyerror=True), 6, np.arange(6), strict=True)[0]
    with pytest.raises(KeyError):
        strict.collect_ppo(actor, critic, 300)


def test_lds_budget_and_sixteen_actions(gpu):
    from rl_offline_simulation_amd import _lib as L
    from rl_offline_simulation_amd.evaluators import MLPPolicy, MLPValue
    d = _cartpole(2000, 126, np.float32)
    g = torch.Generator().manual_seed(0)
    W1, W2 = torch.randn(128, 126, generator=g) * 0.1, torch.randn(2, 128, generator=g)
    actor = MLPPolicy([(W1, None), (W2, None)])  # the whole budget
    env = _twins(d, 4, np.arange(4))[0]
    with pytest.raises(L.OffsimError, match="OFFSIM_COLLECT_MLP_MAX_FLOATS"):
        env.collect_ppo(actor, MLPValue([(torch.ones(1, 126), None)]), 5)
    # sixteen actions: the MLP actor's logp against torch, the MLP critic beside it
    from rl_offline_simulation_amd import synth
    e = synth.synth_iid(4000, 20, 16, seed=3)
    obs = np.stack([e["z"], e["z"] * 0.25], 1).astype(np.float32)
    nobs = np.stack([e["z_next"], e["z_next"] * 0.25], 1).astype(np.float32)
    env = _env(obs=obs, next_obs=nobs, z=e["z"], z_next=e["z_next"], a=e["actions"], r=e["rewards"], done=e["terminals"],
               p_log=e["action_distributions"], t0=e["steps"] == 0, E=16)
    env.reset_sampler(np.arange(16))
    env.reset()
    actor = _mlp(2, 16, 2, "tanh", seed=8)
    _, critic, _, _ = _spinup_pair(2, 16, seed=9)
    p = env.collect_ppo(actor, critic, 50, max_episode_steps=10)
    v = p.valid
    assert int(v.sum()) > 0
    from rl_offline_simulation_amd.evaluators.obs_policy import obs_tensor
    ls = torch.log_softmax(_logits(actor, obs_tensor(p.obs.reshape(-1, 2), gpu)).reshape(50, 16, 16), -1)
    assert float((p.logp - ls.gather(2, p.act.long().unsqueeze(-1))[..., 0])[v].abs().max()) <= 2e-6

