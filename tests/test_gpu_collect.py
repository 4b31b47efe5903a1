"""VectorPSRS.collect (offsim_vector_collect): T steps of policy -> PSRS.step -> reset in one launch, against the driver loop it replaces
(policy forward, step_and_reset, reset of the truncated environments, one step counter), against its own table form, across split calls,
on the reference's fixtures (tests/golden/collect/*.npz), at the edges (exhaustion, empty init queue, KeyError, T = 0) and at the LDS
budget of the in-wave network."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import collect_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "collect", "*.npz")))


@pytest.fixture(scope="module")
def gpu():
    from rl_offline_simulation_amd import _lib
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    _lib.load()
    return torch.device("cuda", 0)


class _LookupEncoder:
    """Latent states given with the log: encode(observations) -> z, encode(next_observations) -> z_next."""

    def __init__(self, obs, z, next_obs, z_next):
        self.pairs = [(np.asarray(obs), np.asarray(z)), (np.asarray(next_obs), np.asarray(z_next))]

    def encode(self, x):
        for a, z in self.pairs:
            if np.array_equal(np.asarray(x), a):
                return z
        raise AssertionError("unknown observations")


def _env(obs, next_obs, z, z_next, a, r, done, p_log, t0, E, strict=False, discrete=False):
    from rl_offline_simulation_amd import OfflineDataset, ProbDistribution, spaces
    from rl_offline_simulation_amd.evaluators import VectorPSRS
    nA = p_log.shape[1]
    n_states = int(max(np.max(z), np.max(z_next))) + 1
    ospace = spaces.Discrete(n_states) if discrete else spaces.Box(low=-np.inf, high=np.inf, shape=tuple(obs.shape[1:]), dtype=obs.dtype)
    ds = OfflineDataset(observation_space=ospace, action_space=spaces.Discrete(nA), action_dist_type=ProbDistribution.Discrete,
                        observations=obs, actions=a, action_distributions=p_log, rewards=r, next_observations=next_obs, terminals=done,
                        steps=np.where(t0, 0, 1))
    if discrete:
        return VectorPSRS(ds, num_envs=E, strict=strict)
    return VectorPSRS(ds, num_envs=E, num_states=n_states, encoder=_LookupEncoder(obs, z, next_obs, z_next), strict=strict)


def _cartpole(N, dO, plog, seed=0):
    """CartPole log with its box-encoded states; observations projected to dO features (dO = 4: the raw ones)."""
    from rl_offline_simulation_amd import synth
    from rl_offline_simulation_amd.encoders import CartpoleBoxEncoder
    e = synth.cartpole_log(N, seed=seed)
    enc = CartpoleBoxEncoder()
    z, zn = np.asarray(enc.encode(e["observations"])), np.asarray(enc.encode(e["next_observations"]))
    obs, nobs = e["observations"], e["next_observations"]
    if dO != 4:
        P = np.random.default_rng(7).standard_normal((4, dO)).astype(np.float32)
        obs, nobs = (obs @ P).astype(np.float32), (nobs @ P).astype(np.float32)
    return dict(obs=obs, next_obs=nobs, z=z, z_next=zn, a=e["actions"], r=e["rewards"], done=e["terminals"],
                p_log=e["action_distributions"].astype(plog), t0=e["steps"] == 0)


def _mlp(dO, nA, depth, act, seed=0, hidden=32):
    from rl_offline_simulation_amd.evaluators import MLPPolicy
    torch.manual_seed(seed)
    mods, w = [], dO
    kind = {"tanh": torch.nn.Tanh, "relu": torch.nn.ReLU}[act]
    for _ in range(depth - 1):
        mods += [torch.nn.Linear(w, hidden), kind()]
        w = hidden
    mods.append(torch.nn.Linear(w, nA))
    net = torch.nn.Sequential(*mods)
    with torch.no_grad():
        for m in net:
            if isinstance(m, torch.nn.Linear):
                m.weight.mul_(3.0)
    return MLPPolicy.from_torch(net)


def _state(env):
    s = env.env.state
    return [x.clone() for x in (env.obs, env.alive, s.cur_slot, s.cursor, s.init_cursor, s.rng)]


def _loop(env, mlp, T, cap):
    """The driver loop collect replaces, on a twin environment: probs = mlp.forward(obs); step_and_reset(probs); reset(mask=truncated)."""
    from rl_offline_simulation_amd import _lib as L
    from rl_offline_simulation_amd.evaluators.obs_policy import obs_tensor
    E = env.num_envs
    ep_t = env._ep_t.clone()
    dead = torch.zeros(E, dtype=torch.bool, device=env.obs.device)
    rows, flags, obs, probs = [], [], [], []
    for _ in range(T):
        o = env.obs.clone()
        p = mlp.forward(obs_tensor(env.obs, env.obs.device))
        live = (env.env.state.cur_slot >= 0) & ~dead
        env.step_and_reset(p)
        st = env.env._status.clone()
        row = env.env._row.clone()
        served = st == L.ST_OK
        dead |= live & ~served
        term = served & env.done
        ep_t = torch.where(served, ep_t + 1, ep_t)
        trunc = served & (cap > 0) & (ep_t >= cap)
        env.reset(mask=trunc & ~term)
        ep_t = torch.where(term | trunc, torch.zeros_like(ep_t), ep_t)
        rst = (term | trunc) & (env.env.state.cur_slot >= 0)
        f = (served.to(torch.int32) * L.COLLECT_SERVED + term.to(torch.int32) * L.COLLECT_TERMINATED + trunc.to(torch.int32) * L.COLLECT_TRUNCATED
             + rst.to(torch.int32) * L.COLLECT_RESET + (served & env.alive).to(torch.int32) * L.COLLECT_ALIVE)
        rows.append(torch.where(served, row, torch.full_like(row, -1)))
        flags.append(f.to(torch.uint8))
        obs.append(o)
        probs.append(p)
    return torch.stack(rows), torch.stack(flags), torch.stack(obs), torch.stack(probs), ep_t


def _twins(d, E, seeds, rejection="pcg64", **kw):
    envs = [_env(**d, E=E, **kw) for _ in range(2)]
    for env in envs:
        env.reset_sampler(seeds, rejection=rejection)
        env.reset()
    return envs


CASES = [  # (rejection, p_log dtype, activation, depth, dO, cap)
    ("pcg64", np.float32, "tanh", 3, 4, 20),
    ("pcg64", np.float64, "relu", 2, 4, None),
    ("philox", np.float32, "relu", 1, 2, 7),
    ("philox", np.float64, "tanh", 3, 128, 15),
    ("pcg64", np.float64, "tanh", 1, 128, None),
    ("pcg64", np.float32, "relu", 3, 2, 500),
]


@pytest.mark.parametrize("rejection,plog,act,depth,dO,cap", CASES)
def test_mlp_collect_equals_the_driver_loop(gpu, rejection, plog, act, depth, dO, cap):
    d = _cartpole(3000, dO, plog)
    E, T = 37, 240
    seeds = np.arange(E) % 11
    a, b = _twins(d, E, seeds, rejection)
    mlp = _mlp(dO, 2, depth, act, seed=depth)
    c = a.collect(mlp, T, max_episode_steps=cap)
    rows, flags, obs, probs, ep_t = _loop(b, mlp, T, 0 if cap is None else cap)
    assert torch.equal(c.row, rows)
    assert torch.equal(_flags(c), flags)
    served = (flags & 1) != 0
    assert torch.equal(c.obs[served], obs[served])
    assert torch.equal(c.probs[served], probs[served])  # bit for bit: the in-wave forward is offsim_policy_mlp's arithmetic
    for x, y in zip(_state(a), _state(b)):
        assert torch.equal(x, y)
    alive = a.alive
    assert torch.equal(a._ep_t[alive], ep_t[alive])
    assert int(served.sum()) > E * T // 2
    if cap and cap < 50:
        assert bool(c.truncated.any())
    # gathered columns
    sv = c.row >= 0
    assert torch.equal(c.action[sv], a._a[c.row[sv].long()]) and torch.equal(c.next_obs[sv], a._next_obs[c.row[sv].long()])
    assert torch.equal(c.final_obs, a.obs)


def _flags(c):
    from rl_offline_simulation_amd import _lib as L
    return ((c.row >= 0).to(torch.int32) * L.COLLECT_SERVED + c.terminated.to(torch.int32) * L.COLLECT_TERMINATED
            + c.truncated.to(torch.int32) * L.COLLECT_TRUNCATED + c.reset.to(torch.int32) * L.COLLECT_RESET
            + c.alive.to(torch.int32) * L.COLLECT_ALIVE).to(torch.uint8)


@pytest.mark.parametrize("plog", [np.float32, np.float64])
def test_mlp_form_equals_table_form(gpu, plog):
    from rl_offline_simulation_amd.evaluators import RowPolicy
    d = _cartpole(3000, 4, plog)
    E, T = 64, 300
    a, b = _twins(d, E, np.arange(E))
    mlp = _mlp(4, 2, 3, "tanh", seed=3)
    c1 = a.collect(mlp, T, max_episode_steps=25)
    c2 = b.collect(mlp, T, max_episode_steps=25, form="rows")
    for f in ("row", "obs", "probs", "terminated", "truncated", "reset", "alive", "final_obs", "status"):
        assert torch.equal(getattr(c1, f), getattr(c2, f)), f
    for x, y in zip(_state(a), _state(b)):
        assert torch.equal(x, y)
    # a RowPolicy of the same per-row probabilities (caller order) is the same table form
    xn = torch.from_numpy(d["next_obs"]).to(gpu)
    x0 = torch.from_numpy(d["obs"]).to(gpu)
    c3_env = _twins(d, E, np.arange(E))[0]
    c3 = c3_env.collect(RowPolicy(mlp.forward(xn), mlp.forward(x0)), T, max_episode_steps=25)
    assert torch.equal(c3.row, c1.row) and torch.equal(c3.probs, c1.probs)


def test_split_calls_and_interleaving(gpu):
    d = _cartpole(3000, 4, np.float32)
    E = 29
    mlp = _mlp(4, 2, 2, "tanh", seed=5)
    a, b = _twins(d, E, np.arange(E) + 3)
    c1, c2 = a.collect(mlp, 70, max_episode_steps=9), a.collect(mlp, 130, max_episode_steps=9)
    c = b.collect(mlp, 200, max_episode_steps=9)
    assert torch.equal(torch.cat([c1.row, c2.row]), c.row)
    assert torch.equal(torch.cat([c1.probs, c2.probs]), c.probs)
    assert torch.equal(torch.cat([_flags(c1), _flags(c2)]), _flags(c))
    for x, y in zip(_state(a), _state(b)):
        assert torch.equal(x, y)
    assert torch.equal(a._ep_t, b._ep_t)
    # collect, a few step_and_reset iterations, collect again (the table form after step_and_reset reads the tracked obs_row) ==
    # one collect of the whole length (no time limit: step_and_reset does not count episode steps)
    from rl_offline_simulation_amd.evaluators.obs_policy import obs_tensor
    a, b = _twins(d, E, np.arange(E) + 5)
    r1 = a.collect(mlp, 40).row
    rs = []
    for _ in range(15):
        a.step_and_reset(mlp.forward(obs_tensor(a.obs, gpu)))
        rs.append(torch.where(a.env._status == 0, a.env._row, torch.full_like(a.env._row, -1)))
    r3 = a.collect(mlp, 60, form="rows").row
    c = b.collect(mlp, 115)
    assert torch.equal(torch.cat([r1, torch.stack(rs), r3]), c.row)
    for x, y in zip(_state(a), _state(b)):
        assert torch.equal(x, y)


def _grid(every_row_initial=False, keyerror=False):
    from rl_offline_simulation_amd import synth
    g = synth.grid_coords_log(20, seed=6)
    d = dict(obs=g["observations"], next_obs=g["next_observations"], z=g["z"], z_next=g["z_next"].copy(), a=g["actions"], r=g["rewards"],
             done=g["terminals"], p_log=g["action_distributions"], t0=g["steps"] == 0)
    if every_row_initial:
        d["t0"] = np.ones(len(d["z"]), bool)
    if keyerror:
        d["z_next"][d["z_next"] == 1] = 30
    return d


def test_exhaustion_and_empty_init_queue(gpu):
    from rl_offline_simulation_amd import _lib as L
    for d, cap in ((_grid(every_row_initial=True), None), (_grid(), 3)):
        E, T = 8, 400
        a, b = _twins(d, E, np.arange(E))
        mlp = _mlp(2, 5, 2, "tanh", seed=1)
        c = a.collect(mlp, T, max_episode_steps=cap)
        rows, flags, _, probs, _ = _loop(b, mlp, T, 0 if cap is None else cap)
        assert torch.equal(c.row, rows) and torch.equal(_flags(c), flags)
        for x, y in zip(_state(a), _state(b)):
            assert torch.equal(x, y)
        st = c.status.cpu().numpy()
        assert not a.alive.any() and set(st) <= {L.ST_EXHAUSTED, L.ST_NO_INIT}
        assert (c.row[-1] == -1).all()


def test_keyerror_strict_and_not(gpu):
    from rl_offline_simulation_amd import _lib as L
    d = _grid(keyerror=True)
    mlp = _mlp(2, 5, 1, "relu", seed=2)
    env = _twins(d, 6, np.arange(6))[0]
    c = env.collect(mlp, 300)
    st = c.status.cpu().numpy()
    assert (st == L.ST_KEYERROR).any()
    assert not env.alive[torch.from_numpy(st == L.ST_KEYERROR).to(gpu)].any()
    strict = _twins(d, 6, np.arange(6), strict=True)[0]
    with pytest.raises(KeyError):
        strict.collect(mlp, 300)


def test_zero_steps_changes_nothing(gpu):
    d = _cartpole(2000, 4, np.float32)
    env = _twins(d, 5, np.arange(5))[0]
    before = _state(env)
    c = env.collect(_mlp(4, 2, 2, "tanh"), 0)
    assert c.row.shape == (0, 5) and c.probs.shape == (0, 5, 2) and c.obs.shape == (0, 5, 4)
    for x, y in zip(before, _state(env)):
        assert torch.equal(x, y)


def test_tabular_form(gpu):
    """pi[state] where observations are states equals the table form with p_next[i] = pi[z_next[i]], p_init[i] = pi[z[i]]."""
    from rl_offline_simulation_amd.evaluators import RowPolicy
    g = _grid()
    d = dict(g, obs=g["z"], next_obs=g["z_next"])
    E = 16
    a, b = _twins(d, E, np.arange(E), discrete=True)
    pi = np.random.default_rng(0).dirichlet(np.ones(5), size=25)
    c1 = a.collect(pi, 200, max_episode_steps=6)
    c2 = b.collect(RowPolicy(pi[d["z_next"]], pi[d["z"]]), 200, max_episode_steps=6)
    for f in ("row", "obs", "probs", "terminated", "truncated", "alive", "status"):
        assert torch.equal(getattr(c1, f), getattr(c2, f)), f
    for x, y in zip(_state(a), _state(b)):
        assert torch.equal(x, y)
    enc = _twins(_grid(), 4, np.arange(4))[0]
    with pytest.raises(NotImplementedError):
        enc.collect(pi, 10)


def test_lds_budget_of_the_network(gpu):
    """The in-wave network takes W and b of all layers up to OFFSIM_COLLECT_MLP_MAX_FLOATS floats; one float more is refused."""
    from rl_offline_simulation_amd import _lib as L
    from rl_offline_simulation_amd.evaluators import MLPPolicy
    d = _cartpole(2000, 126, np.float32)
    g = torch.Generator().manual_seed(0)
    W1, W2 = torch.randn(128, 126, generator=g) * 0.1, torch.randn(2, 128, generator=g)
    assert W1.numel() + W2.numel() == L.COLLECT_MLP_MAX_FLOATS
    a, b = _twins(d, 9, np.arange(9))
    fits = MLPPolicy([(W1, None), (W2, None)])
    c = a.collect(fits, 50, max_episode_steps=10)
    rows, flags, _, probs, _ = _loop(b, fits, 50, 10)
    assert torch.equal(c.row, rows) and torch.equal(c.probs[rows >= 0], probs[rows >= 0])
    over = MLPPolicy([(W1, None), (W2, torch.zeros(2))])
    with pytest.raises(L.OffsimError, match="OFFSIM_COLLECT_MLP_MAX_FLOATS"):
        a.collect(over, 5)
    wide = _mlp(4, 2, 2, "tanh")
    with pytest.raises(ValueError):
        a.collect(wide, 5)  # the network's input width differs from the log's


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_reference_fixtures(gpu, path):
    """The reference's PSRS driven by the example's loop (tests/golden/make_golden_collect.py), reproduced through the table form."""
    from rl_offline_simulation_amd import _lib as L
    from rl_offline_simulation_amd.evaluators import RowPolicy
    f = np.load(path)
    d = {k: f[k] for k in ("obs", "next_obs", "z", "z_next", "a", "r", "done", "p_log", "t0")}
    seeds = f["seeds"]
    T, cap = int(f["T"]), int(f["cap"])
    env = _env(**d, E=len(seeds), strict=False)
    env.reset_sampler(seeds)
    env.reset()
    c = env.collect(RowPolicy(f["P_next"], f["P_init"]), T, max_episode_steps=cap or None)
    row, fl = c.row.cpu().numpy(), _flags(c).cpu().numpy()
    for k, s in enumerate(seeds):
        ref_rows, ref_obs = f[f"rows_{s}"], f[f"obs_row_{s}"]
        n = len(ref_rows)
        assert np.array_equal(row[:n, k], ref_rows), s
        assert (row[n:, k] == -1).all()
        assert np.array_equal((fl[:n, k] & L.COLLECT_TERMINATED) != 0, f[f"terminated_{s}"])
        assert np.array_equal((fl[:n, k] & L.COLLECT_TRUNCATED) != 0, f[f"truncated_{s}"])
        # the observation each step was asked at: obs_row before the step
        got_obs = c.obs.cpu().numpy()[:n, k]
        want = np.stack([d["next_obs"][v] if v >= 0 else d["obs"][-2 - v] for v in ref_obs]) if n else got_obs
        assert np.array_equal(got_obs, want)
        assert (int(c.status[k]) == L.ST_KEYERROR) == (str(f[f"status_{s}"]) == "keyerror"), s
    # the NumPy restatement agrees (tests/collect_host.py)
    o = H.collect_rows(d["z"], d["a"], d["z_next"], d["done"], d["p_log"], d["t0"], f["P_next"], f["P_init"], int(seeds[0]), T, cap)
    assert np.array_equal(o["rows"], f[f"rows_{seeds[0]}"])
