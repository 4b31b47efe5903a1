"""A population of policies over observations on the same seeds, on the device: offsim_policy_mlp_pop against offsim_policy_mlp per learner,
offsim_eval_mc_rows_policy_pop against offsim_eval_mc_rows_policy per (policy, seed) -- on the reference's fixtures and over providers,
modes, orders and reject rules on a synthetic table --, the sampler state it leaves alone, the tiled driver and PPOPopulation.evaluate.
Every comparison is bit for bit."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import obs_policy_host as H  # noqa: E402
import policy_population_host as PH  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "obs_policy", "*.npz")))
KEYS = ("sum_g", "n_ep", "steps", "cand", "n_len", "status", "ep_g", "ep_len", "trace_row", "trace_pop", "obs_row")


@pytest.fixture(scope="module")
def gpu():
    from rl_offline_simulation_amd import _lib
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    _lib.load()
    return torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64) if t.is_floating_point() else t


def _same(a, b):
    """bit for bit (NaNs in the same places with the same payload)"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


# ---- 1. the forward ----
def _mlps(n, sizes, act, seed):
    from rl_offline_simulation_amd.evaluators import MLPPolicy
    g = torch.Generator().manual_seed(seed)
    return [MLPPolicy([(torch.randn(o, i, generator=g) / i ** 0.5, torch.randn(o, generator=g)) for i, o in zip(sizes, sizes[1:])], act, 0.05)
            for _ in range(n)]


@pytest.mark.parametrize("xdt", ["f32", "f16"])
@pytest.mark.parametrize("sizes,act", [((4, 16, 2), "tanh"), ((2, 64, 64, 5), "relu"), ((128, 256, 16), "leaky_relu")], ids=lambda v: str(v))
def test_forward_equals_single_per_learner(sizes, act, xdt, gpu):
    from rl_offline_simulation_amd.evaluators import PolicyPopulation
    pols = _mlps(3, sizes, act, seed=sum(sizes))
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(40, sizes[0], generator=g) * 2).to(torch.float16 if xdt == "f16" else torch.float32).to(gpu)
    rows = torch.randint(0, 40, (33,), generator=g, dtype=torch.int32)  # 33: one full 32-row tile plus one row
    rows[17] = 40  # out of range: NaN probabilities
    rows = rows.to(gpu)
    got = PolicyPopulation.from_policies(pols).forward(x, rows)
    assert got.shape == (3, 33, sizes[-1])
    for l, p in enumerate(pols):
        ref = p.forward(x, rows)
        assert _same(got[l], ref), l
        assert not bool(torch.isnan(ref[:17]).any()) and not bool(torch.isnan(ref[18:]).any())
        if act != "relu":  # (ReLU maps the NaN inputs of that row to 0 in the first hidden layer, in both forms alike)
            assert bool(torch.isnan(ref[17]).all())
    assert not torch.equal(got[0][:17], got[1][:17])
    one = PolicyPopulation.from_policies(pols[1:2]).forward(x, rows)
    assert one.shape[0] == 1 and _same(one[0], pols[1].forward(x, rows))
    # no gather index, and a tile of the population that does not start at learner 0
    assert _same(PolicyPopulation.from_policies(pols).forward(x, None, 1, 3)[1], pols[2].forward(x))


# ---- the single form, per (policy, seed) ----
def _single(table, seed, pn, p0, gamma, reject_mode=0, shuffle="per_rollout", provider="pcg64", **caps):
    from rl_offline_simulation_amd.evaluators import BatchedPSRS
    b = BatchedPSRS(table, 1, reject_mode)
    b.reset_sampler([int(seed)], shuffle, shuffle_seed=7 if shuffle == "shared" else None, rejection=provider)
    return b.eval_mc_rows_policy(pn, p0, gamma, **caps)


def _assert_equals_single(o, table, seeds, pn, p0, gamma, **kw):
    for l in range(pn.shape[0]):
        for j, s in enumerate(seeds):
            ref = _single(table, s, pn[l], p0[l], gamma, **kw)
            for k in KEYS:
                assert _same(o[k][l, j], ref[k][0]), (k, l, j)


# ---- 2. the reference's fixtures ----
@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_scan_on_reference_fixtures(path, gpu):
    from rl_offline_simulation_amd import _lib as L
    from rl_offline_simulation_amd.evaluators import PSRS, BatchedPSRS, PolicyPopulation, RowPolicy
    d = np.load(path)
    table = PSRS.from_arrays(d["z"], d["a"], d["r"], d["z_next"], d["done"], d["p_log"], t0=d["t0"], obs=d["obs"], next_obs=d["next_obs"]).table
    P_next, P_init = PH.fixture_policies(d)
    seeds = [int(s) for s in d["seeds"]]
    if (3 * len(seeds)) % 4 == 0:
        seeds = seeds[:-1]
    assert (3 * len(seeds)) % 4 != 0  # the last workgroup is partial
    pop = PolicyPopulation.from_rows([RowPolicy(P_next[l], P_init[l]) for l in range(3)])
    pn, p0 = pop.row_tables(table)
    assert pn.shape == (3, table.N, table.nA) and p0.shape == (3, table.N0, table.nA)
    if d["P_next"].dtype == np.float32 and d["p_log"].dtype == np.float32:
        assert pn.dtype == torch.float32  # the f32 mode
    gamma, caps = float(d["gamma"]), dict(ep_cap=max(int(table.N0), 1), trace_cap=int(table.N))
    env = BatchedPSRS(table, len(seeds))
    env.reset_sampler(seeds)
    o = env.eval_mc_rows_policy_population(pn, p0, gamma, **caps)
    torch.cuda.synchronize()
    L.check_async_faults()
    assert o["sum_g"].shape == (3, len(seeds)) and o["trace_row"].shape == (3, len(seeds), table.N)
    # policy 0: what the reference recorded
    for j, s in enumerate(seeds):
        n, ne, nl = int(o["steps"][0, j]), int(o["n_ep"][0, j]), int(o["n_len"][0, j])
        assert np.array_equal(o["trace_row"][0, j, :n].cpu().numpy(), d[f"rows_{s}"]), s
        if str(d[f"status_{s}"]) == "keyerror":
            assert int(o["status"][0, j]) == L.ST_KEYERROR
        else:
            assert int(o["status"][0, j]) != L.ST_KEYERROR
            assert np.array_equal(o["ep_g"][0, j, :ne].cpu().numpy(), d[f"Gs_{s}"]), s
            assert np.array_equal(o["ep_len"][0, j, :nl].cpu().numpy(), d[f"lengths_{s}"]), s
    # every (policy, seed): the single form on its own
    _assert_equals_single(o, table, seeds, pn, p0, gamma, **caps)
    # ... and the NumPy restatement for the other policies of the first seed
    inp = H.fixture_inputs(d)
    host = PH.evalmc_rows_population(inp, P_next[1:], P_init[1:], seeds[:1], gamma)
    for l in (1, 2):
        h = host[(l - 1, 0)]
        assert np.array_equal(o["trace_row"][l, 0, :int(o["steps"][l, 0])].cpu().numpy(), h["rows"])
        assert float(o["sum_g"][l, 0]) == PH.sum_in_order(h["Gs"]) and int(o["n_ep"][l, 0]) == len(h["Gs"])
        assert (int(o["status"][l, 0]) == L.ST_KEYERROR) == (h["status"] == "keyerror")


# ---- 3. providers, modes, orders and reject rules on a small synthetic table ----
_SYNTH = {}


def _synth_table(f32):
    from rl_offline_simulation_amd import synth
    from rl_offline_simulation_amd.table import TransitionTable
    if f32 not in _SYNTH:
        e = synth.synth_iid(20_000, 25, 5, seed=1)
        t = TransitionTable(e["z"], e["actions"], e["rewards"], e["z_next"], e["terminals"], e["action_distributions"], e["steps"] == 0,
                            plog_dtype=np.float32 if f32 else np.float64)
        g = np.random.default_rng(5)
        dt = np.float32 if f32 else np.float64
        pn = torch.from_numpy(g.dirichlet(np.ones(5), (5, t.N)).astype(dt)).to(t.device)
        p0 = torch.from_numpy(g.dirichlet(np.ones(5), (5, t.N0)).astype(dt)).to(t.device)
        _SYNTH[f32] = (t, pn, p0)
    return _SYNTH[f32]


_CASES = [(p, m, s, "default") for p in ("pcg64", "philox") for m in ("f64", "f32") for s in ("per_rollout", "shared", "table_order")] + \
    [("pcg64", m, "per_rollout", "never") for m in ("f64", "f32")]  # (REJECT_NEVER draws nothing: one provider and order suffice)


def _run_population(table, seeds, pn, p0, provider, shuffle, rm, caps):
    from rl_offline_simulation_amd import _lib as L
    from rl_offline_simulation_amd.evaluators import BatchedPSRS
    env = BatchedPSRS(table, len(seeds), rm)
    env.reset_sampler(seeds, shuffle, shuffle_seed=7 if shuffle == "shared" else None, rejection=provider)
    o = env.eval_mc_rows_policy_population(pn, p0, 0.99, **caps)
    torch.cuda.synchronize()
    L.check_async_faults()
    return o


@pytest.mark.parametrize("provider,mode,shuffle,reject", _CASES, ids=lambda v: str(v))
def test_matrix_against_single_form(provider, mode, shuffle, reject, gpu):
    from rl_offline_simulation_amd import _lib as L
    table, pn, p0 = _synth_table(mode == "f32")
    assert pn.dtype == (torch.float32 if mode == "f32" else torch.float64)
    rm = L.REJECT_NEVER if reject == "never" else L.REJECT_DEFAULT
    seeds = np.arange(7) + 100  # L = 5, S = 7: 35 rollouts, the last workgroup holds three
    caps = dict(ep_cap=64, trace_cap=512)
    o = _run_population(table, seeds, pn, p0, provider, shuffle, rm, caps)
    assert o["steps"].shape == (5, 7) and int(o["steps"].min()) > 0
    _assert_equals_single(o, table, seeds, pn, p0, 0.99, reject_mode=rm, shuffle=shuffle, provider=provider, **caps)
    if reject == "default":
        assert not torch.equal(o["steps"][0], o["steps"][1])  # the policies do differ


@pytest.mark.parametrize("n_pol,n_seeds", [(1, 1), (5, 1)])
def test_edge_sizes(n_pol, n_seeds, gpu):
    from rl_offline_simulation_amd import _lib as L
    table, pn, p0 = _synth_table(False)
    seeds = np.arange(n_seeds) + 3
    caps = dict(ep_cap=64, trace_cap=512)
    o = _run_population(table, seeds, pn[:n_pol], p0[:n_pol], "pcg64", "per_rollout", L.REJECT_DEFAULT, caps)
    assert o["steps"].shape == (n_pol, n_seeds)
    _assert_equals_single(o, table, seeds, pn[:n_pol], p0[:n_pol], 0.99, **caps)


# ---- 4. an evaluation is a query: the sampler state is left as it was ----
def test_sampler_state_untouched(gpu):
    from rl_offline_simulation_amd.evaluators import BatchedPSRS
    table, pn, p0 = _synth_table(False)
    seeds = np.arange(6) + 40
    caps = dict(ep_cap=64, trace_cap=512)
    env = BatchedPSRS(table, 6)
    env.reset_sampler(seeds)
    before = [x.clone() for x in (env.state.rng, env.state.cursor, env.state.init_cursor, env.state.cur_slot, env.state.perm, env.state.init_perm)]
    env.eval_mc_rows_policy_population(pn, p0, 0.99, **caps)
    after = (env.state.rng, env.state.cursor, env.state.init_cursor, env.state.cur_slot, env.state.perm, env.state.init_perm)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    got = env.eval_mc_rows_policy(pn[2], p0[2], 0.99, **caps)
    fresh = BatchedPSRS(table, 6)
    fresh.reset_sampler(seeds)
    ref = fresh.eval_mc_rows_policy(pn[2], p0[2], 0.99, **caps)
    for k in KEYS:
        assert _same(got[k], ref[k]), k
    assert torch.equal(env.state.rng, fresh.state.rng) and torch.equal(env.state.cursor, fresh.state.cursor)


# ---- 5. and 6. the drivers, on a CartPole-like log with observations ----
_CP = {}


def _cartpole():
    from rl_offline_simulation_amd import synth
    from rl_offline_simulation_amd.encoders.heuristic import CartpoleBoxEncoder
    from rl_offline_simulation_amd.table import TransitionTable
    if not _CP:
        cp = synth.cartpole_log(20_000, seed=8)
        enc = CartpoleBoxEncoder()
        z, z_next = enc.encode(cp["observations"]), enc.encode(cp["next_observations"])
        missing = ~np.isin(z_next, z)  # (boxes that occur only as next states end a run with a KeyError: led back to their from-state)
        z_next[missing] = z[missing]
        _CP["table"] = TransitionTable(z, cp["actions"], cp["rewards"].astype(np.float64), z_next, cp["terminals"], cp["action_distributions"],
                                       cp["steps"] == 0)
        _CP["obs"], _CP["next_obs"] = cp["observations"], cp["next_observations"]
    return _CP["table"], _CP["obs"], _CP["next_obs"]


RES_KEYS = ("sum_g", "n_ep", "steps", "cand", "status", "value")


def test_tiled_driver_equals_untiled(gpu):
    from rl_offline_simulation_amd.evaluators import evalmc_rollouts, evalmc_rollouts_population
    table, obs, nobs = _cartpole()
    pols = _mlps(5, (4, 16, 2), "tanh", seed=3)
    seeds = np.arange(5) + 11
    whole = evalmc_rollouts_population(table, seeds, pols, 0.99, obs=obs, next_obs=nobs)
    tiled = evalmc_rollouts_population(table, seeds, pols, 0.99, obs=obs, next_obs=nobs, tile=2, policy_tile=2)  # 3 x 3 tiles, the last of one
    for k in RES_KEYS + ("mean_value",):
        assert whole[k].shape == ((5, 5) if k != "mean_value" else (5,))
        assert np.array_equal(whole[k], tiled[k], equal_nan=True), k
    assert whole["best"] == tiled["best"] == int(np.nanargmax(whole["mean_value"]))
    one = evalmc_rollouts(table, seeds, pols[3], 0.99, obs=obs, next_obs=nobs)
    for k in RES_KEYS:
        assert np.array_equal(whole[k][3], one[k], equal_nan=True), k
    assert int(whole["steps"].min()) > 0


def test_ppo_population_evaluate_end_to_end(gpu):
    from rl_offline_simulation_amd.evaluators import MLPValue, PPOPopulation, evalmc_rollouts
    table, obs, nobs = _cartpole()
    g = torch.Generator().manual_seed(9)
    critics = [MLPValue([(torch.randn(16, 4, generator=g) / 2, torch.randn(16, generator=g)), (torch.randn(1, 16, generator=g) / 4, torch.randn(1, generator=g))])
               for _ in range(3)]
    ppo = PPOPopulation(_mlps(3, (4, 16, 2), "tanh", seed=4), critics, train_pi_iters=3, train_v_iters=1, target_kl=1e9)
    seeds = np.arange(6) + 70

    def check():
        res = ppo.evaluate(table, seeds, 0.99, obs, nobs)
        for l in range(3):
            one = evalmc_rollouts(table, seeds, ppo.actor(l), 0.99, obs=obs, next_obs=nobs)
            for k in RES_KEYS:
                assert np.array_equal(res[k][l], one[k], equal_nan=True), (k, l)
        with np.errstate(invalid="ignore"):
            assert np.array_equal(res["mean_value"], np.nanmean(res["value"], axis=1), equal_nan=True)
        assert res["best"] == int(np.nanargmax(res["mean_value"]))
        return res

    first = check()
    T, E = 16, 4
    batch = dict(obs=torch.randn(T, 3 * E, 4, generator=g).to(gpu), act=torch.randint(0, 2, (T, 3 * E), generator=g, dtype=torch.int32).to(gpu),
                 adv=torch.randn(T, 3 * E, generator=g).to(gpu), logp=torch.full((T, 3 * E), float(np.log(0.5))).to(gpu),
                 ret=torch.randn(T, 3 * E, generator=g).to(gpu))
    ppo.update(batch)
    second = check()  # the new weights, with no copy in between
    assert not np.array_equal(first["steps"], second["steps"]) or not np.array_equal(first["sum_g"], second["sum_g"])
