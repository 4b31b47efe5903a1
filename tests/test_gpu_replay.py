"""offsim_replay_td (csrc/replay_td.hpp) on the device against the plain loop of tests/replay_host.py -- Q, TD errors, snapshots, n_ep, steps
and status bit for bit -- over tile edges, lane groups, every LPW the chooser returns, the LDS limit, read-after-write through LDS, episode
bookkeeping, orders, both targets, the KeyError stop, lane independence and determinism; then the drop-ins: qlearn_replay on the reference's
recorded qlearn(..., memory=...), an online learner replayed from its own memory, and TDPopulation.replay."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import replay_host as H  # noqa: E402
from test_replay_host import ALPHA_SCHED, FIXTURES, GOLDEN, golden_log  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch.device("cuda", 0)


def device_run(gpu, log, mode, alpha, gamma, q, orders=None, **kw):
    from rl_offline_simulation_amd.evaluators import ReplayLog, replay_td
    dlog = ReplayLog.from_arrays(*log, device=gpu)
    ords = None if orders is None else torch.from_numpy(np.ascontiguousarray(orders, dtype=np.int32)).to(gpu)
    o = replay_td(dlog, mode, alpha, gamma, torch.from_numpy(np.ascontiguousarray(q)).to(gpu), orders=ords, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def check(gpu, log, mode, alpha, gamma, q, orders=None, tag="", **kw):
    """device == host loop on every output; returns both"""
    q = np.asarray(q, np.float64)
    q = q[:, None] if q.ndim == 3 else q
    mine = H.run(log, mode, alpha, gamma, q, orders, **kw)
    o = device_run(gpu, log, mode, alpha, gamma, q, orders, **kw)
    for k in ("n_ep", "steps", "status"):
        assert o[k].tolist() == mine[k].tolist(), (tag, k)
    keys = ("q",) + (("td_err",) if kw.get("td_cap") else ()) + (("q_snap",) if kw.get("snap_cap") else ())
    for k in keys:
        assert np.array_equal(o[k], mine[k], equal_nan=True), (tag, k)
    return o, mine


@pytest.mark.parametrize("N", [1, 63, 64, 65, 129, 2000])
def test_tile_edges(N, gpu):
    log = H.synth_log(N, 5, 3, seed=N)
    alpha, gamma, q = H.learners(3, 5, 3, seed=1)
    o, _ = check(gpu, log, H.QLEARN, alpha, gamma, q, td_cap=N, tag=N)
    assert (o["steps"] == N).all() and o["n_ep"][0] == int(log[4].sum())


@pytest.mark.parametrize("n_l", [1, 3, 64, 65, 130])
def test_lane_groups(n_l, gpu):
    log = H.synth_log(129, 6, 4, seed=7)
    alpha, gamma, q = H.learners(n_l, 6, 4, seed=n_l)
    check(gpu, log, H.QLEARN, alpha, gamma, q, td_cap=129, tag=n_l)


@pytest.mark.parametrize("lpw", [64, 32, 16, 8, 4, 2, 1])
def test_every_lpw(lpw, gpu):
    """nS * nA one entry past what 2 * LPW learners fit (the budget formula of csrc/replay_td.hpp), so the chooser returns LPW; 65 learners:
    more than one lane group, the last one partial."""
    from rl_offline_simulation_amd.evaluators import replay_lpw
    nS = 25 if lpw == 64 else H.LDS_BUDGET // (8 * 2 * lpw) + 1
    assert replay_lpw(nS, 1, 65) == H.lpw(nS, 1, 65) == lpw
    g = np.random.default_rng(lpw)
    N = 150
    hot = g.integers(0, nS, 6).astype(np.int32)  # few states, so that the updates feed one another
    log = (hot[g.integers(0, 6, N)], np.zeros(N, np.int32), g.standard_normal(N), hot[g.integers(0, 6, N)], g.random(N) < 0.1, nS, 1)
    alpha, gamma, q = H.learners(65, nS, 1, seed=2)
    check(gpu, log, H.QLEARN, alpha, gamma, q, td_cap=N, tag=lpw)


def test_lds_limit(gpu):
    """nS * nA = 20480: one learner's Q is exactly 160 KiB; one entry more is refused."""
    from rl_offline_simulation_amd import _lib as L
    from rl_offline_simulation_amd.evaluators import ReplayLog, replay_lpw, replay_td
    nS, nA, N = 4096, 5, 130
    assert replay_lpw(nS, nA, 3) == 1 and nS * nA * 8 == H.LDS_BUDGET
    g = np.random.default_rng(0)
    hot = np.array([0, 1, 2047, 4094, 4095], np.int32)
    log = (hot[g.integers(0, 5, N)], g.integers(0, nA, N).astype(np.int32), g.standard_normal(N), hot[g.integers(0, 5, N)], g.random(N) < 0.1, nS, nA)
    alpha, gamma, q = H.learners(3, nS, nA, seed=3)
    check(gpu, log, H.QLEARN, alpha, gamma, q, td_cap=N)
    nS = 20481
    big = ReplayLog.from_arrays(np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(4), np.zeros(4, np.int32), np.zeros(4, bool), nS, 1, device=gpu)
    assert replay_lpw(nS, 1, 1) == 0
    with pytest.raises(L.OffsimError, match="offsim error -3: replay_td: one learner's Q table exceeds 160 KiB of LDS"):
        replay_td(big, L.TD_QLEARN, [0.1], [0.9], torch.zeros((1, 1, nS, 1), dtype=torch.float64, device=gpu))


def test_read_after_write_through_lds(gpu):
    """Every step reads what the step before wrote: a one-state self-loop with one action, and two (s, a) pairs taking turns."""
    N = 130
    g = np.random.default_rng(11)
    loop = (np.zeros(N, np.int32), np.zeros(N, np.int32), g.standard_normal(N), np.zeros(N, np.int32), np.zeros(N, bool), 1, 1)
    alpha, gamma, q = H.learners(65, 1, 1, seed=4)
    o, _ = check(gpu, loop, H.QLEARN, alpha, gamma, q, td_cap=N, tag="self-loop")
    assert not np.array_equal(o["q"][:, 0], q)
    k = np.arange(N)
    turns = ((k % 2).astype(np.int32), (1 - k % 2).astype(np.int32), g.standard_normal(N), ((k + 1) % 2).astype(np.int32), np.zeros(N, bool), 2, 2)
    alpha, gamma, q = H.learners(65, 2, 2, seed=5)
    check(gpu, turns, H.QLEARN, alpha, gamma, q, td_cap=N, tag="turns")
    check(gpu, turns, H.EXPSARSA, alpha, gamma, q, td_cap=N, pi=np.array([[0.25, 0.75], [0.6, 0.4]]), tag="turns-expsarsa")


def test_episodes(gpu):
    """done at the first and the last entry of a tile, a schedule shorter than the episodes, three passes with the counter carried over."""
    N = 150
    s, a, r, sn, done, nS, nA = H.synth_log(N, 5, 3, seed=21, p_done=0.0)
    done[[0, 63, 64, 127, 128]] = True
    log = (s, a, r, sn, done, nS, nA)
    alpha, gamma, q = H.learners(5, nS, nA, seed=6)
    sched = np.random.default_rng(7).uniform(0.01, 0.9, (5, 20))
    o, _ = check(gpu, log, H.QLEARN, alpha, gamma, q, alpha_ep=sched, td_cap=N, tag="n_sched > episodes")
    assert o["n_ep"].tolist() == [5]
    check(gpu, log, H.QLEARN, alpha, gamma, q, alpha_ep=sched[:, :3], td_cap=N, tag="n_sched < episodes")
    o, mine = check(gpu, log, H.QLEARN, alpha, gamma, q, alpha_ep=sched[:, :12], passes=3, td_cap=3 * N, tag="passes")
    assert o["n_ep"].tolist() == [15] and (o["steps"] == 3 * N).all()
    one = H.run(log, H.QLEARN, alpha, gamma, q[:, None], alpha_ep=sched[:, :12], td_cap=N)
    assert not np.array_equal(mine["td_err"][0, 2 * N:], one["td_err"][0])  # (the later sweeps are not the first one again)


def _three_orders(N, M, seed):
    g = np.random.default_rng(seed)
    return np.stack([np.resize(g.permutation(N), M), g.integers(0, N, M), np.resize(np.arange(N), M)]).astype(np.int32)


@pytest.mark.parametrize("M", [100, 2 * 130 + 7])
def test_orders(M, gpu):
    """S = 3: a permutation, a bootstrap resample with repeats and the identity, shorter and longer than the log."""
    N = 130
    log = H.synth_log(N, 5, 3, seed=31)
    orders = _three_orders(N, M, seed=M)
    assert len(np.unique(orders[1])) < min(M, N)
    alpha, gamma, q = H.learners(3, 5, 3, seed=8)
    q = np.stack([q, q + 1.0, q - 1.0], axis=1)  # Q_init per rollout
    o, _ = check(gpu, log, H.QLEARN, alpha, gamma, q, orders, td_cap=M, passes=2, tag=M)
    assert o["n_ep"].tolist() == [2 * int(log[4][orders[j]].sum()) for j in range(3)]
    if M > N:  # the identity stream's first N steps are the log in log order
        plain = device_run(gpu, log, H.QLEARN, alpha, gamma, q[:, 2:3], td_cap=N)
        assert np.array_equal(plain["td_err"][0], o["td_err"][2, :N])


def test_expected_sarsa(gpu):
    log = H.synth_log(200, 6, 5, seed=41)
    alpha, gamma, q = H.learners(65, 6, 5, seed=9)
    g = np.random.default_rng(10)
    check(gpu, log, H.EXPSARSA, alpha, gamma, q, pi=g.dirichlet(np.ones(5), 6), td_cap=200, tag="shared pi")
    check(gpu, log, H.EXPSARSA, alpha, gamma, q, pi=g.dirichlet(np.ones(5), (65, 6)), td_cap=200, tag="pi per learner")
    check(gpu, H.synth_log(70, 4, 9, seed=42), H.EXPSARSA, alpha[:3], gamma[:3], H.learners(3, 4, 9, 1)[2], pi=g.dirichlet(np.ones(9), 4), td_cap=70, tag="nA = 9")
    check(gpu, H.synth_log(70, 4, 9, seed=43), H.QLEARN, alpha[:3], gamma[:3], H.learners(3, 4, 9, 1)[2], td_cap=70, tag="nA = 9, max")


def test_outputs(gpu):
    """td_cap shorter than the run; snapshots of stride 1 and 7 with a short snap_cap, and a capacity the run does not fill."""
    log = H.synth_log(100, 5, 3, seed=51)
    alpha, gamma, q = H.learners(66, 5, 3, seed=12)
    orders = _three_orders(100, 100, seed=1)
    check(gpu, log, H.QLEARN, alpha, gamma, q[:, None].repeat(3, axis=1), orders, td_cap=37, tag="td_cap")
    check(gpu, log, H.QLEARN, alpha, gamma, q, td_cap=100, snap_stride=1, snap_cap=9, tag="stride 1")
    check(gpu, log, H.QLEARN, alpha, gamma, q[:, None].repeat(3, axis=1), orders, snap_stride=7, snap_cap=5, tag="stride 7")
    o, _ = check(gpu, log, H.QLEARN, alpha[:2], gamma[:2], q[:2], snap_stride=7, snap_cap=20, tag="capacity past the run")
    assert o["q_snap"][:, 0, 14].any() and not o["q_snap"][:, 0, 15:].any()  # step 98 is the last snapshot


@pytest.mark.parametrize("what", ["s_next", "s", "a", "order"])
def test_keyerror_stops_one_stream(what, gpu):
    """Step k = 70 of stream 1 is outside the tables: its rollouts stop before it with Q as step 69 left it; streams 0 and 2 complete."""
    N, k = 100, 70
    s, a, r, sn, done, nS, nA = H.synth_log(N, 5, 3, seed=61)
    orders = np.stack([np.arange(N - 1), np.arange(N - 1), np.arange(N - 1)[::-1]]).astype(np.int32)
    orders[1, k] = N - 1  # only stream 1 visits the last row
    if what == "order":
        orders[1, k] = N
    else:
        dict(s_next=sn, s=s, a=a)[what][N - 1] = dict(s_next=nS, s=-1, a=nA)[what]
    log = (s, a, r, sn, done, nS, nA)
    alpha, gamma, q = H.learners(65, nS, nA, seed=13)
    o, _ = check(gpu, log, H.QLEARN, alpha, gamma, q[:, None].repeat(3, axis=1), orders, td_cap=N - 1, tag=what)
    assert o["status"].tolist() == [[H.ST_OK, H.ST_KEYERROR, H.ST_OK]] * 65 and o["steps"].tolist() == [[N - 1, k, N - 1]] * 65
    before = H.stream(log, H.QLEARN, alpha, gamma, q, order=orders[1, :k])
    assert np.array_equal(o["q"][:, 1], before["q"]) and o["n_ep"][1] == before["n_ep"]


def test_nan_in_a_row_maximum(gpu):
    log = (np.array([0, 0], np.int32), np.array([0, 1], np.int32), np.array([1.0, 1.0]), np.array([1, 2], np.int32), np.array([False, False]), 3, 3)
    q = np.zeros((2, 3, 3))
    q[:, 1] = [np.nan, 5.0, 1.0]
    q[:, 2] = [2.0, np.nan, 1.0]
    o, _ = check(gpu, log, H.QLEARN, [0.5, 0.25], [1.0, 1.0], q, td_cap=2)
    assert np.isnan(o["td_err"][0, 0]).all() and o["td_err"][0, 1].tolist() == [3.0, 3.0]


def test_lanes_are_independent_and_calls_repeat(gpu):
    """Row l of an L = 65 launch is the L = 1 launch of learner l; two identical calls give the same bits."""
    N = 150
    log = H.synth_log(N, 5, 3, seed=71)
    alpha, gamma, q = H.learners(65, 5, 3, seed=14)
    sched = np.random.default_rng(15).uniform(0.01, 0.9, (65, 4))
    kw = dict(alpha_ep=sched, td_cap=N, snap_stride=50, snap_cap=3)
    full = device_run(gpu, log, H.QLEARN, alpha, gamma, q[:, None], **kw)
    again = device_run(gpu, log, H.QLEARN, alpha, gamma, q[:, None], **kw)
    assert all(np.array_equal(full[k], again[k]) for k in full)
    for l in range(65):
        one = device_run(gpu, log, H.QLEARN, alpha[l:l + 1], gamma[l:l + 1], q[l:l + 1, None], **dict(kw, alpha_ep=sched[l:l + 1]))
        assert np.array_equal(one["q"][0], full["q"][l]) and np.array_equal(one["td_err"][:, :, 0], full["td_err"][:, :, l]), l
        assert np.array_equal(one["q_snap"][0], full["q_snap"][l]) and one["steps"][0].tolist() == full["steps"][l].tolist(), l


# ---- the drop-ins ----
@pytest.mark.parametrize("name", FIXTURES)
def test_qlearn_replay_is_the_recorded_reference(name, gpu):
    from rl_offline_simulation_amd.evaluators import qlearn_replay
    log, d = golden_log(name)
    s, a, r, sn, done, nS, nA = log
    memory = [(int(s[i]), int(a[i]), float(r[i]), int(sn[i]), bool(done[i])) for i in range(len(s))]
    gam = float(d["gamma"])
    for tag, kw in (("c", dict(alpha=float(d["alpha"]), nS=nS, nA=nA)), ("s", dict(alpha=ALPHA_SCHED, Q_init=d["q_init"]))):
        Q, info = qlearn_replay(memory, gam, save_Q=1, **kw)
        assert np.array_equal(Q, d[tag + "_Q"]) and np.array_equal(info["TD_errors"], d[tag + "_td"]) and info["memory"] is memory, (name, tag)
        Qs = info["Qs"]
        assert Qs.shape == tuple(d[tag + "_Qs_shape"]) and np.array_equal(Qs[:9], d[tag + "_Qs9"]) and np.array_equal(Qs[::500], d[tag + "_Qs500"]), (name, tag)
        Q0, info0 = qlearn_replay(memory, gam, **kw)
        assert np.array_equal(Q0, Q) and info0["Qs"].shape == (1, nS, nA) and np.array_equal(info0["TD_errors"], info["TD_errors"])


def _uniform(Q, args):
    return np.ones_like(Q) / Q.shape[1]


def test_an_online_learner_is_the_replay_of_its_own_memory(gpu):
    """qlearn_queue / qlearn_psrs under the uniform behaviour, then their own info["memory"] through qlearn_replay with the same gamma, alpha
    and Q_init: Q and TD_errors come back bit for bit."""
    from rl_offline_simulation_amd import OfflineDataset, ProbDistribution, spaces
    from rl_offline_simulation_amd.evaluators import PSRS, QueueEvaluator, qlearn_psrs, qlearn_queue, qlearn_replay
    inp = np.load(os.path.join(GOLDEN, "queue_iid_2k.npz"))
    d = np.load(os.path.join(GOLDEN, "replay", "queue_iid_2k.npz"))
    nS, nA, gam, q_init = int(d["nS"]), int(d["nA"]), float(d["gamma"]), d["q_init"]
    env = QueueEvaluator(OfflineDataset(spaces.Discrete(nS), spaces.Discrete(nA), ProbDistribution.Discrete, observations=inp["in_z"], actions=inp["in_a"],
                                        rewards=inp["in_r"], next_observations=inp["in_z_next"], terminals=inp["in_done"],
                                        action_distributions=inp["in_p_log"], steps=np.where(inp["in_t0"], 0, 1)))
    env.nS = nS
    for alpha, Q_init in ((0.1, None), (ALPHA_SCHED, q_init)):
        env.reset_sampler(0)
        Q, info = qlearn_queue(env, 6, _uniform, gam, alpha=alpha, Q_init=Q_init, seed=1000)
        assert len(info["memory"]) == len(info["TD_errors"]) > 20
        Qr, info_r = qlearn_replay(info["memory"], gam, alpha=alpha, Q_init=Q_init, nS=nS, nA=nA)
        assert np.array_equal(Qr, Q) and np.array_equal(info_r["TD_errors"], info["TD_errors"])
    psrs = PSRS.from_arrays(inp["in_z"], inp["in_a"], inp["in_r"], inp["in_z_next"], inp["in_done"], inp["in_p_log"], inp["in_t0"], nS=nS, nA=nA)
    psrs.reset_sampler(0)
    Q, info = qlearn_psrs(psrs, 10 ** 9, _uniform, gam, alpha=ALPHA_SCHED, epsilon=1.0, Q_init=q_init)
    assert len(info["memory"]) == len(info["TD_errors"]) > 20
    Qr, info_r = qlearn_replay(info["memory"], gam, alpha=ALPHA_SCHED, Q_init=q_init)
    assert np.array_equal(Qr, Q) and np.array_equal(info_r["TD_errors"], info["TD_errors"])


def test_population_replay(gpu):
    """TDPopulation.replay on device-built orders: every learner on every stream as the host loop has it, best() by the last sweep's TD error;
    ReplayLog.from_table gives the rows back in the caller's order."""
    from rl_offline_simulation_amd.evaluators import ReplayLog, TDPopulation, replay_orders
    from rl_offline_simulation_amd.table import TransitionTable
    log, d = golden_log("queue_iid_2k")
    s, a, r, sn, done, nS, nA = log
    inp = np.load(os.path.join(GOLDEN, "queue_iid_2k.npz"))
    table = TransitionTable(inp["in_z"], inp["in_a"], inp["in_r"], inp["in_z_next"], inp["in_done"], inp["in_p_log"], inp["in_t0"], device=gpu)
    dlog = ReplayLog.from_table(table, nS=nS)
    for x, y in zip((dlog.s, dlog.a, dlog.r, dlog.s_next, dlog.done), (s, a, r, sn, done)):
        assert np.array_equal(x.cpu().numpy(), y)
    N = dlog.N
    orders = torch.cat([replay_orders(N, 2, seed=5), replay_orders(N, 1, seed=6, kind="bootstrap")])
    assert orders.shape == (3, N) and orders.dtype == torch.int32 and torch.equal(orders[0].sort().values, torch.arange(N, device=gpu, dtype=torch.int32))
    assert torch.equal(replay_orders(N, 2, seed=5), orders[:2]) and not torch.equal(orders[0], orders[1]) and len(orders[2].unique()) < N
    pop = TDPopulation.grid("qlearn", alpha=[0.5, ALPHA_SCHED, 0.01], gamma=[0.9, 0.5], behaviour="greedy", epsilon=[0.3])  # (both ignored)
    res = pop.replay(dlog, orders, passes=2, td_cap=2 * N, snap_stride=N, snap_cap=2)
    ords = orders.cpu().numpy()
    n_sched = 2 * max(int(done[o].sum()) for o in ords) + 1
    sched = np.stack([np.array([al(e) for e in range(n_sched)]) if callable(al) else np.full(n_sched, al) for al in pop.alpha])
    mine = H.run(log, H.QLEARN, np.zeros(6), pop.gamma, np.zeros((6, 3, nS, nA)), ords, passes=2, alpha_ep=sched, td_cap=2 * N, snap_stride=N, snap_cap=2)
    assert np.array_equal(res.Q.cpu().numpy(), mine["q"]) and np.array_equal(res.td_err.cpu().numpy(), mine["td_err"].transpose(2, 0, 1))
    assert np.array_equal(res.q_snap.cpu().numpy(), mine["q_snap"]) and res.n_ep.cpu().tolist() == mine["n_ep"].tolist()
    assert res.steps.cpu().tolist() == mine["steps"].tolist() and not res.status.any()
    mse = (mine["td_err"][:, N:] ** 2).mean(axis=1).T  # [L, S], the last sweep
    assert np.allclose(res.last_sweep_mse().cpu().numpy(), mse, rtol=1e-12) and res.best() == int(np.argmin(mse.mean(axis=1)))
    one = pop.replay(dlog)  # the log in log order
    assert one.Q.shape == (6, 1, nS, nA) and one.td_err is None and one.n_ep.cpu().tolist() == [int(d["n_ep"])]
    with pytest.raises(ValueError, match="needs pi"):
        TDPopulation("expsarsa", 0.1, 0.9).replay(dlog)
    es = TDPopulation("expsarsa", [0.1, 0.2], 0.9, pi=np.full((nS, nA), 1.0 / nA)).replay(dlog, td_cap=N)
    mine = H.run(log, H.EXPSARSA, [0.1, 0.2], [0.9, 0.9], np.zeros((2, 1, nS, nA)), pi=np.full((nS, nA), 1.0 / nA), td_cap=N)
    assert np.array_equal(es.Q.cpu().numpy(), mine["q"]) and np.array_equal(es.td_err.cpu().numpy(), mine["td_err"].transpose(2, 0, 1))
