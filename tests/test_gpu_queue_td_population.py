"""A population of TD learners on QueueEvaluator in one launch (offsim_eval_queue_pop, csrc/eval_queue.hpp + csrc/td_pop_queue.hpp): the
kernel against the plain Python loop of tests/queue_td_population_host.py over the case list there -- every output row [l, j] and the state
every rollout leaves, bit for bit --, every row against BatchedQueueEvaluator.eval_td run alone with that learner's setting, continuation
from the returned state, TDPopulation.run_queue over seed tiles with its curves, the reference's recorded qlearn / expSARSA runs
(tests/golden/queue_drivers/*.npz) through run_queue with one learner, and what is refused."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import queue_host as Q  # noqa: E402
import queue_td_population_host as H  # noqa: E402
from test_queue_drivers_host import ALPHA_SCHED, EPS_SCHED, FIXTURES, RUNS, golden_log  # noqa: E402
from test_queue_td_population_host import TD_RUNS  # noqa: E402

pytestmark = pytest.mark.gpu

SCALARS = ("sum_g", "n_ep", "steps", "cand", "n_len", "status", "obs_row")
ARRAYS = ("q", "ep_g", "ep_len", "td_err", "trace_row", "trace_pop")
NAMES = {H.F: "fixed", H.E: "eps_greedy", H.SOFT: "soft_greedy"}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch.device("cuda", 0)


def fresh_env(c, gpu):
    from rl_offline_simulation_amd.evaluators import BatchedQueueEvaluator
    env = BatchedQueueEvaluator(*c.log.arrays(), R=c.S, device=gpu)
    assert (env.table.n_slots, env.nZ, env.z_lo) == (c.log.n_slots, c.log.nZ, c.log.z_lo)
    env.reset_sampler(c.seeds)
    env.set_action_seeds(c.action_seeds)
    return env


def device_tie(c):
    return c.tie if c.tie in ("first", "episode") else H.mt_of(c)


def keys_of(c):
    return ARRAYS + (("q_snap",) if c.snap else ()) + (("beh_arg",) if H.E in c.behaviour else ()) + (("tie_mt",) if c.tie != "first" else ())


def as_host(v):
    v = v.cpu().numpy()
    return v.view(np.uint32) if v.dtype == np.int32 and v.shape[-1] == 625 else v


def assert_rows(o, m, c, tag):
    """device dict o [L, S, ...] against the mirror's m"""
    for k in SCALARS:
        assert np.array_equal(o[k].cpu().numpy(), m[k]), (tag, k)
    for k in keys_of(c):
        assert np.array_equal(as_host(o[k]), m[k]), (tag, k)


def assert_state(st, m, tag):
    """the state every rollout leaves (o["_state"]): cursors, init cursors, current base slots and the action stream's row"""
    assert np.array_equal(st["cursor"].cpu().numpy().astype(np.int64), m["cursor"]), (tag, "cursor")
    assert np.array_equal(st["init_cursor"].cpu().numpy().astype(np.int64), m["init_cursor"]), (tag, "init_cursor")
    assert np.array_equal(st["cur_slot"].cpu().numpy().astype(np.int64), m["cur_slot"]), (tag, "cur_slot")
    assert np.array_equal(st["rng"].cpu().numpy().view(np.uint64).reshape(m["rng"].shape), m["rng"]), (tag, "the action stream")


def state_of(env):
    st = env.env.state
    return [t.clone() for t in (st.rng, st.cursor, st.init_cursor, st.cur_slot)]


@pytest.mark.parametrize("name", [c.name for c in H.CASES])
def test_kernel_against_the_mirror_and_eval_td_alone(name, gpu):
    c = H.BY_NAME[name]
    assert not c.shape[2]
    m = H.host(c)
    env = fresh_env(c, gpu)
    before = state_of(env)
    kw = H.population_args(c)
    o = env.eval_td_population(q=H.q_init_of(c), tie=device_tie(c), episode0=c.episode0, n_episodes=c.n_episodes, state=True, **kw)
    torch.cuda.synchronize()
    assert o["_kernel"] == "k_eval_queue_pop" and tuple(o["q"].shape) == (c.L, c.S, c.log.nZ, c.log.nA)
    assert_rows(o, m, c, name)
    assert_state(o["_state"], m, name)
    assert all(torch.equal(a, b) for a, b in zip(before, state_of(env))), (name, "a query")
    # row [l, j] is BatchedQueueEvaluator.eval_td run alone with learner l's setting on the same seeds: every behaviour
    pi, q0, mt = H.pi_of(c), H.q_init_of(c), H.mt_of(c)
    a_ep, e_ep = H.schedules(c)
    for l in range(c.L):
        one = fresh_env(c, gpu)
        tie = c.tie if mt is None else mt[l]
        a = one.eval_td(pi[l] if c.pi_per_learner else pi, c.gamma[l], c.mode, c.alpha[l], q=q0[l], n_episodes=c.n_episodes, ep_cap=kw["ep_cap"],
                        trace_cap=kw["trace_cap"], behaviour=c.behaviour[l], epsilon=c.epsilon[l], alpha_ep=None if a_ep is None else a_ep[l],
                        epsilon_ep=None if e_ep is None else e_ep[l], snap_cap=kw["snap_cap"], snap_stride=kw["snap_stride"], tie=tie, episode0=c.episode0)
        torch.cuda.synchronize()
        for k in SCALARS + tuple(k for k in keys_of(c) if k != "beh_arg" or c.behaviour[l] == H.E):
            assert torch.equal(a[k], o[k][l]), (name, l, k, "eval_td alone")
        for x, k in zip(state_of(one), ("rng", "cursor", "init_cursor", "cur_slot")):
            assert torch.equal(x, o["_state"][k][l]), (name, l, k, "eval_td alone: the state left")


@pytest.mark.parametrize("name", ["qlearn-every-behaviour-fresh", "qlearn-eps-schedules-episode"])
def test_two_episodes_then_a_resumed_call(name, gpu):
    """max_episodes = 2, then every learner resumed (L = 1) from the state its rollouts left -- episode0 and the schedules advanced by the two
    episodes -- against ONE run of the mirror."""
    c = H.BY_NAME[name]
    m = H.host(c)
    kw = H.population_args(c)
    env = fresh_env(c, gpu)
    a = env.eval_td_population(q=H.q_init_of(c), tie=device_tie(c), episode0=c.episode0, n_episodes=2, state=True, **kw)
    assert (a["n_ep"] == 2).all() and (a["status"] == H.ST_OK).all()
    st, pi = a["_state"], H.pi_of(c)
    for l in range(c.L):
        e = fresh_env(c, gpu)
        own = e.env.state
        own.rng.copy_(st["rng"][l]), own.cursor.copy_(st["cursor"][l]), own.init_cursor.copy_(st["init_cursor"][l]), own.cur_slot.copy_(st["cur_slot"][l])
        sched = lambda x: None if x is None else x[l, 2:]  # noqa: E731
        b = e.eval_td_population(c.mode, c.alpha[l], c.gamma[l], c.behaviour[l], c.epsilon[l], pi=pi, q=a["q"][l:l + 1], alpha_ep=sched(kw["alpha_ep"]),
                                 epsilon_ep=sched(kw["epsilon_ep"]), tie="episode" if c.tie == "episode" else a["tie_mt"][l:l + 1], episode0=c.episode0 + 2,
                                 trace_cap=kw["trace_cap"], ep_cap=kw["ep_cap"], state=True)
        torch.cuda.synchronize()
        for j in range(c.S):
            sa, sb = int(a["steps"][l, j]), int(b["steps"][0, j])
            assert 2 + int(b["n_ep"][0, j]) == m["n_ep"][l, j] and sa + sb == m["steps"][l, j], (name, l, j)
            for k in ("trace_row", "trace_pop", "td_err"):
                both = np.concatenate([a[k][l, j, :sa].cpu().numpy(), b[k][0, j, :sb].cpu().numpy()])
                assert np.array_equal(both, m[k][l, j, :sa + sb]), (name, l, j, k)
            gs = np.concatenate([a["ep_g"][l, j, :2].cpu().numpy(), b["ep_g"][0, j, :int(b["n_ep"][0, j]) + 1].cpu().numpy()])
            assert np.array_equal(gs, m["ep_g"][l, j, :m["n_ep"][l, j] + 1]), (name, l, j, "ep_g")
        for k in ("q", "status", "obs_row", "tie_mt"):
            assert np.array_equal(as_host(b[k][0]), m[k][l]), (name, l, k)
        assert_state({k: v[0] for k, v in b["_state"].items()}, {k: m[k][l] for k in ("cursor", "init_cursor", "cur_slot", "rng")}, (name, l))


def population_of(c):
    """TDPopulation of the case with pi / Q_init [nS, nA] by caller state id (nS = nZ; a negative state is NumPy's wrap), and Q_init [L, nS, nA]"""
    from rl_offline_simulation_amd.evaluators import TDPopulation
    lg = c.log
    idx = (lg.z_lo + np.arange(lg.nZ)) % lg.nZ
    return TDPopulation("qlearn" if c.mode == H.QLEARN else "expsarsa", list(c.alpha), list(c.gamma), list(c.epsilon), [NAMES[b] for b in c.behaviour],
                        pi=_scatter(H.pi_of(c), idx), Q_init=_scatter(H.q_init_of(c)[:, 0], idx)), idx


def _scatter(x, idx):
    out = np.zeros_like(x)
    out[..., idx, :] = x
    return out


@pytest.mark.parametrize("name", ["qlearn-every-behaviour-fresh", "qlearn-every-behaviour-neg-state"])
def test_run_queue_tiles_curves_and_best(name, gpu):
    c = H.BY_NAME[name]
    assert c.q0 == "zero" and c.S == 5
    m = H.host(c)
    pop, idx = population_of(c)
    tie = "episode" if c.tie == "episode" else H.mt_of(c)
    res = []
    for tile in (None, 2):  # one launch, and tiles of 2 + 2 + 1 seeds
        r = pop.run_queue(c.log.arrays(), c.seeds, action_seeds=c.action_seeds, tie=tie, tile=tile, trace_cap=c.log.N + 1)
        torch.cuda.synchronize()
        res.append(r)
        ep_cap = r.Gs.shape[2]
        assert tuple(r.Q.shape) == (c.L, c.S, c.log.nZ, c.log.nA) and np.array_equal(r.Q.cpu().numpy()[:, :, idx], m["q"]), (name, tile)
        assert np.array_equal(r.n_ep.cpu().numpy(), m["n_ep"]) and np.array_equal(r.steps.cpu().numpy(), m["steps"]), (name, tile)
        assert np.array_equal(r.Gs.cpu().numpy(), m["ep_g"][:, :, :ep_cap]) and np.array_equal(r.status.cpu().numpy(), m["status"]), (name, tile)
        assert np.array_equal(r.td_err.cpu().numpy(), m["td_err"]) and np.array_equal(as_host(r.tie_mt), m["tie_mt"]), (name, tile)
        n, mean, var = H.curves(m["ep_g"][:, :, :ep_cap], m["n_ep"])
        assert np.array_equal(r.curve_n.cpu().numpy(), n)
        assert np.array_equal(r.curve_mean.cpu().numpy().view(np.uint64), mean.view(np.uint64))  # (bits: NaN where no seed got that far)
        assert np.array_equal(r.curve_var.cpu().numpy().view(np.uint64), var.view(np.uint64))
        assert ((n > 0) & (n < c.S)).any()
        for k in (1, 3):  # best(last=k) ignores the points that not every seed reached
            score = [float(np.mean(mean[l, np.nonzero(n[l] == c.S)[0][-k:]])) if (n[l] == c.S).any() else -np.inf for l in range(c.L)]
            assert r.best(last=k) == int(np.argmax(score))
    for k in ("Q", "Gs", "n_ep", "steps", "status", "curve_n", "td_err", "tie_mt"):
        assert torch.equal(getattr(res[0], k), getattr(res[1], k)), (name, k, "tile = 2 against one tile")
    # the default action seeds are the sampler seeds
    r = pop.run_queue(c.log.arrays(), c.seeds, tie=tie, n_episodes=2)
    r2 = pop.run_queue(c.log.arrays(), c.seeds, action_seeds=c.seeds, tie=tie, n_episodes=2)
    assert torch.equal(r.Q, r2.Q) and not torch.equal(r.Q, res[0].Q) and (r.n_ep <= 2).all()


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(f)[:-4] for f in FIXTURES])
def test_recorded_reference_drivers_through_run_queue(path, gpu):
    from rl_offline_simulation_amd.evaluators import TDPopulation
    d, log = np.load(path), golden_log(path)
    nS, gam, al = int(d["nS"]), float(d["gamma"]), float(d["alpha"])
    kind = {"qu": "fixed", "qe": "eps_greedy", "qs": "eps_greedy", "qg": "greedy", "qf": "soft_greedy", "es": "fixed"}
    for s in (int(v) for v in d["seeds"]):
        for tag in TD_RUNS:
            k = f"s{s}_{tag}_"
            n = int(d[k + "n"])
            mode, beh, eps, q_given, sched = RUNS[tag]
            pop = TDPopulation("expsarsa" if mode == Q.EXPSARSA else "qlearn", ALPHA_SCHED if sched else al, gam, epsilon=EPS_SCHED if sched else eps,
                               behaviour=kind[tag], pi=d["pi"] if tag == "es" else None, Q_init=d["q_init"] if q_given else None)
            with torch.cuda.device(gpu):
                res = pop.run_queue(log.arrays(), [s], n_episodes=n, action_seeds=[1000 + s], tie="episode", trace_cap=log.N + 1)
            torch.cuda.synchronize()
            steps = int(res.steps[0, 0])
            assert int(res.n_ep[0, 0]) == n and int(res.status[0, 0]) == Q.ST_OK and tuple(res.Q.shape) == (1, 1, nS, log.nA), k
            assert np.array_equal(res.Gs[0, 0, :n].cpu().numpy(), d[k + "Gs"]) and np.array_equal(as_host(res.tie_mt[0, 0]), d[k + "mt"]), k
            if tag == "es":  # (the reference's `@` is BLAS: its order of summation is not ours)
                assert np.abs(res.Q[0, 0].cpu().numpy() - d[k + "Q"]).max() <= 1e-12 and np.abs(res.td_err[0, 0, :steps].cpu().numpy() - d[k + "td"]).max() <= 1e-12, k
            else:
                assert np.array_equal(res.Q[0, 0].cpu().numpy(), d[k + "Q"]) and np.array_equal(res.td_err[0, 0, :steps].cpu().numpy(), d[k + "td"]), k


def test_what_is_refused(gpu):
    from rl_offline_simulation_amd import _lib as L
    from rl_offline_simulation_amd.evaluators import BatchedQueueEvaluator, TDPopulation
    c = H.BY_NAME["qlearn-eps-first"]
    env = fresh_env(c, gpu)
    pop = TDPopulation("qlearn", 0.1, 0.9, epsilon=0.1, behaviour="eps_greedy")
    with pytest.raises(ValueError, match="different lengths"):
        env.eval_td_population(L.TD_QLEARN, [0.1, 0.2], [0.9, 0.8, 0.7])
    with pytest.raises(ValueError, match="tie_mt"):
        env.eval_td_population(L.TD_QLEARN, 0.1, 0.9, L.BEHAVIOUR_EPS_GREEDY, 0.1, tie=np.zeros((1, c.S + 1, 625), np.uint32))
    with pytest.raises(ValueError, match="tie_mt"):
        pop.run_queue(c.log.arrays(), [1, 2], tie=np.zeros((2, 2, 625), np.uint32))
    with pytest.raises(ValueError, match="action_seeds"):
        pop.run_queue(c.log.arrays(), [1, 2], action_seeds=[1, 2, 3])
    with pytest.raises(ValueError, match="no seed"):
        pop.run_queue(c.log.arrays(), [])
    # sparse state ids: the table compacts them to ranks, the one-launch drivers have no [nZ, nA] rows for them
    z, a, r, zn, done, p, t0 = c.log.arrays()
    sparse = BatchedQueueEvaluator(z * 100000, a, r, zn * 100000, done, p, t0, R=2, device=gpu)
    assert sparse.nZ is None
    with pytest.raises(L.OffsimError, match="dense state ids"):
        sparse.eval_td_population(L.TD_QLEARN, 0.1, 0.9)
    with pytest.raises(L.OffsimError, match="dense state ids"):
        pop.run_queue((z * 100000, a, r, zn * 100000, done, p, t0), [1, 2])
    # n_slots = 6725 with a learner: one rollout's carve exceeds 160 KiB -- refused before anything is launched
    n = Q.LDS_SLOTS["refused"]
    assert H.launch_shape(n, 5, 1, 2)[2]
    lg = Q.make_log(4000, 5, 5, 31, n_slots=n)  # (2000 filler pairs: enough distinct ids for the table to stay dense)
    big = BatchedQueueEvaluator(*lg.arrays(), R=2, device=gpu)
    assert big.table.n_slots == n
    big.reset_sampler([1, 2])
    before = state_of(big)
    with pytest.raises(L.OffsimError, match=f"offsim error {L.EUNSUPPORTED}: eval_queue_pop: .*160 KiB"):
        big.eval_td_population(L.TD_QLEARN, 0.1, 0.9, L.BEHAVIOUR_EPS_GREEDY, 0.1)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(before, state_of(big)))
