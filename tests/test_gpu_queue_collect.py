"""VectorQueueEvaluator.collect / collect_ppo / collect_ppo_population (offsim_queue_collect*, csrc/collect_queue.hpp) on the device, every
case of tests/queue_collect_host.py held bit for bit to the plain-Python mirror: rows, drawn actions, flags, status and every piece of
carried state; probs to MLPPolicy.forward, the critic's records to MLPValue.forward (bit for bit), logp by tests/test_gpu_ppo.py's rule
(exp(logp) against probs[a] within 1e-6; the MLP form against torch's log_softmax within 2e-6).  Then the identities: split calls,
reset(mask) between calls, the population against single learners, PPOLearner.fit against the loop written by hand, strict mode's
KeyError((z, a)), and the reference's own fixtures through the kernel."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import queue_collect_host as H  # noqa: E402
import queue_host as Q  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "queue_collect", "*.npz")))
ACT = {"tanh": torch.nn.Tanh, "relu": torch.nn.ReLU}


@pytest.fixture(scope="module")
def gpu():
    from rl_offline_simulation_amd import _lib
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    _lib.load()
    return torch.device("cuda", 0)


class _LookupEncoder:
    def __init__(self, obs, z, next_obs, z_next):
        self.pairs = [(np.asarray(obs), np.asarray(z)), (np.asarray(next_obs), np.asarray(z_next))]

    def encode(self, x):
        for a, z in self.pairs:
            if np.array_equal(np.asarray(x), a):
                return z
        raise AssertionError("unknown observations")


def _env(log, E, obs=None, nobs=None, strict=False):
    """A VectorQueueEvaluator over `log`: with observations (and the lookup back to the states), or with the states as observations."""
    from rl_offline_simulation_amd import OfflineDataset, ProbDistribution, spaces
    from rl_offline_simulation_amd.evaluators import VectorQueueEvaluator
    discrete = obs is None
    ospace = spaces.Discrete(log.nZ) if discrete else spaces.Box(low=-np.inf, high=np.inf, shape=tuple(obs.shape[1:]), dtype=obs.dtype)
    ds = OfflineDataset(observation_space=ospace, action_space=spaces.Discrete(log.nA), action_dist_type=ProbDistribution.Discrete,
                        observations=log.z if discrete else obs, actions=log.a, action_distributions=log.p_log, rewards=log.r,
                        next_observations=log.z_next if discrete else nobs, terminals=log.done, steps=np.where(log.t0, 0, 1))
    if discrete:
        return VectorQueueEvaluator(ds, num_envs=E, strict=strict)
    return VectorQueueEvaluator(ds, num_envs=E, num_states=log.nZ, encoder=_LookupEncoder(obs, log.z, nobs, log.z_next), strict=strict)


def _net(dO, n_out, act, seed, hidden=16, gain=3.0):
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(dO, hidden), ACT[act](), torch.nn.Linear(hidden, hidden), ACT[act](), torch.nn.Linear(hidden, n_out))
    with torch.no_grad():
        for m in net:
            if isinstance(m, torch.nn.Linear):
                m.weight.mul_(gain)
    return net


def _nets(c, seed=0, dO=4):
    from rl_offline_simulation_amd.evaluators import MLPPolicy, MLPValue
    return MLPPolicy.from_torch(_net(dO, c.nA, c.act, 100 + seed)), MLPValue.from_torch(_net(dO, 1, c.act, 200 + seed, gain=1.0))


def _same(x, y):
    """equal, NaN in the same places"""
    return torch.equal(torch.nan_to_num(x.double(), nan=-1e300), torch.nan_to_num(y.double(), nan=-1e300))


def _start(c, env, reset_envs="case"):
    env.reset_sampler(c.seeds)
    env.set_action_seeds(c.action_seeds)
    which = c.reset_envs if reset_envs == "case" else reset_envs
    if which is None:
        env.reset()
    else:
        m = torch.zeros(c.E, dtype=torch.bool, device=env.obs.device)
        m[list(which)] = True
        env.reset(mask=m)


def _setup(c, gpu, strict=False):
    """(env, the policy collect takes, the critic or None, mirror keyword arguments, (actor, critic) networks or None)"""
    from rl_offline_simulation_amd.evaluators import RowPolicy, RowValue
    from rl_offline_simulation_amd.evaluators.obs_policy import obs_tensor
    lg = c.log
    nets = None
    if c.form == "tabular":  # observations are the states (a critic beside it reads the state id, dO = 1)
        env = _env(lg, c.E, strict=strict)
    else:
        obs, nobs = H.observations(lg, 4, c.log_seed, c.xtype)
        env = _env(lg, c.E, obs, nobs, strict=strict)
    crit = None
    if c.form == "mlp" or c.vf is not None:
        nets = _nets(c, c.log_seed, 1 if c.form == "tabular" else 4)
        xn, x0 = obs_tensor(env._next_obs, gpu), obs_tensor(env._obs, gpu)
    if c.form == "mlp":
        pol = nets[0]
        kw = dict(P_next=pol.forward(xn).cpu().numpy(), P_init=pol.forward(x0).cpu().numpy())  # the device's own offsim_policy_mlp tables
    elif c.form == "rows":
        pn, p0 = H.row_tables(lg, c.log_seed, c.ptype, c.nan_rows)
        pol, kw = RowPolicy(pn, p0), dict(P_next=pn, P_init=p0)
    else:
        rows = c.pi()
        pol, kw = rows[(np.arange(lg.nZ) - lg.z_lo) % lg.nZ], dict(pi=rows)  # indexed by the state id, NumPy's wrap for z = -1
    if c.vf == "mlp":
        crit = nets[1]
    elif c.vf == "rows":
        crit = RowValue(nets[1].forward(xn), nets[1].forward(x0))
    return env, pol, crit, kw, nets


def _flags(col):
    return ((col.row >= 0).to(torch.uint8) * H.SERVED + col.terminated.to(torch.uint8) * H.TERMINATED + col.truncated.to(torch.uint8) * H.TRUNCATED
            + col.reset.to(torch.uint8) * H.RESET + col.alive.to(torch.uint8) * H.ALIVE).cpu().numpy()


def _check_records(env, col, outs, k0=0):
    """rows, drawn actions, flags and status of every environment against the mirror's `outs`"""
    row, drawn, fl, status = col.row.cpu().numpy(), env.drawn_action.cpu().numpy(), _flags(col), col.status.cpu().numpy()
    for k, o in enumerate(outs):
        assert np.array_equal(row[:, k0 + k], o["row"]), ("row", k)
        assert np.array_equal(drawn[:, k0 + k], o["action"]), ("action", k)
        assert np.array_equal(fl[:, k0 + k], o["flags"]), ("flags", k)
        assert status[k0 + k] == o["status"], ("status", k, status[k0 + k], o["status"])


def _check_state(env, envs, k0=0):
    s = env.env.state
    cursor, ic, slot, rng = s.cursor.cpu().numpy(), s.init_cursor.cpu().numpy(), s.cur_slot.cpu().numpy(), s.rng.cpu().numpy().view(np.uint64).reshape(-1, 4)
    ep_t, obs_row, alive = env._ep_t.cpu().numpy(), env._obs_row.cpu().numpy(), env.alive.cpu().numpy()
    for k, e in enumerate(envs):
        st, r = e.state(), k0 + k
        assert np.array_equal(cursor[r].astype(np.int64), st["cursor"]), ("cursor", k)
        assert (int(ic[r]), int(slot[r]), int(ep_t[r]), bool(alive[r])) == (st["init_cursor"], st["cur_slot"], st["ep_t"], st["alive"]), ("state", k)
        if e.sm.cur is not None or st["obs_row"] == -1:
            assert int(obs_row[r]) == st["obs_row"], ("obs_row", k)
        assert np.array_equal(rng[r], st["rng"]), ("rng", k)


def _check_obs(env, col, outs):
    """obs records, final_obs and self.obs: the rows the mirror says the policy was asked at / the environment holds"""
    if col.obs is None:
        return
    at = np.stack([o["asked_at"] for o in outs], 1)
    src = torch.where(torch.as_tensor(at >= 0, device=col.obs.device).reshape(at.shape + (1,) * (col.obs.dim() - 2)),
                      env._next_obs[torch.as_tensor(np.clip(at, 0, None), device=col.obs.device)],
                      env._obs[torch.as_tensor(np.clip(-2 - at, 0, None), device=col.obs.device)])
    asked = torch.as_tensor(np.stack([o["action"] for o in outs], 1) >= 0, device=col.obs.device)
    m = asked.reshape(asked.shape + (1,) * (col.obs.dim() - 2))
    assert torch.equal(torch.where(m, col.obs, torch.zeros_like(col.obs)), torch.where(m, src, torch.zeros_like(src)))
    assert bool((torch.where(m, torch.zeros_like(col.obs), col.obs) == 0).all())
    assert torch.equal(col.final_obs, env.obs)


def _run_case(c, gpu):
    from rl_offline_simulation_amd.evaluators.obs_policy import obs_tensor
    env, pol, crit, kw, nets = _setup(c, gpu)
    _start(c, env)
    envs = c.envs()
    outs = [H.collect(e, c.T, c.cap, **kw) for e in envs]
    T, E, nA = c.T, c.E, c.nA
    if crit is None:
        col = env.collect(pol, T, max_episode_steps=c.cap or None, record_obs=c.record_obs, record_probs=c.record_probs)
        batch = None
    else:
        batch = env.collect_ppo(pol, crit, T, max_episode_steps=c.cap or None, bootstrap=c.bootstrap)
        col = batch.collected
    _check_records(env, col, outs)
    _check_state(env, envs)
    _check_obs(env, col, outs)
    served = col.row >= 0
    asked = torch.as_tensor(np.stack([o["action"] for o in outs], 1) >= 0, device=gpu) if T else served
    rl = col.row.clamp(min=0).long()
    # action / reward / next_obs of the served row; the drawn action is the row's logged action
    assert torch.equal(col.action[served].long(), env._a[rl][served].long()) and torch.equal(col.reward[served], env._r[rl][served])
    assert torch.equal(env.drawn_action[served].long(), env._a[rl][served].long()) and bool((col.action[~served] == 0).all())
    if not c.record_obs:
        assert col.obs is None
    if not c.record_probs:
        assert col.probs is None
    elif T:
        want = torch.as_tensor(np.stack([o["p"] for o in outs], 1).astype(np.float32), device=gpu)
        assert torch.equal(col.probs[asked].view(torch.int32), want[asked].view(torch.int32)) and bool((col.probs[~asked] == 0).all())
        if c.form == "mlp" and c.record_obs:  # probs is MLPPolicy.forward at the observation asked at, bit for bit
            fw = pol.forward(obs_tensor(col.obs.reshape(T * E, -1), gpu)).reshape(T, E, nA)
            assert torch.equal(col.probs[asked], fw[asked])
    if batch is not None and T:
        critic = nets[1]
        dO = critic.dO
        v = batch.valid
        assert torch.equal(v, served) and int(v.sum()) > 0
        want = critic.forward(obs_tensor(batch.obs.reshape(T * E, dO), gpu)).reshape(T, E)
        assert torch.equal(batch.val[v], want[v]) and bool((batch.val[~v] == 0).all())
        had = torch.as_tensor([o["status"] != H.ST_INACTIVE for o in outs], device=gpu)
        fv = critic.forward(obs_tensor(env.obs.reshape(E, dO), gpu))
        assert torch.equal(batch.final_value[had], fv[had]) and bool((batch.final_value[~had] == 0).all())
        if c.bootstrap == "spinup":
            tr = col.truncated & ~col.terminated
            assert bool(tr.any())
            vt = critic.forward(obs_tensor(env._next_obs, gpu))[rl]
            assert torch.equal(batch.v_trunc[tr], vt[tr]) and bool((batch.v_trunc[~tr] == 0).all())
        act = batch.act.long()
        pa = col.probs.gather(2, act.unsqueeze(-1))[..., 0]
        assert float((batch.logp.exp() - pa)[v].abs().max()) <= 1e-6 and bool((batch.logp[~v] == 0).all())
        if c.form == "mlp":
            h = obs_tensor(batch.obs.reshape(T * E, dO), gpu).float()
            ws = pol.weights
            for i, (W, b) in enumerate(ws):
                h = h @ W.to(gpu).T + b.to(gpu)
                if i < len(ws) - 1:
                    h = torch.tanh(h) if c.act == "tanh" else torch.relu(h)
            ls = torch.log_softmax(h.reshape(T, E, nA), -1).gather(2, act.unsqueeze(-1))[..., 0]
            assert float((batch.logp - ls)[v].abs().max()) <= 2e-6
    return env, outs


@pytest.mark.parametrize("c", H.CASES, ids=[c.name for c in H.CASES])
def test_case_equals_the_mirror(gpu, c):
    _run_case(c, gpu)


def test_two_workgroups_and_the_case_list(gpu):
    """E = 9 is two workgroups of 8 waves, the second with one live wave; T = 0 leaves every piece of state where it was"""
    assert H.BY_NAME["mlp-f32"].E == 9
    c = H.BY_NAME["T0"]
    env, pol, _, _, _ = _setup(c, gpu)
    _start(c, env)
    before = [x.clone() for x in (env.obs, env.alive, env._ep_t, env._obs_row, env.env.state.cursor, env.env.state.rng, env.env.state.cur_slot)]
    col = env.collect(pol, 0)
    assert col.row.shape == (0, c.E) and bool((col.status == 0).all())
    for x, y in zip(before, (env.obs, env.alive, env._ep_t, env._obs_row, env.env.state.cursor, env.env.state.rng, env.env.state.cur_slot)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("name", ["mlp-f32", "rows-f64", "vf-mlp-spinup"])
def test_three_calls_equal_one_and_reset_between_calls(gpu, name):
    c = H.BY_NAME[name]
    T = c.T // 2
    a, pol, crit, kw, _ = _setup(c, gpu)
    b = _setup(c, gpu)[0]
    _start(c, a)
    _start(c, b)

    def run(env, steps):
        if crit is None:
            return env.collect(pol, steps, max_episode_steps=c.cap), None
        p = env.collect_ppo(pol, crit, steps, max_episode_steps=c.cap, bootstrap=c.bootstrap, normalize=False)
        return p.collected, p

    one, p1 = run(a, 3 * T)
    drawn1 = a.drawn_action.clone()
    parts, drawn3 = [], []
    for _ in range(3):
        parts.append(run(b, T))
        drawn3.append(b.drawn_action.clone())
    for f in ("row", "obs", "probs", "terminated", "truncated", "reset", "alive"):
        assert torch.equal(getattr(one, f), torch.cat([getattr(p[0], f) for p in parts])), f
    assert torch.equal(drawn1, torch.cat(drawn3)) and torch.equal(one.status, parts[-1][0].status) and torch.equal(one.final_obs, parts[-1][0].final_obs)
    if p1 is not None:
        for f in ("val", "logp"):
            assert torch.equal(getattr(p1, f), torch.cat([getattr(p[1], f) for p in parts])), f
        assert torch.equal(p1.final_value, parts[-1][1].final_value)
    sa, sb = a.env.state, b.env.state
    for x, y in ((sa.cursor, sb.cursor), (sa.rng, sb.rng), (sa.cur_slot, sb.cur_slot), (sa.init_cursor, sb.init_cursor), (a._ep_t, b._ep_t),
                 (a._obs_row, b._obs_row), (a.alive, b.alive), (a.obs, b.obs)):
        assert torch.equal(x, y)
    # reset(mask) between calls: the mirror resets the same environments
    envs = c.envs()
    outs = [H.collect(e, 3 * T, c.cap, **kw) for e in envs]
    mask = torch.zeros(c.E, dtype=torch.bool, device=gpu)
    mask[[1, 4, 8]] = True
    a.reset(mask=mask)
    for k in (1, 4, 8):
        envs[k].reset()
    col, _ = run(a, T)
    _check_records(a, col, [H.collect(e, T, c.cap, **kw) for e in envs])
    _check_state(a, envs)


def test_population_equals_single_learners(gpu):
    from rl_offline_simulation_amd.evaluators import PPOPopulation
    c = H.BY_NAME["vf-mlp-spinup"]
    nl, E, T = 3, 3, 24
    lg = c.log
    obs, nobs = H.observations(lg, 4, c.log_seed, c.xtype)
    nets = [_nets(c, 40 + l) for l in range(nl)]
    pop = PPOPopulation([n[0] for n in nets], [n[1] for n in nets])
    env = _env(lg, nl * E, obs, nobs)
    env.reset_sampler(c.seeds[:nl * E])
    env.set_action_seeds(c.action_seeds[:nl * E])
    env.reset()
    pb = env.collect_ppo_population(pop, T, max_episode_steps=c.cap, bootstrap="spinup")
    drawn = env.drawn_action.clone()
    assert int(pb.valid.sum()) > nl * E * T // 2
    for l in range(nl):
        one = _env(lg, E, obs, nobs)
        sl = slice(l * E, (l + 1) * E)
        one.reset_sampler(c.seeds[sl])
        one.set_action_seeds(c.action_seeds[sl])
        one.reset()
        p = one.collect_ppo(nets[l][0], nets[l][1], T, max_episode_steps=c.cap, bootstrap="spinup")
        for f in ("obs", "act", "rew", "val", "logp", "adv", "adv_raw", "ret", "valid", "v_trunc"):
            assert torch.equal(getattr(pb, f)[:, sl], getattr(p, f)), (l, f)
        for f in ("row", "probs", "terminated", "truncated", "reset", "alive"):
            assert torch.equal(getattr(pb.collected, f)[:, sl], getattr(p.collected, f)), (l, f)
        assert torch.equal(pb.final_value[sl], p.final_value) and torch.equal(drawn[:, sl], one.drawn_action)
        assert torch.equal(pb.collected.status[sl], p.collected.status) and torch.equal(pb.collected.final_obs[sl], p.collected.final_obs)
        s, so = env.env.state, one.env.state
        for x, y in ((s.cursor[sl], so.cursor), (s.rng.reshape(-1, 4)[sl], so.rng.reshape(-1, 4)), (s.cur_slot[sl], so.cur_slot),
                     (s.init_cursor[sl], so.init_cursor), (env._ep_t[sl], one._ep_t), (env._obs_row[sl], one._obs_row), (env.alive[sl], one.alive)):
            assert torch.equal(x, y), l


def test_fit_equals_the_loop_by_hand(gpu):
    from rl_offline_simulation_amd.evaluators import EpisodeTracker, PPOLearner, ppo_epoch_log
    c = H.BY_NAME["vf-mlp-reference"]
    T, epochs = 16, 2
    obs, nobs = H.observations(c.log, 4, c.log_seed, c.xtype)
    envs, learners = [], []
    for _ in range(2):
        env = _env(c.log, c.E, obs, nobs)
        _start(c, env)
        envs.append(env)
        a, v = _nets(c, 7)
        learners.append(PPOLearner(a, v, train_pi_iters=3, train_v_iters=3))
    log = learners[0].fit(envs[0], epochs, T, max_episode_steps=c.cap)
    tracker = EpisodeTracker(c.E, gpu)
    for ep in range(epochs):
        b = envs[1].collect_ppo(learners[1].actor, learners[1].critic, T, max_episode_steps=c.cap)
        lg = ppo_epoch_log(b, tracker)
        info = learners[1].update(b)
        for k in lg._fields:
            assert _same(getattr(log, k)[ep], getattr(lg, k)), k
        for k in info._fields:
            assert _same(getattr(log, k)[ep], getattr(info, k)), k
    for net in ("actor", "critic"):
        sa, sb = getattr(learners[0], net).state_dict(gpu), getattr(learners[1], net).state_dict(gpu)
        assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert torch.equal(envs[0].env.state.rng, envs[1].env.state.rng) and torch.equal(envs[0].env.state.cursor, envs[1].env.state.cursor)
    assert int(log.TotalEnvInteracts[-1]) == epochs * T * c.E


def test_strict_raises_the_pair(gpu):
    c = H.BY_NAME["holes-keyerror"]
    env, pol, _, kw, _ = _setup(c, gpu, strict=True)
    _start(c, env)
    envs = c.envs()
    outs = [H.collect(e, c.T, c.cap, **kw) for e in envs]
    k = [o["status"] for o in outs].index(H.ST_KEYERROR)
    a = int(outs[k]["action"][np.flatnonzero(outs[k]["action"] >= 0)[-1]])
    z = envs[k].sm.cur
    assert (z, a) not in envs[k].sm.queues
    with pytest.raises(KeyError) as ei:
        env.collect(pol, c.T, max_episode_steps=c.cap)
    assert ei.value.args[0] == (z, a)


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_reference_fixtures_through_the_kernel(gpu, path):
    from rl_offline_simulation_amd.evaluators import RowPolicy
    d = np.load(path)
    i = np.load(os.path.join(ROOT, "tests", "golden", os.path.basename(path)))
    log = Q.Log(*(i["in_" + k] for k in ("z", "a", "r", "z_next", "done", "p_log", "t0")))
    seeds, T = [int(s) for s in d["seeds"]], int(d["T"])
    obs, nobs = H.observations(log, 4, 0)
    for cap in d["caps"]:
        env = _env(log, len(seeds), obs, nobs)
        env.reset_sampler(seeds)
        env.set_action_seeds([500 + s for s in seeds])
        env.reset()
        col = env.collect(RowPolicy(d["P_next"], d["P_init"]), T, max_episode_steps=int(cap))
        fl, rng = _flags(col), env.env.state.rng.cpu().numpy().view(np.uint64).reshape(-1, 4)
        for k, s in enumerate(seeds):
            key = f"s{s}_cap{cap}_"
            assert np.array_equal(col.row[:, k].cpu().numpy(), d[key + "rows"]) and np.array_equal(env.drawn_action[:, k].cpu().numpy(), d[key + "actions"])
            assert np.array_equal(fl[:, k], d[key + "flags"]) and int(col.status[k]) == int(d[key + "status"])
            assert np.array_equal(rng[k, :2], d[key + "rng"])
