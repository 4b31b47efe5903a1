"""PPOPopulation on the device: every population entry point against the single-learner path it stacks, bit for bit -- collect
(offsim_vector_collect_ppo_pop against L collect_ppo calls on environments of the same seeds), the per-learner advantage statistics
(offsim_ppo_advantages_pop against the single call on each contiguous slice), one gradient pass and the whole update (offsim_ppo_grad_pop /
offsim_ppo_update_pop against ppo_grad / PPOLearner.update per learner, with per-learner early stops and a learner without a valid
record), two epochs end to end, determinism, and the relu / three-action instances.  Learners are independent and the per-learner orders
coincide with the single path's, so every comparison is torch.equal: there is no tolerance here.

Base shape: L = 3 learners of E = 5 environments, T = 7 steps -- a workgroup of eight environments would straddle two learners, and a
learner's 35 records are one full tile of 32 and one partial."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_collect import _cartpole, _env, _state  # noqa: E402

pytestmark = pytest.mark.gpu
NL, NE, NT = 3, 5, 7
BATCH_FIELDS = ("obs", "act", "rew", "val", "logp", "adv", "adv_raw", "ret", "valid")
COLLECTED_FIELDS = ("obs", "probs", "row", "action", "reward", "next_obs", "terminated", "truncated", "reset", "alive")


@pytest.fixture(scope="module")
def gpu():
    from rl_offline_simulation_amd import _lib
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    _lib.load()
    return torch.device("cuda", 0)


_LOGS = {}


def _log(kind):
    """A CartPole-like f32 log of 2000 rows with its box-encoded states, made once: 'f32', 'f16' (the same rows with f16 observations) and
    'na3' (three actions under a uniform logging policy)."""
    if kind not in _LOGS:
        d = _cartpole(2000, 4, np.float32)
        if kind == "f16":
            d = dict(d, obs=d["obs"].astype(np.float16), next_obs=d["next_obs"].astype(np.float16))
        elif kind == "na3":
            n = len(d["a"])
            d = dict(d, a=np.random.default_rng(5).integers(0, 3, n).astype(d["a"].dtype), p_log=np.full((n, 3), 1.0 / 3.0, np.float32))
        _LOGS[kind] = d
    return _LOGS[kind]


def _torch_nets(seed, nA, act, hidden=16, dO=4):
    kind = {"tanh": torch.nn.Tanh, "relu": torch.nn.ReLU}[act]
    torch.manual_seed(seed)

    def mlp(out):
        return torch.nn.Sequential(torch.nn.Linear(dO, hidden), kind(), torch.nn.Linear(hidden, hidden), kind(), torch.nn.Linear(hidden, out),
                                   torch.nn.Identity())

    pi, v = mlp(nA), mlp(1)
    with torch.no_grad():
        pi[0].weight.mul_(3.0)  # (a policy that is far from uniform: different learners serve different rows)
    return pi, v


def _nets(nl=NL, nA=2, act="tanh", base=0):
    """(actors, critics) of nl learners, different weights per learner; every call makes fresh objects of the same weights"""
    from rl_offline_simulation_amd.evaluators import MLPPolicy, MLPValue
    pairs = [_torch_nets(1000 * base + 10 * l + 1, nA, act) for l in range(nl)]
    return [MLPPolicy.from_torch(p) for p, _ in pairs], [MLPValue.from_torch(v) for _, v in pairs]


def _seeds(nl=NL, ne=NE):
    return (np.arange(nl * ne) * 7 + 11).astype(np.int64)


def _envs(d, nl=NL, ne=NE):
    """(the population's environment on seeds s[0 : nl * ne], the learners' own on s[l * ne : (l + 1) * ne]), reset"""
    s = _seeds(nl, ne)
    whole = _env(**d, E=nl * ne)
    whole.reset_sampler(s)
    whole.reset()
    parts = []
    for l in range(nl):
        e = _env(**d, E=ne)
        e.reset_sampler(s[l * ne:(l + 1) * ne])
        e.reset()
        parts.append(e)
    return whole, parts


def _cols(x, l, ne=NE):
    return x[:, l * ne:(l + 1) * ne]


def _same_batch(p, singles, ne=NE):
    """every field of the population's PPOBatch against the learners' own batches"""
    for l, s in enumerate(singles):
        for f in BATCH_FIELDS:
            assert torch.equal(_cols(getattr(p, f), l, ne), getattr(s, f)), (l, f)
        for f in COLLECTED_FIELDS:
            assert torch.equal(_cols(getattr(p.collected, f), l, ne), getattr(s.collected, f)), (l, f)
        assert torch.equal(p.final_value[l * ne:(l + 1) * ne], s.final_value), l
        assert torch.equal(p.collected.final_obs[l * ne:(l + 1) * ne], s.collected.final_obs), l
        assert torch.equal(p.collected.status[l * ne:(l + 1) * ne], s.collected.status), l
        assert (p.v_trunc is None) == (s.v_trunc is None)
        if p.v_trunc is not None:
            assert torch.equal(_cols(p.v_trunc, l, ne), s.v_trunc), l
        assert torch.equal(p.adv_mean[l], s.adv_mean) and torch.equal(p.adv_std[l], s.adv_std), l


def _same_state(whole, parts, ne=NE):
    for l, e in enumerate(parts):
        for x, y in zip(_state(whole), _state(e)):
            assert torch.equal(x[l * ne:(l + 1) * ne], y), l
        assert torch.equal(whole._ep_t[l * ne:(l + 1) * ne], e._ep_t) and torch.equal(whole._obs_row[l * ne:(l + 1) * ne], e._obs_row), l


# ---- 1. collect ----
@pytest.mark.parametrize("log,cap,boot", [("f32", 500, "reference"), ("f32", 3, "spinup"), ("f16", 3, "reference")])
def test_collect_population_is_the_learners_own_collect(gpu, log, cap, boot):
    from rl_offline_simulation_amd.evaluators import PPOPopulation
    d = _log(log)
    whole, parts = _envs(d)
    actors, critics = _nets()
    pop = PPOPopulation(*_nets())
    served = 0
    for call in range(2):  # the second call starts from the carried state
        p = whole.collect_ppo_population(pop, NT, max_episode_steps=cap, bootstrap=boot)
        singles = [parts[l].collect_ppo(actors[l], critics[l], NT, max_episode_steps=cap, bootstrap=boot) for l in range(NL)]
        assert p.obs.shape[:2] == (NT, NL * NE) and p.adv_mean.shape == (NL,) and p.adv_std.shape == (NL,)
        if log == "f16":
            assert p.obs.dtype == torch.float16
        _same_batch(p, singles)
        _same_state(whole, parts)
        served += int(p.valid.sum())
        if cap == 3:
            assert bool(p.collected.truncated.any()) and bool(p.collected.reset.any())
    assert served > NT * NL * NE  # (most steps are served)
    # the learners differ: no two learners' columns hold the same probabilities
    assert not torch.equal(_cols(p.collected.probs, 0), _cols(p.collected.probs, 1))


# ---- 2. the advantages alone ----
def _records(T, R, seed, dev):
    from rl_offline_simulation_amd import _lib as L
    g = torch.Generator().manual_seed(seed)
    rew, val, vt = (torch.randn(T, R, generator=g) for _ in range(3))
    fv = torch.randn(R, generator=g)
    u = torch.rand(T, R, generator=g)
    served = u > 0.15
    term = served & (torch.rand(T, R, generator=g) < 0.2)
    trunc = served & (torch.rand(T, R, generator=g) < 0.2)
    flags = (served.to(torch.uint8) * L.COLLECT_SERVED + term.to(torch.uint8) * L.COLLECT_TERMINATED + trunc.to(torch.uint8) * L.COLLECT_TRUNCATED)
    return [x.to(dev).contiguous() for x in (rew, val, flags.to(torch.uint8), fv, vt)]


@pytest.mark.parametrize("boot", ["reference", "spinup"])
@pytest.mark.parametrize("T,nl,ne", [(NT, NL, NE), (3, 2, 300)])  # (300 environments: two blocks of partial sums per learner)
def test_advantages_population_against_the_single_call_on_each_slice(gpu, boot, T, nl, ne):
    from rl_offline_simulation_amd.evaluators.ppo_buffer import _advantages
    rew, val, flags, fv, vt = _records(T, nl * ne, 3, gpu)
    dead = nl - 1
    flags[:, dead * ne:] = 0  # the last learner's environments are all dead: n = 0
    vt = vt if boot == "spinup" else None
    for normalize in (True, False):
        adv_raw, ret, adv, mean, std = _advantages(rew, val, flags, fv, vt, 0.99, 0.97, normalize, boot, learners=nl)
        assert mean.shape == (nl,) and std.shape == (nl,)
        for l in range(nl):
            sl = slice(l * ne, (l + 1) * ne)
            one = _advantages(rew[:, sl].contiguous(), val[:, sl].contiguous(), flags[:, sl].contiguous(), fv[sl].contiguous(),
                              None if vt is None else vt[:, sl].contiguous(), 0.99, 0.97, normalize, boot)
            for got, want in zip((adv_raw[:, sl], ret[:, sl], adv[:, sl], mean[l], std[l]), one):
                assert torch.equal(got, want), (l, normalize)
        assert float(std[dead]) == 0.0 and float(mean[dead]) == 0.0 and torch.equal(adv[:, dead * ne:], adv_raw[:, dead * ne:])
        assert not normalize or float(std[0]) > 0.0


# ---- 3. one gradient pass ----
def _flat_batch(T, nl, ne, nets, seed, dev, nA=2):
    """A step-major [T, nl * ne] batch of random records; logp_old is the learner's own network's (torch, f32), so kl starts near 0."""
    g = torch.Generator().manual_seed(seed)
    R = nl * ne
    obs = torch.randn(T, R, 4, generator=g)
    act = torch.randint(0, nA, (T, R), generator=g, dtype=torch.int32)
    adv, ret = torch.randn(T, R, generator=g), torch.randn(T, R, generator=g)
    logp = torch.zeros(T, R)
    with torch.no_grad():
        for l, net in enumerate(nets):
            lp = torch.log_softmax(net.to_torch()(obs[:, l * ne:(l + 1) * ne]), -1)
            logp[:, l * ne:(l + 1) * ne] = lp.gather(-1, act[:, l * ne:(l + 1) * ne].long().unsqueeze(-1))[..., 0]
    valid = torch.rand(T, R, generator=g) > 0.2
    return {k: v.to(dev).contiguous() for k, v in dict(obs=obs, act=act, adv=adv, logp=logp, ret=ret, valid=valid).items()}


def _slice(batch, l, ne):
    return {k: v[:, l * ne:(l + 1) * ne].contiguous() for k, v in batch.items()}


@pytest.mark.parametrize("T,ne", [(1, 1), (NT, NE), (8, 8), (13, 5)])  # T * E = 1, 35, 64, 65: a lone record, the tile's edge either side
def test_grad_population_against_ppo_grad_per_learner(gpu, T, ne):
    from rl_offline_simulation_amd.evaluators import PPOPopulation, ppo_grad, ppo_grad_population
    actors, critics = _nets()
    pop = PPOPopulation(*_nets())
    b = _flat_batch(T, NL, ne, actors, 7, gpu)
    if T * ne > 1:
        b["valid"][0, :] = True
        b["valid"][-1, ::2] = False  # some invalid records in every learner
        b["act"][0, ne] = 5           # one action out of range (learner 1's first record)
        b["adv"][-1, 0] = float("nan")  # an invalid record may hold anything
    clips = [0.2, 0.05, 0.4]
    for kind, nets in (("actor", actors), ("critic", critics)):
        got = ppo_grad_population(pop, b, kind, clip_ratio=clips)
        assert got.grad.shape[0] == NL and got.n.shape == (NL,)
        for l in range(NL):
            want = ppo_grad(nets[l], _slice(b, l, ne), kind, clip_ratio=clips[l])
            assert torch.equal(got.grad[l], want.grad), (kind, l)
            for f in ("n", "loss", "kl", "entropy", "clipfrac"):
                assert torch.equal(getattr(got, f)[l], getattr(want, f)), (kind, l, f)
        if T * ne > 1:
            assert bool(torch.isfinite(got.grad).all()) and float(got.grad.abs().max()) > 0.0
            assert int(got.n[1]) == int(_slice(b, 1, ne)["valid"].sum()) - (1 if kind == "actor" else 0)


# ---- 4. the update ----
ITERS = 6
# Learner 0 never stops.  On the update test's batch the f64 host update (tests/ppo_update_host.py) gives learner 1 the kl trace 0, .0044,
# .0095, .0151, .0188, .0215 and learner 2 the trace 0, -.0064, -.0006, .0139, .0272, .0370: against 1.5 * target_kl = .012 and .01995 they
# stop at passes 3 and 4, each with a margin of 20 % or more either side.
PI_LR = [3e-4, 3e-3, 1e-2]
TARGET_KL = [1e9, 0.008, 0.0133]


def _learners(actors, critics, **kw):
    from rl_offline_simulation_amd.evaluators import PPOLearner
    return [PPOLearner(actors[l], critics[l], pi_lr=PI_LR[l], vf_lr=[1e-3, 2e-3, 5e-4][l], clip_ratio=[0.2, 0.1, 0.3][l], train_pi_iters=ITERS,
                       train_v_iters=ITERS, target_kl=TARGET_KL[l], **kw) for l in range(NL)]


def _population(**kw):
    from rl_offline_simulation_amd.evaluators import PPOPopulation
    return PPOPopulation(*_nets(), pi_lr=PI_LR, vf_lr=[1e-3, 2e-3, 5e-4], clip_ratio=[0.2, 0.1, 0.3], train_pi_iters=ITERS, train_v_iters=ITERS,
                         target_kl=TARGET_KL, **kw)


def _same_learners(pop, info, learners, infos, actors, critics, dev):
    """weights, m, v, t, every PPOUpdateInfo field and both traces of the population against the learners' own"""
    (pm, pv, pt), (vm, vv, vt) = pop.adam_state()
    for l, lrn in enumerate(learners):
        for f in info._fields:
            assert torch.equal(getattr(info, f)[l], getattr(infos[l], f)), (l, f)
        assert torch.equal(pop.pi_trace[l], lrn.pi_trace) or _same_with_nan(pop.pi_trace[l], lrn.pi_trace), l
        assert torch.equal(pop.v_trace[l], lrn.v_trace) or _same_with_nan(pop.v_trace[l], lrn.v_trace), l
        (am, av, at), (cm, cv, ct) = lrn.adam_state()
        assert torch.equal(pm[l], am) and torch.equal(pv[l], av) and int(pt[l]) == int(at), l
        assert torch.equal(vm[l], cm) and torch.equal(vv[l], cv) and int(vt[l]) == int(ct), l
        for mine, theirs in ((pop.actor(l), actors[l]), (pop.critic(l), critics[l])):
            ws, _ = theirs._device_weights(dev)
            for (W, b), (W1, b1) in zip(mine.weights, ws):
                assert torch.equal(W, W1.cpu()) and torch.equal(b, b1.cpu()), l


def _same_with_nan(a, b):
    """bitwise equality of two f64 tensors (NaN rows of a trace included)"""
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_update_population_against_the_learners_own_updates(gpu):
    actors, critics = _nets()
    b = _flat_batch(NT, NL, NE, actors, 9, gpu)
    learners = _learners(actors, critics)
    infos = [learners[l].update(_slice(b, l, NE)) for l in range(NL)]
    # the inputs must exercise the per-learner stop: checked on the SINGLE-learner results, before anything is compared
    stops = [int(i.StopIter) for i in infos]
    traces = [lrn.pi_trace.cpu() for lrn in learners]
    print("single-learner StopIter", stops, "kl", [t[:, 1].tolist() for t in traces])
    assert len(set(stops)) >= 2, stops
    assert any(s == ITERS - 1 and not bool(torch.isnan(t).any()) for s, t in zip(stops, traces)), stops
    assert any(bool(torch.isnan(t).any()) for t in traces), stops  # (and at least one learner does stop)
    pop = _population()
    info = pop.update(b)
    assert info.StopIter.shape == (NL,) and pop.pi_trace.shape == (NL, ITERS, 2) and pop.v_trace.shape == (NL, ITERS, 2)
    _same_learners(pop, info, learners, infos, actors, critics, gpu)
    # a second update from the carried optimiser state
    infos = [learners[l].update(_slice(b, l, NE)) for l in range(NL)]
    info = pop.update(b)
    _same_learners(pop, info, learners, infos, actors, critics, gpu)


def test_update_population_learner_without_a_valid_record(gpu):
    actors, critics = _nets()
    b = _flat_batch(NT, NL, NE, actors, 9, gpu)
    b["valid"][:, NE:2 * NE] = False  # learner 1 has no valid record
    learners = _learners(actors, critics)
    infos = [learners[l].update(_slice(b, l, NE)) for l in range(NL)]
    pop = _population()
    before = [[(W.clone(), c.clone()) for W, c in pop.actor(1).weights], [(W.clone(), c.clone()) for W, c in pop.critic(1).weights]]
    info = pop.update(b)
    _same_learners(pop, info, learners, infos, actors, critics, gpu)  # the neighbours are unaffected
    for net, was in ((pop.actor(1), before[0]), (pop.critic(1), before[1])):
        for (W, c), (W0, c0) in zip(net.weights, was):
            assert torch.equal(W, W0) and torch.equal(c, c0)
    for m, v, t in pop.adam_state():
        assert not bool(m[1].any()) and not bool(v[1].any()) and int(t[1]) == 0
        assert int(t[0]) > 0 and bool(m[0].any())
    assert int(info.StopIter[1]) == 0 and float(info.LossPi[1]) == 0.0


# ---- 5. two epochs end to end ----
def test_two_epochs_collect_update_collect_update(gpu):
    d = _log("f32")
    whole, parts = _envs(d)
    actors, critics = _nets()
    learners = _learners(actors, critics)
    pop = _population()
    for epoch in range(2):
        p = whole.collect_ppo_population(pop, NT, max_episode_steps=4)
        singles = [parts[l].collect_ppo(actors[l], critics[l], NT, max_episode_steps=4) for l in range(NL)]
        _same_batch(p, singles)
        _same_state(whole, parts)
        info = pop.update(p)
        infos = [learners[l].update(singles[l]) for l in range(NL)]
        _same_learners(pop, info, learners, infos, actors, critics, gpu)
    assert int(pop.adam_state()[1][2].min()) == 2 * ITERS  # the critics stepped in both epochs: the second collect ran the new weights


# ---- 6. determinism ----
def test_update_population_twice_from_the_same_state_gives_the_same_bits(gpu):
    actors, _ = _nets()
    b = _flat_batch(NT, NL, NE, actors, 9, gpu)
    runs = []
    for _ in range(2):
        pop = _population()
        info = pop.update(b)
        (pm, pv, pt), (vm, vv, vt) = pop.adam_state()
        ws = [W for st in (pop._pi, pop._v) for W, c in st.ws] + [c for st in (pop._pi, pop._v) for W, c in st.ws]
        runs.append([x.clone() for x in (*info, pop.pi_trace, pop.v_trace, pm, pv, pt, vm, vv, vt, *ws)])
    for x, y in zip(*runs):
        assert torch.equal(x, y) or (x.dtype == torch.float64 and _same_with_nan(x, y))


# ---- 7. relu, three actions ----
def test_relu_three_actions_population(gpu):
    from rl_offline_simulation_amd.evaluators import PPOLearner, PPOPopulation, ppo_grad, ppo_grad_population
    nl = 2
    d = _log("na3")
    whole, parts = _envs(d, nl)
    actors, critics = _nets(nl, nA=3, act="relu", base=1)
    kw = dict(pi_lr=1e-3, train_pi_iters=3, train_v_iters=3, target_kl=1e9)
    pop = PPOPopulation(*_nets(nl, nA=3, act="relu", base=1), **kw)
    learners = [PPOLearner(actors[l], critics[l], **kw) for l in range(nl)]
    p = whole.collect_ppo_population(pop, NT, max_episode_steps=4)
    singles = [parts[l].collect_ppo(actors[l], critics[l], NT, max_episode_steps=4) for l in range(nl)]
    assert p.collected.probs.shape[-1] == 3 and int(p.act.max()) == 2
    _same_batch(p, singles)
    _same_state(whole, parts)
    for kind, nets in (("actor", actors), ("critic", critics)):
        got = ppo_grad_population(pop, p, kind)
        for l in range(nl):
            want = ppo_grad(nets[l], singles[l], kind)
            assert torch.equal(got.grad[l], want.grad) and torch.equal(got.loss[l], want.loss) and torch.equal(got.n[l], want.n), (kind, l)
    info = pop.update(p)
    infos = [learners[l].update(singles[l]) for l in range(nl)]
    _same_learners(pop, info, learners, infos, actors, critics, gpu)
