"""ppo_epoch_log (offsim_ppo_epoch_log / _pop) and PPOLearner.fit / PPOPopulation.fit on the device: the reference agent's stored EpRet /
EpLen lists through VectorPSRS.collect_ppo (tests/golden/ppo_log/*.npz), hand-built records against the NumPy restatement
(tests/ppo_log_host.py), the independence of the learners, and fit against the loop written by hand.

Tolerances.  The lists, the counts, the carry, min and max are exact.  A mean is a sum of n f64 terms in some fixed order: any order is
within n * 2^-52 * sum|x| of any other (the summation bound), which is the bound used.  A std is sqrt(Q / n) with Q the sum of the n squared
deviations, itself within n * 2^-52 * Q: carried through the square root that is (n / 2) * 2^-52 * std, plus 2^-52 * std for the division and
the square root themselves."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_log_host as H  # noqa: E402
from test_gpu_ppo import _fixture_env, _nets as _fixture_nets  # noqa: E402
from test_gpu_ppo_population import _envs, _learners, _log, _nets, _population  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ppo_log", "*.npz")))
EPS = 2.0 ** -52
STAT_FIELDS = ("EpRet", "StdEpRet", "MaxEpRet", "MinEpRet", "EpLen", "VVals", "StdVVals", "MaxVVals", "MinVVals")


@pytest.fixture(scope="module")
def gpu():
    from rl_offline_simulation_amd import _lib
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    _lib.load()
    return torch.device("cuda", 0)


def _bits(a, b):
    """bitwise equality of two tensors (NaN included)"""
    if a.dtype == torch.float64:
        return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))
    return torch.equal(a, b)


def _check_stats(log, l, want, what):
    """learner l of a PPOEpochLog against ppo_log_host.learner_log"""
    pick = (lambda x: x.cpu().numpy()) if l is None else (lambda x: x[l].cpu().numpy())
    got = {k: pick(getattr(log, k)) for k in log._fields}
    print(what, {k: float(v) for k, v in got.items()})
    assert int(got["Entries"]) == want["entries"] and int(got["EpisodesInEpoch"]) == want["episodes"] and int(got["StepsServed"]) == want["steps"], what
    for mean, std, lo, hi, s in (("EpRet", "StdEpRet", "MinEpRet", "MaxEpRet", want["ret"]), ("VVals", "StdVVals", "MinVVals", "MaxVVals", want["v"])):
        if s["n"] == 0:
            assert all(np.isnan(got[k]) for k in (mean, std, lo, hi)), what
            continue
        print(what, mean, "error", abs(got[mean] - s["mean"]), "bound", s["n"] * EPS * s["sum_abs"], "| std error", abs(got[std] - s["std"]), "bound",
              (s["n"] / 2 + 1) * EPS * s["std"])
        assert abs(got[mean] - s["mean"]) <= s["n"] * EPS * s["sum_abs"], (what, mean)
        assert abs(got[std] - s["std"]) <= (s["n"] / 2 + 1) * EPS * s["std"], (what, std)
        assert got[lo] == s["min"] and got[hi] == s["max"], (what, lo, hi)
    if want["len"]["n"] == 0:
        assert np.isnan(got["EpLen"]), what
    else:
        assert abs(got["EpLen"] - want["len"]["mean"]) <= want["len"]["n"] * EPS * want["len"]["sum_abs"], (what, "EpLen")


def _lists(eps, r):
    """environment r's ended episodes of a PPOEpisodes: [(ret, len), ...]"""
    n = int(eps.n_ep[r])
    assert n <= eps.ep_ret.shape[1]
    return list(zip(eps.ep_ret[r, :n].tolist(), eps.ep_len[r, :n].tolist()))


def _entries(eps, r):
    if bool(eps.open[r]):
        assert int(eps.n_ep[r]) == 0
        return [(float(eps.open_ret[r]), int(eps.open_len[r]))]
    return _lists(eps, r)


def _host(x):
    return x.cpu().numpy()


# ---- 1. the reference's agent, through the real path ----
@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
@pytest.mark.parametrize("together", [False, True], ids=["one_env_per_seed", "all_seeds_one_learner"])
def test_reference_lists_through_collect_ppo(gpu, path, together):
    from rl_offline_simulation_amd.evaluators import EpisodeTracker, ppo_epoch_log
    f = np.load(path)
    T, cap = int(f["T"]), int(f["cap"])
    actor, critic = _fixture_nets(f)
    seeds = [int(s) for s in f["seeds"]]
    for group in ([seeds] if together else [[s] for s in seeds]):
        env = _fixture_env(f, len(group))
        env.reset_sampler(group)
        env.reset()
        tracker, carry = EpisodeTracker(len(group), gpu), H.Carry(len(group))
        for j in range(3):
            p = env.collect_ppo(actor, critic, T, max_episode_steps=cap)
            log, eps = ppo_epoch_log(p, tracker, episodes=True)
            for e, s in enumerate(group):
                assert np.array_equal(_host(p.collected.row[:, e]), f[f"rows_{s}"][j * T:(j + 1) * T]), (s, j)
                ent = _entries(eps, e)
                assert [g for g, _ in ent] == list(f[f"EpRet_{s}_{j}"]), (s, j)  # exact
                assert [n for _, n in ent] == list(f[f"EpLen_{s}_{j}"]), (s, j)
                assert int(eps.n_ep[e]) == int(f[f"episodes_{s}_{j}"]), (s, j)
            assert int(log.EpisodesInEpoch) == sum(int(f[f"episodes_{s}_{j}"]) for s in group)
            assert int(log.Entries) == sum(len(f[f"EpRet_{s}_{j}"]) for s in group) and int(log.StepsServed) == T * len(group)
            c = p.collected
            ended, entries, vvals = H.epoch(_host(p.rew), _host(p.val), _host(p.valid), _host(c.terminated), _host(c.truncated), carry)
            _check_stats(log, None, H.learner_log(ended, entries, vvals, range(len(group))), (os.path.basename(path), group, j))
            assert tracker.open_ret.tolist() == carry.open_ret and tracker.open_len.tolist() == carry.open_len


# ---- 2. hand-built records against the restatement ----
def _records(T, E, nl, seed):
    """[T, nl * E] records that hold, where the shape has room: per learner an environment with no ending (0), one ending at the last step
    (1), one with both flags set (2), one whose valid stops mid-epoch (3), one with no valid step (4); the last learner of several has no
    valid step at all."""
    g = np.random.default_rng(seed)
    R = nl * E
    rew, val = g.standard_normal((T, R)).astype(np.float32), g.standard_normal((T, R)).astype(np.float32)
    term, trunc = g.random((T, R)) < 0.15, g.random((T, R)) < 0.1
    valid = np.arange(T)[:, None] < g.integers(1, T + 1, R)[None, :]  # every environment stops somewhere, most at the end
    valid[:, g.random(R) < 0.7] = True
    for l in range(nl):
        c = l * E
        if E > 0:
            term[:, c], trunc[:, c], valid[:, c] = False, False, True
        if E > 1:
            term[T - 1, c + 1], valid[:, c + 1] = True, True
        if E > 2:
            term[T // 2, c + 2], trunc[T // 2, c + 2], valid[:, c + 2] = True, True, True
        if E > 3:
            valid[:, c + 3] = np.arange(T) < max(1, T // 2)
        if E > 4:
            valid[:, c + 4] = False
    if nl > 1:
        valid[:, (nl - 1) * E:] = False
    return rew, val, valid, term, trunc


def _dev(gpu, *xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(gpu) for x in xs]


SHAPES = [(1, 1, 1), (7, 65, 3), (40, 257, 2)]  # one past a wavefront; one past the workgroup of 256 (a lane with two environments)


@pytest.mark.parametrize("mode", ["reference", "steps"])
@pytest.mark.parametrize("T,E,nl", SHAPES)
def test_hand_built_records_against_the_restatement(gpu, T, E, nl, mode):
    from rl_offline_simulation_amd.evaluators import EpisodeTracker, ppo_epoch_log_records
    R = nl * E
    halves = [_records(T, E, nl, 100 * T + E), _records(T, E, nl, 100 * T + E + 1)]
    tracker, carry = EpisodeTracker(R, gpu), H.Carry(R)
    got_lists = [[] for _ in range(R)]
    for k, rec in enumerate(halves):  # two consecutive calls share the carry
        log, eps = ppo_epoch_log_records(*_dev(gpu, *rec), tracker, learners=nl, ep_len=mode, episodes=True)
        ended, entries, vvals = H.epoch(*rec, carry, mode)
        for r in range(R):
            assert _lists(eps, r) == ended[r], (k, r)  # bit-equal: the same f64 sums in the same order
            assert _entries(eps, r) == entries[r], (k, r)
            got_lists[r] += _lists(eps, r)
        assert tracker.open_ret.tolist() == carry.open_ret and tracker.open_len.tolist() == carry.open_len, k
        for l in range(nl):
            _check_stats(log, l if nl > 1 else None, H.learner_log(ended, entries, vvals, range(l * E, (l + 1) * E)), (T, E, nl, mode, k, l))
        if nl > 1:  # the learner without a valid step: NaN and zero
            assert all(bool(torch.isnan(getattr(log, f)[nl - 1])) for f in STAT_FIELDS)
            assert int(log.Entries[nl - 1]) == int(log.EpisodesInEpoch[nl - 1]) == int(log.StepsServed[nl - 1]) == 0
    # one call on the 2 T records gives the two calls' lists, concatenated
    both = [np.concatenate([a, b]) for a, b in zip(*halves)]
    one = EpisodeTracker(R, gpu)
    _, eps = ppo_epoch_log_records(*_dev(gpu, *both), one, learners=nl, ep_len=mode, episodes=True)
    for r in range(R):
        assert _lists(eps, r) == got_lists[r], r
    assert _bits(one.open_ret, tracker.open_ret) and torch.equal(one.open_len, tracker.open_len)


def test_records_hold_the_cases_by_construction():
    rew, val, valid, term, trunc = _records(7, 65, 3, 0)
    end = valid & (term | trunc)
    assert not end[:, 0].any() and valid[:, 0].all() and end[6, 1] and (term & trunc & valid)[3, 2] and valid[:3, 3].all() and not valid[3:, 3].any()
    assert not valid[:, 4].any() and not valid[:, 130:].any() and valid[:, 65:130].any()


def test_learners_are_independent_and_two_calls_give_the_same_bits(gpu):
    from rl_offline_simulation_amd.evaluators import EpisodeTracker, ppo_epoch_log_records
    T, E, nl = 7, 65, 3
    rec = _records(T, E, nl, 5)
    start = torch.from_numpy(np.random.default_rng(1).standard_normal(nl * E)).to(gpu)  # a carry that is not zero
    runs = []
    for _ in range(2):
        tr = EpisodeTracker(nl * E, gpu)
        tr.open_ret.copy_(start)
        tr.open_len.fill_(3)
        runs.append((ppo_epoch_log_records(*_dev(gpu, *rec), tr, learners=nl, episodes=True), tr))
    (log, eps), tr = runs[0]
    (log2, eps2), tr2 = runs[1]
    for a, b in zip(tuple(log) + (eps.ep_ret, eps.ep_len, eps.n_ep, tr.open_ret, tr.open_len), tuple(log2) + (eps2.ep_ret, eps2.ep_len, eps2.n_ep, tr2.open_ret, tr2.open_len)):
        assert _bits(a, b)
    for l in range(nl):
        sl = slice(l * E, (l + 1) * E)
        one = EpisodeTracker(E, gpu)
        one.open_ret.copy_(start[sl])
        one.open_len.fill_(3)
        slog, seps = ppo_epoch_log_records(*_dev(gpu, *[x[:, sl] for x in rec]), one, episodes=True)
        for f in log._fields:
            assert getattr(slog, f).dim() == 0 and _bits(getattr(log, f)[l], getattr(slog, f)), (l, f)
        assert _bits(eps.ep_ret[sl], seps.ep_ret) and torch.equal(eps.ep_len[sl], seps.ep_len) and torch.equal(eps.n_ep[sl], seps.n_ep), l
        assert torch.equal(eps.open[sl], seps.open) and _bits(tr.open_ret[sl], one.open_ret) and torch.equal(tr.open_len[sl], one.open_len), l


def test_ep_cap_keeps_the_first_episodes_and_counts_all(gpu):
    from rl_offline_simulation_amd.evaluators import EpisodeTracker, ppo_epoch_log_records
    T, E = 9, 3
    rew = np.ones((T, E), np.float32)
    term = np.zeros((T, E), bool)
    term[[1, 4, 8], 0] = True
    term[2, 1] = True
    valid = np.ones((T, E), bool)
    args = _dev(gpu, rew, rew, valid, term, np.zeros_like(term))
    log, eps = ppo_epoch_log_records(*args, EpisodeTracker(E, gpu), episodes=True, ep_cap=2)
    assert eps.ep_ret.shape == (E, 2) and eps.n_ep.tolist() == [3, 1, 0] and eps.open.tolist() == [False, False, True]
    assert eps.ep_ret[0].tolist() == [2.0, 3.0] and eps.ep_len[0].tolist() == [1, 2] and eps.ep_ret[1, 0].item() == 3.0
    assert int(log.EpisodesInEpoch) == 4 and int(log.Entries) == 5 and float(log.EpRet) == (2 + 3 + 4 + 3 + 9) / 5 and float(log.MaxEpRet) == 9.0
    bare = ppo_epoch_log_records(*args, EpisodeTracker(E, gpu))  # without the lists: the same log
    assert all(_bits(a, b) for a, b in zip(log, bare))


# ---- 3. fit ----
FIT_E, FIT_T, FIT_EPOCHS, FIT_CAP = 4, 16, 3, 6


def _same_weights(a, b, dev):
    for (W, c), (W1, c1) in zip(a._device_weights(dev)[0], b._device_weights(dev)[0]):
        assert torch.equal(W, W1) and torch.equal(c, c1)


def test_learner_fit_is_the_loop_written_by_hand(gpu):
    from rl_offline_simulation_amd.evaluators import EpisodeTracker, PPOTrainLog, ppo_epoch_log
    d = _log("f32")
    (ea, (eb, *_)) = _envs(d, nl=1, ne=FIT_E)
    (actors_a, critics_a), (actors_b, critics_b) = _nets(), _nets()
    la, lb = _learners(actors_a, critics_a)[1], _learners(actors_b, critics_b)[1]
    got = la.fit(ea, FIT_EPOCHS, FIT_T, max_episode_steps=FIT_CAP)
    tracker, rows = EpisodeTracker(FIT_E, gpu), []
    for _ in range(FIT_EPOCHS):
        b = eb.collect_ppo(lb.actor, lb.critic, FIT_T, max_episode_steps=FIT_CAP)
        log = ppo_epoch_log(b, tracker)
        rows.append(tuple(log) + tuple(lb.update(b)))
    assert isinstance(got, PPOTrainLog)
    for k, f in enumerate(got._fields[:-1]):
        assert getattr(got, f).shape == (FIT_EPOCHS,) and _bits(getattr(got, f), torch.stack([r[k] for r in rows])), f
    assert got.TotalEnvInteracts.tolist() == [(j + 1) * FIT_T * FIT_E for j in range(FIT_EPOCHS)]
    assert int(got.EpisodesInEpoch.sum()) > 0 and int(got.StepsServed.min()) == FIT_T * FIT_E and not bool(torch.isnan(got.EpRet).any())
    _same_weights(la.actor, lb.actor, gpu)
    _same_weights(la.critic, lb.critic, gpu)
    for x, y in zip(la.adam_state(), lb.adam_state()):
        assert all(torch.equal(p, q) for p, q in zip(x, y))


def test_population_fit_gives_every_learner_its_own_fit(gpu):
    d = _log("f32")
    whole, parts = _envs(d, nl=3, ne=FIT_E)
    actors, critics = _nets()
    learners = _learners(actors, critics)
    pop = _population()
    got = pop.fit(whole, FIT_EPOCHS, FIT_T, max_episode_steps=FIT_CAP)
    for l, lrn in enumerate(learners):
        own = lrn.fit(parts[l], FIT_EPOCHS, FIT_T, max_episode_steps=FIT_CAP)
        for f in got._fields:
            assert getattr(got, f).shape == (FIT_EPOCHS, 3) and _bits(getattr(got, f)[:, l], getattr(own, f)), (l, f)
        for mine, theirs in ((pop.actor(l), actors[l]), (pop.critic(l), critics[l])):
            for (W, c), (W1, c1) in zip(mine.weights, theirs._device_weights(gpu)[0]):
                assert torch.equal(W, W1.cpu()) and torch.equal(c, c1.cpu()), l
    assert len({float(x) for x in got.LossPi[0]}) == 3  # the learners differ
