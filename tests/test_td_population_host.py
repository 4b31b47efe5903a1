"""TDPopulation without a device: the grid, broadcasting and its refusals, the schedule tabulation, best(), the struct mirror; the host
curve loop of tests/td_population_host.py against NumPy; and that the population cases of tests/test_gpu_td_population.py are not vacuous
(checked on the host loop)."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import td_cases as K  # noqa: E402
import td_host as H  # noqa: E402
import td_population_host as P  # noqa: E402

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_grid_is_the_cartesian_product():
    from rl_offline_simulation_amd.evaluators import TDPopulation
    a, e, g = [0.1, 0.5], [0.0, 0.2, 1.0], [0.9, 0.99]
    pop = TDPopulation.grid("qlearn", alpha=a, epsilon=e, gamma=g, behaviour="eps_greedy")
    assert len(pop) == 12 and pop.L == 12
    assert [(d["alpha"], d["epsilon"], d["gamma"]) for d in pop.learners] == list(itertools.product(a, e, g))
    assert all(d["behaviour"] == "eps_greedy" for d in pop.learners)
    one = TDPopulation.grid("expsarsa", alpha=0.1)
    assert len(one) == 1 and one.learners == [dict(alpha=0.1, epsilon=1.0, gamma=0.99, behaviour="fixed")]
    with pytest.raises(ValueError, match="empty axis"):
        TDPopulation.grid("qlearn", alpha=[], gamma=[0.9])


def test_broadcasting_and_refusal_of_mismatched_lengths():
    from rl_offline_simulation_amd import _lib as L
    from rl_offline_simulation_amd.evaluators import TDPopulation
    pop = TDPopulation("qlearn", alpha=[0.1, 0.2, 0.3], gamma=0.9, epsilon=0.5, behaviour=["fixed", "greedy", "soft_greedy"])
    assert pop.L == 3 and pop.mode == L.TD_QLEARN
    assert pop.gamma == [0.9] * 3 and pop.epsilon == [0.5] * 3 and pop.alpha == [0.1, 0.2, 0.3]
    assert TDPopulation("expsarsa", 0.1, 0.9).L == 1 and TDPopulation("expsarsa", 0.1, 0.9).mode == L.TD_EXPSARSA
    # a [L, nS, nA] table counts as a per-learner argument, a [nS, nA] table is shared
    assert TDPopulation("expsarsa", 0.1, 0.9, pi=np.full((4, 6, 2), 0.5)).L == 4
    assert TDPopulation("expsarsa", 0.1, [0.9, 0.8], pi=np.full((6, 2), 0.5), Q_init=np.zeros((2, 6, 2))).L == 2
    with pytest.raises(ValueError, match="different lengths"):
        TDPopulation("qlearn", alpha=[0.1, 0.2, 0.3], gamma=[0.9, 0.99])
    with pytest.raises(ValueError, match="different lengths"):
        TDPopulation("qlearn", alpha=[0.1, 0.2], gamma=0.9, pi=np.full((3, 6, 2), 0.5))
    with pytest.raises(ValueError, match="behaviour"):
        TDPopulation("qlearn", 0.1, 0.9, behaviour="boltzmann")
    with pytest.raises(ValueError, match="mode"):
        TDPopulation("sarsa", 0.1, 0.9)
    with pytest.raises(ValueError, match="nS,nA"):
        TDPopulation("qlearn", 0.1, 0.9, pi=np.zeros(5))


def test_schedules_are_tabulated_as_the_single_learner_drivers_do():
    from rl_offline_simulation_amd.evaluators import TDPopulation
    from rl_offline_simulation_amd.evaluators.psrs import _schedule
    decay = lambda ep: 1.0 / (ep + 1)  # noqa: E731
    half = lambda ep: 0.5 ** ep  # noqa: E731
    pop = TDPopulation("qlearn", alpha=[0.1, decay, 0.3], gamma=0.9, epsilon=[half, 0.2, 0.7], behaviour=["eps_greedy", "eps_greedy", "greedy"])
    a, e, a_tab, e_tab = pop.tabulate(4)
    assert a.tolist() == [0.1, 0.0, 0.3] and e.tolist() == [0.0, 0.2, 0.0]          # a callable's constant is 0; greedy is epsilon 0
    assert a_tab.shape == e_tab.shape == (3, 4)
    assert np.array_equal(a_tab[1], _schedule(decay, 4)) and np.array_equal(a_tab[0], np.full(4, 0.1)) and np.array_equal(a_tab[2], np.full(4, 0.3))
    assert np.array_equal(e_tab[0], _schedule(half, 4)) and np.array_equal(e_tab[1], np.full(4, 0.2)) and np.array_equal(e_tab[2], np.zeros(4))
    assert pop.tabulate(0)[2].shape == (3, 1)                                     # _schedule's max(n_ep, 1)
    a, e, a_tab, e_tab = TDPopulation("qlearn", [0.1, 0.2], 0.9, epsilon=0.3, behaviour=["eps_greedy", "greedy"]).tabulate(4)
    assert a_tab is None and e_tab is None and a.tolist() == [0.1, 0.2] and e.tolist() == [0.3, 0.0]


def test_struct_mirror_of_the_population_arguments(tmp_path):
    """sizeof / offsetof of offsim_td_pop as gcc lays it out, against _lib.TDPop."""
    from rl_offline_simulation_amd import _lib
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "offsim.h"', "int main(void) {", '  printf("size %zu\\n", sizeof(offsim_td_pop));']
    for f, _ in _lib.TDPop._fields_:
        lines.append(f'  printf("{f} %zu\\n", offsetof(offsim_td_pop, {f}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(_lib.TDPop)
    for f, _ in _lib.TDPop._fields_:
        assert int(got[f]) == getattr(_lib.TDPop, f).offset, f


def test_argument_validation_needs_no_device():
    """offsim_eval_td_pop and offsim_td_curves refuse bad arguments before any HIP call."""
    from rl_offline_simulation_amd import _lib as L
    lib = L.load()
    t = L.Table(N=0, n_slots=3, nA=2, plog_dtype=L.F32, r_dtype=L.F32)
    ro = L.Rollouts(R=7)
    out = L.EvalMCOut(sum_g=8, n_ep=8, steps=8, cand=8, n_len=8, status=8)
    beh = (ctypes.c_int32 * 2)(L.BEHAVIOUR_EPS_GREEDY, 5)
    pop = L.TDPop(mode=L.TD_QLEARN, alpha=8, epsilon=8, gamma=8, behaviour=8, behaviour_host=beh, pi=8, q=8, snap_stride=1)
    call = lambda L_, S_: lib.offsim_eval_td_pop(ctypes.byref(t), ctypes.byref(ro), L_, S_, ctypes.byref(pop), L.REJECT_DEFAULT, 1, ctypes.byref(out), None)  # noqa: E731
    assert call(2, 3) == L.EINVAL and b"ro->R must be L * S" in lib.offsim_last_error()
    assert call(0, 7) == L.EINVAL and call(7, 0) == L.EINVAL and b"L must be" in lib.offsim_last_error()
    ro.R = 6
    assert call(2, 3) == L.EINVAL and b"bad behaviour" in lib.offsim_last_error()
    beh[1] = L.BEHAVIOUR_FIXED
    pop.mode = 0
    assert call(2, 3) == L.EINVAL and b"bad td mode" in lib.offsim_last_error()
    pop.mode, pop.gamma = L.TD_EXPSARSA, None
    assert call(2, 3) == L.EINVAL and b"per-learner array" in lib.offsim_last_error()
    pop.gamma, pop.alpha_ep = 8, 8
    assert call(2, 3) == L.EINVAL and b"n_sched" in lib.offsim_last_error()
    ro.R = 0  # nothing to run: OK without a launch
    pop.alpha_ep = None
    assert call(2, 3) == L.OK
    assert lib.offsim_td_curves(None, None, 2, 3, 4, None, None, None, None) == L.EINVAL and b"td_curves" in lib.offsim_last_error()
    assert lib.offsim_td_curves(None, None, -1, 3, 4, None, None, None, None) == L.EINVAL
    assert lib.offsim_td_curves(None, None, 2, 3, 0, None, None, None, None) == L.OK


def test_curve_loop_against_numpy_on_ragged_counts():
    g = np.random.default_rng(5)
    n_l, n_s, n_e = 4, 7, 9
    ep_g = g.standard_normal((n_l, n_s, n_e)) * 3 + 1
    n_ep = g.integers(0, n_e - 1, (n_l, n_s))  # ragged, and nobody completes the last episode
    n_ep[2] = 0                                  # a learner without any completed episode
    n, mean, var = P.curves(ep_g, n_ep)
    mask = np.arange(n_e)[None, None, :] < n_ep[:, :, None]
    assert np.array_equal(n, mask.sum(1)) and n.min() == 0 and 0 < n[0].max() <= n_s and len(np.unique(n)) > 3
    with np.errstate(invalid="ignore", divide="ignore"):
        ref_mean = np.where(mask, ep_g, 0.0).sum(1) / mask.sum(1)
        ref_var = (np.where(mask, ep_g - ref_mean[:, None, :], 0.0) ** 2).sum(1) / mask.sum(1)
    assert np.isnan(mean[n == 0]).all() and np.isnan(var[n == 0]).all() and np.isnan(mean[2]).all() and np.isnan(mean[:, -1]).all()
    assert np.allclose(mean[n > 0], ref_mean[n > 0], rtol=0, atol=1e-12) and np.allclose(var[n > 0], ref_var[n > 0], rtol=0, atol=1e-12)
    assert (var[n == 1] == 0).all()


def _result(curve_mean, curve_n, S):
    from rl_offline_simulation_amd.evaluators import TDPopulationResult
    n_l, n_e = np.shape(curve_mean)
    z = torch.zeros(n_l, S)
    return TDPopulationResult(Q=torch.zeros(n_l, S, 1, 1), Gs=torch.zeros(n_l, S, n_e), n_ep=z, steps=z, status=z, curve_mean=torch.tensor(curve_mean),
                              curve_var=torch.zeros(n_l, n_e), curve_n=torch.tensor(curve_n))


def test_best_ignores_curve_points_some_seed_did_not_reach():
    mean = [[1.0, 2.0, 3.0, 100.0], [1.0, 2.5, 3.5, -50.0], [9.0, 9.0, float("nan"), float("nan")]]
    n = [[4, 4, 4, 2], [4, 4, 4, 3], [4, 3, 0, 0]]
    r = _result(mean, n, 4)
    assert r.best(last=1) == 2        # 3.0 / 3.5 / 9.0: the points with n < 4 (100, -50, the second 9) do not count
    assert r.best(last=2) == 2        # 2.5 / 3.0 / 9.0 (learner 2 has one full point only)
    r = _result(mean[:2], n[:2], 4)
    assert r.best(last=1) == 1 and r.best(last=3) == 1      # (1 + 2.5 + 3.5) / 3 > (1 + 2 + 3) / 3
    assert _result(mean[:2], n[:2], 5).best() == -1          # no point every seed reached


def test_population_launch_shape_one_learner_per_workgroup():
    """td_cases.launch_shape restated for the population: the carve is the single-learner one, a workgroup holds seeds of one learner."""
    want = {"qlearn-every-behaviour-mt-fresh": (4, 3 * 2), "expsarsa-own-pi-waves2": (2, 3 * 3), "qlearn-eps-lds-above-64k": (1, 3 * 5),
            "expsarsa-few-init": (4, 3 * 2)}
    for name, (waves, groups) in want.items():
        c = P.BY_NAME[name]
        w, lds, refused, wg = c.shape
        assert (w, wg) == (waves, groups) and not refused and (w, lds, refused) == K.launch_shape(c.table.nS, c.table.nA)
        assert wg == c.L * -(-c.S // w) and (c.S % w != 0 or w == 1)   # S = 5 fills no workgroup of 4 or 2 evenly
        assert wg >= (c.L * c.S + w - 1) // w                           # never fewer than rollout-major packing would take
    assert P.BY_NAME["qlearn-eps-lds-above-64k"].shape[1] > 64 * 1024
    assert {c.table for c in P.CASES} >= {K.T5, K.T16, K.T15_BIG, K.T_FEW_INIT}
    assert K.launch_shape(K.T_OVER.nS, K.T_OVER.nA)[2]
    for c in P.CASES:   # the grid: no two learners agree in alpha, epsilon or gamma
        for v in (c.alpha, c.epsilon, c.gamma):
            assert len(set(v)) == c.L == 3
    assert {b for c in P.CASES if c.mode == H.QLEARN for b in c.behaviour} == {H.FIXED, H.EPS_GREEDY, H.SOFT_GREEDY}
    assert any(c.mode == H.EXPSARSA and c.pi_per_learner for c in P.CASES) and {c.mt for c in P.CASES} == {"none", "fresh", "mid"}
    assert any(c.stream == "philox" for c in P.CASES) and any(c.alpha_ep and c.epsilon_ep for c in P.CASES) and any(c.resume_k for c in P.CASES)


@pytest.mark.parametrize("name", [c.name for c in P.CASES])
def test_cases_are_not_vacuous(name):
    case = P.BY_NAME[name]
    outs = P.host(case)
    o = outs[-1]
    trace_cap, ep_cap = P.caps_of(case)
    assert o["q"].shape == (case.L, case.S, case.table.nS, case.table.nA)
    steps = sum(x["steps"] for x in outs)
    assert (steps >= 20).all(), steps
    # at least two learners end with different Q (on the same seed), and the seeds of a learner differ too
    assert any(not np.array_equal(o["q"][a, 0], o["q"][b, 0]) for a in range(case.L) for b in range(a))
    assert not np.array_equal(o["q"][0, 0], o["q"][0, 1])
    if case.mt != "none":  # every eps-greedy learner drew from its tie stream on every seed
        words = sum(x["mt_words"] for x in outs)
        for l in range(case.L):
            if case.behaviour[l] == H.EPS_GREEDY:
                assert (words[l] > 0).all(), (name, l, words[l])
            else:
                assert (words[l] == 0).all()
        assert any(b == H.EPS_GREEDY for b in case.behaviour)
    if case.trace_cap is not None:
        assert (steps > trace_cap).all() and (o["n_ep"] > ep_cap).all() and (steps > case.snap_cap * case.snap_stride).all()
    if case.resume_k is not None:
        assert (outs[0]["n_ep"] == case.resume_k).all() and (outs[1]["n_ep"] > 0).all()
        assert np.array_equal(outs[0]["cursor"][0], outs[0]["cursor"][1]) and np.array_equal(outs[0]["cursor"][0], outs[0]["cursor"][2])
    if case in P.CURVE_CASES:  # ragged: some episode index was completed by some seeds of a learner and not by all
        n, mean, var = P.curves(o["ep_g"], o["n_ep"])
        assert ((n > 0) & (n < case.S)).any(), (name, o["n_ep"])
        assert (n[:, 0] == case.S).all() and (n[:, -1] == 0).all() and np.isnan(mean[:, -1]).all()
    elif not case.curve:
        assert (o["status"] == H.ST_NO_INIT).all()
