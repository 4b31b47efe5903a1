"""CPU side of the population evaluation (L policies over observations on the same seeds): the C ABI of offsim_policy_mlp_pop and
offsim_eval_mc_rows_policy_pop -- exported, bound, documented, every refusal before any HIP call (the pointers are fake addresses: a launch
would fault), zero-size calls --, the host side of PolicyPopulation, and the NumPy restatement (tests/policy_population_host.py) pinned on
the reference's fixtures."""
import ctypes
import glob
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import obs_policy_host as H  # noqa: E402
import policy_population_host as PH  # noqa: E402
from test_collect import _args  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "obs_policy", "*.npz")))
ENTRIES = ("offsim_policy_mlp_pop", "offsim_eval_mc_rows_policy_pop")
F = 0x1000


# ---- the C ABI ----
def test_symbols_exported_bound_and_documented():
    from rl_offline_simulation_amd import _lib
    src = open(os.path.join(ROOT, "include", "offsim.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ENTRIES:
        assert "int " + n + "(" in src, n
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
        assert "rgument validation happens before any HIP call" in src[src.index("/* " + n + ":"):src.index("int " + n + "(")], n


def _mlp_pop(L_, M=0, sizes=(4, 8, 2), dO=4, x_dtype=None, act=1, n_x=10, x=F, out=F):
    from rl_offline_simulation_amd import _lib as L
    layers = (L.MLPLayer * (len(sizes) - 1))()
    for i in range(len(sizes) - 1):
        layers[i].W, layers[i].b, layers[i].out = F, F, sizes[i + 1]
        setattr(layers[i], "in", sizes[i])
    return L.load().offsim_policy_mlp_pop(x, L.F32 if x_dtype is None else x_dtype, n_x, dO, None, M, layers, len(sizes) - 1, act, 0.01, L_, out, None)


def test_policy_mlp_pop_validation_before_any_hip_call():
    from rl_offline_simulation_amd import _lib as L
    lib = L.load()
    assert _mlp_pop(3) == L.OK, lib.offsim_last_error()  # M = 0 validates and launches nothing
    assert _mlp_pop(1) == L.OK and _mlp_pop(65535) == L.OK
    for l_ in (0, -1, 65536):
        assert _mlp_pop(l_) == L.EINVAL and lib.offsim_last_error().startswith(b"policy_mlp_pop") and b"65535" in lib.offsim_last_error(), l_
    # the network's limits are offsim_policy_mlp's, reported with this entry point's name
    for kw in (dict(sizes=(4, 257, 2)), dict(sizes=(4, 8, 17)), dict(sizes=(129, 8, 2), dO=129), dict(sizes=(4, 8, 2), dO=5), dict(sizes=(4,)),
               dict(sizes=(4, 8, 8, 8, 8, 2)), dict(act=9), dict(x_dtype=L.F64)):
        assert _mlp_pop(3, **kw) == L.EINVAL and lib.offsim_last_error().startswith(b"policy_mlp_pop"), kw
    assert _mlp_pop(3, M=-1) == L.EINVAL
    assert _mlp_pop(3, M=5, x=None) == L.EINVAL and b"NULL" in lib.offsim_last_error()
    assert _mlp_pop(3, M=5, out=None) == L.EINVAL and b"NULL" in lib.offsim_last_error()


def _scan_pop(L_, S_, R=None, p_next=F, p_init=F, prob_mode=None, out=True, **tab):
    from rl_offline_simulation_amd import _lib as L
    t, ro, _, _, _, _ = _args(R=L_ * S_ if R is None else R)
    for k, v in tab.items():
        setattr(t, k, v)
    oc = L.EvalMCOut(sum_g=F, n_ep=F, steps=F, cand=F, n_len=F, status=F)
    return L.load().offsim_eval_mc_rows_policy_pop(ctypes.byref(t), ctypes.byref(ro), p_next, p_init, L_, S_, L.PROB_F64 if prob_mode is None else prob_mode,
                                                   L.REJECT_DEFAULT, 0.99, None, 0, 10, ctypes.byref(oc) if out else None, None, None)


def test_eval_mc_rows_policy_pop_validation_before_any_hip_call():
    from rl_offline_simulation_amd import _lib as L
    lib = L.load()
    assert _scan_pop(3, 5, R=0) == L.OK, lib.offsim_last_error()  # R = 0 validates and launches nothing
    for l_, s_ in ((0, 5), (-1, 5), (65536, 1), (3, 0), (3, -2)):
        assert _scan_pop(l_, s_, R=15) == L.EINVAL and lib.offsim_last_error().startswith(b"eval_mc_rows_policy_pop"), (l_, s_)
    for r in (14, 16, 5, 3):
        assert _scan_pop(3, 5, R=r) == L.EINVAL and b"L * S" in lib.offsim_last_error(), r
    assert _scan_pop(3, 5, p_next=None) == L.EINVAL and b"NULL" in lib.offsim_last_error()
    assert _scan_pop(3, 5, p_init=None) == L.EINVAL and b"NULL" in lib.offsim_last_error()
    assert _scan_pop(3, 5, R=0, p_next=None, p_init=None, N=0, N0=0) == L.OK  # an empty table needs no tables
    assert _scan_pop(3, 5, out=False) == L.EINVAL
    assert _scan_pop(3, 5, prob_mode=7) == L.EINVAL
    assert _scan_pop(3, 5, prob_mode=L.PROB_F32, plog_dtype=L.F64) == L.EINVAL and b"f32 p_log" in lib.offsim_last_error()
    assert _scan_pop(3, 5, init_slot=None) == L.EINVAL and b"init rows" in lib.offsim_last_error()
    t, ro, _, _, _, _ = _args(R=15)
    oc = L.EvalMCOut(sum_g=F, n_ep=F, steps=F, cand=F, n_len=F)  # no status
    assert lib.offsim_eval_mc_rows_policy_pop(ctypes.byref(t), ctypes.byref(ro), F, F, 3, 5, L.PROB_F64, L.REJECT_DEFAULT, 0.99, None, 0, 10, ctypes.byref(oc),
                                              None, None) == L.EINVAL
    assert lib.offsim_eval_mc_rows_policy_pop(ctypes.byref(t), None, F, F, 3, 5, L.PROB_F64, L.REJECT_DEFAULT, 0.99, None, 0, 10, ctypes.byref(oc), None,
                                              None) == L.EINVAL
    assert lib.offsim_eval_mc_rows_policy_pop(None, ctypes.byref(ro), F, F, 3, 5, L.PROB_F64, L.REJECT_DEFAULT, 0.99, None, 0, 10, ctypes.byref(oc), None,
                                              None) == L.EINVAL


# ---- PolicyPopulation, host side ----
def _policies(n, sizes=(4, 16, 2), act="tanh", seed=0):
    from rl_offline_simulation_amd.evaluators import MLPPolicy
    g = torch.Generator().manual_seed(seed)
    return [MLPPolicy([(torch.randn(o, i, generator=g), torch.randn(o, generator=g)) for i, o in zip(sizes, sizes[1:])], act) for _ in range(n)]


def test_from_policies_stacks_in_order():
    from rl_offline_simulation_amd.evaluators import PolicyPopulation
    pols = _policies(3)
    pop = PolicyPopulation.from_policies(pols)
    assert len(pop) == 3 and all(pop.policy(l) is pols[l] for l in range(3))
    ws, arr = pop._stack._device_weights("cpu")
    assert [tuple(W.shape) for W, _ in ws] == [(3, 16, 4), (3, 2, 16)] and [tuple(b.shape) for _, b in ws] == [(3, 16), (3, 2)]
    for l in range(3):
        for i in range(2):
            assert torch.equal(ws[i][0][l], pols[l].weights[i][0]) and torch.equal(ws[i][1][l], pols[l].weights[i][1])
    assert arr[0].W == ws[0][0].data_ptr() and arr[1].b == ws[1][1].data_ptr() and (getattr(arr[0], "in"), arr[0].out) == (4, 16)  # learner 0
    assert pop._stack._device_weights("cpu")[0] is ws  # stacked once
    with pytest.raises(IndexError):
        pop.policy(3)


def test_layer_array_of_a_policy_tile_points_at_its_first_learner():
    from rl_offline_simulation_amd.evaluators.obs_policy import PolicyPopulation, _stacked_layers
    ws, _ = PolicyPopulation.from_policies(_policies(4))._stack._device_weights("cpu")
    arr = _stacked_layers(ws, 2)
    assert arr[0].W == ws[0][0].data_ptr() + 2 * 16 * 4 * 4 and arr[0].b == ws[0][1].data_ptr() + 2 * 16 * 4
    assert arr[1].W == ws[1][0].data_ptr() + 2 * 2 * 16 * 4 and arr[1].b == ws[1][1].data_ptr() + 2 * 2 * 4


def test_mixed_architectures_refused():
    from rl_offline_simulation_amd.evaluators import PolicyPopulation, RowPolicy
    a = _policies(2)
    for other in (_policies(1, sizes=(4, 8, 2)), _policies(1, act="relu"), _policies(1, sizes=(4, 16, 16, 2))):
        with pytest.raises(ValueError, match="one architecture"):
            PolicyPopulation.from_policies(a + other)
    nob = _policies(1)[0]
    nob.weights[0] = (nob.weights[0][0], None)
    with pytest.raises(ValueError, match="one architecture"):
        PolicyPopulation.from_policies(a + [nob])
    with pytest.raises(ValueError):
        PolicyPopulation.from_policies(a + [RowPolicy(np.zeros((3, 2)), np.zeros((3, 2)))])
    with pytest.raises(ValueError):
        PolicyPopulation.from_policies([])
    with pytest.raises(ValueError):
        PolicyPopulation.from_rows([object()])
    with pytest.raises(TypeError):
        PolicyPopulation.from_ppo(a[0])


def test_from_ppo_aliases_the_populations_tensors():
    from rl_offline_simulation_amd.evaluators import MLPValue, PolicyPopulation, PPOPopulation
    g = torch.Generator().manual_seed(1)
    critics = [MLPValue([(torch.randn(16, 4, generator=g), torch.randn(16, generator=g)), (torch.randn(1, 16, generator=g), torch.randn(1, generator=g))])
               for _ in range(3)]
    ppo = PPOPopulation(_policies(3), critics)
    pop = PolicyPopulation.from_ppo(ppo)
    assert len(pop) == 3 and pop._stack is ppo._pi
    ws, arr = pop._stack._device_weights("cpu")
    assert all(W is W2 and b is b2 for (W, b), (W2, b2) in zip(ws, ppo._pi.ws))  # the same tensors: nothing copied
    ppo._pi.ws[0][0][1].add_(1.0)  # an in-place update, as offsim_ppo_update_pop does on the device
    assert torch.equal(pop.policy(1).weights[0][0], ppo._pi.ws[0][0][1]) and arr[0].W == ppo._pi.ws[0][0].data_ptr()
    assert hasattr(ppo, "evaluate")


def test_from_rows_needs_observations_only_for_callables():
    from rl_offline_simulation_amd.evaluators import CallablePolicy, PolicyPopulation, RowPolicy
    rows = [RowPolicy(np.zeros((3, 2)), np.zeros((3, 2))) for _ in range(2)]
    assert not PolicyPopulation.from_rows(rows).needs_obs()
    assert PolicyPopulation.from_rows(rows + [CallablePolicy(lambda x: x)]).needs_obs()
    assert PolicyPopulation.from_policies(_policies(2)).needs_obs()
    assert PolicyPopulation.from_rows(rows).policy(1) is rows[1]


# ---- the NumPy restatement ----
@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_restatement_policy_0_reproduces_the_reference(path):
    d = np.load(path)
    P_next, P_init = PH.fixture_policies(d)
    assert np.array_equal(P_next[0], d["P_next"]) and P_next.dtype == d["P_next"].dtype and P_next.shape[0] == 3
    got = PH.evalmc_rows_population(H.fixture_inputs(d), P_next[:1], P_init[:1], d["seeds"], float(d["gamma"]))
    assert sorted(got) == [(0, j) for j in range(len(d["seeds"]))]
    for j, s in enumerate(d["seeds"]):
        o = got[(0, j)]
        assert o["status"] == str(d[f"status_{s}"])
        assert np.array_equal(o["rows"], d[f"rows_{s}"])
        if o["status"] == "ok":
            assert np.array_equal(o["Gs"], d[f"Gs_{s}"]) and np.array_equal(o["lengths"], d[f"lengths_{s}"])


def test_restatement_rollouts_depend_on_their_policy_only():
    d = np.load(os.path.join(ROOT, "tests", "golden", "obs_policy", "obs_policy_grid_f64.npz"))
    P_next, P_init = PH.fixture_policies(d)
    seeds = d["seeds"][:2]
    got = PH.evalmc_rows_population(H.fixture_inputs(d), P_next, P_init, seeds, 0.99)
    assert len(got) == 6
    alone = PH.evalmc_rows_population(H.fixture_inputs(d), P_next[2:], P_init[2:], seeds[1:], 0.99)[(0, 0)]
    assert np.array_equal(got[(2, 1)]["rows"], alone["rows"]) and np.array_equal(got[(2, 1)]["Gs"], alone["Gs"])
    assert not np.array_equal(got[(0, 0)]["rows"], got[(1, 0)]["rows"])  # another policy accepts other rows from the same queues
