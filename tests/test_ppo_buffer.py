"""CPU side of VectorPSRS.collect_ppo: the NumPy restatement of the PPO buffer rules (tests/ppo_host.py) pinned on fixtures recorded from
the reference's PPO agent (tests/golden/ppo/*.npz, made by tests/golden/make_golden_ppo.py), the C ABI (structs and argument validation of
offsim_value_mlp, offsim_vector_collect_ppo, offsim_ppo_advantages), and MLPPolicy / MLPValue.from_torch on spinup's actor-critic."""
import ctypes
import glob
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_host as H  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ppo", "*.npz")))


def _standins():
    """The spinup stand-ins of the fixture generator (mlp, MLPActorCritic; nothing of the reference is read)."""
    spec = importlib.util.spec_from_file_location("make_golden_ppo", os.path.join(ROOT, "tests", "golden", "make_golden_ppo.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def epochs(d):
    """(seed, epoch j, its [T] records) of a fixture"""
    T = int(d["T"])
    for s in d["seeds"]:
        for j in range(2):
            sl = slice(j * T, (j + 1) * T)
            yield int(s), j, dict(rows=d[f"rows_{s}"][sl], obs_row=d[f"obs_row_{s}"][sl], term=d[f"terminated_{s}"][sl],
                                  trunc=d[f"truncated_{s}"][sl], **{k: d[f"{k}_{s}_{j}"] for k in ("obs", "act", "rew", "val", "logp", "adv_raw",
                                                                                                   "ret", "adv", "adv_mean", "adv_std", "last_val")})


def close(got, want, rel=1e-4):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all(np.abs(got - want) <= rel * np.maximum(1.0, np.abs(want))))


def test_fixtures_present_and_cover_every_branch():
    names = {os.path.basename(p)[:-4] for p in FIXTURES}
    assert {"ppo_cartpole_f32_cap500", "ppo_cartpole_f64_cap8", "ppo_cartpole_f32_end_at_last"} <= names
    cover = dict(term=0, trunc=0, both=0, end_at_last=0, cut=0)
    dtypes = set()
    for p in FIXTURES:
        d = np.load(p)
        dtypes.add(d["p_log"].dtype)
        T = int(d["T"])
        for s, j, e in epochs(d):
            cover["term"] += int((e["term"] & ~e["trunc"]).sum())
            cover["trunc"] += int((e["trunc"] & ~e["term"]).sum())
            cover["both"] += int((e["term"] & e["trunc"]).sum())
            cover["end_at_last"] += int(e["term"][T - 1] and not e["trunc"][T - 1])
            cover["cut"] += int(not (e["term"][T - 1] or e["trunc"][T - 1]))
            assert np.isnan(e["last_val"]) == bool(e["term"][T - 1] or e["trunc"][T - 1])
    assert all(v > 0 for v in cover.values()), cover
    assert dtypes == {np.dtype(np.float32), np.dtype(np.float64)}


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_host_restatement_matches_reference(path):
    d = np.load(path)
    gamma, lam = float(d["gamma"]), float(d["lam"])
    for s, j, e in epochs(d):
        T = len(e["rew"])
        valid = np.ones(T, bool)
        fv = 0.0 if np.isnan(e["last_val"]) else float(e["last_val"])
        adv, ret = H.gae(e["rew"], e["val"], e["term"], e["trunc"], valid, fv, gamma, lam)
        assert close(adv, e["adv_raw"]) and close(ret, e["ret"]), (s, j)
        mean, std = H.statistics(adv.astype(np.float32))
        assert close(mean, e["adv_mean"]) and close(std, e["adv_std"]), (s, j)
        assert close((adv.astype(np.float32) - mean) / std, e["adv"]), (s, j)
        # the buffer's inputs are the served rows' (reward, action, observation asked at)
        assert np.array_equal(e["rew"], d["r"][e["rows"]].astype(np.float32)) and np.array_equal(e["act"], d["a"][e["rows"]].astype(np.float32))
        src = np.where((e["obs_row"] >= 0)[:, None], d["next_obs"][np.maximum(e["obs_row"], 0)], d["obs"][np.maximum(-2 - e["obs_row"], 0)])
        assert np.array_equal(e["obs"], src.astype(np.float32)), (s, j)


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_recorded_val_and_logp_are_the_networks(path):
    """val / logp as recorded: the stored weights under spinup's forward (one observation at a time, as the agent asks)."""
    m = _standins()
    d = np.load(path)
    pi = m.mlp([4, 16, 16, 2], torch.nn.Tanh)
    v = m.mlp([4, 16, 16, 1], torch.nn.Tanh)
    for name, net in (("pi", pi), ("v", v)):
        lin = [x for x in net if isinstance(x, torch.nn.Linear)]
        with torch.no_grad():
            for k, x in enumerate(lin):
                x.weight.copy_(torch.from_numpy(d[f"{name}_W{k}"]))
                x.bias.copy_(torch.from_numpy(d[f"{name}_b{k}"]))
    with torch.no_grad():
        for s, j, e in epochs(d):
            for t in range(0, len(e["rew"]), 7):
                o = torch.as_tensor(e["obs"][t], dtype=torch.float32)
                assert torch.squeeze(v(o), -1).numpy() == e["val"][t]
                lp = torch.distributions.Categorical(logits=pi(o)).log_prob(torch.as_tensor(e["act"][t]))
                assert lp.numpy() == e["logp"][t]


def test_host_batch_rules():
    """The two bootstrap modes and the open path on a hand-made [T, E] example."""
    rew = np.array([[1.0, 1.0], [1.0, 1.0], [1.0, 1.0]])
    val = np.array([[0.5, 2.0], [0.25, 3.0], [0.125, 4.0]])
    term = np.array([[False, True], [True, False], [False, False]])
    trunc = np.array([[False, True], [False, False], [False, True]])
    valid = np.array([[True, True], [True, True], [True, False]])
    fv = np.array([10.0, 20.0])
    vt = np.full((3, 2), 7.0)
    g = 0.5
    adv, ret, _, _, _ = H.batch(rew, val, term, trunc, valid, fv, g, 1.0)
    # env 0: path [0, 1] terminated at 1 (not the last step): bootstrap 0; path [2] open: final_value
    assert ret[2, 0] == 1 + g * 10 and ret[1, 0] == 1.0 and ret[0, 0] == 1 + g * 1
    # env 1: step 0 terminated and truncated: reference bootstraps with val (2.0); step 1 open (step 2 invalid): final_value
    assert ret[0, 1] == 1 + g * 2.0 and ret[1, 1] == 1 + g * 20
    adv, ret, _, _, _ = H.batch(rew, val, term, trunc, valid, fv, g, 1.0, mode="spinup", v_trunc=vt)
    assert ret[0, 1] == 1.0 and ret[1, 1] == 1 + g * 20
    assert adv[1, 1] == 1 + g * 20 - 3.0


def test_ppo_struct_layout(tmp_path):
    """sizeof / offsetof of the new structs of include/offsim.h as gcc lays them out, against the ctypes mirrors in _lib.py."""
    from rl_offline_simulation_amd import _lib
    pairs = {"offsim_collect_value": _lib.CollectValue, "offsim_collect_ppo_out": _lib.CollectPPOOut}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "offsim.h"', "int main(void) {"]
    for c_name, cls in pairs.items():
        lines.append(f'  printf("{c_name} %zu\\n", sizeof({c_name}));')
        for f, _ in cls._fields_:
            lines.append(f'  printf("{c_name}.{f} %zu\\n", offsetof({c_name}, {f}));')
    lines.append('  printf("work %d\\n", (int)OFFSIM_PPO_WORK_DOUBLES(1000));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for c_name, cls in pairs.items():
        assert int(got[c_name]) == ctypes.sizeof(cls), c_name
        for f, _ in cls._fields_:
            assert int(got[f"{c_name}.{f}"]) == getattr(cls, f).offset, (c_name, f)
    assert int(got["work"]) == _lib.ppo_work_doubles(1000)
    src_h = open(os.path.join(ROOT, "include", "offsim.h")).read()
    for name, v in (("OFFSIM_VALUE_MLP", _lib.VALUE_MLP), ("OFFSIM_VALUE_ROWS", _lib.VALUE_ROWS),
                    ("OFFSIM_PPO_BOOT_REFERENCE", _lib.PPO_BOOT_REFERENCE), ("OFFSIM_PPO_BOOT_SPINUP", _lib.PPO_BOOT_SPINUP)):
        assert f"#define {name} {v}" in src_h, name


def _layers(sizes):
    from rl_offline_simulation_amd import _lib as L
    arr = (L.MLPLayer * (len(sizes) - 1))()
    for i in range(len(sizes) - 1):
        arr[i].W, arr[i].b, arr[i].out = 0x1000, 0x1000, sizes[i + 1]
        setattr(arr[i], "in", sizes[i])
    return arr


def test_value_mlp_validation_before_any_hip_call():
    from rl_offline_simulation_amd import _lib as L
    lib = L.load()
    ok = _layers([4, 8, 1])
    assert lib.offsim_value_mlp(0x1000, L.F32, 10, 4, None, 0, ok, 2, L.ACT_TANH, 0.01, 0x1000, None) == L.OK  # M = 0: nothing launched
    assert lib.offsim_value_mlp(0x1000, L.F32, 10, 4, None, 0, _layers([4, 8, 2]), 2, L.ACT_TANH, 0.01, 0x1000, None) == L.EINVAL
    assert b"one output" in lib.offsim_last_error() and b"value_mlp" in lib.offsim_last_error()
    assert lib.offsim_value_mlp(0x1000, L.F64, 10, 4, None, 0, ok, 2, L.ACT_TANH, 0.01, 0x1000, None) == L.EINVAL
    assert lib.offsim_value_mlp(None, L.F32, 10, 4, None, 3, ok, 2, L.ACT_TANH, 0.01, 0x1000, None) == L.EINVAL
    # offsim_policy_mlp's messages are unchanged
    assert lib.offsim_policy_mlp(0x1000, L.F64, 10, 4, None, 0, ok, 2, L.ACT_TANH, 0.01, 0x1000, None) == L.EINVAL
    assert lib.offsim_last_error() == b"policy_mlp: x_dtype must be OFFSIM_F32 or OFFSIM_F16"


def _collect_args():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_collect import _args
    return _args()


def test_collect_ppo_validation_before_any_hip_call():
    from rl_offline_simulation_amd import _lib as L
    lib = L.load()
    t, ro, pol, st, out, layers = _collect_args()
    vl = _layers([4, 8, 1])
    val = L.CollectValue(form=L.VALUE_MLP, n_layers=2, layers_host=ctypes.cast(vl, ctypes.POINTER(L.MLPLayer)), activation=L.ACT_TANH,
                         x_dtype=L.F32, dO=4, x_start=0x1000, x_next=0x1000, x_init=0x1000)
    ppo = L.CollectPPOOut(value=0x1000, logp=0x1000, final_value=0x1000)

    def call(T=0, v=val, p=ppo, pl=pol):
        return lib.offsim_vector_collect_ppo(ctypes.byref(t), ctypes.byref(ro), ctypes.byref(pl), ctypes.byref(v) if v is not None else None,
                                             L.PROB_F64, L.REJECT_DEFAULT, T, 0, ctypes.byref(st), ctypes.byref(out),
                                             ctypes.byref(p) if p is not None else None, None)
    assert call() == L.OK
    assert call(v=None) == L.EINVAL and call(p=None) == L.EINVAL
    ro.R = 0
    assert call(T=1, p=L.CollectPPOOut(value=0x1000, logp=0x1000)) == L.EINVAL and b"final_value" in lib.offsim_last_error()
    ro.R = 2
    assert call(T=-1) == L.EINVAL  # collect's own checks come first
    for field, bad in (("form", 5), ("x_dtype", L.F16), ("activation", 9), ("dO", 129), ("n_layers", 0)):
        old = getattr(val, field)
        setattr(val, field, bad)
        assert call() == L.EINVAL, field
        setattr(val, field, old)
    vl[1].out = 2  # a critic has one output unit
    assert call() == L.EINVAL and b"one output" in lib.offsim_last_error()
    vl[1].out = 1
    rows = L.CollectValue(form=L.VALUE_ROWS)
    assert call(v=rows) == L.EINVAL  # v_next / v_init NULL
    assert call(v=L.CollectValue(form=L.VALUE_ROWS, v_next=0x1000, v_init=0x1000)) == L.OK
    # the actor's and the critic's weights share OFFSIM_COLLECT_MLP_MAX_FLOATS
    big = _layers([4, 120, 120, 1])  # 4*120+120 + 120*120+120 + 121 = 15321 floats; with the actor's 4*8+8+8*2+2 = 58: fits
    vb = L.CollectValue(form=L.VALUE_MLP, n_layers=3, layers_host=ctypes.cast(big, ctypes.POINTER(L.MLPLayer)), activation=L.ACT_TANH,
                        x_dtype=L.F32, dO=4, x_start=0x1000, x_next=0x1000, x_init=0x1000)
    assert call(v=vb) == L.OK
    big[1].out = 129
    setattr(big[2], "in", 129)  # 600 + 129*121 + 130 = 16339 floats of the critic, + 58 of the actor > 16384
    assert call(v=vb) == L.EUNSUPPORTED and b"MAX_FLOATS" in lib.offsim_last_error()
    tab = L.CollectPolicy(form=L.COLLECT_TABULAR, pi=0x1000)
    assert call(v=vb, pl=tab) == L.OK  # alone within the budget


def test_ppo_advantages_validation_before_any_hip_call():
    from rl_offline_simulation_amd import _lib as L
    lib = L.load()
    f = 0x1000

    def call(T=4, E=3, boot=L.PPO_BOOT_REFERENCE, v_trunc=None, gamma=0.99, lam=0.97, adv_norm=None, stats=None, work=None, rew=f):
        return lib.offsim_ppo_advantages(rew, f, f, f, v_trunc, T, E, gamma, lam, boot, f, f, adv_norm, stats, work, None)
    assert call(T=0) == L.OK and call(E=0) == L.OK
    assert call(T=-1) == L.EINVAL and call(E=-1) == L.EINVAL
    assert call(T=0, boot=2) == L.EINVAL and b"bootstrap" in lib.offsim_last_error()
    assert call(T=0, gamma=1.5) == L.EINVAL and call(T=0, lam=-0.1) == L.EINVAL and call(T=0, gamma=float("nan")) == L.EINVAL
    assert call(rew=None) == L.EINVAL
    assert call(boot=L.PPO_BOOT_SPINUP) == L.EINVAL and b"v_trunc" in lib.offsim_last_error()
    assert call(adv_norm=f) == L.EINVAL and b"stats" in lib.offsim_last_error()


def test_from_torch_loads_spinup_actor_critic():
    """spinup's mlp() ends every network in nn.Identity (its output activation); MLPPolicy / MLPValue.from_torch take the actor and the
    critic of an MLPActorCritic as they are."""
    from rl_offline_simulation_amd.evaluators import MLPPolicy, MLPValue
    m = _standins()

    class Box:
        shape = (4,)

    class Discrete:
        n, shape = 2, ()

    torch.manual_seed(0)
    ac = m.MLPActorCritic(Box(), Discrete(), hidden_sizes=(64, 64))
    assert isinstance(ac.pi.logits_net[-1], torch.nn.Identity)
    p, v = MLPPolicy.from_torch(ac.pi), MLPValue.from_torch(ac.v)
    assert p.activation == "tanh" and p.nA == 2 and len(p.weights) == 3 and p.dO == 4
    assert v.activation == "tanh" and v.nA == 1 and len(v.weights) == 3
    assert torch.equal(v.weights[2][0], ac.v.v_net[4].weight.detach())
    assert MLPPolicy.from_torch(m.mlp([3, 5], torch.nn.ReLU)).activation == "identity"  # Linear, Identity
    with pytest.raises(ValueError):
        MLPValue.from_torch(ac.pi.logits_net)  # two outputs
    with pytest.raises(TypeError):
        MLPValue.from_torch(torch.nn.Sequential(torch.nn.Linear(4, 1), torch.nn.Identity(), torch.nn.Identity()))
    with pytest.raises(TypeError):  # an Identity is dropped only after the last Linear
        MLPPolicy.from_torch(torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.Tanh(), torch.nn.Identity()))
