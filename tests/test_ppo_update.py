"""CPU side of PPOLearner.update: the NumPy f64 restatement of the PPO update (tests/ppo_update_host.py) pinned on fixtures recorded from the
reference's PPOAgentRevealed.adapt() (tests/golden/ppo_update/*.npz, made by tests/golden/make_golden_ppo_update.py), and the C ABI of
offsim_ppo_grad / offsim_ppo_update (struct layouts, argument validation before any HIP call, the float cap, zero-size calls)."""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_update_host as U  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ppo_update", "*.npz")))
IDS = [os.path.basename(p)[:-4] for p in FIXTURES]
MARGIN = 0.05


def close(got, want, rel=1e-4):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all(np.abs(got - want) <= rel * np.maximum(1.0, np.abs(want))))


def nets(d):
    """(actor, critic) before the update, as lists of (W, b) in f32"""
    out = []
    for key, sizes in (("pi_before", d["sizes_pi"]), ("v_before", d["sizes_v"])):
        like = [(np.zeros((int(o), int(i)), np.float32), np.zeros(int(o), np.float32)) for i, o in zip(sizes[:-1], sizes[1:])]
        out.append([(W.astype(np.float32), b.astype(np.float32)) for W, b in U.unflatten(d[key], like)])
    return out


def hyper(d):
    return {k[6:]: float(d[k]) for k in d.files if k.startswith("hyper_")}


def host_run(d):
    """the f64 host update of both networks on a fixture's data"""
    h, act = hyper(d), str(d["activation"])
    pi, v = nets(d)
    data = {k: d[k] for k in ("obs", "act", "adv", "logp", "ret")}
    a = U.update(pi, "actor", data, int(h["train_pi_iters"]), h["pi_lr"], h["clip_ratio"], h["target_kl"], act)
    c = U.update(v, "critic", data, int(h["train_v_iters"]), h["vf_lr"], h["clip_ratio"], h["target_kl"], act)
    return a, c


def test_fixtures_present_and_cover_the_cases():
    assert {"ppo_update_full_tanh", "ppo_update_stop_tanh", "ppo_update_relu_na3"} <= set(IDS)
    full = stop = other = 0
    for p in FIXTURES:
        d = np.load(p)
        h = hyper(d)
        lim = 1.5 * h["target_kl"]
        kl = d["pi_trace"][:, 1]
        assert np.all(np.abs(kl - lim) >= MARGIN * lim), p  # no recorded kl near the threshold: ulps cannot move StopIter
        assert 2000 <= len(d["adv"]) <= 5000 and os.path.getsize(p) < 170_000
        iters, si = int(h["train_pi_iters"]), int(d["log_StopIter"])
        stopped = kl[-1] > lim
        assert len(kl) == si + 1 and (stopped or si == iters - 1)
        full += int(not stopped)
        stop += int(stopped and 3 <= si <= iters - 10)
        other += int(d["sizes_pi"][-1] > 2 and str(d["activation"]) != "tanh")
    assert full and stop and other


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_host_first_pass_matches_reference(path):
    d = np.load(path)
    h, act = hyper(d), str(d["activation"])
    pi, v = nets(d)
    loss, kl, ent, cf, g, n = U.loss_pi(pi, d["obs"], d["act"], d["adv"], d["logp"], h["clip_ratio"], act)
    assert n == len(d["adv"])
    assert close(loss, d["pi_old"][0]) and close(kl, d["pi_old"][1]) and close(ent, d["ent_old"]) and close(ent, d["log_Entropy"])
    assert close(loss, d["log_LossPi"])
    assert close(g / np.abs(d["g_pi"]).max(), d["g_pi"] / np.abs(d["g_pi"]).max())
    lv, gv, _ = U.loss_v(v, d["obs"], d["ret"], act)
    assert close(lv, d["v_old"]) and close(lv, d["log_LossV"])
    assert close(gv / np.abs(d["g_v"]).max(), d["g_v"] / np.abs(d["g_v"]).max())
    # valid = all ones and a masked copy with garbage in the invalid entries give the same numbers
    M = len(d["adv"])
    valid = np.ones(2 * M, bool)
    valid[1::2] = False
    dbl = lambda x: np.repeat(np.asarray(x), 2, axis=0)  # noqa: E731
    loss2, kl2, _, _, g2, n2 = U.loss_pi(pi, dbl(d["obs"]), dbl(d["act"]), dbl(d["adv"]), dbl(d["logp"]), h["clip_ratio"], act, valid=valid)
    assert n2 == M and loss2 == loss and kl2 == kl and np.array_equal(g2, g)


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_host_update_matches_reference(path, capsys):
    d = np.load(path)
    a, c = host_run(d)
    assert a["stop_iter"] == int(d["log_StopIter"])
    assert a["trace"].shape == d["pi_trace"].shape and close(a["trace"], d["pi_trace"])
    assert c["trace"].shape == d["v_trace"].shape and close(c["trace"][:, 0], d["v_trace"][:, 0])
    assert close(a["last"]["kl"], d["log_KL"]) and close(a["last"]["cf"], d["log_ClipFrac"]) and close(a["first"]["ent"], d["log_Entropy"])
    assert close(a["last"]["loss"] - a["first"]["loss"], d["log_DeltaLossPi"]) and close(c["last"]["loss"] - c["first"]["loss"], d["log_DeltaLossV"])
    # the reference's own f32 error on the final weights: the scale of the device test's bound
    d_pi = float(np.abs(U.flatten(a["net"]) - d["pi_after"]).max())
    d_v = float(np.abs(U.flatten(c["net"]) - d["v_after"]).max())
    with capsys.disabled():
        print(f"\n  {os.path.basename(path)[:-4]}: d_ref actor {d_pi:.3e}  critic {d_v:.3e}  "
              f"(max|w| {np.abs(d['pi_after']).max():.3f} / {np.abs(d['v_after']).max():.3f})")
    assert d_pi < 1e-3 and d_v < 1e-3  # (sanity only: Adam moves a weight by about lr per step)


def test_host_adam_is_torch_adam():
    import torch
    rng = np.random.default_rng(0)
    p0 = rng.normal(size=7)
    p = torch.nn.Parameter(torch.tensor(p0, dtype=torch.float64))
    opt = torch.optim.Adam([p], lr=1e-2)
    mine, flat = U.Adam(7, 1e-2), p0.copy()
    for i in range(5):
        g = rng.normal(size=7) * 10.0 ** -i
        p.grad = torch.tensor(g)
        opt.step()
        flat = mine.step(flat, g)
        assert np.allclose(flat, p.detach().numpy(), rtol=1e-12, atol=1e-14)


# ---- the C ABI ----
def test_ppo_update_struct_layout(tmp_path):
    from rl_offline_simulation_amd import _lib
    pairs = {"offsim_ppo_layer": _lib.MLPLayer, "offsim_ppo_net": _lib.PPONet, "offsim_ppo_batch": _lib.PPOBatchC, "offsim_ppo_adam": _lib.PPOAdam}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "offsim.h"', "int main(void) {"]
    for c_name, cls in pairs.items():
        lines.append(f'  printf("{c_name} %zu\\n", sizeof({c_name}));')
        for f, _ in cls._fields_:
            lines.append(f'  printf("{c_name}.{f} %zu\\n", offsetof({c_name}, {f}));')
    lines.append('  printf("work %lld\\n", (long long)OFFSIM_PPO_UPDATE_WORK_DOUBLES(4611));')
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
    assert int(got["work"]) == _lib.ppo_update_work_doubles(4611)
    src_h = open(os.path.join(ROOT, "include", "offsim.h")).read()
    for name, v in (("OFFSIM_PPO_ACTOR", _lib.PPO_ACTOR), ("OFFSIM_PPO_CRITIC", _lib.PPO_CRITIC), ("OFFSIM_PPO_MAX_BLOCKS", _lib.PPO_MAX_BLOCKS)):
        assert f"#define {name} {v}" in src_h, name


def _layers(sizes, bias=True):
    from rl_offline_simulation_amd import _lib as L
    arr = (L.MLPLayer * (len(sizes) - 1))()
    for i in range(len(sizes) - 1):
        arr[i].W, arr[i].b, arr[i].out = 0x1000, (0x1000 if bias else None), sizes[i + 1]
        setattr(arr[i], "in", sizes[i])
    return arr


def _net(sizes, act=1, slope=0.01, bias=True):
    from rl_offline_simulation_amd import _lib as L
    arr = _layers(sizes, bias)
    n = L.PPONet(n_layers=len(sizes) - 1, activation=act, layers_host=ctypes.cast(arr, ctypes.POINTER(L.MLPLayer)), slope=slope)
    n._keep = arr
    return n


def test_ppo_grad_and_update_validation_before_any_hip_call():
    from rl_offline_simulation_amd import _lib as L
    lib = L.load()
    f = 0x1000
    net = _net([4, 8, 2])

    def batch(M=0, **kw):
        b = L.PPOBatchC(obs=f, x_dtype=L.F32, dO=4, act=f, adv=f, logp=f, ret=f, valid=None, M=M)
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    def grad(n=net, kind=L.PPO_ACTOR, b=None, clip=0.2, g=f, stats=f, work=f):
        b = batch() if b is None else b
        return lib.offsim_ppo_grad(ctypes.byref(n) if n is not None else None, kind, ctypes.byref(b), clip, g, stats, work, None)

    def upd(n=net, kind=L.PPO_ACTOR, b=None, clip=0.2, kl=0.01, iters=3, opt=-1, stats=f, trace=f, work=f):
        b = batch() if b is None else b
        o = L.PPOAdam(m=f, v=f, t=f, lr=1e-3) if opt == -1 else opt
        return lib.offsim_ppo_update(ctypes.byref(n) if n is not None else None, kind, ctypes.byref(b), clip, kl, iters,
                                     ctypes.byref(o) if o is not None else None, stats, trace, work, None)

    # zero-size calls launch nothing (every pointer here is a fake address: a launch would fault)
    assert grad() == L.OK and upd() == L.OK and upd(b=batch(M=5), iters=0) == L.OK
    assert grad(n=None) == L.EINVAL and b"ppo_grad" in lib.offsim_last_error()
    assert upd(n=None) == L.EINVAL and b"ppo_update" in lib.offsim_last_error()
    assert grad(kind=2) == L.EINVAL and upd(kind=-1) == L.EINVAL
    assert grad(b=batch(M=-1)) == L.EINVAL
    assert grad(b=batch(x_dtype=L.F64)) == L.EINVAL and b"x_dtype" in lib.offsim_last_error()
    assert grad(b=batch(dO=0)) == L.EINVAL and grad(b=batch(dO=129)) == L.EINVAL
    assert grad(b=batch(dO=5)) == L.EINVAL and b"chain" in lib.offsim_last_error()
    assert grad(n=_net([4, 8, 2], act=9)) == L.EINVAL and b"activation" in lib.offsim_last_error()
    assert grad(n=_net([4, 8, 2], act=L.ACT_LEAKY_RELU, slope=-0.1)) == L.EINVAL and b"slope" in lib.offsim_last_error()
    assert grad(n=_net([4, 8, 2], act=L.ACT_LEAKY_RELU, slope=0.1)) == L.OK
    assert grad(n=_net([4, 257, 2])) == L.EINVAL and b"hidden" in lib.offsim_last_error()
    assert grad(n=_net([4, 8, 17])) == L.EINVAL and b"16 actions" in lib.offsim_last_error()
    assert grad(n=_net([4, 8, 2]), kind=L.PPO_CRITIC) == L.EINVAL and b"one output" in lib.offsim_last_error()
    assert grad(n=_net([4, 8, 1]), kind=L.PPO_CRITIC) == L.OK
    five = _net([4, 8, 8, 8, 8, 2])
    assert grad(n=five) == L.EINVAL and b"1 to 4" in lib.offsim_last_error()
    nullw = _net([4, 8, 2])
    nullw._keep[1].W = None
    assert grad(n=nullw) == L.EINVAL and b"W is NULL" in lib.offsim_last_error()
    for c in (-0.1, 1.0, float("nan")):
        assert grad(clip=c) == L.EINVAL and upd(clip=c) == L.EINVAL
    # M > 0: the columns of the kind and the outputs must be there
    assert grad(b=batch(M=3, obs=None)) == L.EINVAL
    assert grad(b=batch(M=3, adv=None)) == L.EINVAL and b"act, adv and logp" in lib.offsim_last_error()
    assert grad(n=_net([4, 8, 1]), kind=L.PPO_CRITIC, b=batch(M=3, ret=None)) == L.EINVAL and b"ret" in lib.offsim_last_error()
    assert grad(b=batch(M=3), g=None) == L.EINVAL and grad(b=batch(M=3), work=None) == L.EINVAL
    assert upd(kl=-1.0) == L.EINVAL and upd(iters=-1) == L.EINVAL and upd(opt=None) == L.EINVAL
    assert upd(opt=L.PPOAdam(m=f, v=f, t=f, lr=-1.0)) == L.EINVAL
    assert upd(b=batch(M=3), opt=L.PPOAdam(m=f, v=None, t=f, lr=1e-3)) == L.EINVAL and b"opt->m" in lib.offsim_last_error()
    assert upd(b=batch(M=3), trace=None) == L.EINVAL and upd(b=batch(M=3), stats=None) == L.EINVAL


# One table of bad networks through every entry point that takes a network: pmlp_describe (csrc/policy_mlp.hpp) is the one validator, so
# each refusal must come back with OFFSIM_EINVAL, that entry point's prefix and the same key word, before any HIP call (fake pointers).
# A case: (what differs from the good network 4 -> 8 -> 2 | 1, the key word for an actor, for a critic (None: a good actor, not run)).
_BAD_NETS = {
    "five_layers": (dict(sizes=[4, 8, 8, 8, 8, None]), b"1 to 4", b"1 to 4"),
    "null_W": (dict(null_w=1), b"W is NULL", b"W is NULL"),
    "no_chain": (dict(sizes=[4, 8, None], in1=9), b"chain", b"chain"),
    "hidden_257": (dict(sizes=[4, 257, None]), b"hidden", b"hidden"),
    "outputs_17": (dict(sizes=[4, 8, 17]), b"16 actions", b"one output"),
    "critic_2_outputs": (dict(sizes=[4, 8, 2]), None, b"one output"),
    "activation_9": (dict(act=9), b"activation", b"activation"),
    "x_dtype_f64": (dict(x_dtype="F64"), b"x_dtype", b"x_dtype"),
    "dO_0": (dict(sizes=[0, 8, None], dO=0), b"observation width", b"observation width"),
    "dO_129": (dict(sizes=[129, 8, None], dO=129), b"observation width", b"observation width"),
}
# entry point -> (error prefix, whether its network is a critic)
_NET_ENTRIES = {
    "policy_mlp": (b"policy_mlp: ", False), "value_mlp": (b"value_mlp: ", True),
    "vector_collect": (b"vector_collect: ", False),
    "vector_collect_ppo_actor": (b"vector_collect_ppo: ", False), "vector_collect_ppo_critic": (b"vector_collect_ppo critic: ", True),
    "ppo_grad_actor": (b"ppo_grad: ", False), "ppo_grad_critic": (b"ppo_grad: ", True),
    "ppo_update_actor": (b"ppo_update: ", False), "ppo_update_critic": (b"ppo_update: ", True),
}


def _call_with_net(entry, critic, sizes=(4, 8, None), act=1, x_dtype="F32", dO=4, null_w=None, in1=None):
    """The entry point's return code for a network of these sizes (None: the good last width, 1 for a critic, 2 for an actor)."""
    from rl_offline_simulation_amd import _lib as L
    from test_collect import _args
    lib, f = L.load(), 0x1000
    sizes = [(1 if critic else 2) if w is None else w for w in sizes]
    arr = _layers(sizes)
    if null_w is not None:
        arr[null_w].W = None
    if in1 is not None:
        setattr(arr[1], "in", in1)
    n, xd, lp = len(sizes) - 1, getattr(L, x_dtype), ctypes.cast(arr, ctypes.POINTER(L.MLPLayer))
    if entry in ("policy_mlp", "value_mlp"):
        return getattr(lib, "offsim_" + entry)(f, xd, 10, dO, None, 0, arr, n, act, 0.01, f, None)
    if entry.startswith("ppo_"):
        net = L.PPONet(n_layers=n, activation=act, layers_host=lp, slope=0.01)
        b = L.PPOBatchC(obs=f, x_dtype=xd, dO=dO, act=f, adv=f, logp=f, ret=f, valid=None, M=0)
        kind = L.PPO_CRITIC if critic else L.PPO_ACTOR
        if entry.startswith("ppo_grad"):
            return lib.offsim_ppo_grad(ctypes.byref(net), kind, ctypes.byref(b), 0.2, f, f, f, None)
        o = L.PPOAdam(m=f, v=f, t=f, lr=1e-3)
        return lib.offsim_ppo_update(ctypes.byref(net), kind, ctypes.byref(b), 0.2, 0.01, 3, ctypes.byref(o), f, f, f, None)
    t, ro, pol, st, out, _ = _args()  # a good MLP actor (4 -> 8 -> 2, the table's nA = 2)
    bad = dict(n_layers=n, layers_host=lp, activation=act, x_dtype=xd, dO=dO)
    if entry == "vector_collect_ppo_critic":
        val = L.CollectValue(form=L.VALUE_MLP, x_start=f, x_next=f, x_init=f, **bad)
    else:
        for k, v in bad.items():
            setattr(pol, k, v)
        good = _layers([4, 8, 1])
        val = L.CollectValue(form=L.VALUE_MLP, n_layers=2, layers_host=ctypes.cast(good, ctypes.POINTER(L.MLPLayer)), activation=1, x_dtype=xd, dO=4,
                             x_start=f, x_next=f, x_init=f)
    if entry == "vector_collect":
        return lib.offsim_vector_collect(ctypes.byref(t), ctypes.byref(ro), ctypes.byref(pol), L.PROB_F64, L.REJECT_DEFAULT, 0, 0, ctypes.byref(st),
                                         ctypes.byref(out), None)
    ppo = L.CollectPPOOut(value=f, logp=f, final_value=f)
    return lib.offsim_vector_collect_ppo(ctypes.byref(t), ctypes.byref(ro), ctypes.byref(pol), ctypes.byref(val), L.PROB_F64, L.REJECT_DEFAULT, 0, 0,
                                         ctypes.byref(st), ctypes.byref(out), ctypes.byref(ppo), None)


@pytest.mark.parametrize("entry", sorted(_NET_ENTRIES))
def test_every_entry_point_accepts_the_good_network(entry):
    from rl_offline_simulation_amd import _lib as L
    assert _call_with_net(entry, _NET_ENTRIES[entry][1]) == L.OK, L.load().offsim_last_error()


@pytest.mark.parametrize("entry,case", [(e, c) for e in sorted(_NET_ENTRIES) for c in sorted(_BAD_NETS)
                                        if _BAD_NETS[c][2 if _NET_ENTRIES[e][1] else 1] is not None])
def test_bad_network_refused_alike_by_every_entry_point(entry, case):
    from rl_offline_simulation_amd import _lib as L
    prefix, critic = _NET_ENTRIES[entry]
    kw, word_actor, word_critic = _BAD_NETS[case]
    word = word_critic if critic else word_actor
    rc = _call_with_net(entry, critic, **kw)
    err = L.load().offsim_last_error()
    assert rc == L.EINVAL, (rc, err)
    assert err.startswith(prefix), err
    assert word in err, err


def test_ppo_update_float_cap_and_work_size():
    from rl_offline_simulation_amd import _lib as L
    lib = L.load()
    b = L.PPOBatchC(obs=0x1000, x_dtype=L.F32, dO=4, act=0x1000, adv=0x1000, logp=0x1000, ret=0x1000, M=0)
    fits = _net([4, 120, 120, 1])  # 600 + 14520 + 121 = 15241 floats
    assert lib.offsim_ppo_grad(ctypes.byref(fits), L.PPO_CRITIC, ctypes.byref(b), 0.2, None, None, None, None) == L.OK
    assert lib.offsim_ppo_update_work_doubles(ctypes.byref(fits)) == L.ppo_update_work_doubles(15241)
    big = _net([4, 128, 124, 1])  # 640 + 15996 + 125 = 16761 > 16384
    assert lib.offsim_ppo_grad(ctypes.byref(big), L.PPO_CRITIC, ctypes.byref(b), 0.2, None, None, None, None) == L.EUNSUPPORTED
    assert b"MAX_FLOATS" in lib.offsim_last_error()
    o = L.PPOAdam(m=0x1000, v=0x1000, t=0x1000, lr=1e-3)
    assert lib.offsim_ppo_update(ctypes.byref(big), L.PPO_CRITIC, ctypes.byref(b), 0.2, 0.01, 3, ctypes.byref(o), None, None, None, None) == L.EUNSUPPORTED
    nobias = _net([4, 8, 2], bias=False)
    assert lib.offsim_ppo_update_work_doubles(ctypes.byref(nobias)) == L.ppo_update_work_doubles(48)
    assert lib.offsim_ppo_update_work_doubles(None) == L.EINVAL


def test_learner_python_surface():
    """What needs no device: the exports, PPOLearner's argument checks, and to_torch / state_dict round trips of the host copy."""
    import torch
    from rl_offline_simulation_amd.evaluators import MLPPolicy, MLPValue, PPOLearner, PPOUpdateInfo, ppo_grad  # noqa: F401
    assert PPOUpdateInfo._fields == ("LossPi", "LossV", "KL", "Entropy", "ClipFrac", "DeltaLossPi", "DeltaLossV", "StopIter")
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.ReLU(), torch.nn.Linear(8, 3), torch.nn.Identity())
    p = MLPPolicy.from_torch(net)
    back = p.to_torch()
    x = torch.randn(5, 4)
    assert torch.equal(back(x), net(x)) and set(p.state_dict()) == {"0.weight", "0.bias", "2.weight", "2.bias"}
    v = MLPValue.from_torch(torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.Tanh(), torch.nn.Linear(8, 1)))
    lrn = PPOLearner(p, v)
    assert (lrn.pi_lr, lrn.vf_lr, lrn.clip_ratio, lrn.train_pi_iters, lrn.train_v_iters, lrn.target_kl) == (3e-4, 1e-3, 0.2, 80, 80, 0.01)
    with pytest.raises(TypeError):
        PPOLearner(v, p)
    with pytest.raises(ValueError):
        PPOLearner(p, v, clip_ratio=1.5)
    with pytest.raises(ValueError):
        PPOLearner(p, MLPValue.from_torch(torch.nn.Sequential(torch.nn.Linear(5, 1))))
