"""CPU side of HOMEREncoder.train: the NumPy f64 restatement (tests/homer_train_host.py) pinned on fixtures recorded from the reference's
HOMEREncoder.train (tests/golden/homer_train/*.npz, made by tests/golden/make_golden_homer_train.py), and the C ABI of offsim_homer_grad /
offsim_homer_step (struct layouts, argument validation before any HIP call, the scratch size, the flat gradient's layout)."""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import homer_train_host as HH  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "homer_train", "*.npz")))
IDS = [os.path.basename(p)[:-4] for p in FIXTURES]


def close(got, want, tol=1e-4):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all(np.abs(got - want) <= tol * np.maximum(1.0, np.abs(want))))


def model_of(d, which="init"):
    return [d[f"{which}.{k}"] for k in HH.KEYS]


def steps_of(d):
    """the recorded steps in order: (is_val, idx_real, idx_impo, noise, loss, tau)"""
    off = d["step_off"]
    return [(bool(d["step_is_val"][s]), d["idx_real"][off[s]:off[s + 1]], d["idx_impo"][off[s]:off[s + 1]], d["noise"][off[s]:off[s + 1]],
             float(d["step_loss"][s]), float(d["step_tau"][s])) for s in range(len(off) - 1)]


def epochs_of(d):
    """per epoch: (train idx_real, idx_impo, noise, tau), (val idx_real, idx_impo, noise) -- the recorded batches concatenated, which
    train_epoch / eval_epoch cut again at batch_size"""
    st, out, s = steps_of(d), [], 0
    for _ in range(int(d["epochs"])):
        parts = []
        for want_val in (False, True):
            chunk = []
            while s < len(st) and st[s][0] == want_val:
                chunk.append(st[s])
                s += 1
            parts.append((np.concatenate([c[1] for c in chunk]), np.concatenate([c[2] for c in chunk]), np.concatenate([c[3] for c in chunk]), chunk[0][5]))
        out.append(tuple(parts))
    assert s == len(st)
    return out


def host_replay(d, dtype=np.float64):
    """the f64 host loop over the recorded indices and noise: (final model, per-step losses, per-epoch train / val losses, optimiser)"""
    model = [np.asarray(t, np.float64) for t in model_of(d)]
    opt = HH.Adam(HH.flatten(model).size, float(d["lr"]), float(d["weight_decay"]))
    tr, va = (d["train_x"], d["train_a"], d["train_x_next"]), (d["val_x"], d["val_a"], d["val_x_next"])
    B, losses, et, ev = int(d["batch_size"]), [], [], []
    for (ti, tj, tn, tau), (vi, vj, vn, _) in epochs_of(d):
        model, lt = HH.train_epoch(model, opt, tr, ti, tj, tn, B, tau)
        lv = HH.eval_epoch(model, va, vi, vj, vn, B)
        losses += list(lt) + list(lv)
        et.append(lt.mean())
        ev.append(lv.mean())
    return model, np.asarray(losses), np.asarray(et), np.asarray(ev), opt


def test_fixtures_present_and_cover_the_cases():
    assert {"homer_2_5_25_64", "homer_4_2_10_16_decay_wd"} <= set(IDS)
    biggest = max(os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")))
    d = np.load(os.path.join(ROOT, "tests", "golden", "homer_train", "homer_2_5_25_64.npz"))
    assert d["dims"].tolist() == [2, 5, 25, 64] and len(d["train_a"]) == 150 and len(d["val_a"]) == 70 and int(d["epochs"]) == 3
    assert np.diff(d["step_off"]).tolist() == [64, 64, 22, 64, 6] * 3
    d2 = np.load(os.path.join(ROOT, "tests", "golden", "homer_train", "homer_4_2_10_16_decay_wd.npz"))
    assert d2["dims"].tolist() == [4, 2, 10, 16] and int(d2["temperature_decay"]) == 1 and float(d2["weight_decay"]) == 0.01 and int(d2["epochs"]) == 2
    assert len(set(d2["step_tau"].tolist())) == 3  # 1.0 for the validation passes, exp(-0.005 epoch) for two epochs
    for p in FIXTURES:
        assert os.path.getsize(p) <= biggest


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_host_matches_the_reference_run(path, capsys):
    d = np.load(path)
    st = steps_of(d)
    loss, g, n = HH.loss_grad(model_of(d), d["train_x"], d["train_a"], d["train_x_next"], st[0][1], st[0][2], st[0][3], st[0][5])
    assert n == len(st[0][1]) and close(loss, st[0][4])
    scale = np.abs(d["grad0"]).max()
    assert g.size == HH.n_params(*d["dims"]) == d["grad0"].size and close(g / scale, d["grad0"] / scale)
    model, losses, et, ev, opt = host_replay(d)
    assert close(losses, d["step_loss"]) and close(et, d["epoch_train"]) and close(ev, d["epoch_val"])
    final = HH.flatten(model_of(d, "final"))
    err = float(np.abs(HH.flatten(model) - final).max())
    with capsys.disabled():
        print(f"\n  {os.path.basename(path)[:-4]}: reference f32 final weights against the f64 host: {err:.3e} (max|w| {np.abs(final).max():.3f})")
    assert close(HH.flatten(model), final)
    assert opt.t == int((~d["step_is_val"]).sum())


def test_host_gradient_is_torch_autograd_f64():
    """the restatement against torch autograd in f64 on a model of odd sizes, with duplicated indices, tau 0.5 and invalid records"""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(5)
    dO, nA, nZ, H, n_rows, M = 3, 3, 4, 5, 20, 17
    model = [rng.normal(size=s) * 0.7 for s in HH.shapes(dO, nA, nZ, H)]
    obs, nxt, act = rng.normal(size=(n_rows, dO)), rng.normal(size=(n_rows, dO)), rng.integers(0, nA, n_rows)
    act[3] = nA  # a row whose action is out of range
    i, j = rng.integers(0, n_rows, M), rng.integers(0, n_rows, M)
    i[0], j[1], i[2] = -1, n_rows, 3
    noise = -np.log(rng.exponential(size=(M, 4, nZ)))
    noise[:3] = np.nan
    ok = HH.valid_records(act, i, j, n_rows, nA)
    assert ok.sum() == M - 3 - int((i[3:] == 3).sum())
    loss, g, n = HH.loss_grad(model, obs, act, nxt, i, j, noise, 0.5)
    ps = [torch.tensor(t, dtype=torch.float64, requires_grad=True) for t in model]
    W1, b1, W2, b2, V1, c1, V2, c2 = ps
    enc = lambda x: F.linear(F.leaky_relu(F.linear(torch.tensor(x), W1, b1)), W2, b2)  # noqa: E731
    ii, jj, gn = i[ok], j[ok], torch.tensor(noise[ok])
    oh = F.one_hot(torch.tensor(act[ii]), nA).double()
    z = [F.softmax((e + gn[:, q]) / 0.5, -1) for q, e in enumerate((enc(obs[ii]), enc(nxt[ii]), enc(obs[ii]), enc(nxt[jj])))]
    cls = lambda a, b: F.log_softmax(F.linear(F.leaky_relu(F.linear(torch.cat([a, oh, b], 1), V1, c1)), V2, c2), 1)  # noqa: E731
    want = (-cls(z[0], z[1])[:, 1].mean() - cls(z[2], z[3])[:, 0].mean()) / 2
    want.backward()
    assert n == int(ok.sum()) and abs(loss - float(want.detach())) <= 1e-12
    assert np.allclose(g, torch.cat([p.grad.reshape(-1) for p in ps]).numpy(), rtol=1e-10, atol=1e-13)
    # the hard forward is F.gumbel_softmax(hard=True)'s value
    lh, gh, _ = HH.loss_grad(model, obs, act, nxt, i, j, noise, 1.0, hard=True)
    with torch.no_grad():
        zh = []
        for q, e in enumerate((enc(obs[ii]), enc(nxt[ii]), enc(obs[ii]), enc(nxt[jj]))):
            y = F.softmax(e + gn[:, q], -1)
            zh.append((torch.zeros_like(y).scatter_(-1, y.argmax(-1, keepdim=True), 1.0) - y) + y)
        wh = (-cls(zh[0], zh[1])[:, 1].mean() - cls(zh[2], zh[3])[:, 0].mean()) / 2
    assert gh is None and abs(lh - float(wh)) <= 1e-12


def test_host_clip_and_adam_are_torch():
    import torch
    rng = np.random.default_rng(0)
    p0 = rng.normal(size=9)
    p = torch.nn.Parameter(torch.tensor(p0, dtype=torch.float64))
    opt = torch.optim.Adam([p], lr=1e-2, weight_decay=0.01)
    mine, flat = HH.Adam(9, 1e-2, 0.01), p0.copy()
    for k in range(5):
        g = rng.normal(size=9) * 10.0 ** (1 - k)
        p.grad = torch.tensor(g)
        total = float(torch.nn.utils.clip_grad_norm_([p], 2.0))
        opt.step()
        t, coef = HH.clip_coef(g, 2.0)
        assert abs(t - total) <= 1e-12 * total and (coef < 1.0) == (total > 2.0)
        flat = mine.step(flat, g * coef)
        assert np.allclose(flat, p.detach().numpy(), rtol=1e-12, atol=1e-14)


# ---- the C ABI ----
def test_homer_struct_layout_and_work_size(tmp_path):
    from rl_offline_simulation_amd import _lib
    pairs = {"offsim_homer_net": _lib.HomerNet, "offsim_homer_batch": _lib.HomerBatch, "offsim_homer_adam": _lib.HomerAdam}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "offsim.h"', "int main(void) {"]
    for c_name, cls in pairs.items():
        lines.append(f'  printf("{c_name} %zu\\n", sizeof({c_name}));')
        for f, _ in cls._fields_:
            lines.append(f'  printf("{c_name}.{f} %zu\\n", offsetof({c_name}, {f}));')
    lines.append('  printf("work %lld\\n", (long long)OFFSIM_HOMER_WORK_DOUBLES(18420));')
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
    assert int(got["work"]) == _lib.homer_work_doubles(18420)
    src_h = open(os.path.join(ROOT, "include", "offsim.h")).read()
    for name, v in (("OFFSIM_HOMER_MAX_BLOCKS", _lib.HOMER_MAX_BLOCKS), ("OFFSIM_HOMER_MAX_FLOATS", _lib.HOMER_MAX_FLOATS)):
        assert f"#define {name} {v}" in src_h, name


def _net(dO=4, nA=2, nZ=10, H=16, slope=0.01, **ptrs):
    from rl_offline_simulation_amd import _lib as L
    f = 0x1000
    n = L.HomerNet(f, f, f, f, f, f, f, f, dO, nA, nZ, H, slope, 0)
    for k, v in ptrs.items():
        setattr(n, k, v)
    return n


def test_homer_validation_before_any_hip_call():
    from rl_offline_simulation_amd import _lib as L
    lib, f = L.load(), 0x1000

    def batch(M=0, **kw):
        b = L.HomerBatch(obs=f, next_obs=f, x_dtype=L.F32, act=f, n_rows=10, idx_real=f, idx_impo=f, noise=None, M=M)
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    def grad(n=None, b=None, tau=1.0, hard=0, g=f, stats=f, work=f, null_net=False):
        n, b = n or _net(), b or batch()
        return lib.offsim_homer_grad(None if null_net else ctypes.byref(n), ctypes.byref(b), tau, hard, g, stats, work, None)

    def step(n=None, b=None, tau=1.0, mx=40.0, opt=-1, stats=f, work=f):
        n, b = n or _net(), b or batch()
        o = L.HomerAdam(m=f, v=f, t=f, lr=1e-3, weight_decay=0.0) if opt == -1 else opt
        return lib.offsim_homer_step(ctypes.byref(n), ctypes.byref(b), tau, mx, ctypes.byref(o) if o is not None else None, stats, work, None)

    # M = 0 launches nothing (every pointer here is a fake address: a launch would fault)
    assert grad() == L.OK and step() == L.OK
    assert grad(null_net=True) == L.EINVAL and b"homer_grad" in lib.offsim_last_error()
    for bad in (0.0, -1.0, float("nan")):
        assert grad(tau=bad) == L.EINVAL and b"tau" in lib.offsim_last_error()
        assert step(tau=bad) == L.EINVAL and b"homer_step" in lib.offsim_last_error()
    assert grad(n=_net(nZ=1)) == L.EINVAL and b"nZ" in lib.offsim_last_error()
    assert grad(n=_net(nZ=2)) == L.OK
    assert grad(n=_net(slope=-0.1)) == L.EINVAL and b"slope" in lib.offsim_last_error()
    assert grad(n=_net(slope=0.0)) == L.OK
    for k in ("enc_W1", "enc_b1", "enc_W2", "enc_b2", "cls_W1", "cls_b1", "cls_W2", "cls_b2"):
        assert grad(n=_net(**{k: None})) == L.EINVAL and b"NULL" in lib.offsim_last_error(), k
    assert grad(n=_net(dO=0)) == L.EINVAL and grad(n=_net(dO=129)) == L.EINVAL and grad(n=_net(H=257)) == L.EINVAL
    assert grad(n=_net(nA=0)) == L.EINVAL and grad(n=_net(nA=17)) == L.EINVAL
    assert grad(b=batch(x_dtype=L.F64)) == L.EINVAL and b"x_dtype" in lib.offsim_last_error()
    assert grad(b=batch(M=-1)) == L.EINVAL
    for k in ("obs", "next_obs", "act", "idx_real", "idx_impo"):
        assert grad(b=batch(M=3, **{k: None})) == L.EINVAL and b"NULL" in lib.offsim_last_error(), k
    assert grad(b=batch(M=3), stats=None) == L.EINVAL and grad(b=batch(M=3), work=None) == L.EINVAL
    assert grad(hard=1) == L.EINVAL and b"forward only" in lib.offsim_last_error()
    assert grad(hard=1, g=None) == L.OK
    assert step(opt=None) == L.EINVAL and step(mx=-1.0) == L.EINVAL and step(mx=float("nan")) == L.EINVAL
    assert step(opt=L.HomerAdam(m=f, v=f, t=f, lr=-1.0, weight_decay=0.0)) == L.EINVAL
    assert step(opt=L.HomerAdam(m=f, v=f, t=f, lr=1e-3, weight_decay=-0.1)) == L.EINVAL
    assert step(b=batch(M=3), opt=L.HomerAdam(m=f, v=None, t=f, lr=1e-3, weight_decay=0.0)) == L.EINVAL and b"adam->m" in lib.offsim_last_error()
    assert step(b=batch(M=3), stats=None) == L.EINVAL and step(b=batch(M=3), work=None) == L.EINVAL


def test_homer_shapes_budget_and_work_doubles():
    from rl_offline_simulation_amd import _lib as L
    lib = L.load()
    b = L.HomerBatch(obs=0x1000, next_obs=0x1000, x_dtype=L.F32, act=0x1000, n_rows=10, idx_real=0x1000, idx_impo=0x1000, noise=None, M=0)
    for dO, H, nZ in ((2, 64, 25), (4, 16, 10), (128, 64, 50)):  # the encoder shapes of tests/golden/enc_mlp_*.npz, nA = 5
        n = _net(dO=dO, nA=5, nZ=nZ, H=H)
        assert lib.offsim_homer_grad(ctypes.byref(n), ctypes.byref(b), 1.0, 0, None, None, None, None) == L.OK, lib.offsim_last_error()
        P = L.homer_params(dO, 5, nZ, H)
        assert P == HH.n_params(dO, 5, nZ, H) and lib.offsim_homer_work_doubles(ctypes.byref(n)) == L.homer_work_doubles(P)
    assert L.homer_params(128, 5, 50, 64) == 18420 > L.COLLECT_MLP_MAX_FLOATS  # the collect cap does not apply here
    assert L.homer_work_doubles(18420) == 128 * 2 + 8 + 72 + 9210 + 128 * 9210
    big = _net(dO=128, nA=5, nZ=50, H=128)  # 36 340 parameters
    assert lib.offsim_homer_grad(ctypes.byref(big), ctypes.byref(b), 1.0, 0, None, None, None, None) == L.EUNSUPPORTED
    assert b"MAX_FLOATS" in lib.offsim_last_error()
    assert lib.offsim_homer_work_doubles(None) == L.EINVAL


def test_flat_gradient_layout_is_state_dict_order():
    dO, nA, nZ, H = 2, 5, 25, 64
    sizes = [int(np.prod(s)) for s in HH.shapes(dO, nA, nZ, H)]
    assert sizes == [H * dO, H, nZ * H, nZ, H * (2 * nZ + nA), H, 2 * H, 2] and sum(sizes) == HH.n_params(dO, nA, nZ, H)
    model = [np.full(s, float(k)) for k, s in enumerate(HH.shapes(dO, nA, nZ, H))]
    flat = HH.flatten(model)
    assert np.array_equal(flat, np.repeat(np.arange(8.0), sizes))
    back = HH.unflatten(flat, model)
    assert all(np.array_equal(x, y) for x, y in zip(back, model))


def test_state_dict_round_trips_through_the_reference_key_set():
    import torch
    from rl_offline_simulation_amd.encoders import HOMEREncoder
    from rl_offline_simulation_amd.encoders.homer import CLS_KEYS, ENC_KEYS
    assert ENC_KEYS + CLS_KEYS == HH.KEYS
    torch.manual_seed(3)
    enc = HOMEREncoder(3, 4, 6, 8)
    sd = enc.state_dict()
    assert list(sd) == list(ENC_KEYS) + ["action_emb.weight"] + list(CLS_KEYS)  # EncoderModel.state_dict()'s keys, in its order
    assert torch.equal(sd["action_emb.weight"], torch.eye(4))
    assert [tuple(sd[k].shape) for k in HH.KEYS] == HH.shapes(3, 4, 6, 8)
    # torch's default nn.Linear initialisation, the modules in the model's construction order under the same seed
    torch.manual_seed(3)
    lin = [torch.nn.Linear(3, 8), torch.nn.Linear(8, 6)]
    torch.nn.Embedding(4, 4)
    lin += [torch.nn.Linear(16, 8), torch.nn.Linear(8, 2)]
    for k, t in zip(HH.KEYS, [t for m in lin for t in (m.weight, m.bias)]):
        assert torch.equal(sd[k], t.detach()), k
    # a torch module with the reference's structure loads it strictly
    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.obs_encoder = torch.nn.Sequential(torch.nn.Linear(3, 8), torch.nn.LeakyReLU(), torch.nn.Linear(8, 6))
            self.action_emb = torch.nn.Embedding(4, 4)
            self.classifier = torch.nn.Sequential(torch.nn.Linear(16, 8), torch.nn.LeakyReLU(), torch.nn.Linear(8, 2))
    m = Model()
    m.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    with pytest.raises(ValueError):
        enc.encode_device(torch.zeros(2, 3))  # not trained, nothing loaded (homer.py:160-161)
