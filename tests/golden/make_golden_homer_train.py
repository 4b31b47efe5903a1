#!/usr/bin/env python3
"""Generate tests/golden/homer_train/*.npz by RUNNING THE REFERENCE's HOMEREncoder.train on CPU torch.

Run from the repo root:   python tests/golden/make_golden_homer_train.py
Needs /root/reference (read-only); nothing of it is copied -- the fixtures hold inputs, weights and the numbers the reference produced.

Loaded from the reference unmodified, by file path: offsim4rl/encoders/models.py (EncoderModel) and offsim4rl/encoders/homer.py
(HOMEREncoder).  tensorboard is not installed and the loop needs neither hdf5 files nor plots: stand-ins for offsim4rl.utils.tb_utils
(TensorboardWriter: log_scalar keeps the values), dataset_utils, vis_utils and offsim4rl.data are put into sys.modules first.

The reference's own train() runs with loss_fn= a recording wrapper around its own _calc_loss: the wrapper keeps torch.get_rng_state(),
calls _calc_loss, re-draws the four noise tensors from the kept state as -torch.empty(B, nZ).exponential_().log() in the order prev, curr
of the real call, prev, curr of the impostor call (asserting that the generator ends where _calc_loss left it, and that replaying the
noise through the reference's modules reproduces its loss bit for bit), and keeps the batch.  Rows of the tiny datasets are unique, so a
batch maps back to row indices.  The first training step's gradient is taken with torch.autograd.grad on the wrapper's loss.

The seed of a fixture is the first of range(50) for which, on the reference's numbers alone, (a) in every hard (validation) forward the two
largest perturbed logits of every record are at least 1e-4 apart, so an ulp cannot flip an argmax, and (b) no hidden pre-activation of
any forward is within 1e-6 of 0.
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "homer_train")
KEYS = ("obs_encoder.0.weight", "obs_encoder.0.bias", "obs_encoder.2.weight", "obs_encoder.2.bias",
        "classifier.0.weight", "classifier.0.bias", "classifier.2.weight", "classifier.2.bias")


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


class _Writer:
    def __init__(self, log_dir=None):
        self.scalars = {}

    def log_scalar(self, key, value):
        self.scalars.setdefault(key, []).append(float(value))


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def load_reference():
    for pkg in ("offsim4rl", "offsim4rl.encoders", "offsim4rl.utils"):
        _module(pkg).__path__ = []
    _module("offsim4rl.utils.tb_utils", TensorboardWriter=_Writer)
    _module("offsim4rl.utils.dataset_utils", load_h5_dataset=None)
    _module("offsim4rl.utils.vis_utils", plot_latent_state_color_map=None)
    _module("offsim4rl.data", SAS_Dataset=None)
    _load("offsim4rl.encoders.models", "offsim4rl/encoders/models.py")
    return _load("offsim4rl.encoders.homer", "offsim4rl/encoders/homer.py")


class Triples(torch.utils.data.Dataset):
    def __init__(self, x, a, xn):
        self.x, self.a, self.x_next = torch.from_numpy(x), torch.from_numpy(a), torch.from_numpy(xn)

    def __len__(self):
        return len(self.a)

    def __getitem__(self, i):
        return self.x[i], self.a[i], self.x_next[i]


def make_data(rng, n, dO, nA):
    """unique rows: x uniform, a random, x_next = x moved along a direction that depends on a, plus a little noise"""
    x = rng.random((n, dO)).astype(np.float32)
    a = rng.integers(0, nA, n).astype(np.int64)
    move = rng.normal(size=(nA, dO)).astype(np.float32)
    xn = (x + 0.1 * move[a] + 0.01 * rng.normal(size=(n, dO)).astype(np.float32)).astype(np.float32)
    assert len({r.tobytes() for r in x}) == n and len({r.tobytes() for r in xn}) == n
    return x, a, xn


class Recorder:
    def __init__(self, H, sets):
        self.H, self.sets, self.steps, self.grad0, self.ok = H, sets, [], None, True
        self.maps = {k: ({r.tobytes(): i for i, r in enumerate(x)}, {r.tobytes(): i for i, r in enumerate(xn)}) for k, (x, a, xn) in sets.items()}

    def __call__(self, model, batch, temperature=1.0, discretized=False):
        kind = "val" if discretized else "train"
        (obs, a, nxt_real), (_, _, nxt_impo) = batch
        B, nZ = len(obs), model.nZ
        before = torch.get_rng_state()
        loss, info = self.H._calc_loss(model, batch, temperature, discretized)
        after = torch.get_rng_state()
        torch.set_rng_state(before)
        noise = [-torch.empty(B, nZ).exponential_().log() for _ in range(4)]
        assert torch.equal(torch.get_rng_state(), after)
        by_x, by_xn = self.maps[kind]
        i = np.array([by_x[r.numpy().tobytes()] for r in obs], np.int32)
        j = np.array([by_xn[r.numpy().tobytes()] for r in nxt_impo], np.int32)
        x, act, xn = self.sets[kind]
        assert np.array_equal(xn[i], nxt_real.numpy()) and np.array_equal(act[i], a.numpy())
        # replay through the reference's modules: its loss bit for bit, and the margins of conditions (a) and (b)
        with torch.no_grad():
            pres, us = [], []
            for q, src in enumerate((obs, nxt_real, obs, nxt_impo)):
                pre = model.obs_encoder[0](src)
                pres.append(pre)
                us.append((model.obs_encoder[2](model.obs_encoder[1](pre)) + noise[q]) / temperature)
            zs = []
            for u in us:
                y = u.softmax(-1)
                zs.append((torch.zeros_like(y).scatter_(-1, y.max(-1, keepdim=True)[1], 1.0) - y) + y if discretized else y)
            lps = []
            for c in (0, 1):
                pre = model.classifier[0](torch.cat([zs[2 * c], model.action_emb(a).squeeze(), zs[2 * c + 1]], dim=1))
                pres.append(pre)
                lps.append(F.log_softmax(model.classifier[2](model.classifier[1](pre)), dim=1))
            replay = (F.nll_loss(lps[0], torch.ones(B, dtype=torch.long)) + F.nll_loss(lps[1], torch.zeros(B, dtype=torch.long))) / 2
        assert torch.equal(replay, loss.detach()), (float(replay), float(loss))
        if min(float(p.abs().min()) for p in pres) < 1e-6:
            self.ok = False
        if discretized:
            top = torch.stack([u.topk(2, -1)[0] for u in us])
            if float((top[..., 0] - top[..., 1]).min()) < 1e-4:
                self.ok = False
        if kind == "train" and self.grad0 is None:
            ps = [dict(model.named_parameters())[k] for k in KEYS]
            self.grad0 = torch.cat([g.reshape(-1) for g in torch.autograd.grad(loss, ps, retain_graph=True)]).numpy().copy()
        self.steps.append(dict(kind=kind, idx_real=i, idx_impo=j, noise=torch.stack(noise, 1).numpy(), loss=float(loss.detach()), tau=float(temperature)))
        return loss, info


def run(H, seed, dO, nA, nZ, hid, sets, epochs, batch, wd, decay):
    torch.manual_seed(seed)
    enc = H.HOMEREncoder(dO, nA, nZ, hid, log_dir=None)
    assert str(enc.device) == "cpu"
    init = {k: v.detach().numpy().copy() for k, v in enc.model.state_dict().items()}
    rec = Recorder(H.HOMEREncoder, sets)
    with tempfile.TemporaryDirectory() as tmp:
        enc.train(Triples(*sets["train"]), Triples(*sets["val"]), lr=1e-3, weight_decay=wd, loss_fn=rec, num_epochs=epochs, batch_size=batch,
                  temperature_decay=decay, model_dir=tmp)
    final = {k: v.detach().numpy().copy() for k, v in enc.model.state_dict().items()}
    sc = enc.tb_writer.scalars
    return rec, init, final, np.asarray(sc["train_loss"]), np.asarray(sc["val_loss"])


def make(H, name, data_seed, dO, nA, nZ, hid, n_train, n_val, epochs, batch, wd, decay):
    rng = np.random.default_rng(data_seed)
    sets = dict(train=make_data(rng, n_train, dO, nA), val=make_data(rng, n_val, dO, nA))
    for seed in range(50):
        rec, init, final, tl, vl = run(H, seed, dO, nA, nZ, hid, sets, epochs, batch, wd, decay)
        if rec.ok and len(tl) == epochs:
            break
    else:
        raise SystemExit(f"{name}: no seed in range(50) satisfies the margins")
    assert np.array_equal(init["action_emb.weight"], np.eye(nA, dtype=np.float32)) and np.array_equal(final["action_emb.weight"], np.eye(nA, dtype=np.float32))
    st = rec.steps
    off = np.concatenate([[0], np.cumsum([len(s["idx_real"]) for s in st])]).astype(np.int64)
    out = dict(dims=np.array([dO, nA, nZ, hid], np.int32), seed=seed, epochs=epochs, batch_size=batch, lr=1e-3, weight_decay=wd, temperature_decay=int(decay),
               step_is_val=np.array([s["kind"] == "val" for s in st]), step_off=off, step_loss=np.array([s["loss"] for s in st], np.float32),
               step_tau=np.array([s["tau"] for s in st]), idx_real=np.concatenate([s["idx_real"] for s in st]),
               idx_impo=np.concatenate([s["idx_impo"] for s in st]), noise=np.concatenate([s["noise"] for s in st]).astype(np.float32),
               grad0=rec.grad0, epoch_train=tl, epoch_val=vl)
    for k, (x, a, xn) in sets.items():
        out.update({f"{k}_x": x, f"{k}_a": a.astype(np.int32), f"{k}_x_next": xn})
    for k in KEYS:
        out["init." + k], out["final." + k] = init[k], final[k]
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    biggest = max(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(os.path.join(ROOT, "tests", "golden")) for f in fs
                  if "homer_train" not in d and not f.endswith(".py"))
    assert os.path.getsize(path) <= biggest
    print(f"{name}: seed {seed}, {len(st)} steps, batches {np.diff(off).tolist()}, train {tl.tolist()}, val {vl.tolist()}, {os.path.getsize(path)} bytes")


def main():
    H = load_reference()
    make(H, "homer_2_5_25_64", 1, 2, 5, 25, 64, 150, 70, 3, 64, 0.0, False)
    make(H, "homer_4_2_10_16_decay_wd", 2, 4, 2, 10, 16, 90, 40, 2, 32, 0.01, True)


if __name__ == "__main__":
    main()
