"""HOMEREncoder.loss_grad / train_epoch / eval_epoch / train (offsim_homer_grad, offsim_homer_step) on the device against the NumPy f64
restatement (tests/homer_train_host.py), with DESIGN section 13's bound: torch's f32 autograd on the CPU is the f32 reference, the f64
host is the truth, and the device's error must stay within 4 x the f32 reference's own error, floored at 4 f32 ulps of the max norm.
The fixtures (tests/golden/homer_train/*.npz) carry the reference's own run: its first gradient, per-step losses and final weights are the
f32 reference there."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import homer_train_host as HH  # noqa: E402
from test_homer_train_host import FIXTURES, IDS, epochs_of, host_replay, model_of, steps_of  # noqa: E402

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def gpu():
    from rl_offline_simulation_amd import _lib
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    _lib.load()
    return torch.device("cuda", 0)


def bound(want64, ref32):
    """4 x the f32 reference's own error against the f64 value, floored at 4 f32 ulps of the max norm"""
    want64 = np.asarray(want64, np.float64)
    return max(4.0 * float(np.abs(np.asarray(ref32, np.float64) - want64).max()), 4.0 * ULP * max(float(np.abs(want64).max()), 1e-30))


def encoder(model, dims):
    from rl_offline_simulation_amd.encoders import HOMEREncoder
    dO, nA, nZ, H = (int(v) for v in dims)
    return HOMEREncoder(dO, nA, nZ, H, state_dict={k: np.asarray(t, np.float32) for k, t in zip(HH.KEYS, model)})


def flat_dev(enc):
    return torch.cat([t.reshape(-1) for t in enc._params()]).cpu().numpy().astype(np.float64)


def torch_ref(model, obs, act, nxt, i, j, noise, tau, hard=False, dtype=torch.float32, slope=HH.SLOPE):
    """torch on the CPU in `dtype`: (loss, flat autograd gradient or None) over the valid records; slope: leaky_relu's"""
    ps = [torch.tensor(np.asarray(t), dtype=dtype, requires_grad=not hard) for t in model]
    W1, b1, W2, b2, V1, c1, V2, c2 = ps
    nZ, nA = W2.shape[0], V1.shape[1] - 2 * W2.shape[0]
    ok = HH.valid_records(act, i, j, len(obs), nA)
    i, j = np.asarray(i)[ok].astype(np.int64), np.asarray(j)[ok].astype(np.int64)
    g = torch.zeros((len(i), 4, nZ), dtype=dtype) if noise is None else torch.tensor(np.asarray(noise)[ok], dtype=dtype)
    x, xn = torch.tensor(np.asarray(obs, np.float64), dtype=dtype), torch.tensor(np.asarray(nxt, np.float64), dtype=dtype)
    enc = lambda v: F.linear(F.leaky_relu(F.linear(v, W1, b1), slope), W2, b2)  # noqa: E731
    oh = F.one_hot(torch.tensor(np.asarray(act)[i].astype(np.int64)), nA).to(dtype)
    zs = []
    for q, e in enumerate((enc(x[i]), enc(xn[i]), enc(x[i]), enc(xn[j]))):
        y = F.softmax((e + g[:, q]) / tau, -1)
        zs.append((torch.zeros_like(y).scatter_(-1, y.max(-1, keepdim=True)[1], 1.0) - y) + y if hard else y)
    cls = lambda a, b: F.log_softmax(F.linear(F.leaky_relu(F.linear(torch.cat([a, oh, b], 1), V1, c1), slope), V2, c2), 1)  # noqa: E731
    n = len(i)
    loss = (F.nll_loss(cls(zs[0], zs[1]), torch.ones(n, dtype=torch.long)) + F.nll_loss(cls(zs[2], zs[3]), torch.zeros(n, dtype=torch.long))) / 2
    if hard:
        return float(loss), None
    loss.backward()
    return float(loss.detach()), torch.cat([p.grad.reshape(-1) for p in ps]).double().numpy()


def make_case(dims, M, seed, half=False, n_rows=40, scale=0.5, noise=True):
    """a random model and batch: duplicated indices, idx_impo == idx_real for a third of the records"""
    dO, nA, nZ, H = dims
    rng = np.random.default_rng(seed)
    model = [(rng.normal(size=s) * scale).astype(np.float32) for s in HH.shapes(dO, nA, nZ, H)]
    xd = np.float16 if half else np.float32
    obs, nxt = rng.normal(size=(n_rows, dO)).astype(xd), rng.normal(size=(n_rows, dO)).astype(xd)
    act = rng.integers(0, nA, n_rows).astype(np.int32)
    i, j = rng.integers(0, n_rows, M).astype(np.int32), rng.integers(0, n_rows, M).astype(np.int32)
    j[::3] = i[::3]
    g = (-np.log(rng.exponential(size=(M, 4, nZ)))).astype(np.float32) if noise else None
    return model, obs, act, nxt, i, j, g


def check_pass(gpu, dims, model, obs, act, nxt, i, j, g, tau, tag=""):
    enc = encoder(model, dims)
    loss, grad = enc.loss_grad(torch.from_numpy(obs), act, torch.from_numpy(nxt), i, j, g, tau)
    l64, g64, n = HH.loss_grad(model, obs, act, nxt, i, j, g, tau)
    l32, g32 = torch_ref(model, obs, act, nxt, i, j, g, tau)
    assert int(enc.last_n) == n
    e_g, b_g = float(np.abs(grad.cpu().numpy().astype(np.float64) - g64).max()), bound(g64, g32)
    e_l, b_l = abs(float(loss) - l64), max(4.0 * abs(l32 - l64), 4.0 * ULP * max(1.0, abs(l64)))
    print(f"{tag} dims {dims} M {len(i)} tau {tau}: grad err {e_g:.3e} bound {b_g:.3e} ({e_g / b_g:.2f})  loss err {e_l:.3e} bound {b_l:.3e}")
    assert e_g <= b_g and e_l <= b_l
    return e_g / b_g


# ---- the fixtures: the reference's own run ----
@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_fixture_first_gradient_and_replayed_training(gpu, path):
    d = np.load(path)
    st = steps_of(d)
    tr_np, va_np = (d["train_x"], d["train_a"], d["train_x_next"]), (d["val_x"], d["val_a"], d["val_x_next"])
    enc = encoder(model_of(d), d["dims"])
    loss, grad = enc.loss_grad(*tr_np, st[0][1], st[0][2], st[0][3], st[0][5])
    l64, g64, _ = HH.loss_grad(model_of(d), *tr_np, st[0][1], st[0][2], st[0][3], st[0][5])
    e, b = float(np.abs(grad.cpu().numpy() - g64).max()), bound(g64, d["grad0"])
    print(f"first gradient err {e:.3e} bound {b:.3e} ({e / b:.2f})")
    assert e <= b
    # the whole run replayed: per-step losses, per-epoch means and final weights against the f64 host, the reference's f32 error the scale
    h_model, h_losses, h_et, h_ev, h_opt = host_replay(d)
    enc.lr, enc.weight_decay, enc.max_grad_norm = float(d["lr"]), float(d["weight_decay"]), 40.0
    enc.reset_optimizer()
    tr, va = enc.upload(tr_np), enc.upload(va_np)
    B, got, et, ev = int(d["batch_size"]), [], [], []
    for (ti, tj, tn, tau), (vi, vj, vn, _) in epochs_of(d):
        lt = enc.train_epoch(tr, ti, tj, B, tau, noise=torch.from_numpy(tn))
        lv = enc.eval_epoch(va, vi, vj, B, noise=torch.from_numpy(vn))
        got += [lt, lv]
        et.append(lt.mean())
        ev.append(lv.mean())
    got = torch.cat(got).cpu().numpy()
    for name, x, host, ref in (("step losses", got, h_losses, d["step_loss"]), ("epoch train", torch.stack(et).cpu().numpy(), h_et, d["epoch_train"]),
                               ("epoch val", torch.stack(ev).cpu().numpy(), h_ev, d["epoch_val"])):
        e, b = float(np.abs(x - host).max()), max(4.0 * float(np.abs(ref - host).max()), 4.0 * ULP)
        print(f"{name}: err {e:.3e} bound {b:.3e} ({e / b:.2f})")
        assert e <= b, name
    final64 = HH.flatten(h_model)
    e, b = float(np.abs(flat_dev(enc) - final64).max()), bound(final64, HH.flatten(model_of(d, "final")))
    print(f"final weights: err {e:.3e} bound {b:.3e} ({e / b:.2f})")
    assert e <= b
    assert int(enc.adam_state()[2]) == h_opt.t


# ---- one pass against f64 ----
SHAPES = [(2, 5, 25, 64), (4, 2, 10, 16), (3, 3, 2, 5), (128, 5, 50, 64)]


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("dims", SHAPES, ids=["2_5_25_64", "4_2_10_16", "3_3_2_5", "128_5_50_64"])
def test_loss_grad_matches_f64(gpu, dims, half):
    for k, M in enumerate((1, 31, 32, 33, 86)):
        tau, noise = ((1.0, True), (0.5, False), (0.5, True), (1.0, False), (1.0, True))[k]
        model, obs, act, nxt, i, j, g = make_case(dims, M, 100 + k, half, noise=noise)
        check_pass(gpu, dims, model, obs, act, nxt, i, j, g, tau, "f16" if half else "f32")


def test_invalid_records_are_excluded(gpu):
    dims = (4, 2, 10, 16)
    model, obs, act, nxt, i, j, g = make_case(dims, 50, 7)
    act[5] = 2       # an action outside [0, nA): every record whose idx_real is 5 is invalid
    i[3], j[4], i[9], j[10], i[11] = -1, 40, 2 ** 31 - 1, -(2 ** 31), 5
    bad = ~HH.valid_records(act, i, j, 40, 2)
    assert bad.sum() >= 5
    g[bad] = np.nan  # their noise is never read
    check_pass(gpu, dims, model, obs, act, nxt, i, j, g, 1.0, "invalid")
    # the compacted batch is the same sum in another order: both lie within the bound of the f64 gradient, so within twice it of each other
    enc = encoder(model, dims)
    keep = ~bad
    la, ga = enc.loss_grad(obs, act, nxt, i, j, g)
    lb, gb = enc.loss_grad(obs, act, nxt, i[keep], j[keep], g[keep])
    _, g64, _ = HH.loss_grad(model, obs, act, nxt, i, j, g)
    b = bound(g64, torch_ref(model, obs, act, nxt, i, j, g, 1.0)[1])
    assert int(enc.last_n) == keep.sum() and abs(float(la) - float(lb)) <= 4.0 * ULP
    assert float((ga - gb).abs().max()) <= 2.0 * b


def test_logits_in_the_hundreds(gpu):
    dims = (2, 5, 25, 64)
    model, obs, act, nxt, i, j, g = make_case(dims, 33, 11)
    model[2], model[3] = model[2] * 60.0, model[3] * 200.0  # the encoder's last layer: logits of a few hundred
    e = HH._mlp(obs.astype(np.float64), *[np.asarray(t, np.float64) for t in model[:4]], HH.SLOPE)[0]
    assert np.abs(e).max() > 300.0
    check_pass(gpu, dims, model, obs, act, nxt, i, j, g, 1.0, "hundreds")


def test_more_than_one_tile_per_workgroup(gpu):
    """4500 patterned records on the smallest net: 141 tiles of 32 on 128 workgroups, a short last tile"""
    from rl_offline_simulation_amd import _lib as L
    dims, M, n_rows = (3, 3, 2, 5), 4500, 97
    assert M > 32 * L.HOMER_MAX_BLOCKS and M % 32 != 0
    model, obs, act, nxt, _, _, _ = make_case(dims, 1, 13, n_rows=n_rows)
    m = np.arange(M)
    i, j = (m * 7 % n_rows).astype(np.int32), (m * 13 % n_rows).astype(np.int32)
    g = (np.sin(m[:, None, None] * 0.37 + np.arange(4)[None, :, None] + np.arange(2)[None, None, :] * 2.0)).astype(np.float32)
    check_pass(gpu, dims, model, obs, act, nxt, i, j, g, 1.0, "tiles")


@pytest.mark.parametrize("dims", [(2, 5, 25, 64), (3, 3, 2, 5)], ids=["2_5_25_64", "3_3_2_5"])
def test_hard_forward_matches_f64(gpu, dims):
    model, obs, act, nxt, i, j, g = make_case(dims, 86, 21)
    info = {}
    HH.loss_grad(model, obs, act, nxt, i, j, g, 1.0, hard=True, info=info)
    top = np.stack([np.sort(u, 1)[:, -2:] for u in info["u"]])
    keep = ((top[..., 1] - top[..., 0]) >= 1e-4).all(0)  # an ulp cannot flip an argmax
    assert keep.sum() >= 80
    i, j, g = i[keep], j[keep], g[keep]
    enc = encoder(model, dims)
    loss, grad = enc.loss_grad(obs, act, nxt, i, j, g, hard=True)
    l64, _, n = HH.loss_grad(model, obs, act, nxt, i, j, g, 1.0, hard=True)
    l32, _ = torch_ref(model, obs, act, nxt, i, j, g, 1.0, hard=True)
    e, b = abs(float(loss) - l64), max(4.0 * abs(l32 - l64), 4.0 * ULP * max(1.0, abs(l64)))
    print(f"hard dims {dims}: loss err {e:.3e} bound {b:.3e}")
    assert grad is None and int(enc.last_n) == n and e <= b


# ---- the step ----
def _one_step(enc, data, i, j, g, tau=1.0):
    enc.train_epoch(data, i, j, len(i), tau, noise=torch.from_numpy(g))
    return enc.last_stats[0].cpu().numpy()


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("clip", ["active", "inactive"])
def test_one_step_in_closed_form_from_the_device_gradient(gpu, wd, clip):
    dims = (4, 2, 10, 16)
    model, obs, act, nxt, i, j, g = make_case(dims, 50, 31, scale=1.0)
    _, g64, _ = HH.loss_grad(model, obs, act, nxt, i, j, g)
    host_norm = float(np.sqrt((g64 ** 2).sum()))
    max_norm = 0.5 * host_norm if clip == "active" else 40.0
    assert (host_norm > max_norm) == (clip == "active")
    enc = encoder(model, dims)
    loss, grad = enc.loss_grad(obs, act, nxt, i, j, g)
    gd = grad.cpu().numpy().astype(np.float64)
    enc.lr, enc.weight_decay, enc.max_grad_norm = 1e-3, wd, max_norm
    enc.reset_optimizer()
    p0 = flat_dev(enc)
    stats = _one_step(enc, enc.upload((obs, act, nxt)), i, j, g)
    total, coef = HH.clip_coef(gd, max_norm)
    assert stats[0] == 50 and stats[1] == float(loss) and abs(stats[2] - total) <= 1e-12 * total
    # against the host's norm: | |a| - |b| | <= |a - b|_2 <= sqrt(P) x the gradient's bound
    assert abs(stats[2] - host_norm) <= np.sqrt(gd.size) * bound(g64, torch_ref(model, obs, act, nxt, i, j, g, 1.0)[1])
    gg = gd * coef + wd * p0
    m = (0.1 * gg).astype(np.float32).astype(np.float64)
    v = (0.001 * gg * gg).astype(np.float32).astype(np.float64)
    want = p0 - (1e-3 / (1 - 0.9)) * m / (np.sqrt(v) / np.sqrt(1 - 0.999) + 1e-8)
    dm, dv, dt = enc.adam_state()
    assert int(dt) == 1
    tiny = 2.0 ** -126
    assert np.all(np.abs(dm.cpu().numpy() - m) <= 2 * ULP * np.abs(m) + tiny) and np.all(np.abs(dv.cpu().numpy() - v) <= 2 * ULP * np.abs(v) + tiny)
    assert np.all(np.abs(flat_dev(enc) - want) <= ULP * np.abs(want) + 1e-6 * 1e-3)


def test_three_steps_against_the_host_optimiser(gpu):
    """weights, m and v after t = 1, 2, 3 against the f64 host, within 4 x the error of an f32 torch loop (autograd, clip_grad_norm_,
    optim.Adam with weight decay) fed the same indices and noise"""
    dims, wd, lr = (4, 2, 10, 16), 0.01, 1e-3
    model, obs, act, nxt, _, _, _ = make_case(dims, 1, 41)
    batches = [make_case(dims, 40, 50 + k)[4:] for k in range(3)]
    enc = encoder(model, dims)
    enc.lr, enc.weight_decay, enc.max_grad_norm = lr, wd, 40.0
    enc.reset_optimizer()
    data = enc.upload((obs, act, nxt))
    h_model, h_opt = [np.asarray(t, np.float64) for t in model], HH.Adam(HH.n_params(*dims), lr, wd)
    ps = [torch.nn.Parameter(torch.tensor(t)) for t in model]
    t_opt = torch.optim.Adam(ps, lr=lr, weight_decay=wd)
    for k, (i, j, g) in enumerate(batches):
        _one_step(enc, data, i, j, g)
        h_model, _, _, _ = HH.step(h_model, h_opt, (obs, act, nxt), i, j, g, 1.0)
        _, g32 = torch_ref([p.detach().numpy() for p in ps], obs, act, nxt, i, j, g, 1.0)
        t_opt.zero_grad()
        o = 0
        for p in ps:
            p.grad = torch.tensor(g32[o:o + p.numel()], dtype=torch.float32).reshape(p.shape)
            o += p.numel()
        torch.nn.utils.clip_grad_norm_(ps, 40.0)
        t_opt.step()
        dm, dv, dt = enc.adam_state()
        assert int(dt) == k + 1 == h_opt.t
        tm = torch.cat([t_opt.state[p]["exp_avg"].reshape(-1) for p in ps]).numpy()
        tv = torch.cat([t_opt.state[p]["exp_avg_sq"].reshape(-1) for p in ps]).numpy()
        tw = torch.cat([p.detach().reshape(-1) for p in ps]).numpy()
        for name, got, host, ref in (("w", flat_dev(enc), HH.flatten(h_model), tw), ("m", dm.cpu().numpy(), h_opt.m, tm), ("v", dv.cpu().numpy(), h_opt.v, tv)):
            e, b = float(np.abs(got - host).max()), bound(host, ref)
            print(f"t {k + 1} {name}: err {e:.3e} bound {b:.3e} ({e / b:.2f})")
            assert e <= b, (k, name)


def test_two_train_epochs_give_the_same_bits(gpu):
    dims = (2, 5, 25, 64)
    model, obs, act, nxt, i, j, g = make_case(dims, 150, 61)
    outs = []
    for _ in range(2):
        enc = encoder(model, dims)
        enc.weight_decay = 0.01
        enc.reset_optimizer()
        losses = enc.train_epoch(enc.upload((obs, act, nxt)), i, j, 64, 0.7, noise=torch.from_numpy(g))
        outs.append([losses.clone()] + [t.clone() for t in enc._params()] + [t.clone() for t in enc.adam_state()])
    assert len(outs[0][0]) == 3
    for x, y in zip(*outs):
        assert torch.equal(x, y)


def test_empty_and_all_invalid_batches_change_nothing(gpu):
    dims = (4, 2, 10, 16)
    model, obs, act, nxt, i, j, g = make_case(dims, 20, 71)
    enc = encoder(model, dims)
    enc.reset_optimizer()
    data = enc.upload((obs, act, nxt))
    before = flat_dev(enc)
    empty = np.zeros(0, np.int32)
    assert enc.train_epoch(data, empty, empty, 64, 1.0).numel() == 0
    stats = _one_step(enc, data, np.full(20, -1, np.int32), j, g)
    assert stats[0] == 0 and stats[1] == 0 and np.array_equal(flat_dev(enc), before)
    assert int(enc.adam_state()[2]) == 0 and not bool(enc.adam_state()[0].any()) and not bool(enc.adam_state()[1].any())
    loss, grad = enc.loss_grad(obs, act, nxt, np.full(20, 40, np.int32), j, g)
    assert int(enc.last_n) == 0 and float(loss) == 0.0 and not bool(grad.any())
    # the next call is unaffected
    check_pass(gpu, dims, model, obs, act, nxt, i, j, g, 1.0, "after empty")
    stats = _one_step(enc, data, i, j, g)
    assert stats[0] == 20 and int(enc.adam_state()[2]) == 1 and not np.array_equal(flat_dev(enc), before)


# ---- train() end to end ----
def _grid_walk(n=200, seed=0):
    """a 1-d grid walk: x in {0, .., 9} / 10, a in {left, right}, x_next = the neighbour (clipped)"""
    rng = np.random.default_rng(seed)
    pos, a = rng.integers(0, 10, n), rng.integers(0, 2, n)
    nxt = np.clip(pos + 2 * a - 1, 0, 9)
    return (pos[:, None] / 10.0).astype(np.float32), a.astype(np.int32), (nxt[:, None] / 10.0).astype(np.float32)


def _stop_rule(val_losses, patience_threshold):
    """the reference's early-stopping rule on a list of validation losses: (epochs run, best epoch, best val loss)"""
    best, best_epoch, patience = 0.69, -1, 0
    for e, v in enumerate(val_losses, 1):
        if v < best:
            best, best_epoch, patience = v, e, 0
        else:
            patience += 1
            if v > 0.8 or patience == patience_threshold:
                return e, best_epoch, best
    return len(val_losses), best_epoch, best


def test_train_end_to_end(gpu, tmp_path):
    from rl_offline_simulation_amd.encoders import HOMEREncoder
    x, a, xn = _grid_walk()
    tr, va = (x[:160], a[:160], xn[:160]), (x[160:], a[160:], xn[160:])
    torch.manual_seed(1)
    enc = HOMEREncoder(1, 2, 4, 16)
    init = enc.state_dict()
    E = 4
    res = enc.train(tr, va, lr=1e-2, num_epochs=E, batch_size=64, patience_threshold=50, model_dir=str(tmp_path), seed=0)
    assert len(res.train_losses) == len(res.val_losses) == res.epochs_run
    assert (res.epochs_run, res.best_epoch, res.best_val_loss) == _stop_rule(res.val_losses, 50) and res.epochs_run <= E
    assert np.isfinite(res.train_losses).all() and np.isfinite(res.val_losses).all()
    z = enc.encode(x)
    assert z.shape == (200,) and z.min() >= 0 and z.max() < 4
    saved = torch.load(os.path.join(str(tmp_path), "encoder_model.pt"))
    best = enc.best_state_dict()
    assert list(saved) == list(best) and all(torch.equal(saved[k], best[k]) for k in best)
    # the same run replayed epoch by epoch (the draws in train()'s order): the weights after the best epoch are best_state_dict()
    enc2 = HOMEREncoder(1, 2, 4, 16, state_dict=init)
    enc2.lr = 1e-2
    enc2.reset_optimizer()
    torch.manual_seed(0)
    d_tr, d_va = enc2.upload(tr), enc2.upload(va)
    perm = lambda n: torch.randperm(n, device=gpu).to(torch.int32)  # noqa: E731
    want = init
    for epoch in range(1, res.epochs_run + 1):
        lt = enc2.train_epoch(d_tr, perm(160), perm(160), 64, 1.0)
        lv = enc2.eval_epoch(d_va, perm(40), perm(40), 64)
        assert float(lt.mean()) == res.train_losses[epoch - 1] and float(lv.mean()) == res.val_losses[epoch - 1]
        if epoch == res.best_epoch:
            want = enc2.state_dict()
    assert all(torch.equal(best[k], want[k]) for k in best)
    last = enc2.state_dict()
    assert all(torch.equal(enc.state_dict()[k], last[k]) for k in last)  # encode runs the last weights
    # best_state_dict() in a fresh encoder: the evaluation loss of the encoder it came from, on the same indices and noise
    vi, vj = perm(40), perm(40)
    vn = -torch.empty((40, 4, 4), device=gpu).exponential_().log()
    enc3, enc4 = HOMEREncoder(1, 2, 4, 16, state_dict=best), HOMEREncoder(1, 2, 4, 16, state_dict=want)
    assert torch.equal(enc3.eval_epoch(d_va, vi, vj, 64, noise=vn), enc4.eval_epoch(d_va, vi, vj, 64, noise=vn))


def test_train_stops_at_the_patience_limit(gpu):
    from rl_offline_simulation_amd.encoders import HOMEREncoder
    x, a, xn = _grid_walk()
    torch.manual_seed(1)
    enc = HOMEREncoder(1, 2, 4, 16)
    before = enc.state_dict()
    res = enc.train((x[:160], a[:160], xn[:160]), (x[160:], a[160:], xn[160:]), lr=0.0, num_epochs=30, patience_threshold=2, seed=0)
    run, best_epoch, best = _stop_rule(res.val_losses, 2)
    assert res.epochs_run == run == len(res.val_losses) < 30 and (res.best_epoch, res.best_val_loss) == (best_epoch, best)
    # exactly two epochs without improvement ended it
    assert all(v >= min([0.69] + res.val_losses[:-2]) for v in res.val_losses[-2:])
    after = enc.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)  # lr = 0: the weights never move
