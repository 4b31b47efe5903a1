"""HOMERPopulation (offsim_homer_grad_pop, offsim_homer_step_pop) on the device: every learner against a HOMEREncoder fed that learner's own
indices and noise, bit for bit -- no tolerance anywhere.  The population is the single path's kernels with the learner on gridDim.y, and per
learner every order (tiles of a workgroup, partials, reduction, norm tree, Adam) is the single call's on the same M; a differing bit means
one of those orders differs.  The cases and the f64-checked single path come from tests/test_gpu_homer_train.py."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import homer_train_host as HH  # noqa: E402
import test_gpu_homer_train as T  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from rl_offline_simulation_amd import _lib
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    _lib.load()
    return torch.device("cuda", 0)


def population(models, dims):
    from rl_offline_simulation_amd.encoders import HOMERPopulation
    return HOMERPopulation(*dims, state_dicts=[{k: torch.from_numpy(np.asarray(t, np.float32)) for k, t in zip(HH.KEYS, m)} for m in models])


def make_learners(dims, n_learners, M, seed, half=False, n_rows=40, pad=(3, 4), scale=0.5):
    """n_learners models and record sets over ONE dataset (learner 0's), the records as column slices [:, pad[0] : pad[0] + M] of arrays
    pad[0] + M + pad[1] wide whose other columns hold indices that must not be read (out of range) and NaN noise"""
    cases = [T.make_case(dims, M, seed + 17 * l, half, n_rows=n_rows, scale=scale) for l in range(n_learners)]
    models, (obs, act, nxt) = [c[0] for c in cases], cases[0][1:4]
    W, nZ = pad[0] + M + pad[1], dims[2]
    i = np.full((n_learners, W), -7, np.int32)
    j = np.full((n_learners, W), 2 ** 30, np.int32)
    g = np.full((n_learners, W, 4, nZ), np.nan, np.float32)
    for l, c in enumerate(cases):
        i[l, pad[0]:pad[0] + M], j[l, pad[0]:pad[0] + M], g[l, pad[0]:pad[0] + M] = c[4], c[5], c[6]
    return models, obs, act, nxt, i, j, g, slice(pad[0], pad[0] + M)


def on(gpu, *arrays):
    return [torch.from_numpy(a).to(gpu) for a in arrays]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def check_pass(gpu, dims, models, obs, act, nxt, i, j, g, cols, tau=1.0, hard=False, noise=True):
    """one pass of the population over the column slice against the single encoder per learner: loss, n and grad [L, P]"""
    pop = population(models, dims)
    di, dj, dg = on(gpu, i, j, g)
    noise_arg = dg[:, cols] if noise else None
    if len(models) > 1:  # the slice goes to the kernels as it is: the learner stride is the arrays' width
        assert pop._records(di[:, cols], dj[:, cols], noise_arg, gpu)[4] == i.shape[1] > cols.stop - cols.start
    loss, grad = pop.loss_grad(obs, act, nxt, di[:, cols], dj[:, cols], noise_arg, tau, hard)
    assert loss.shape == pop.last_n.shape == (len(models),) and (grad is None if hard else grad.shape == (len(models), pop.n_params))
    for l, model in enumerate(models):
        enc = T.encoder(model, dims)
        l1, g1 = enc.loss_grad(obs, act, nxt, i[l, cols], j[l, cols], g[l, cols] if noise else None, tau, hard)
        assert same(loss[l], l1) and same(pop.last_n[l], enc.last_n), (l, float(loss[l]), float(l1))
        assert (g1 is None and grad is None) if hard else same(grad[l], g1), l
    return pop, loss, grad


# ---- 1. one pass ----
PASS_SHAPES = [(3, 3, 2, 5), (2, 5, 25, 64), (128, 5, 50, 64)]


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("dims", PASS_SHAPES, ids=["3_3_2_5", "2_5_25_64", "128_5_50_64"])
def test_one_pass_equals_the_single_encoder(gpu, dims, half):
    for k, M in enumerate((1, 33, 86)):
        tau, noise = ((1.0, True), (0.5, False), (0.7, True))[k]
        models, obs, act, nxt, i, j, g, cols = make_learners(dims, 3, M, 200 + k, half)
        _, loss, _ = check_pass(gpu, dims, models, obs, act, nxt, i, j, g, cols, tau, noise=noise)
        assert len({float(x) for x in loss}) == 3  # three different learners


def test_invalid_records_in_one_learner_only(gpu):
    dims = (2, 5, 25, 64)
    models, obs, act, nxt, i, j, g, cols = make_learners(dims, 3, 33, 300)
    act = act.copy()
    act[5] = 5                                # an action outside [0, nA): a record whose idx_real is 5 is invalid ...
    for l in (0, 2):
        i[l][i[l] == 5] = 6                   # ... and only learner 1 has such records
    i[1, cols][:2], j[1, cols][4] = 5, 40
    i[1, cols][7], j[1, cols][8], i[1, cols][9] = -1, -(2 ** 31), 2 ** 31 - 1
    bad = ~HH.valid_records(act, i[1, cols], j[1, cols], 40, 5)
    assert bad.sum() >= 6 and all(HH.valid_records(act, i[l, cols], j[l, cols], 40, 5).all() for l in (0, 2))
    g[1, cols][bad] = np.nan                  # their noise is never read
    pop, loss, grad = check_pass(gpu, dims, models, obs, act, nxt, i, j, g, cols)
    assert pop.last_n.tolist() == [33.0, 33.0 - bad.sum(), 33.0] and bool(torch.isfinite(grad).all())


def test_a_learner_without_a_valid_record(gpu):
    dims = (3, 3, 2, 5)
    models, obs, act, nxt, i, j, g, cols = make_learners(dims, 3, 33, 310)
    i[2, cols] = 40
    pop, loss, grad = check_pass(gpu, dims, models, obs, act, nxt, i, j, g, cols)
    assert pop.last_n.tolist() == [33.0, 33.0, 0.0] and float(loss[2]) == 0.0 and not bool(grad[2].any()) and bool(grad[:2].any(dim=1).all())


@pytest.mark.parametrize("dims", [(2, 5, 25, 64), (3, 3, 2, 5)], ids=["2_5_25_64", "3_3_2_5"])
def test_hard_forward(gpu, dims):
    models, obs, act, nxt, i, j, g, cols = make_learners(dims, 3, 86, 320)
    _, loss, grad = check_pass(gpu, dims, models, obs, act, nxt, i, j, g, cols, hard=True)
    _, soft, _ = check_pass(gpu, dims, models, obs, act, nxt, i, j, g, cols)
    assert grad is None and not torch.equal(loss, soft)


# ---- 2. more than one tile per workgroup ----
def test_more_than_one_tile_per_workgroup(gpu):
    """4500 patterned records per learner on the smallest net: 141 tiles of 32 on 128 workgroups per learner, a short last tile"""
    from rl_offline_simulation_amd import _lib as L
    dims, M, n_rows, n_learners = (3, 3, 2, 5), 4500, 97, 2
    assert M > 32 * L.HOMER_MAX_BLOCKS and M % 32 != 0
    models, obs, act, nxt, i, j, g, cols = make_learners(dims, n_learners, 1, 330, n_rows=n_rows, pad=(0, 0))
    m = np.arange(M + 5)
    i = np.stack([(m * (7 + 4 * l) % n_rows) for l in range(n_learners)]).astype(np.int32)
    j = np.stack([(m * (13 + 6 * l) % n_rows) for l in range(n_learners)]).astype(np.int32)
    g = np.stack([np.sin(m[:, None, None] * (0.37 + 0.1 * l) + np.arange(4)[None, :, None] + np.arange(2)[None, None, :] * 2.0) for l in range(n_learners)])
    check_pass(gpu, dims, models, obs, act, nxt, i, j, g.astype(np.float32), slice(2, 2 + M))


# ---- 3. / 4. steps ----
def _step_both(pop, encs, data, i, j, g, cols, gpu, tau=1.0, active=None, stepped=None):
    """one step of the population on the column slice and of every single encoder in `stepped` (default: all) on its learner's records;
    returns the population's stats [L, 3]"""
    di, dj, dg = on(gpu, i, j, g)
    M = cols.stop - cols.start
    pop.train_epoch(data, di[:, cols], dj[:, cols], M, tau, noise=dg[:, cols], active=active)
    stats = pop.last_stats[0].clone()
    for l in (range(len(encs)) if stepped is None else stepped):
        one = T._one_step(encs[l], data, i[l, cols], j[l, cols], g[l, cols], tau)
        assert np.array_equal(stats[l].cpu().numpy(), one), (l, stats[l], one)
    return stats


def _state_equal(pop, l, enc):
    """learner l's weights, m, v and t against the single encoder's, bit for bit"""
    ok = all(same(a[l], b) for a, b in zip(pop._params(), enc._params()))
    pm, pv, pt = pop.adam_state()
    em, ev, et = enc.adam_state()
    return ok and same(pm[l], em) and same(pv[l], ev) and same(pt[l:l + 1], et)


def _snapshot(pop, l):
    return [t[l].clone() for t in pop._params()] + [t[l].clone() for t in pop.adam_state()]


def test_three_steps_with_per_learner_hyperparameters(gpu):
    dims, n_learners, M = (4, 2, 10, 16), 4, 40
    models, obs, act, nxt, i, j, g, cols = make_learners(dims, n_learners, M, 400, scale=1.0)
    pop = population(models, dims)
    norms = torch.linalg.vector_norm(pop.loss_grad(obs, act, nxt, i[:, cols], j[:, cols], g[:, cols])[1].double(), dim=1).cpu().numpy()
    lr, wd = [1e-3, 1e-2, 3e-3, 5e-4], [0.0, 0.01, 0.001, 0.0]
    mx = [0.25 * norms[0], 40.0, 0.25 * norms[2], 1e3]  # the clip is active for learners 0 and 2, inactive for 1 and 3
    pop.lr, pop.weight_decay, pop.max_grad_norm = lr, wd, mx
    pop.reset_optimizer()
    data = pop.upload((obs, act, nxt))
    encs = [T.encoder(m, dims) for m in models]
    for l, enc in enumerate(encs):
        enc.lr, enc.weight_decay, enc.max_grad_norm = lr[l], wd[l], mx[l]
        enc.reset_optimizer()
    for k in range(3):
        _, _, _, _, i, j, g, cols = make_learners(dims, n_learners, M, 410 + k, pad=(k, 5))
        stats = _step_both(pop, encs, data, i, j, g, cols, gpu, tau=(1.0, 0.8, 0.6)[k])
        total = stats[:, 2].cpu().numpy()
        assert (total > np.asarray(mx)).tolist() == [True, False, True, False], (total, mx)
        assert stats[:, 0].tolist() == [M] * n_learners and pop.adam_state()[2].tolist() == [k + 1] * n_learners
        for l, enc in enumerate(encs):
            assert _state_equal(pop, l, enc), (k, l)
    assert len({float(x) for x in pop._params()[0][:, 0, 0]}) == n_learners


def test_inactive_learners_and_all_invalid_batches_change_nothing(gpu):
    dims, M = (2, 5, 25, 64), 33
    models, obs, act, nxt, i, j, g, cols = make_learners(dims, 3, M, 500)
    pop = population(models, dims)
    pop.weight_decay = 0.01
    pop.reset_optimizer()
    data = pop.upload((obs, act, nxt))
    encs = [T.encoder(m, dims) for m in models]
    for enc in encs:
        enc.weight_decay = 0.01
        enc.reset_optimizer()
    _step_both(pop, encs, data, i, j, g, cols, gpu)  # everybody once, so that m, v and t are not zero
    quiet = _snapshot(pop, 1)
    assert bool(quiet[8].any()) and int(quiet[10]) == 1
    for k in range(2):
        _, _, _, _, i, j, g, cols = make_learners(dims, 3, M, 510 + k)
        stats = _step_both(pop, encs, data, i, j, g, cols, gpu, active=[1, 0, 1], stepped=(0, 2))
        assert stats[1].tolist() == [0.0, 0.0, 0.0]  # its stats row is not written
    assert all(same(a, b) for a, b in zip(quiet, _snapshot(pop, 1)))
    assert pop.adam_state()[2].tolist() == [3, 1, 3]
    assert _state_equal(pop, 0, encs[0]) and _state_equal(pop, 2, encs[2]) and _state_equal(pop, 1, encs[1])
    # an all-invalid batch for an active learner: nothing of it changes, t included, and the others step as ever
    before = _snapshot(pop, 0)
    _, _, _, _, i, j, g, cols = make_learners(dims, 3, M, 520)
    i[0, cols] = -1
    stats = _step_both(pop, encs, data, i, j, g, cols, gpu, active=torch.tensor([1, 1, 1]))
    assert stats[0].tolist() == [0.0, 0.0, 0.0] and stats[1, 0] == M
    assert all(same(a, b) for a, b in zip(before, _snapshot(pop, 0)))
    assert pop.adam_state()[2].tolist() == [3, 2, 4]
    assert all(_state_equal(pop, l, encs[l]) for l in range(3))
    # the same through eval_epoch: a quiet learner's loss stays 0
    di, dj, dg = on(gpu, i, j, g)
    lv = pop.eval_epoch(data, di[:, cols], dj[:, cols], M, noise=dg[:, cols], active=[0, 1, 1])
    assert lv.shape == (1, 3) and float(lv[0, 0]) == 0.0
    for l in (1, 2):
        assert same(lv[:, l], encs[l].eval_epoch(data, i[l, cols], j[l, cols], M, noise=torch.from_numpy(g[l, cols])))


# ---- 5. epochs ----
def test_train_epoch_twice_and_eval_epoch(gpu):
    dims, n_learners, n = (2, 5, 25, 64), 3, 150
    models, obs, act, nxt, i, j, g, cols = make_learners(dims, n_learners, n, 600, pad=(0, 0))
    di, dj, dg = on(gpu, i, j, g)
    outs = []
    for _ in range(2):
        pop = population(models, dims)
        pop.weight_decay, pop.lr = 0.01, [1e-3, 2e-3, 1e-2]
        pop.reset_optimizer()
        data = pop.upload((obs, act, nxt))
        losses = pop.train_epoch(data, di, dj, 64, 0.7, noise=dg)
        outs.append([losses.clone()] + [t.clone() for t in pop._params()] + [t.clone() for t in pop.adam_state()])
    assert outs[0][0].shape == (3, n_learners) and pop.adam_state()[2].tolist() == [3] * n_learners
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    # against the single encoders: the epoch (batches of 64, 64 and 22 records) and the evaluation of the stepped weights
    lv = pop.eval_epoch(data, dj, di, 64, noise=dg)
    for l, model in enumerate(models):
        enc = T.encoder(model, dims)
        enc.weight_decay, enc.lr = 0.01, pop.lr[l]
        enc.reset_optimizer()
        lt1 = enc.train_epoch(data, i[l], j[l], 64, 0.7, noise=torch.from_numpy(g[l]))
        assert same(outs[0][0][:, l], lt1) and _state_equal(pop, l, enc), l
        assert same(lv[:, l], enc.eval_epoch(data, j[l], i[l], 64, noise=torch.from_numpy(g[l]))), l
    # noise drawn on the device when none is given: finite losses, one step per batch
    lt = pop.train_epoch(data, di, dj, 64, 1.0)
    assert lt.shape == (3, n_learners) and bool(torch.isfinite(lt).all()) and pop.adam_state()[2].tolist() == [6] * n_learners
    empty = torch.zeros((n_learners, 0), dtype=torch.int32)
    assert pop.train_epoch(data, empty, empty, 64, 1.0).shape == (0, n_learners)


# ---- 6. / 7. train() end to end ----
def _grid_walk_2d(n=200, seed=0):
    """a walk on a 5 x 5 grid: x = (column, row) / 5, a in {stay, right, left, up, down}, x_next = the neighbour (clipped)"""
    rng = np.random.default_rng(seed)
    pos, a = rng.integers(0, 5, (n, 2)), rng.integers(0, 5, n)
    nxt = np.clip(pos + np.array([[0, 0], [1, 0], [-1, 0], [0, 1], [0, -1]])[a], 0, 4)
    return (pos / 5.0).astype(np.float32), a.astype(np.int32), (nxt / 5.0).astype(np.float32)


def _train_and_replay(gpu, tmp_path, dims, inits, lr, wd, mx, seed, num_epochs, patience):
    """HOMERPopulation.train against its replay: epoch_draws from an equally seeded generator, every learner's draws through a single
    HOMEREncoder's train_epoch / eval_epoch and the reference's stop rule"""
    from rl_offline_simulation_amd.encoders import HOMEREncoder, HOMERPopulation, epoch_draws
    x, a, xn = _grid_walk_2d()
    tr, va = (x[:160], a[:160], xn[:160]), (x[160:], a[160:], xn[160:])
    n_learners, nZ, B = len(inits), dims[2], 32
    pop = HOMERPopulation(*dims, state_dicts=inits)
    res = pop.train(tr, va, lr=lr, weight_decay=wd, num_epochs=num_epochs, batch_size=B, patience_threshold=patience, temperature_decay=True,
                    max_grad_norm=mx, seed=seed, model_dir=str(tmp_path))
    # the replay
    encs = [HOMEREncoder(*dims, state_dict=sd) for sd in inits]
    for l, enc in enumerate(encs):
        enc.lr, enc.weight_decay, enc.max_grad_norm = lr[l], wd[l], mx[l]
        enc.reset_optimizer()
    d_tr, d_va = encs[0].upload(tr), encs[0].upload(va)
    gen = torch.Generator(device=gpu)
    gen.manual_seed(seed)
    running, patience_of = [True] * n_learners, [0] * n_learners
    best_val, best_epoch, epochs_run = [0.69] * n_learners, [-1] * n_learners, [0] * n_learners
    best_sd = [enc.state_dict() for enc in encs]
    t_loss, v_loss = [[] for _ in encs], [[] for _ in encs]
    for epoch in range(1, num_epochs + 1):
        if not any(running):
            break
        tau = max(0.5, math.exp(-0.005 * epoch))
        ti, tj, tn = epoch_draws(gen, n_learners, 160, nZ)
        vi, vj, vn = epoch_draws(gen, n_learners, 40, nZ)
        for l, enc in enumerate(encs):
            if not running[l]:
                continue
            lt = enc.train_epoch(d_tr, ti[l], tj[l], B, tau, noise=tn[l])
            lv = enc.eval_epoch(d_va, vi[l], vj[l], B, noise=vn[l])
            t_loss[l].append(float(lt.mean()))
            v_loss[l].append(float(lv.mean()))
            epochs_run[l] = epoch
            if v_loss[l][-1] < best_val[l]:
                patience_of[l], best_val[l], best_epoch[l], best_sd[l] = 0, v_loss[l][-1], epoch, enc.state_dict()
            else:
                patience_of[l] += 1
                running[l] = not (v_loss[l][-1] > 0.8 or patience_of[l] == patience)
    print("val losses:", v_loss, "best epochs:", best_epoch, "epochs run:", epochs_run)
    for l, enc in enumerate(encs):
        assert res.train_losses[l] == t_loss[l] and res.val_losses[l] == v_loss[l], l
        assert T._stop_rule(v_loss[l], patience) == (epochs_run[l], best_epoch[l], best_val[l])
        last, best = pop.state_dict(l), pop.best_state_dict(l)
        want = enc.state_dict()
        assert list(last) == list(want) and all(torch.equal(last[k], want[k]) for k in want), l
        assert all(torch.equal(best[k], best_sd[l][k]) for k in want), l
        assert _state_equal(pop, l, enc), l
        assert np.array_equal(pop.encoder(l).encode(x), enc.encode(x)), l
        saved = torch.load(os.path.join(str(tmp_path), f"encoder_model_{l}.pt"))
        loaded = HOMEREncoder(*dims, state_dict=saved)
        assert list(saved) == list(best) and all(torch.equal(saved[k], best[k]) for k in best), l
        assert np.array_equal(loaded.encode(x), pop.encoder(l, best=True).encode(x)), l
        assert np.array_equal(loaded.encode(x), HOMEREncoder(*dims, state_dict=best_sd[l]).encode(x)), l
    assert res.best_epoch.tolist() == best_epoch and res.best_val_loss.tolist() == best_val and res.epochs_run.tolist() == epochs_run
    assert pop.best() == int(np.argmin(best_val)) and pop.result is res
    return res


def _inits(dims, n_learners, first_seed=10):
    from rl_offline_simulation_amd.encoders import HOMEREncoder
    out = []
    for l in range(n_learners):
        torch.manual_seed(first_seed + l)
        out.append(HOMEREncoder(*dims).state_dict())
    return out


def test_train_end_to_end_against_its_replay(gpu, tmp_path):
    from rl_offline_simulation_amd.encoders import HOMERPopulation
    dims, n_learners = (2, 5, 10, 16), 4
    inits = _inits(dims, n_learners)
    # seeds give the same weights as encoders constructed under those seeds
    by_seed = HOMERPopulation(*dims, seeds=[10, 11, 12, 13])
    assert all(torch.equal(by_seed.state_dict(l)[k], inits[l][k]) for l in range(n_learners) for k in inits[l])
    # learner 1 never moves (lr = 0) and starts from weights six times as large: a validation loss near 2, so it stops in epoch 1
    # (val_loss > 0.8), while the others need at least `patience` epochs -- the quiet-learner path runs from epoch 2 on
    inits[1] = {k: (v * 6.0 if k != "action_emb.weight" else v) for k, v in inits[1].items()}
    res = _train_and_replay(gpu, tmp_path, dims, inits, lr=[3e-2, 0.0, 3e-2, 1e-2], wd=[0.0, 0.0, 0.01, 0.0], mx=[40.0, 40.0, 0.05, 40.0], seed=3,
                            num_epochs=6, patience=3)
    assert len(set(res.epochs_run.tolist())) > 1 and res.epochs_run[1] == 1 and res.best_epoch[1] == -1
    assert all(len(res.val_losses[l]) == res.epochs_run[l] for l in range(n_learners))
    # this seed has learners that improve (the masked copy of the best weights runs) next to learners that never do
    assert (res.best_epoch > 0).any() and (res.best_epoch < 0).any()


# ---- 7. one learner is the single encoder ----
def test_one_learner_is_the_single_encoder(gpu, tmp_path):
    dims = (2, 5, 25, 64)
    for k, (M, hard) in enumerate(((1, False), (33, False), (86, True))):
        models, obs, act, nxt, i, j, g, cols = make_learners(dims, 1, M, 700 + k)
        check_pass(gpu, dims, models, obs, act, nxt, i, j, g, cols, 0.7 if not hard else 1.0, hard=hard)
    models, obs, act, nxt, i, j, g, cols = make_learners((3, 3, 2, 5), 1, 4500, 710, n_rows=97)
    check_pass(gpu, (3, 3, 2, 5), models, obs, act, nxt, i, j, g, cols)
    # steps, an epoch with a short last batch, the evaluation
    models, obs, act, nxt, i, j, g, cols = make_learners(dims, 1, 86, 720)
    pop, enc = population(models, dims), T.encoder(models[0], dims)
    pop.lr, pop.weight_decay, pop.max_grad_norm = 2e-3, 0.01, 0.01
    enc.lr, enc.weight_decay, enc.max_grad_norm = 2e-3, 0.01, 0.01
    pop.reset_optimizer(), enc.reset_optimizer()
    data = pop.upload((obs, act, nxt))
    for _ in range(2):
        _step_both(pop, [enc], data, i, j, g, cols, gpu)
        assert _state_equal(pop, 0, enc)
    di, dj, dg = on(gpu, i, j, g)
    lt = pop.train_epoch(data, di[:, cols], dj[:, cols], 32, 0.9, noise=dg[:, cols])
    assert same(lt[:, 0], enc.train_epoch(data, i[0, cols], j[0, cols], 32, 0.9, noise=torch.from_numpy(g[0, cols]))) and lt.shape == (3, 1)
    assert _state_equal(pop, 0, enc)
    lv = pop.eval_epoch(data, di[:, cols], dj[:, cols], 32, noise=dg[:, cols])
    assert same(lv[:, 0], enc.eval_epoch(data, i[0, cols], j[0, cols], 32, noise=torch.from_numpy(g[0, cols])))
    # train()
    small = (2, 5, 10, 16)
    _train_and_replay(gpu, tmp_path, small, _inits(small, 1), lr=[1e-2], wd=[0.0], mx=[40.0], seed=4, num_epochs=3, patience=2)
