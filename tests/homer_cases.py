"""The cases of the k_homer_grad / k_homer_reduce / k_homer_adam matrix (tests/test_gpu_homer_matrix.py on the device,
tests/test_homer_matrix_host.py for what needs none): networks, batches, the NumPy f64 reference of each (tests/homer_train_host.py, the
case's slope passed through), torch's own f32 autograd on the CPU, which sets every bound, and ht_prepare's tile and LDS arithmetic
(csrc/homer_train.hpp) restated.

A case is built once per process and then only read."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import homer_train_host as HH  # noqa: E402
from test_gpu_homer_train import bound as grad_bound, torch_ref  # noqa: E402

ULP = 2.0 ** -23
MAX_FLOATS, MAX_BLOCKS, THREADS, OWN, RED_BLOCK = 20480, 128, 512, 40, 256  # OFFSIM_HOMER_MAX_FLOATS / _MAX_BLOCKS, HT_THREADS, HT_OWN, HT_RED_BLOCK
LDS_MAX = 160 * 1024
TENSORS = ("enc.W1", "enc.b1", "enc.W2", "enc.b2", "cls.W1", "cls.b1", "cls.W2", "cls.b2")
REL_TENSOR = 1e-3      # the per-tensor check of the device gradient: |got - g64|_2 / |g64|_2
REL_TENSOR_F32 = 1e-4  # what torch's own f32 gradient has to stay below on every tensor of every case: a tenfold margin
PRE_MARGIN, GAP_MARGIN = 1e-6, 1e-4


# ---- ht_prepare's layout arithmetic ----
def homer_plan(dims, M):
    """ht_prepare restated: P, the padded weight floats, the four leading dimensions, the floats per record of a tile, TM from the LDS
    budget, the TM of a batch of M records, its LDS bytes, its workgroups, and whether ht_prepare refuses the net (more than 160 KiB at
    TM = 4)."""
    dO, nA, nZ, H = dims
    K = 2 * nZ + nA
    ins, outs = (dO, H, K, H), (H, nZ, H, 2)
    P = sum(i * o + o for i, o in zip(ins, outs))
    w_floats = (sum(i * (o | 1) + o for i, o in zip(ins, outs)) + 3) & ~3
    lda_e, ldd_e, lda_c, ldd_c = (dO + H + 1) | 1, (H + nZ) | 1, (K + H + 1) | 1, (H + 2 + K) | 1
    per_record = 3 * (lda_e + ldd_e) + 2 * (lda_c + ldd_c) + 4 + 8  # activations and deltas, the record's three ints (4 reserved), two f64 sums per classifier row
    lds = lambda TM: 4 * (w_floats + TM * per_record)  # noqa: E731
    TM = 32
    while lds(TM) > LDS_MAX and TM > 4:
        TM //= 2
    tm_lds = TM
    while TM > 8 and M < 8 * TM:
        TM //= 2
    tiles = -(-M // TM)
    return SimpleNamespace(P=P, w_floats=w_floats, lda_e=lda_e, ldd_e=ldd_e, lda_c=lda_c, ldd_c=ldd_c, per_record=per_record, tm_lds=tm_lds, TM=TM,
                           lds=lds(TM), lds_at_tm_lds=lds(tm_lds), lds_at_4=lds(4), refused=lds(tm_lds) > LDS_MAX, tiles=tiles,
                           workgroups=min(tiles, MAX_BLOCKS), nred=-(-P // RED_BLOCK), slots=-(-P // THREADS))


def tensor_slices(dims):
    out, o = [], 0
    for shape in HH.shapes(*dims):
        n = int(np.prod(shape))
        out.append(slice(o, o + n))
        o += n
    return out


# ---- the case table ----
def _c(name, dims, M, xdt="f32", slope=0.01, tau=1.0, noise="iid", pattern="iid", n_rows=40, gains=(1.0, 1.0, 2.0, 1.0), x_scale=1.0, seed=0, mask=None,
       big_logits=False, group="edges"):
    return SimpleNamespace(name=name, dims=tuple(dims), M=M, xdt=xdt, slope=slope, tau=tau, noise=noise, pattern=pattern, n_rows=n_rows, gains=gains,
                           x_scale=x_scale, seed=seed, mask=mask, big_logits=big_logits, group=group)


def _matrix():
    """Small nets, every width at most 24, M in 200..220: TM = 16 (16 <- 32 by M < 256), 13 or 14 tiles, each with f32 and f16 observations"""
    nets = [  # (dO, nA, nZ, H), slope, tau, noise
        ((1, 1, 2, 5), 0.2, 1.0, "iid"),
        ((3, 2, 7, 12), 0.01, 0.5, None),
        ((4, 3, 10, 16), 0.0, 0.7, "iid"),
        ((7, 16, 5, 9), 0.01, 1.0, "iid"),
        ((2, 2, 24, 24), 0.2, 0.1, "iid"),
        ((5, 3, 3, 7), 0.0, 2.0, "iid"),
        ((6, 1, 8, 11), 0.2, 0.5, "iid"),
        ((9, 16, 6, 8), 0.01, 0.7, None),
        ((1, 2, 9, 24), 0.0, 0.7, "iid"),
        ((8, 3, 4, 13), 0.01, 1.0, None),
    ]
    out = []
    for k, (dims, slope, tau, noise) in enumerate(nets):
        for xdt in ("f32", "f16"):
            tag = "-".join(str(v) for v in dims)
            out.append(_c(f"m{k}-{tag}-{xdt}-s{slope}-t{tau}-{'noise' if noise else 'nonoise'}", dims, 200 + 2 * k + (xdt == "f16"), xdt, slope, tau, noise,
                          n_rows=64, seed=k, group="matrix"))
    return out


REAL = (2, 5, 25, 64)  # the reference's own shape


def _edges():
    out = []
    for M in (1, 3, 4, 5, 21):  # 3 TM = 12 rows: three HT_RB blocks; M = 21: six tiles, the last of one record
        out.append(_c(f"TM4-H256-M{M}", (12, 4, 19, 256), M, slope=0.2 if M <= 3 else 0.01, tau=2.0, seed=20 + M))
    out.append(_c("TM4-H256-M21-f16", (12, 4, 19, 256), 21, "f16", seed=47))
    for M in (5, 21):
        out.append(_c(f"TM4-nZ256-M{M}", (4, 2, 256, 24), M, slope=0.2, tau=8.0, seed=50 + M, gains=(1.0, 2.0, 16.0, 1.0)))
    for M in (7, 8, 9, 86):
        out.append(_c(f"P-20480-M{M}", (120, 9, 62, 64), M, seed=60 + M, n_rows=64))
    for M in (256, 300):
        out.append(_c(f"LDS-160K-TM32-M{M}", (1, 1, 85, 17), M, seed=70 + M % 7, gains=(1.0, 2.0, 6.0, 1.0), n_rows=64))
    for M in (40, 200):
        out.append(_c(f"LDS-160K-TM16-M{M}", (1, 1, 2, 230), M, seed=80 + M % 7, n_rows=64))
    out.append(_c("LDS-160K-TM8-M30", (1, 16, 190, 34), 30, tau=4.0, seed=90, gains=(1.0, 2.0, 8.0, 1.0), n_rows=64))
    for M in (128, 129, 255):
        out.append(_c(f"TM16-by-M-M{M}", REAL, M, seed=100 + M % 11, n_rows=64))
    out.append(_c("TM16-by-M-M129-f16", REAL, 129, "f16", seed=115, n_rows=64))
    for M in (256, 257, 300):
        out.append(_c(f"TM32-real-net-M{M}", REAL, M, seed=120 + M % 11, n_rows=64))
    out.append(_c("TM32-real-net-M257-f16", REAL, 257, "f16", seed=135, n_rows=64))
    # more tiles than workgroups: tiles b, b + 128 of workgroups 0 and 1; a pattern, not noise, so that no two tiles look alike
    out.append(_c("TM32-tiles-per-workgroup", (4, 2, 10, 16), MAX_BLOCKS * 32 + 37, seed=140, pattern="det", noise="det", n_rows=97))
    out.append(_c("TM8-tiles-per-workgroup", (128, 5, 50, 64), MAX_BLOCKS * 8 + 11, "f16", seed=141, pattern="det", noise="det", n_rows=97))
    for M in (1, 33):
        out.append(_c(f"smallest-M{M}", (1, 1, 2, 1), M, seed=150 + M, n_rows=16))
    out.append(_c("masked-tiles-nan", (5, 3, 7, 12), 16 * 6 + 7, seed=160, mask="tiles", n_rows=64))
    out.append(_c("logits-in-the-hundreds", REAL, 200, seed=170, big_logits=True, n_rows=64))
    return out


MATRIX = _matrix()
EDGES = _edges()
CASES = {c.name: c for c in MATRIX + EDGES}
assert len(CASES) == len(MATRIX) + len(EDGES)
# the forward-only instances and the hard forward run at these, f32 and f16: (TM, f32 case, f16 case)
FORWARD_CASES = [(4, "TM4-H256-M21", "TM4-H256-M21-f16"), (16, "TM16-by-M-M129", "TM16-by-M-M129-f16"), (32, "TM32-real-net-M257", "TM32-real-net-M257-f16")]


# ---- building a case ----
def make_model(c, rng):
    """W ~ N(0, 1) * gain / sqrt(fan-in) per layer (the classifier's first layer by sqrt(nZ + nA): its z inputs sum to 1), b ~ 0.3 N(0, 1)"""
    dO, nA, nZ, H = c.dims
    fan = (dO, H, nZ + nA, H)
    model = []
    for l, (ws, bs) in enumerate(zip(HH.shapes(*c.dims)[0::2], HH.shapes(*c.dims)[1::2])):
        model.append((rng.normal(size=ws) * c.gains[l] / np.sqrt(fan[l])).astype(np.float32))
        model.append((rng.normal(size=bs) * 0.3).astype(np.float32))
    if c.big_logits:  # logits around 300: exp overflows without the max subtraction.  A shift, not the scaling of test_logits_in_the_hundreds
        # (tests/test_gpu_homer_train.py), whose nearly one-hot z leaves the encoder's gradient below the bound: here every tensor keeps its signal
        model[2], model[3] = model[2] * 3.0, model[3] + np.float32(300.0)
    return model


def make_batch(c, rng):
    dO, nA, nZ, H = c.dims
    M, n = c.M, c.n_rows
    xd = np.float16 if c.xdt == "f16" else np.float32
    obs, nxt = (rng.normal(size=(n, dO)) * c.x_scale).astype(xd), (rng.normal(size=(n, dO)) * c.x_scale).astype(xd)
    act = rng.permutation((np.arange(n) * 7 + 3) % nA).astype(np.int32)
    m = np.arange(M)
    if c.pattern == "det":
        i, j = (m * 7 % n).astype(np.int32), (m * 13 % n).astype(np.int32)
    else:
        i, j = rng.integers(0, n, M).astype(np.int32), rng.integers(0, n, M).astype(np.int32)
        j[2::3] = i[2::3]       # idx_impo == idx_real on a third of the records
        if M >= 8:
            i[6], j[6] = i[3], j[3]  # a duplicated record, besides the duplicated indices that M > n_rows or chance gives
        if j[0] == i[0]:        # (record 0 always tells next_obs[j] from next_obs[i])
            j[0] = (i[0] + 1) % n
    if c.noise == "det":
        g = np.sin(m[:, None, None] * 0.37 + np.arange(4)[None, :, None] * 1.3 + np.arange(nZ)[None, None, :] * 2.0).astype(np.float32)
    elif c.noise == "iid":
        g = (-np.log(rng.exponential(size=(M, 4, nZ)))).astype(np.float32)
    else:
        g = None
    return obs, act, nxt, i, j, g


def _mask(c, obs, act, nxt, i, j, g, rng):
    """whole tiles (of 8 and of 16), the tail and scattered records invalid, in each of the ways valid_records knows; NaN in their noise"""
    M, n, nA = c.M, c.n_rows, c.dims[1]
    act = act.copy()
    bad_rows = np.array([3, 11])
    act[bad_rows[0]], act[bad_rows[1]] = nA, -1  # every record whose idx_real is one of these rows is invalid
    i[np.isin(i, bad_rows)] = 0
    bad = np.zeros(M, bool)
    bad[16:32] = bad[48:64] = bad[96:] = True
    bad[rng.choice(M, size=M // 10, replace=False)] = True
    for k, m in enumerate(np.flatnonzero(bad)):
        way = k % 6
        if way == 0:
            i[m] = -1 - (k % 5)
        elif way == 1:
            i[m] = n + (k % 7)
        elif way == 2:
            j[m] = -(2 ** 31)
        elif way == 3:
            j[m] = 2 ** 31 - 1 if k % 2 else n
        else:
            i[m] = bad_rows[way - 4]
    ok = HH.valid_records(act, i, j, n, nA)
    assert np.array_equal(~ok, bad)
    g[bad] = np.nan
    return act, i, j, g


def _margins(c, model, obs, act, nxt, i, j, g):
    """(the smallest |hidden pre-activation| of either network, the top-two gap per record of the four perturbed logit vectors)"""
    info = {}
    HH.loss_grad(model, obs, act, nxt, i, j, g, c.tau, slope=c.slope, info=info)
    pre = min(float(np.abs(p).min()) for p in info["enc_pre"] + info["cls_pre"])
    top = np.stack([np.sort(u, 1)[:, -2:] for u in info["u"]])
    return pre, (top[..., 1] - top[..., 0]).min(0) * c.tau  # (the gap of e + g itself: what an f32 ulp of e is measured against)


@functools.lru_cache(maxsize=None)
def build(name):
    c = CASES[name]
    for attempt in range(50):  # the first seed of the case's sequence without a hidden pre-activation within 1e-6 of 0
        rng = np.random.default_rng(5000 + 100 * c.seed + attempt)
        model = make_model(c, rng)
        obs, act, nxt, i, j, g = make_batch(c, rng)
        if c.mask == "tiles":
            act, i, j, g = _mask(c, obs, act, nxt, i, j, g, rng)
        pre, gaps = _margins(c, model, obs, act, nxt, i, j, g)
        if pre >= PRE_MARGIN:
            break
    else:
        raise AssertionError(f"{name}: no seed keeps the pre-activations clear of 0")
    l64, g64, n = HH.loss_grad(model, obs, act, nxt, i, j, g, c.tau, slope=c.slope)
    l32, g32 = torch_ref(model, obs, act, nxt, i, j, g, c.tau, slope=c.slope)
    for v in model + [obs, act, nxt, i, j] + ([g] if g is not None else []):
        v.setflags(write=False)
    return SimpleNamespace(case=c, plan=homer_plan(c.dims, c.M), model=model, obs=obs, act=act, nxt=nxt, i=i, j=j, noise=g, attempt=attempt, pre_margin=pre,
                           ok=HH.valid_records(act, i, j, c.n_rows, c.dims[1]), l64=l64, g64=g64, n=n, l32=l32, g32=g32, bound=grad_bound(g64, g32),
                           loss_bound=scalar_bound(l64, l32), slices=tensor_slices(c.dims))


@functools.lru_cache(maxsize=None)
def build_hard(name):
    """the case's records without those whose top-two gap of any of the four perturbed logit vectors is below 1e-4 (an ulp cannot flip an
    argmax), and the hard (discretized) forward over them in f64 and in torch's f32"""
    b = build(name)
    c = b.case
    _, gaps = _margins(c, b.model, b.obs, b.act, b.nxt, b.i, b.j, b.noise)
    keep = np.ones(c.M, bool)
    keep[np.flatnonzero(b.ok)[gaps < GAP_MARGIN]] = False
    i, j, g = b.i[keep], b.j[keep], None if b.noise is None else b.noise[keep]
    l64, _, n = HH.loss_grad(b.model, b.obs, b.act, b.nxt, i, j, g, c.tau, hard=True, slope=c.slope)
    l32, _ = torch_ref(b.model, b.obs, b.act, b.nxt, i, j, g, c.tau, hard=True, slope=c.slope)
    return SimpleNamespace(case=c, base=b, keep=keep, dropped=int((~keep).sum()), i=i, j=j, noise=g, l64=l64, n=n, l32=l32, loss_bound=scalar_bound(l64, l32))


# ---- the comparator ----
def scalar_bound(want, ref32):
    """test_gpu_homer_train.py's rule for the loss: 4 x the f32 reference's own error, floored at 4 ulps of max(1, |value|)"""
    return max(4.0 * abs(float(ref32) - want), 4.0 * ULP * max(1.0, abs(want)))


def tensor_errors(g, b):
    """|g - g64|_2 / |g64|_2 per tensor (0 where both vanish)"""
    g = np.asarray(g, np.float64)
    out = []
    for s in b.slices:
        den, num = float(np.linalg.norm(b.g64[s])), float(np.linalg.norm(g[s] - b.g64[s]))
        out.append(num / den if den > 0.0 else (0.0 if num == 0.0 else np.inf))
    return out


def max_error(g, b):
    return float(np.abs(np.asarray(g, np.float64) - b.g64).max())


def passes(g, b):
    """the two assertions of the device test on a gradient: the project's rule (max norm of the difference to the f64 gradient within 4 x
    torch's f32 error, floor 4 ulps of the max norm) and every tensor within 1e-3 in relative 2-norm"""
    return bool(np.isfinite(g).all()) and max_error(g, b) <= b.bound and max(tensor_errors(g, b)) <= REL_TENSOR


# ---- subtly wrong backward passes: the f64 pass restated with one thing changed at a time ----
def mutant_grad(b, kind=None, drop=None):
    """HH.loss_grad's gradient of a case (kind None: the same numbers) with one mistake: 'slope' (the backward's slope off by 0.05), 'tau' (the
    / tau of the softmax backward dropped), 'z2' (z2's share of the obs[i] row's de dropped), 'impostor' (next_obs[j] read as next_obs[i]),
    'noise' (the noise of q = 1 and q = 3 swapped); drop: a record left out of the sums, the divisor kept."""
    c = b.case
    W1, b1, W2, b2, V1, c1, V2, c2 = [np.asarray(t, np.float64) for t in b.model]
    nZ, nA, tau, slope = c.dims[2], c.dims[1], c.tau, c.slope
    ok = b.ok.copy()
    n = int(ok.sum())  # the divisor: every valid record
    if drop is not None:
        assert ok[drop]
        ok[drop] = False
    i, j = b.i.astype(np.int64)[ok], b.j.astype(np.int64)[ok]
    k = len(i)
    g = np.zeros((k, 4, nZ)) if b.noise is None else np.asarray(b.noise, np.float64)[ok]
    if kind == "noise":
        g = g[:, [0, 3, 2, 1]]
    obs, nxt = b.obs.astype(np.float64), b.nxt.astype(np.float64)
    onehot = np.zeros((k, nA))
    onehot[np.arange(k), b.act.astype(np.int64)[i]] = 1.0
    xs = [obs[i], nxt[i], nxt[i] if kind == "impostor" else nxt[j]]
    bslope = slope + 0.05 if kind == "slope" else slope
    enc = [HH._mlp(x, W1, b1, W2, b2, slope) for x in xs]
    src = (0, 1, 0, 2)
    zs = [HH._softmax((enc[src[q]][0] + g[:, q]) / tau) for q in range(4)]
    gV, gW = [0.0] * 4, [0.0] * 4
    d_enc = [np.zeros((k, nZ)) for _ in range(3)]
    for cc, target in ((0, 1), (1, 0)):
        x = np.concatenate([zs[2 * cc], onehot, zs[2 * cc + 1]], 1)
        logits, pre, h = HH._mlp(x, V1, c1, V2, c2, slope)
        mx = logits.max(1, keepdims=True)
        logp = logits - (mx + np.log(np.exp(logits - mx).sum(1, keepdims=True)))
        t = np.zeros_like(logp)
        t[:, target] = 1.0
        d_out = (np.exp(logp) - t) / (2.0 * n)
        *gs, dpre = HH._mlp_back(d_out, x, pre, h, V2, bslope)
        gV = [p + q for p, q in zip(gV, gs)]
        dx = dpre @ V1
        for q, dz in ((2 * cc, dx[:, :nZ]), (2 * cc + 1, dx[:, nZ + nA:])):
            if kind == "z2" and q == 2:
                continue
            z = zs[q]
            d_enc[src[q]] += z * (dz - (dz * z).sum(1, keepdims=True)) / (1.0 if kind == "tau" else tau)
    for s in range(3):
        _, pre, h = enc[s]
        *gs, _ = HH._mlp_back(d_enc[s], xs[s], pre, h, W2, bslope)
        gW = [p + q for p, q in zip(gW, gs)]
    return np.concatenate([np.asarray(t).ravel() for t in gW + gV])
