"""The cases of the k_policy_mlp matrix (csrc/policy_mlp.hpp, launched by mlp_forward in csrc/offsim_hip.hip; tests/test_gpu_policy_mlp_matrix.py
on the device, tests/test_policy_mlp_matrix_host.py for what needs none): the launch shape restated, a NumPy f64 forward, a running
forward-error bound computed next to it, a NumPy emulation of the kernel's f32 arithmetic with mutants, and the case table.

The bound, with u = 2^-24 (the unit roundoff of f32), err the bound on |kernel activation - f64 activation| per row and unit, x the f64 activation:
  * a unit of a layer (one fmaf chain of `in` products in k order, then + b):
        err_out = sum_k |w_k| err_in_k + (in + 1) u (sum_k (|x_k| + err_in_k) |w_k| + |b|)
    err_in of the first layer is 0: f32 and f16 observations are exact in f64.  (in + 1 roundings, each at most u of a partial sum that the sum of
    absolute terms bounds; the kernel's terms are those of x + err.)
  * the activation: err times its Lipschitz constant (1 for identity, ReLU, tanh; max(1, |slope|) for leaky ReLU), plus
    C_TANH u |tanh(v)| for tanhf and u |slope v| for the product on leaky ReLU's negative side.
  * a value net's output: the last layer's err_out.
  * a policy's probabilities: with G = max_b (err_b + u |z_b - max z|) (the logit errors and the rounding of z - max),
        |dp_a| <= p_a (exp(2 G) - 1) + (C_EXP + nA + 2) u p_a + TINY
    The first term is the exact form (p_a exp(d_a) / sum_b p_b exp(d_b) lies in p_a exp(+-2 G)), not its first order 2 G p_a, so it holds at
    the extreme-logit cases too; the second is expf, the left-to-right sum of nA terms and the division; TINY = 8 * 2^-149 covers a tail
    probability in the subnormal range, where each of expf and the division is wrong by a few subnormal spacings and not by a relative error.
C_TANH = C_EXP = 8 (in units of u, that is 4 ulps): a ROCm installation carries no table of the device library's ulp errors (no document
in its tree names tanhf or expf), so 4 ulps stand in for each; profiles/policy_mlp_instances_error.jsonl records how much of the bound
every case uses.

A case is built once per process and then only read."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

U = 2.0 ** -24
C_TANH = 8.0
C_EXP = 8.0
TINY = 8.0 * 2.0 ** -149
TM = 32                  # PMLP_TM
W_FLOATS_CAP = 64 * 257  # PMLP_W_FLOATS
LDS_DEFAULT = 64 * 1024
ACT = {"identity": 0, "tanh": 1, "relu": 2, "leaky_relu": 3}
INT32_MAX = 2 ** 31 - 1


# ---- mlp_forward / policy_mlp_lds_bytes restated ----
def launch_shape(sizes):
    """sizes = (dO, out_1, ..., out_n) -> w_max, w_floats, per layer jc_max and the chunk sizes, the LDS bytes and whether they need the opt-in"""
    sizes = tuple(int(s) for s in sizes)
    w_max = max(sizes)
    layers = list(zip(sizes, sizes[1:]))
    w_floats = max(min(o * (i + 1), W_FLOATS_CAP) for i, o in layers)
    jc_max = [w_floats // (i + 1) for i, _ in layers]
    chunks = [[min(jc, o - j0) for j0 in range(0, o, jc)] for (_, o), jc in zip(layers, jc_max)]
    lds = 4 * (2 * TM * (w_max + 1) + w_floats)
    return SimpleNamespace(w_max=w_max, ld=w_max + 1, w_floats=w_floats, jc_max=jc_max, chunks=chunks, lds_bytes=lds, big_lds=lds > LDS_DEFAULT)


@functools.lru_cache(maxsize=None)
def lds_edges():
    """((dO, H, nA) with the largest LDS at or below 64 KiB, the one with the smallest above), over every one-hidden-layer network; ties go
    to the most actions, then to the smallest dO and H"""
    dO, H, nA = np.meshgrid(np.arange(1, 129), np.arange(1, 257), np.arange(1, 17), indexing="ij")
    w_floats = np.maximum(np.minimum(H * (dO + 1), W_FLOATS_CAP), np.minimum(nA * (H + 1), W_FLOATS_CAP))
    lds = 4 * (2 * TM * (np.maximum(np.maximum(dO, H), nA) + 1) + w_floats)
    below = np.where(lds <= LDS_DEFAULT, lds, -1)
    above = np.where(lds > LDS_DEFAULT, lds, 1 << 30)
    pick = lambda hit: max((int(k), -int(i), -int(j)) for i, j, k in np.argwhere(hit))  # noqa: E731 (index triples; the most actions first)
    (kb, ib, jb), (ka, ia, ja) = pick(below == below.max()), pick(above == above.min())
    return (1 - ib, 1 - jb, kb + 1), (1 - ia, 1 - ja, ka + 1)


# ---- the f64 reference and the bound ----
def _act64(v, act, slope):
    if act == "tanh":
        return np.tanh(v)
    if act == "relu":
        return np.where(v > 0, v, 0.0)
    if act == "leaky_relu":
        return np.where(v > 0, v, np.float64(slope) * v)
    return v


def forward_f64(x, layers, act, slope, value):
    """x [M, dO] and layers [(W, b or None)] promoted to f64 -> logits (a value net: [M]), the max-subtracted softmax of them (a value net:
    the same [M]), the bound on the kernel's output, and every layer's pre-activations"""
    h = np.asarray(x).astype(np.float64)
    err = np.zeros_like(h)
    pres = []
    for l, (W, b) in enumerate(layers):
        W = np.asarray(W).astype(np.float64)
        bb = np.zeros(W.shape[0]) if b is None else np.asarray(b).astype(np.float64)
        v = h @ W.T + bb
        aw = np.abs(W)
        err = err @ aw.T + (W.shape[1] + 1) * U * ((np.abs(h) + err) @ aw.T + np.abs(bb))
        pres.append(v)
        if l == len(layers) - 1:
            break
        h = _act64(v, act, slope)
        if act == "tanh":
            err = err + C_TANH * U * np.abs(h)
        elif act == "leaky_relu":
            err = err * max(1.0, abs(float(slope))) + U * np.abs(h)
    if value:
        return v[:, 0], v[:, 0], err[:, 0], pres
    mx = v.max(axis=1, keepdims=True)
    e = np.exp(v - mx)
    p = e / e.sum(axis=1, keepdims=True)
    G = (err + U * np.abs(v - mx)).max(axis=1, keepdims=True)
    nA = v.shape[1]
    bound = p * np.expm1(2.0 * G) + (C_EXP + nA + 2) * U * p + TINY
    return v, p, bound, pres


# ---- the kernel's arithmetic in NumPy f32 ----
MUTANTS = ("drop_product", "drop_bias", "chunk_bias_shift", "skip_ragged_last", "wrong_pingpong", "softmax_no_max", "leaky_wrong_side",
           "pop_bias0")


def _fma32(x, w, acc):
    """float32(float64(x) * float64(w) + float64(acc)): fmaf but for rare double roundings"""
    return (x.astype(np.float64) * w.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def _act32(v, act, slope, wrong_side=False):
    if act == "tanh":
        return np.tanh(v.astype(np.float64)).astype(np.float32)
    if act == "relu":
        return np.where(v > 0, v, np.float32(0.0)).astype(np.float32)
    if act == "leaky_relu":
        scaled = (v * np.float32(slope)).astype(np.float32)
        return np.where(v > 0, scaled, v) if wrong_side else np.where(v > 0, v, scaled)
    return v


def emulate_f32(b, mutant=None, learner=0):
    """The output of k_policy_mlp on the built case b for one learner, every unit a running f32 sum in k order; rows outside x are NaN.
    mutant: one of MUTANTS, placed where the case's shape puts it (mutant_applies says whether it has a place)."""
    assert mutant is None or (mutant in MUTANTS and mutant_applies(b.case, mutant)), mutant
    c = b.case
    shape = launch_shape(c.sizes)
    layers = b.weights[learner]
    cur = np.where(b.valid[:, None], b.xg, 0).astype(np.float32)
    prev_in = np.zeros((cur.shape[0], shape.ld), np.float32)  # what the buffer a layer writes held before: LDS never written reads as 0 here
    n = len(layers)
    for l, (W, bias) in enumerate(layers):
        out, in_ = W.shape
        acc = np.zeros((cur.shape[0], out), np.float32)
        for k in range(in_):
            term = _fma32(cur[:, k:k + 1], W[None, :, k], acc)
            if mutant == "drop_product" and l == n - 1 and k == in_ - 1:
                term[:, 0] = acc[:, 0]
            acc = term
        if bias is not None:
            bv = np.array(b.weights[0][l][1] if mutant == "pop_bias0" else bias, np.float32)
            if mutant == "chunk_bias_shift" and l == _chunked_layer(c):
                j = shape.jc_max[l]
                bv[j] = bv[j - 1]
            add = (acc + bv[None, :]).astype(np.float32)
            if mutant == "drop_bias" and l == 0:
                add[:, 0] = acc[:, 0]
            acc = add
        h = acc if l == n - 1 else _act32(acc, c.act, c.slope, wrong_side=mutant == "leaky_wrong_side")
        if mutant == "skip_ragged_last" and l == _chunked_layer(c):
            h = h.copy()
            h[:, out - 1] = prev_in[:, out - 1]
        full = np.zeros_like(prev_in)
        full[:, :out] = h
        prev_in_next = np.zeros_like(prev_in)
        prev_in_next[:, :cur.shape[1]] = cur
        if mutant == "wrong_pingpong" and l == n - 1:
            full = prev_in_next  # the buffer the last layer read, not the one it wrote
        prev_in, cur = prev_in_next, full[:, :out]
    if c.value:
        res = cur[:, 0].copy()
        res[~b.valid] = np.nan
        return res
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        mx = np.zeros((cur.shape[0], 1), np.float32) if mutant == "softmax_no_max" else cur.max(axis=1, keepdims=True)
        e = np.exp((cur - mx).astype(np.float32).astype(np.float64)).astype(np.float32)
        s = np.zeros(cur.shape[0], np.float32)
        for a in range(cur.shape[1]):
            s = (s + e[:, a]).astype(np.float32)
        res = (e / s[:, None]).astype(np.float32)
    res[~b.valid] = np.nan
    return res


def _chunked_layer(c):
    """the first layer whose weights go through LDS in more than one chunk (None: no layer does)"""
    for l, ch in enumerate(launch_shape(c.sizes).chunks):
        if len(ch) > 1:
            return l
    return None


def mutant_applies(c, mutant):
    l = _chunked_layer(c)
    n = len(c.sizes) - 1
    if mutant == "drop_bias":
        return c.bias[0]
    if mutant == "chunk_bias_shift":
        return l is not None and c.bias[l]
    if mutant == "skip_ragged_last":
        return l is not None and launch_shape(c.sizes).chunks[l][-1] < launch_shape(c.sizes).jc_max[l]
    if mutant == "wrong_pingpong":
        return n == 4
    if mutant == "softmax_no_max":
        return not c.value
    if mutant == "leaky_wrong_side":
        return c.act == "leaky_relu" and n > 1
    if mutant == "pop_bias0":
        return c.L > 1 and any(c.bias)
    return True


def ratio(got, ref, bound, valid=None):
    """max |got - ref| / bound over the valid rows; inf where got is not finite"""
    got, ref, bound = (np.asarray(a, np.float64) for a in (got, ref, bound))
    if valid is not None:
        got, ref, bound = got[valid], ref[valid], bound[valid]
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref) / bound).max())


# ---- the case table ----
def _c(name, sizes, xdt="f32", value=False, L=0, act="tanh", slope=0.01, M=65, rows="none", n_x=None, bias=None, data="normal", fam=""):
    sizes = tuple(sizes)
    n = len(sizes) - 1
    bias = (True,) * n if bias is None else tuple(bias)
    assert len(bias) == n and (not value or sizes[-1] == 1)
    inst = f"{xdt}-{'value' if value else 'pop' if L else 'policy'}"
    if n_x is None:
        n_x = M if rows in ("none", "arange", "perm") else max(M // 2, 3)
    return SimpleNamespace(name=name, sizes=sizes, xdt=xdt, value=value, L=L, act=act, slope=slope, M=M, rows=rows, n_x=n_x, bias=bias, data=data,
                           inst=inst, fam=fam, seed=0)


# Seeds that are not the case's number (5000 + its index).  tests/test_policy_mlp_matrix_host.py states the two conditions a seed has to
# meet; with the default seeds the emulation's largest share of a bound is 0.23 (depth-n1-val) and the mutant closest to its bound is at 42
# times it, so neither condition needed a search.  The activation cases take seed 7000, the first from 7000 on at which every hidden unit
# of every one of them sees both signs before its activation (at 5000 + index one ReLU unit of the second layer never went negative).
SEEDS = {f"act-{tag}-{kind}": 7000 for tag in ("identity", "tanh", "relu", "leaky005", "leaky15") for kind in ("pol3", "val")}


def _twin(cs, name, sizes, nA, fam, **kw):
    """a policy case and its value twin (the same hidden layers, one output)"""
    cs.append(_c(f"{name}-pol{nA}", tuple(sizes) + (nA,), fam=fam, **kw))
    cs.append(_c(f"{name}-val", tuple(sizes) + (1,), value=True, fam=fam, **kw))


def _table():
    cs = []
    # instances: all six at M = 65 and M = 1; f16 observations of odd width
    for xdt, dO in (("f32", 4), ("f16", 3)):
        for M in (65, 1):
            cs.append(_c(f"inst-{xdt}-policy-M{M}", (dO, 9, 5), xdt, M=M, fam="inst"))
            cs.append(_c(f"inst-{xdt}-value-M{M}", (dO, 9, 1), xdt, value=True, M=M, fam="inst"))
            cs.append(_c(f"inst-{xdt}-pop-M{M}", (dO, 9, 5), xdt, L=3, M=M, fam="inst"))
    # depth on distinct widths
    widths = (5, 7, 11, 13, 6)
    for n in (1, 2, 3, 4):
        _twin(cs, f"depth-n{n}", widths[:n], 3, "depth", M=33)
    # tiles, with and without rows; rows with repeats and M > n_x
    for M in (1, 31, 32, 33, 65):
        for rows in ("none", "perm"):
            _twin(cs, f"tile-M{M}-{rows}", (6, 10), 4, "tile", M=M, rows=rows)
    _twin(cs, "tile-M65-repeat", (6, 10), 4, "tile", M=65, rows="repeat", n_x=20)
    _twin(cs, "tile-M65-arange", (6, 10), 4, "tile", M=65, rows="arange")
    # chunk edges (the layer in -> out named in the tag), each asserted through launch_shape
    for tag, sizes, nA in (("127x128", (127, 128), 2), ("256x64", (8, 256, 64), 5), ("128x128", (128, 128), 2), ("256x65", (8, 256, 65), 5),
                           ("128x256", (128, 256), 16), ("256x250", (8, 256, 250), 2), ("128-256-256", (128, 256, 256), 16),
                           ("1-256", (1, 256), 16)):
        _twin(cs, f"chunk-{tag}", sizes, nA, "chunk", M=33, act="relu" if tag in ("256x64", "256x250") else "tanh")
    # w_max from the input
    cs.append(_c("wmax-128-8-2", (128, 8, 2), M=33, fam="wmax"))
    cs.append(_c("wmax-128-1", (128, 1), value=True, M=33, fam="wmax"))
    cs.append(_c("wmax-128-8-1", (128, 8, 1), value=True, M=33, fam="wmax"))
    # narrow work: tm * jc below one wavefront
    cs.append(_c("narrow-1-1-1", (1, 1, 1), value=True, M=1, fam="narrow"))
    cs.append(_c("narrow-2-3-2", (2, 3, 2), M=1, fam="narrow"))
    cs.append(_c("narrow-2-3-1", (2, 3, 1), value=True, M=1, fam="narrow"))
    # no bias: on all layers, and on the middle layer only
    for tag, bias in (("all", (False, False, False)), ("mid", (True, False, True))):
        cs.append(_c(f"nobias-{tag}-policy", (4, 9, 7, 3), bias=bias, M=33, fam="nobias"))
        cs.append(_c(f"nobias-{tag}-value", (4, 9, 7, 1), value=True, bias=bias, M=33, fam="nobias"))
        cs.append(_c(f"nobias-{tag}-pop", (4, 9, 7, 3), L=3, bias=bias, M=33, fam="nobias"))
    # activations
    for tag, act, slope in (("identity", "identity", 0.01), ("tanh", "tanh", 0.01), ("relu", "relu", 0.01), ("leaky005", "leaky_relu", 0.05),
                            ("leaky15", "leaky_relu", 1.5)):
        _twin(cs, f"act-{tag}", (5, 12, 9), 3, "act", M=33, act=act, slope=slope)
    # actions
    for nA in (1, 2, 5, 16):
        cs.append(_c(f"actions-{nA}", (4, 9, nA), M=33, fam="actions"))
    cs.append(_c("actions-val", (4, 9, 1), value=True, M=33, fam="actions"))
    # softmax extremes (their value twins are the depth / act cases of the same hidden layers: the last layer alone is rescaled here)
    for data in ("spread50", "spread200", "abs1e4p", "abs1e4m", "tie"):
        cs.append(_c(f"softmax-{data}", (5, 12, 6), M=33, data=data, fam="softmax"))
    cs.append(_c("softmax-twin-val", (5, 12, 1), value=True, M=33, fam="softmax"))
    # exact cases: identity, small integers everywhere
    for n in (1, 2, 3, 4):
        cs.append(_c(f"exact-val-n{n}", widths[:n] + (1,), value=True, act="identity", data="int", M=65, rows="perm", fam="exact"))
    cs.append(_c("exact-val-3chunk", (128, 256, 1), value=True, act="identity", data="int", M=33, rows="repeat", n_x=12, fam="exact"))
    cs.append(_c("exact-val-f16", (3, 7, 1), "f16", value=True, act="identity", data="int", M=65, rows="perm", fam="exact"))
    cs.append(_c("exact-pop-nA1", (128, 256, 1), L=3, act="identity", data="int", M=33, rows="repeat", n_x=12, fam="exact"))
    cs.append(_c("exact-pop-nA1-f16", (3, 7, 1), "f16", L=3, act="identity", data="int", M=33, fam="exact"))
    # rows outside [0, n_x): NaN rows among valid ones, under every activation
    for act in ("tanh", "relu", "leaky_relu", "identity"):
        cs.append(_c(f"oob-policy-{act}", (4, 9, 5), act=act, slope=0.05, M=40, rows="oob", n_x=17, fam="oob"))
        cs.append(_c(f"oob-value-{act}", (4, 9, 1), value=True, act=act, slope=0.05, M=40, rows="oob", n_x=17, fam="oob"))
    cs.append(_c("oob-pop-f16", (3, 9, 5), "f16", L=3, M=40, rows="oob", n_x=17, fam="oob"))
    # LDS on both sides of 64 KiB, and the maximum
    below, above = lds_edges()
    cs.append(_c("lds-below", below, M=33, fam="lds"))
    cs.append(_c("lds-above", above, M=33, fam="lds"))
    cs.append(_c("lds-below-val", below[:2] + (1,), value=True, M=33, fam="lds"))
    cs.append(_c("lds-above-val", above[:2] + (1,), value=True, M=33, fam="lds"))
    cs.append(_c("lds-max", (128, 256, 256, 16), "f16", M=33, fam="lds"))
    cs.append(_c("lds-max-val", (128, 256, 256, 1), "f16", value=True, M=33, fam="lds"))
    # population: three learners, a learner stride M * nA that is no multiple of the tile, a chunked hidden layer
    for xdt in ("f32", "f16"):
        for tag, bias in (("bias", (True, True)), ("nobias", (False, False))):
            cs.append(_c(f"pop-{xdt}-{tag}", (128, 128, 5), xdt, L=3, M=33, rows="perm", bias=bias, fam="pop"))
    cs.append(_c("pop-f32-bias-val", (128, 128, 1), value=True, M=33, rows="perm", fam="pop"))
    for i, c in enumerate(cs):
        c.seed = SEEDS.get(c.name, 5000 + i)
    names = [c.name for c in cs]
    assert len(set(names)) == len(names) and set(SEEDS) <= set(names)
    return cs


def np_dtype(c):
    return np.float16 if c.xdt == "f16" else np.float32


def make_inputs(c):
    """x [n_x, dO], rows [M] i32 or None, and per learner [(W, b or None)]: standard normal x times 2, W over sqrt(fan_in), biases 0.5 N(0, 1)
    (different per unit); `int` data: integers in [-3, 3], [-2, 2] and [-4, 4]"""
    g = np.random.default_rng(c.seed)
    ints = c.data.startswith("int")
    dO = c.sizes[0]
    if ints:
        x = g.integers(-3, 4, (c.n_x, dO)).astype(np.float32)
    else:
        x = (2.0 * g.standard_normal((c.n_x, dO))).astype(np.float32)
    x = x.astype(np_dtype(c))
    weights = []
    for _ in range(max(c.L, 1)):
        layers = []
        for l, (i, o) in enumerate(zip(c.sizes, c.sizes[1:])):
            if ints:
                W, b = g.integers(-2, 3, (o, i)).astype(np.float32), g.integers(-4, 5, o).astype(np.float32)
            else:
                W, b = (g.standard_normal((o, i)) / np.sqrt(i)).astype(np.float32), (0.5 * g.standard_normal(o)).astype(np.float32)
            layers.append((W, b if c.bias[l] else None))
        weights.append(layers)
    rows = None
    if c.rows == "arange":
        rows = np.arange(c.M, dtype=np.int32)
    elif c.rows == "perm":
        assert c.n_x == c.M
        rows = g.permutation(c.M).astype(np.int32)
    elif c.rows in ("repeat", "oob"):
        assert c.M > c.n_x
        rows = g.integers(0, c.n_x, c.M).astype(np.int32)
        if c.rows == "oob":
            rows[[1, c.M // 2, c.M - 1]] = (-1, c.n_x, INT32_MAX)
            rows[33] = -(2 ** 31)  # in the second tile
    else:
        assert c.n_x == c.M
    if c.data in ("spread50", "spread200", "abs1e4p", "abs1e4m", "tie"):
        xg = x.astype(np.float64)
        for layers in weights:
            W, b = layers[-1]
            if c.data == "tie":
                W[1], b[1] = W[0], b[0]
                b[:2] += np.float32(1.0)
            elif c.data.startswith("spread"):
                z = forward_f64(xg, layers, c.act, c.slope, False)[0]
                s = np.float32(float(c.data[6:]) / np.median(z.max(axis=1) - z.min(axis=1)))
                W *= s
                b *= s
            else:
                b += np.float32(1e4 if c.data == "abs1e4p" else -1e4)
    return x, rows, weights


@functools.lru_cache(maxsize=None)
def build(name):
    """inputs, the gathered observations, and per learner the f64 logits, outputs and bound of a case"""
    c = CASES[name]
    x, rows, weights = make_inputs(c)
    src = np.arange(c.M, dtype=np.int64) if rows is None else rows.astype(np.int64)
    valid = (src >= 0) & (src < c.n_x)
    xg = np.zeros((c.M, c.sizes[0]), np.float64)
    xg[valid] = x.astype(np.float64)[src[valid]]
    logits, ref, bound, pres = [], [], [], []
    for layers in weights:
        z, o, bd, pr = forward_f64(xg, layers, c.act, c.slope, c.value)
        logits.append(z), ref.append(o), bound.append(bd), pres.append(pr)
    for a in [x, xg, valid] + ([rows] if rows is not None else []) + logits + ref + bound + [w for ls in weights for wb in ls for w in wb if w is not None]:
        a.setflags(write=False)
    return SimpleNamespace(case=c, x=x, rows=rows, weights=weights, xg=xg, valid=valid, logits=logits, ref=ref, bound=bound, pres=pres,
                           shape=launch_shape(c.sizes))


CASE_LIST = _table()
CASES = {c.name: c for c in CASE_LIST}

# the case each mutant of emulate_f32 must show on (tests/test_policy_mlp_matrix_host.py: at least 4/3 of the bound), and the learner it reads
MUTANT_CASE = {
    "drop_product": ("depth-n3-val", 0),
    "drop_bias": ("depth-n3-val", 0),
    "chunk_bias_shift": ("chunk-128x256-val", 0),
    "skip_ragged_last": ("chunk-256x65-val", 0),
    "wrong_pingpong": ("depth-n4-val", 0),
    "softmax_no_max": ("softmax-abs1e4p", 0),
    "leaky_wrong_side": ("act-leaky005-val", 0),
    "pop_bias0": ("pop-f32-bias", 1),
}
