"""The cases of the offsim_encode_mlp matrix (tests/test_gpu_encoder_matrix.py on the device, tests/test_encoder_matrix_host.py for what needs
none): the dispatcher's rule restated (csrc/offsim_hip.hip: launch_mlp_mfma, offsim_encode_mlp), a NumPy f64 forward, the scale rounding error
is measured on, a NumPy emulation of the bf16 x 3 kernel (csrc/encode_mfma.hpp: k_encode_mlp_mfma_split), and the tolerance.

Paths: S = k_encode_mlp_mfma_split (bf16 x 3, the default of its shapes), R = k_encode_mlp_mfma_reg (the same shapes under
OFFSIM_ENCODER_F32=1), G = k_encode_mlp_mfma (weights in LDS), V = k_encode_mlp (VALU).

The tolerance of a case: |gpu - f64| <= (4 max(rho_ref, 2^-24) + s 2^-22) B elementwise, where B is the sum of absolute terms of a logit
(magnitude_f64), rho_ref = max |oracle f32 forward - f64| / B on the case's own inputs, and s = 1 on path S only: the products the split drops
on purpose (m l, l m, l l) are below 2^-23 of each term per layer, over two layers.  The factor 4 is a margin for another order of summation.

A case is built once per process and then only read."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SLOPE = np.float32(0.01)
F32_PRODUCTS = False
try:  # the dispatcher's own reading of the switch: atoi(getenv) != 0, once per process
    F32_PRODUCTS = int(os.environ.get("OFFSIM_ENCODER_F32", "0").strip() or "0") != 0
except ValueError:
    F32_PRODUCTS = False

MAX_H = 128
LDS_LIMIT, LDS_DEFAULT = 160 * 1024, 64 * 1024
REG_SHAPES = {(128, 1): 1, (128, 2): 1, (2, 1): 2, (2, 2): 2, (4, 1): 2, (4, 2): 2}  # (dO, ZT) -> WPE at HT = 2
G_TILES = ((1, 1), (2, 1), (2, 2), (1, 2), (4, 1), (4, 2))


# ---- the dispatcher's rule ----
def dispatch(dO, H, nZ, aligned=True, f32_products=False):
    """(path, instance, LDS bytes) a call takes: path in S / R / G / V, or "refused"."""
    if H > MAX_H:
        return "refused", None, 0
    HT, ZT = (H + 31) // 32, (nZ + 31) // 32
    if HT == 2 and aligned and (dO, ZT) in REG_SHAPES:
        return ("R" if f32_products else "S"), (dO, ZT), 0
    dOp = (dO + 1) & ~1
    lds = 4 * (HT * 32 * (dOp + 1) + ZT * 32 * (HT * 32 + 1) + HT * 32 + ZT * 32)
    if lds > LDS_LIMIT:
        return "refused", None, lds
    if (HT, ZT) in G_TILES:
        return "G", (HT, ZT), lds
    lds = 4 * (H * dO + H + nZ * H + nZ)
    if lds > LDS_LIMIT:
        return "refused", None, lds
    return "V", (), lds


def sweep_rows(path, inst):
    """rows one pass of the whole grid covers: a larger N sends wavefronts round the grid-stride loop"""
    if path in ("S", "R"):
        dO, _ = inst
        item_pf = 1 if dO == 128 else 2  # PF = 1 where a lane's share of a row is >= 64 bytes (both dtypes at dO = 128), else 2
        return 256 * REG_SHAPES[inst] * 4 * 32 * item_pf
    return 1024 * 4 * 32 if path == "G" else 2048 * 256


# ---- references ----
def _leaky64(v):
    return np.where(v > 0, v, np.float64(SLOPE) * v)


def forward_f64(x, W1, b1, W2, b2):
    """the logits in float64 of exactly the f32 / f16 values handed to the kernel"""
    x, W1, b1, W2, b2 = (np.asarray(a).astype(np.float64) for a in (x, W1, b1, W2, b2))
    return _leaky64(x @ W1.T + b1) @ W2.T + b2


def magnitude_f64(x, W1, b1, W2, b2):
    """B = |W2| leaky(|W1| |x| + |b1|) + |b2| per logit: the sum of absolute terms"""
    x, W1, b1, W2, b2 = (np.abs(np.asarray(a).astype(np.float64)) for a in (x, W1, b1, W2, b2))
    return _leaky64(x @ W1.T + b1) @ W2.T + b2


def trunc_bf16(v):
    """enc_trunc_bf16: the f32 word with its low half cleared"""
    v = np.ascontiguousarray(v, np.float32)
    return (v.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def split3(v):
    """enc_split3: v = h + m + l exactly, each part a bf16 value held in f32"""
    v = np.ascontiguousarray(v, np.float32)
    h = trunc_bf16(v)
    r = v - h
    m = trunc_bf16(r)
    return {"h": h, "m": m, "l": trunc_bf16(r - m)}


def layer1_is_split(dO, x_dtype):
    """L1_SPLIT of k_encode_mlp_mfma_split: a lane's half row is whole groups of eight elements and whole 16-byte words"""
    half = ((dO + 1) & ~1) // 2
    return half % 8 == 0 and (half * np.dtype(x_dtype).itemsize) % 16 == 0


# (weight part, operand part) in the kernel's order of accumulation, smallest first; the three left out are m l, l m, l l
L1_PRODUCTS = (("h", "l"), ("l", "h"), ("m", "m"), ("h", "m"), ("m", "h"), ("h", "h"))
L2_PRODUCTS = (("l", "h"), ("h", "l"), ("m", "m"), ("m", "h"), ("h", "m"), ("h", "h"))


def kept_products(dO, x_dtype):
    """{layer: products} path S forms.  Narrow observations (dO = 2, 4) run layer 1 on exact f32 products; an fp16 observation is two bf16
    parts, so its l part does not exist and h l is not formed."""
    l1 = ()
    if layer1_is_split(dO, x_dtype):
        l1 = tuple(p for p in L1_PRODUCTS if not (np.dtype(x_dtype) == np.float16 and p[1] == "l"))
    return {1: l1, 2: L2_PRODUCTS}


def split3_emulated(x, W1, b1, W2, b2, drop=None):
    """path S in NumPy: bf16 parts by truncation, the kept partial products each accumulated in f32 from the bias, the hidden layer split
    again before layer 2.  drop = (layer, (weight part, operand part)) leaves one kept product out."""
    x = np.asarray(x)
    W1, b1, W2, b2 = (np.ascontiguousarray(a, np.float32) for a in (W1, b1, W2, b2))
    kept = kept_products(x.shape[1], x.dtype)
    xf = x.astype(np.float32)
    acc = np.broadcast_to(b1, (x.shape[0], W1.shape[0])).astype(np.float32)
    if kept[1]:
        xp, wp = split3(xf), split3(W1)
        for (pw, px) in kept[1]:
            if drop != (1, (pw, px)):
                acc = acc + xp[px] @ wp[pw].T
    else:
        assert drop is None or drop[0] != 1
        acc = acc + xf @ W1.T
    hid = np.maximum(acc, SLOPE * acc)
    hp, wp = split3(hid), split3(W2)
    acc = np.broadcast_to(b2, (x.shape[0], W2.shape[0])).astype(np.float32)
    for (pw, ph) in kept[2]:
        if drop != (2, (pw, ph)):
            acc = acc + hp[ph] @ wp[pw].T
    assert acc.dtype == np.float32
    return acc


def droppable(case):
    """every (layer, product) whose loss must show on an S case"""
    kept = kept_products(case.dO, np.float16 if case.xdt == "f16" else np.float32)
    return [(layer, p) for layer in (1, 2) for p in kept[layer]]


# ---- the case table ----
def _c(path, inst, N, dO, H, nZ, xdt, seed=0, kind="normal", scale=1.0, unaligned=False, tag=""):
    name = f"{path}-{xdt}-d{dO}-H{H}-z{nZ}-N{N}" + (f"-{tag}" if tag else "")
    return SimpleNamespace(name=name, path=path, inst=inst, N=N, dO=dO, H=H, nZ=nZ, xdt=xdt, seed=seed, kind=kind, scale=scale,
                           unaligned=unaligned)


# Seeds that are not the case's number.  The tolerance is far above what a correct bf16 x 3 forward needs (its emulation uses a few percent of it),
# and the two smallest kept products (h l, l h: about 2^-17 of a term, one-sided) reach it only through the maximum over many logits: with
# the default seed these cases left one of them between 0.5 and 1.2 times the tolerance, too close for a check that has to hold on another
# BLAS.  They were searched for a seed at which every lost product exceeds the tolerance by at least a third; the two one-row cases have 25
# and 50 logits in all, and the best of 3000 seeds gives them 1.09 and 1.15 (tests/test_encoder_matrix_host.py).
SEEDS = {
    "S-f32-d128-H64-z25-N1": 1207000,
    "S-f32-d128-H64-z25-N33": 115002,
    "S-f32-d128-H64-z25-N65": 149003,
    "S-f32-d128-H64-z50-N1": 2699005,
    "S-f32-d128-H64-z50-N31": 26006,
    "S-f32-d128-H64-z50-N33": 22007,
    "S-f16-d128-H64-z1-N129": 3062,
    "S-f32-d128-H64-z33-N129": 8063,
}


def _table():
    cs = []
    # S (R under OFFSIM_ENCODER_F32=1): the 12 instances; 65 rows leave the second tile of a PF = 2 group partial, 33 start it past the end
    for xdt, (z1, z2) in (("f32", (25, 50)), ("f16", (32, 64))):
        for dO in (128, 2, 4):
            for nZ in (z1, z2):
                for N in (1, 31, 33, 65, 129):
                    cs.append(_c("S", (dO, (nZ + 31) // 32), N, dO, 64, nZ, xdt))
    for i, dO in enumerate((128, 2, 4)):
        xa, xb = ("f32", "f16") if i % 2 == 0 else ("f16", "f32")
        cs += [_c("S", (dO, 1), 129, dO, 33, 25, xa), _c("S", (dO, 2), 129, dO, 50, 50, xb),
               _c("S", (dO, 1), 129, dO, 64, 1, xb), _c("S", (dO, 2), 129, dO, 64, 33, xa)]
    cs += [_c("S", (4, 1), 129, 4, 64, 25, "f32", kind="zero_rows", tag="zerorows"),
           _c("S", (128, 2), 129, 128, 64, 50, "f32", scale=2.0 ** 20, tag="x2p20"),
           _c("S", (128, 2), 129, 128, 64, 50, "f32", scale=2.0 ** -20, tag="x2m20")]
    # the grid-stride loop: N = 2 sweeps + 32 + 7
    for xdt in ("f32", "f16"):
        cs += [_c("S", (128, 2), 2 * 32768 + 39, 128, 64, 50, xdt, tag="stride"),
               _c("S", (2, 1), 2 * 131072 + 39, 2, 64, 25, xdt, tag="stride"),
               _c("S", (4, 2 if xdt == "f32" else 1), 2 * 131072 + 39, 4, 64, 50 if xdt == "f32" else 25, xdt, tag="stride"),
               _c("G", (1, 1), 2 * 131072 + 39, 3, 32 if xdt == "f32" else 20, 10, xdt, tag="stride"),
               _c("V", (), 2 * 524288 + 39, 4, 96, 5, xdt, tag="stride")]
    # G: every (HT, ZT) with both dtypes; dO odd, even and 1 (the whole hi = 1 lane half has k >= dO); tiles filled and partial
    cs += [_c("G", (1, 1), 129, 3, 16, 10, "f32"), _c("G", (1, 1), 97, 1, 32, 32, "f16"),
           _c("G", (2, 1), 129, 8, 64, 25, "f32"), _c("G", (2, 1), 129, 3, 50, 32, "f16"),
           _c("G", (2, 2), 129, 7, 33, 33, "f32"), _c("G", (2, 2), 129, 8, 64, 64, "f16"),
           _c("G", (1, 2), 129, 1, 32, 64, "f32"), _c("G", (1, 2), 129, 7, 20, 50, "f16"),
           _c("G", (4, 1), 129, 7, 128, 25, "f32"), _c("G", (4, 1), 129, 3, 97, 32, "f16"),
           _c("G", (4, 2), 129, 3, 128, 33, "f32"), _c("G", (4, 2), 129, 8, 100, 50, "f16"),
           _c("G", (4, 2), 129, 128, 128, 64, "f32", tag="biglds"),
           _c("G", (2, 1), 129, 1, 64, 5, "f16"), _c("G", (1, 1), 1, 7, 32, 1, "f32"),
           _c("G", (2, 2), 129, 8, 64, 50, "f32", kind="neg_hidden", tag="neghid"),
           _c("G", (2, 1), 129, 3, 64, 25, "f16", kind="zero_rows", tag="zerorows"),
           _c("G", (2, 2), 129, 8, 64, 50, "f32", scale=2.0 ** 20, tag="x2p20"),
           _c("G", (2, 2), 129, 8, 64, 50, "f32", scale=2.0 ** -20, tag="x2m20")]
    # G at HT = 2 by an x that is not 16-byte aligned, on the shapes S / R would take
    cs += [_c("G", (2, 1), 129, 2, 64, 25, "f32", unaligned=True, tag="unaligned"),
           _c("G", (2, 2), 65, 4, 64, 50, "f16", unaligned=True, tag="unaligned"),
           _c("G", (2, 2), 129, 128, 64, 50, "f32", unaligned=True, tag="unaligned"),
           _c("G", (2, 1), 33, 128, 64, 25, "f16", unaligned=True, tag="unaligned")]
    # V: HT = 3 or nZ > 64; 300 rows are more than one workgroup
    for xdt in ("f32", "f16"):
        cs += [_c("V", (), 300, 4, 96, 5, xdt), _c("V", (), 129, 7, 128, 65, xdt), _c("V", (), 129, 128, 80, 100, xdt)]
    for i, c in enumerate(cs):
        c.seed = SEEDS.get(c.name, 1000 + i)
    assert set(SEEDS) <= {c.name for c in cs}
    names = [c.name for c in cs]
    assert len(set(names)) == len(names)
    return cs


CASE_LIST = _table()
CASES = {c.name: c for c in CASE_LIST}


def taken_path(case, f32_products=None):
    """The path the case runs in this process.  THE place that decides: the dispatcher's rule applied to the case's shape and alignment must
    give the path and instance the case is listed under; a case that would land elsewhere fails here."""
    f32p = F32_PRODUCTS if f32_products is None else f32_products
    path, inst, lds = dispatch(case.dO, case.H, case.nZ, aligned=not case.unaligned, f32_products=f32p)
    want = "R" if (case.path == "S" and f32p) else case.path
    assert (path, inst) == (want, case.inst), (case.name, path, inst)
    return path, inst, lds


def np_dtype(case):
    return np.float16 if case.xdt == "f16" else np.float32


def make_inputs(case):
    """x standard normal (times the case's scale), W over sqrt(fan_in), b1 small so that about half the hidden units take the leaky branch"""
    g = np.random.default_rng(case.seed)
    N, dO, H, nZ = case.N, case.dO, case.H, case.nZ
    x = g.standard_normal((N, dO)).astype(np.float32) * np.float32(case.scale)
    W1 = (g.standard_normal((H, dO)) / np.sqrt(dO)).astype(np.float32)
    b1 = (0.1 * g.standard_normal(H)).astype(np.float32)
    W2 = (g.standard_normal((nZ, H)) / np.sqrt(H)).astype(np.float32)
    b2 = (0.1 * g.standard_normal(nZ)).astype(np.float32)
    if case.scale != 1.0:  # the biases go along, so that every term of B scales and the case is the unscaled one at another exponent
        b1, b2 = b1 * np.float32(case.scale), b2 * np.float32(case.scale)
    if case.kind == "neg_hidden":
        b1 = (b1 - np.float32(10.0)).astype(np.float32)
    if case.kind == "zero_rows":
        x[[0, 5, N - 1]] = 0.0
    if case.xdt == "f16":
        x = x.astype(np.float16)
        flat = x.reshape(-1)
        specials = np.array([2.0 ** -24, -3 * 2.0 ** -24, 2.0 ** -15, 65504.0, -65504.0], np.float16)  # subnormals and the largest finite
        if flat.size >= 2 * specials.size:
            flat[g.choice(flat.size, specials.size, replace=False)] = specials
        else:
            flat[-1] = specials[flat.size % specials.size]
    return x, W1, b1, W2, b2


@functools.lru_cache(maxsize=None)
def build(name):
    """inputs, f64 logits, B, rho_ref and both tolerances of a case"""
    from oracle import oracle as O
    c = CASES[name]
    x, W1, b1, W2, b2 = make_inputs(c)
    ref = forward_f64(x, W1, b1, W2, b2)
    B = magnitude_f64(x, W1, b1, W2, b2)
    _, lo = O.mlp_encode(x.astype(np.float32), W1, b1, W2, b2)
    rho_ref = float((np.abs(lo.astype(np.float64) - ref) / B).max())
    base = 4.0 * max(rho_ref, 2.0 ** -24)
    for a in (x, W1, b1, W2, b2, ref, B, lo):
        a.setflags(write=False)
    return SimpleNamespace(case=c, x=x, W1=W1, b1=b1, W2=W2, b2=b2, ref=ref, B=B, oracle=lo, rho_ref=rho_ref,
                           tol_f32=base, tol_split=base + 2.0 ** -22)


def tolerance(b, path):
    return b.tol_split if path == "S" else b.tol_f32


def first_argmax(logits):
    return np.argmax(logits, axis=1)  # NumPy's argmax is the first maximal index


def clear_rows(b, tol):
    """rows whose f64 top-2 gap exceeds 2 tol times the B of those two logits: there every in-tolerance forward has the f64 argmax"""
    if b.case.nZ == 1:
        return np.ones(b.case.N, bool)
    order = np.argsort(-b.ref, axis=1, kind="stable")[:, :2]
    rows = np.arange(b.case.N)
    top, second = b.ref[rows, order[:, 0]], b.ref[rows, order[:, 1]]
    return (top - second) > 2.0 * tol * np.maximum(b.B[rows, order[:, 0]], b.B[rows, order[:, 1]])
