"""What the k_policy_mlp matrix (tests/test_gpu_policy_mlp_matrix.py) rests on, checked without a device: the case table of
tests/policy_mlp_host.py reaches every chunk, tile, depth, LDS and population edge it claims (asserted from launch_shape, the cases' data
and the f64 pre-activations), the C ABI's validation that comes before any HIP call, and the bound tells a wrong kernel from a right one:
the NumPy f32 emulation of the kernel's arithmetic stays below half of it on every case, and every mutant of the emulation exceeds it by
at least a third on its named case."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_mlp_host as P  # noqa: E402

ALL = [c.name for c in P.CASE_LIST]


def _chunks(name):
    return P.launch_shape(P.CASES[name].sizes).chunks


def test_launch_shape_on_named_networks():
    s = P.launch_shape((127, 128, 2))
    assert s.w_floats == 16384 and s.chunks[0] == [128] and s.jc_max[0] == 128
    s = P.launch_shape((8, 256, 64, 5))
    assert s.w_floats == 16448 == P.W_FLOATS_CAP and s.chunks[1] == [64] and s.jc_max[1] == 64
    assert P.launch_shape((128, 128, 2)).chunks[0] == [127, 1]
    assert P.launch_shape((8, 256, 65, 5)).chunks[1] == [64, 1]
    assert P.launch_shape((128, 256, 16)).chunks[0] == [127, 127, 2]
    assert P.launch_shape((8, 256, 250, 2)).chunks[1] == [64, 64, 64, 58]
    s = P.launch_shape((128, 256, 256, 16))
    assert s.jc_max == [127, 64, 64] and s.chunks[0] == [127, 127, 2] and s.chunks[1] == [64] * 4 and s.chunks[2] == [16]
    assert s.w_max == 256 and s.lds_bytes == 131584 and s.big_lds
    s = P.launch_shape((1, 256, 16))
    assert s.w_floats == 16 * 257 < P.W_FLOATS_CAP and s.w_floats > 256 * 2 and s.chunks == [[256], [16]]
    s = P.launch_shape((128, 8, 2))
    assert s.w_max == 128 and s.ld == 129 and s.lds_bytes == 4 * (64 * 129 + 8 * 129)
    assert P.launch_shape((128, 1)).w_max == 128 and P.launch_shape((1, 1, 1)).lds_bytes == 4 * (64 * 2 + 2)


def test_cases_hold_their_edges():
    C = P.CASES
    # instances: all six at M = 65 and M = 1, the f16 ones on an odd width
    for inst in ("f32-policy", "f16-policy", "f32-value", "f16-value", "f32-pop", "f16-pop"):
        for M in (65, 1):
            c = C[f"inst-{inst}-M{M}"]
            assert c.inst == inst and c.M == M and (c.xdt == "f32" or c.sizes[0] == 3)
    assert {c.inst for c in P.CASE_LIST} == {"f32-policy", "f16-policy", "f32-value", "f16-value", "f32-pop", "f16-pop"}
    # depth 1..4 on widths that differ per layer, policy and value
    for n in (1, 2, 3, 4):
        for c in (C[f"depth-n{n}-pol3"], C[f"depth-n{n}-val"], C[f"exact-val-n{n}"]):
            assert len(c.sizes) == n + 1 and len(set(c.sizes)) == n + 1
        assert C[f"depth-n{n}-val"].value and not C[f"depth-n{n}-pol3"].value
    assert C["depth-n4-pol3"].sizes == (5, 7, 11, 13, 3)
    # tiles
    for M in (1, 31, 32, 33, 65):
        for rows in ("none", "perm"):
            for kind in ("pol4", "val"):
                c = C[f"tile-M{M}-{rows}-{kind}"]
                assert c.M == M and (P.build(c.name).rows is None) == (rows == "none")
    b = P.build("tile-M65-repeat-pol4")
    assert b.case.M > b.case.n_x and len(set(b.rows.tolist())) < b.case.M and b.valid.all()
    assert np.array_equal(P.build("tile-M65-arange-val").rows, np.arange(65))
    # chunk edges, each with biases that differ per unit
    want = {"chunk-127x128": (0, [128]), "chunk-256x64": (1, [64]), "chunk-128x128": (0, [127, 1]), "chunk-256x65": (1, [64, 1]),
            "chunk-128x256": (0, [127, 127, 2]), "chunk-256x250": (1, [64, 64, 64, 58])}
    for stem, (layer, chunks) in want.items():
        for name in (n for n in ALL if n.startswith(stem + "-")):
            assert _chunks(name)[layer] == chunks, name
            bias = P.build(name).weights[0][layer][1]
            assert len(set(bias.tolist())) == len(bias), name
    assert P.launch_shape(C["chunk-127x128-val"].sizes).w_floats == 16384
    assert P.launch_shape(C["chunk-256x64-val"].sizes).w_floats == 16448
    for name in ("chunk-128-256-256-pol16", "chunk-128-256-256-val", "lds-max", "lds-max-val"):
        s = P.launch_shape(C[name].sizes)
        assert len(s.chunks[0]) == 3 and len(s.chunks[1]) == 4 and s.jc_max[0] != s.jc_max[1], name
    s = P.launch_shape(C["chunk-1-256-pol16"].sizes)
    assert s.w_floats < P.W_FLOATS_CAP and s.w_floats == 16 * 257 and s.w_floats > 256 * 2  # set by the last layer
    # w_max from the input; narrow work
    for name in ("wmax-128-8-2", "wmax-128-1", "wmax-128-8-1"):
        assert P.launch_shape(C[name].sizes).w_max == C[name].sizes[0] == 128 and max(C[name].sizes[1:]) < 128
    for name in ("narrow-1-1-1", "narrow-2-3-2", "narrow-2-3-1"):
        c = C[name]
        assert c.M == 1 and all(c.M * jc < 64 for ch in P.launch_shape(c.sizes).chunks for jc in ch)
    # no bias
    for kind in ("policy", "value", "pop"):
        assert all(b is None for _, b in P.build(f"nobias-all-{kind}").weights[0])
        mid = P.build(f"nobias-mid-{kind}").weights[-1]
        assert [b is None for _, b in mid] == [False, True, False]
    assert C["nobias-all-pop"].L == 3 and C["nobias-mid-pop"].L == 3
    # activations: all four, both leaky slopes, both signs before every activation
    assert {(c.act, c.slope) for c in P.CASE_LIST if c.fam == "act"} == {("identity", 0.01), ("tanh", 0.01), ("relu", 0.01), ("leaky_relu", 0.05),
                                                                         ("leaky_relu", 1.5)}
    for c in P.CASE_LIST:
        if c.fam == "act":
            for pre in P.build(c.name).pres[0][:-1]:
                assert ((pre > 0).any(axis=0) & (pre < 0).any(axis=0)).all(), c.name  # every unit sees both
    # actions
    assert [C[f"actions-{nA}"].sizes[-1] for nA in (1, 2, 5, 16)] == [1, 2, 5, 16] and not C["actions-1"].value
    assert (P.build("actions-1").ref[0] == 1.0).all()
    # softmax extremes
    for name, lo, hi in (("softmax-spread50", 35, 70), ("softmax-spread200", 140, 280)):
        z = P.build(name).logits[0]
        spread = z.max(axis=1) - z.min(axis=1)
        assert lo < np.median(spread) < hi and np.isfinite(P.build(name).ref[0]).all(), (name, np.median(spread))
    p = P.build("softmax-spread200").ref[0]
    assert (p < 2.0 ** -149).any() and (P.build("softmax-spread50").ref[0] < 1e-15).any()  # tails below the smallest f32 / far below u
    assert (P.build("softmax-abs1e4p").logits[0] > 9.9e3).all() and (P.build("softmax-abs1e4m").logits[0] < -9.9e3).all()
    with np.errstate(over="ignore", invalid="ignore"):
        for name in ("softmax-abs1e4p", "softmax-abs1e4m"):  # without the max subtraction: inf / inf and 0 / 0
            e = np.exp(P.build(name).logits[0].astype(np.float32))
            assert np.isnan(e / e.sum(axis=1, keepdims=True)).all()
    z = P.build("softmax-tie").logits[0]
    assert (z[:, 0] == z[:, 1]).all() and ((z[:, 0] == z.max(axis=1)).sum() >= 1)
    # exact cases: integers everywhere, every partial sum below 2^24 (the sum of absolute terms bounds each)
    for c in P.CASE_LIST:
        if c.fam != "exact":
            continue
        b = P.build(c.name)
        assert c.act == "identity" and (b.x.astype(np.float64) == np.rint(b.x)).all()
        for layers, z in zip(b.weights, b.logits):
            mag = np.abs(b.xg)
            for W, bias in layers:
                assert (W == np.rint(W)).all() and (bias == np.rint(bias)).all()
                mag = mag @ np.abs(W.astype(np.float64)).T + np.abs(bias)
            assert mag.max() < 2 ** 24 and (z == np.rint(z)).all() and np.abs(z).max() > 10, c.name
    assert len(_chunks("exact-val-3chunk")[0]) == 3 and len(_chunks("exact-pop-nA1")[0]) == 3
    assert C["exact-val-f16"].xdt == "f16" and C["exact-pop-nA1-f16"].xdt == "f16" and C["exact-pop-nA1"].sizes[-1] == 1
    assert not np.array_equal(P.build("exact-pop-nA1").logits[1], P.build("exact-pop-nA1").logits[2])
    # rows outside [0, n_x)
    for c in P.CASE_LIST:
        if c.fam == "oob":
            b = P.build(c.name)
            bad = set(b.rows[~b.valid].tolist())
            assert bad == {-1, c.n_x, P.INT32_MAX, -2 ** 31} and b.valid.sum() == c.M - 4 and not b.valid[33] and not b.valid[1]
    assert {c.act for c in P.CASE_LIST if c.fam == "oob"} == set(P.ACT)
    # LDS: the nearest networks on either side of 64 KiB, and the maximum
    below, above = P.lds_edges()
    lb, la = P.launch_shape(below).lds_bytes, P.launch_shape(above).lds_bytes
    assert C["lds-below"].sizes == below and C["lds-above"].sizes == above and lb <= P.LDS_DEFAULT < la
    assert not P.launch_shape(below).big_lds and P.launch_shape(above).big_lds
    for dO in (1, 2, 55, 112, 128):  # the search against launch_shape itself on some columns
        for H in range(1, 257):
            for nA in (1, 5, 16):
                v = P.launch_shape((dO, H, nA)).lds_bytes
                assert v <= lb or v >= la, (dO, H, nA)
    assert lb == 65536 and la == 65540
    assert P.launch_shape(C["lds-max"].sizes).lds_bytes == 131584 == 4 * (64 * 257 + 16448)
    # population: three learners with different weights, 33 rows, a chunked hidden layer, both dtypes, with and without bias
    for xdt in ("f32", "f16"):
        for tag in ("bias", "nobias"):
            c = C[f"pop-{xdt}-{tag}"]
            b = P.build(c.name)
            assert c.L == 3 and c.M == 33 and (c.M * c.sizes[-1]) % P.TM != 0 and len(b.shape.chunks[0]) == 2 and c.xdt == xdt
            assert all((bias is None) == (tag == "nobias") for _, bias in b.weights[0])
            assert not np.array_equal(b.weights[0][0][0], b.weights[1][0][0]) and np.abs(b.ref[0] - b.ref[2]).max() > 1e-3
    # every policy family has a value twin
    for fam in {c.fam for c in P.CASE_LIST}:
        assert any(c.value for c in P.CASE_LIST if c.fam == fam), fam


def _layers(sizes, b=0x1000):
    from rl_offline_simulation_amd import _lib as L
    arr = (L.MLPLayer * (len(sizes) - 1))()
    for i in range(len(sizes) - 1):
        arr[i].W, arr[i].b, arr[i].out = 0x1000, b, sizes[i + 1]
        setattr(arr[i], "in", sizes[i])
    return arr


def test_validation_before_any_hip_call():
    from rl_offline_simulation_amd import _lib as L
    lib = L.load()
    ok = _layers([4, 8, 3])

    def pop(n_pop, M=0, x=0x1000, out=0x1000, layers=ok, n=2):
        return lib.offsim_policy_mlp_pop(x, L.F32, 10, 4, None, M, layers, n, L.ACT_TANH, 0.01, n_pop, out, None)
    assert pop(0) == L.EINVAL and b"L must be 1..65535" in lib.offsim_last_error()
    assert pop(65536) == L.EINVAL and b"policy_mlp_pop" in lib.offsim_last_error()
    assert pop(-1) == L.EINVAL
    assert pop(1) == L.OK and pop(65535) == L.OK  # M = 0: nothing launched
    assert pop(3, M=0, x=None, out=None) == L.OK
    assert pop(3, M=-1) == L.EINVAL and b"bad argument" in lib.offsim_last_error()
    assert pop(3, M=5, x=None) == L.EINVAL and pop(3, M=5, out=None) == L.EINVAL
    assert pop(3, layers=_layers([4, 257, 3])) == L.EINVAL and pop(3, layers=_layers([4, 8, 17])) == L.EINVAL
    assert pop(3, layers=_layers([4, 8, 3], b=None)) == L.OK  # no bias is a network
    for entry, sizes in ((lib.offsim_policy_mlp, [4, 8, 3]), (lib.offsim_value_mlp, [4, 8, 1])):
        ly = _layers(sizes)
        assert entry(None, L.F16, 10, 4, None, 0, ly, 2, L.ACT_RELU, 0.0, None, None) == L.OK  # M = 0 with NULL buffers
        assert entry(0x1000, L.F32, 10, 4, None, -1, ly, 2, L.ACT_RELU, 0.0, 0x1000, None) == L.EINVAL
        assert entry(0x1000, L.F32, -1, 4, None, 0, ly, 2, L.ACT_RELU, 0.0, 0x1000, None) == L.EINVAL
        assert entry(0x1000, L.F32, 10, 4, None, 0, ly, 5, L.ACT_RELU, 0.0, 0x1000, None) == L.EINVAL
        assert entry(0x1000, L.F32, 10, 4, None, 0, ly, 2, 4, 0.0, 0x1000, None) == L.EINVAL and b"activation" in lib.offsim_last_error()
        assert entry(0x1000, L.F32, 10, 129, None, 0, _layers([129] + sizes[1:]), 2, L.ACT_RELU, 0.0, 0x1000, None) == L.EINVAL
        assert entry(0x1000, L.F32, 10, 5, None, 0, ly, 2, L.ACT_RELU, 0.0, 0x1000, None) == L.EINVAL and b"chain" in lib.offsim_last_error()
        assert entry(0x1000, L.F32, 10, 4, None, 7, ly, 2, L.ACT_RELU, 0.0, None, None) == L.EINVAL and b"NULL" in lib.offsim_last_error()


# ---- the tolerance tells a wrong kernel from a right one ----
@pytest.mark.parametrize("name", ALL)
def test_the_emulation_stays_below_half_the_bound(name):
    b = P.build(name)
    c = b.case
    for l in range(max(c.L, 1)):
        assert np.isfinite(b.ref[l]).all() and (b.bound[l] > 0).all()
        emu = P.emulate_f32(b, None, l)
        assert emu.dtype == np.float32 and np.isnan(emu[~b.valid]).all() and np.isfinite(emu[b.valid]).all()
        r = P.ratio(emu, b.ref[l], b.bound[l], b.valid)
        print(f"{name} learner {l}: emulation at {r:.4f} of the bound")
        assert r < 0.5, (name, l, r)
        if c.fam == "exact":
            assert np.array_equal(emu, b.ref[l].astype(np.float32))


@pytest.mark.parametrize("mutant", P.MUTANTS)
def test_every_mutant_exceeds_the_bound_on_its_case(mutant):
    name, l = P.MUTANT_CASE[mutant]
    b = P.build(name)
    assert P.mutant_applies(b.case, mutant)
    r = P.ratio(P.emulate_f32(b, mutant, l), b.ref[l], b.bound[l], b.valid)
    others = {c.name: P.ratio(P.emulate_f32(P.build(c.name), mutant, max(c.L, 1) - 1), P.build(c.name).ref[-1], P.build(c.name).bound[-1],
                              P.build(c.name).valid) for c in P.CASE_LIST if P.mutant_applies(c, mutant)}
    caught = sum(v >= 4.0 / 3.0 for v in others.values())
    print(f"{mutant}: {r:.3g} times the bound on {name}; outside the bound by a third on {caught} of the {len(others)} cases it has a place in")
    assert r >= 4.0 / 3.0, (mutant, name, r)


def test_a_policy_hides_what_its_value_twin_shows():
    """Why every family has a value twin: a bias lost in the first layer moves a value net's output by thousands of bounds."""
    b = P.build("depth-n3-val")
    assert P.ratio(P.emulate_f32(b, "drop_bias"), b.ref[0], b.bound[0]) > 100
