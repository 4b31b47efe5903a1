"""What the encoder matrix (tests/test_gpu_encoder_matrix.py) rests on, checked without a device: the case table reaches every kernel
instance and sends every path round its grid-stride loop, each case lands on the path it is listed under, the tolerance of
tests/encoder_host.py is one that correct arithmetic stays inside (the f32 oracle in natural order and the NumPy emulation of the bf16 x 3
kernel, each against the f64 forward) and that a bf16 x 3 forward with one kept partial product lost does not, and the f64 reference alone
leaves at least 90 % of every case's rows with a clear argmax."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_host as E  # noqa: E402

ALL = [c.name for c in E.CASE_LIST]
S_CASES = [c.name for c in E.CASE_LIST if c.path == "S"]


def test_the_table_reaches_every_instance_and_every_stride_loop():
    for f32p, split_path in ((False, "S"), (True, "R")):
        seen = {}
        for c in E.CASE_LIST:
            path, inst, _ = E.taken_path(c, f32_products=f32p)
            seen.setdefault((path, inst, c.xdt), []).append(c)
        for xdt in ("f32", "f16"):
            for inst in E.REG_SHAPES:  # 6 shapes x 2 dtypes of S, and of R
                assert (split_path, inst, xdt) in seen, (split_path, inst, xdt)
            for inst in E.G_TILES:
                assert ("G", inst, xdt) in seen, (inst, xdt)
            assert ("V", (), xdt) in seen
        assert not any(p == ("R" if split_path == "S" else "S") for (p, _, _) in seen)
        for path in (split_path, "G", "V"):
            for xdt in ("f32", "f16"):
                assert any(c.N > 2 * E.sweep_rows(p, i) for (p, i, d), cs in seen.items() if p == path and d == xdt for c in cs), (path, xdt)
        # each group of the split kernels' sweeps: 32768 rows at dO = 128 (PF = 1), 131072 at dO = 2 and at dO = 4 (PF = 2, two wavefronts per SIMD)
        for dO in (128, 2, 4):
            for xdt in ("f32", "f16"):
                assert any(c.N > 2 * E.sweep_rows(p, i) for (p, i, d), cs in seen.items() if p == split_path and i[0] == dO and d == xdt for c in cs)
    assert E.sweep_rows("S", (128, 2)) == 32768 and E.sweep_rows("S", (2, 1)) == 131072 and E.sweep_rows("R", (4, 2)) == 131072
    assert E.sweep_rows("G", (1, 1)) == 131072 and E.sweep_rows("V", ()) == 524288


def test_the_dispatch_rule_on_named_shapes():
    assert E.dispatch(128, 64, 50) == ("S", (128, 2), 0) and E.dispatch(128, 64, 50, f32_products=True)[0] == "R"
    assert E.dispatch(2, 33, 25)[:2] == ("S", (2, 1)) and E.dispatch(2, 32, 25)[:2] == ("G", (1, 1))
    assert E.dispatch(128, 64, 50, aligned=False)[:2] == ("G", (2, 2)) and E.dispatch(3, 64, 50)[:2] == ("G", (2, 2))
    assert E.dispatch(4, 96, 5)[0] == "V" and E.dispatch(7, 128, 65)[0] == "V" and E.dispatch(4, 64, 65)[0] == "V"
    path, inst, lds = E.dispatch(128, 128, 64)
    assert (path, inst) == ("G", (4, 2)) and E.LDS_DEFAULT < lds <= E.LDS_LIMIT  # takes allow_big_lds
    assert E.dispatch(128, 80, 100)[0] == "V" and E.dispatch(128, 80, 100)[2] > E.LDS_DEFAULT
    assert E.dispatch(300, 128, 64)[0] == "refused" and E.dispatch(4, 129, 5)[0] == "refused"
    c = E.CASES["G-f32-d128-H64-z50-N129-unaligned"]
    with pytest.raises(AssertionError):  # a case whose alignment sends it elsewhere than it is listed fails, it does not pass
        E.taken_path(E.SimpleNamespace(**{**vars(c), "unaligned": False}))


def test_split3_is_exact_and_ordered():
    g = np.random.default_rng(0)
    v = (g.standard_normal(4096) * np.exp2(g.integers(-30, 30, 4096))).astype(np.float32)
    p = E.split3(v)
    assert np.array_equal(p["h"].astype(np.float64) + p["m"].astype(np.float64) + p["l"].astype(np.float64), v.astype(np.float64))
    for k in "hml":
        assert not (p[k].view(np.uint32) & 0xFFFF).any()
    h = (g.standard_normal(4096) * np.exp2(g.integers(-20, 12, 4096))).astype(np.float16).astype(np.float32)  # an fp16 value is two parts
    assert not E.split3(h)["l"].any()
    assert E.kept_products(128, np.float32)[1] == E.L1_PRODUCTS and len(E.kept_products(128, np.float16)[1]) == 5
    assert E.kept_products(2, np.float32)[1] == () and E.kept_products(4, np.float16)[1] == ()
    for prods in (E.L1_PRODUCTS, E.L2_PRODUCTS):
        assert set(prods) == {(a, b) for a in "hml" for b in "hml"} - {("m", "l"), ("l", "m"), ("l", "l")}


def _ratio(got, b):
    return float((np.abs(got.astype(np.float64) - b.ref) / b.B).max())


@pytest.mark.parametrize("name", ALL)
def test_correct_arithmetic_stays_inside_the_tolerance(name):
    b = E.build(name)
    c = b.case
    assert np.isfinite(b.ref).all() and (b.B > 0).all()
    assert b.rho_ref <= 2.0 ** -20, b.rho_ref  # an f32 forward of at most 128 + 128 terms: nothing odd about the inputs
    r_oracle = _ratio(b.oracle, b)
    assert r_oracle <= b.tol_f32
    line = f"{name}: rho_ref {b.rho_ref:.3e} tol_f32 {b.tol_f32:.3e}"
    if c.path == "S":
        r_split = _ratio(E.split3_emulated(b.x, b.W1, b.b1, b.W2, b.b2), b)
        line += f" split {r_split:.3e} tol_split {b.tol_split:.3e}"
        assert r_split <= b.tol_split, (r_split, b.tol_split)
    print(line)
    # the f64 reference alone leaves a clear argmax on at least 90 % of the rows, under the wider of the two tolerances
    clear = E.clear_rows(b, b.tol_split)
    assert clear.mean() >= 0.9, clear.mean()
    # inputs as described: about half of the hidden units on the leaky branch (none positive in the all-negative case)
    pre = b.x.astype(np.float64) @ b.W1.astype(np.float64).T + b.b1
    if c.kind == "neg_hidden":
        assert (pre < 0).all()
    elif c.N * c.H >= 2000:
        assert 0.3 < (pre < 0).mean() < 0.7
    if c.xdt == "f16" and c.N * c.dO >= 10:
        a = np.abs(b.x.astype(np.float32))
        assert (a == 65504.0).sum() >= 2 and ((a > 0) & (a < 2.0 ** -14)).sum() >= 2


@pytest.mark.parametrize("name", S_CASES)
def test_a_lost_partial_product_exceeds_the_tolerance(name):
    """The bound discriminates: the emulation with any one of the kept products left out, in either layer, is outside it.  (The three
    products the kernel drops on purpose are not in the set; layer 1 of the narrow shapes runs on exact f32 products and has none.)"""
    b = E.build(name)
    drops = E.droppable(b.case)
    assert len(drops) == (6 + (6 if b.case.xdt == "f32" else 5) if b.case.dO == 128 else 6)
    for drop in drops:
        r = _ratio(E.split3_emulated(b.x, b.W1, b.b1, b.W2, b.b2, drop=drop), b)
        assert r > b.tol_split, (drop, r, b.tol_split)
