"""What the k_homer_grad / k_homer_reduce / k_homer_adam matrix (tests/test_gpu_homer_matrix.py) rests on, checked without a device: the case
list covers every instance, tile size and layout edge, homer_plan (ht_prepare restated) gives the TM, LDS and workgroup numbers the cases are
named for and agrees with the library's own count, no net under the float cap is refused for LDS, the comparator with each case's bound accepts
torch's f32 gradient and rejects subtly wrong backward passes, nearly every parameter of every case carries a gradient far above the bound,
and no decision of a case sits within rounding of its threshold."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import homer_cases as K  # noqa: E402
import homer_train_host as HH  # noqa: E402

ALL = [c.name for c in K.MATRIX + K.EDGES]


# ---- coverage ----
def test_the_matrix_covers_every_listed_value():
    for c in K.MATRIX:
        p = K.homer_plan(c.dims, c.M)
        assert 200 <= c.M <= 220 and max(c.dims) <= 24 and p.TM == 16 and p.tm_lds == 32 and p.tiles in (13, 14) and p.lds < 64 * 1024
    for xdt in ("f32", "f16"):
        cs = [c for c in K.MATRIX if c.xdt == xdt]
        assert {c.slope for c in cs} == {0.0, 0.01, 0.2}
        assert {c.dims[3] % 2 for c in cs} == {0, 1} and {c.dims[2] % 2 for c in cs} == {0, 1}  # the out | 1 padding of W^T either way
        assert {c.dims[1] for c in cs} >= {1, 2, 3, 16}
        assert 1 in {c.dims[0] for c in cs} and {c.dims[0] % 2 for c in cs if c.dims[0] > 1} == {0, 1}
        assert {c.tau for c in cs} == {0.1, 0.5, 0.7, 1.0, 2.0} and sum(c.tau == 0.1 for c in cs) == 1 and sum(c.tau == 2.0 for c in cs) == 1
        assert {c.noise for c in cs} == {"iid", None}
    assert any(c.xdt == "f16" and c.dims[0] % 2 and c.dims[0] > 1 for c in K.MATRIX)
    for c in K.MATRIX:
        b = K.build(c.name)
        same = b.i == b.j
        assert same[2::3].all() and 0.3 <= same.mean() <= 0.4                  # idx_impo == idx_real on a third of the records
        assert len(np.unique(b.i)) < c.M and (b.i[6], b.j[6]) == (b.i[3], b.j[3])  # duplicated indices, a duplicated record
        assert set(b.act[b.i].tolist()) == set(range(c.dims[1]))              # every one-hot column is selected by some record
        assert b.n == c.M and (b.noise is None) == (c.noise is None)


EDGE_PLANS = {  # name: (dims, P, TM from LDS, TM, LDS bytes, workgroups)
    "TM4-H256-M1": ((12, 4, 19, 256), 19733, 4, 4, 125680, 1), "TM4-H256-M3": ((12, 4, 19, 256), 19733, 4, 4, 125680, 1),
    "TM4-H256-M4": ((12, 4, 19, 256), 19733, 4, 4, 125680, 1), "TM4-H256-M5": ((12, 4, 19, 256), 19733, 4, 4, 125680, 2),
    "TM4-H256-M21": ((12, 4, 19, 256), 19733, 4, 4, 125680, 6), "TM4-H256-M21-f16": ((12, 4, 19, 256), 19733, 4, 4, 125680, 6),
    "TM4-nZ256-M5": ((4, 2, 256, 24), 18930, 4, 4, 127616, 2), "TM4-nZ256-M21": ((4, 2, 256, 24), 18930, 4, 4, 127616, 6),
    "P-20480-M7": ((120, 9, 62, 64), 20480, 8, 8, 139264, 1), "P-20480-M8": ((120, 9, 62, 64), 20480, 8, 8, 139264, 1),
    "P-20480-M9": ((120, 9, 62, 64), 20480, 8, 8, 139264, 2), "P-20480-M86": ((120, 9, 62, 64), 20480, 8, 8, 139264, 11),
    "LDS-160K-TM32-M256": ((1, 1, 85, 17), 4524, 32, 32, 163840, 8), "LDS-160K-TM32-M300": ((1, 1, 85, 17), 4524, 32, 32, 163840, 10),
    "LDS-160K-TM16-M40": ((1, 1, 2, 230), 2764, 16, 8, 88384, 5), "LDS-160K-TM16-M200": ((1, 1, 2, 230), 2764, 16, 16, 163840, 13),
    "LDS-160K-TM8-M30": ((1, 16, 190, 34), 20286, 8, 8, 163840, 4),
    "TM16-by-M-M128": ((2, 5, 25, 64), 5531, 32, 16, 84304, 8), "TM16-by-M-M129": ((2, 5, 25, 64), 5531, 32, 16, 84304, 9),
    "TM16-by-M-M255": ((2, 5, 25, 64), 5531, 32, 16, 84304, 16), "TM16-by-M-M129-f16": ((2, 5, 25, 64), 5531, 32, 16, 84304, 9),
    "TM32-real-net-M256": ((2, 5, 25, 64), 5531, 32, 32, 146000, 8), "TM32-real-net-M257": ((2, 5, 25, 64), 5531, 32, 32, 146000, 9),
    "TM32-real-net-M300": ((2, 5, 25, 64), 5531, 32, 32, 146000, 10), "TM32-real-net-M257-f16": ((2, 5, 25, 64), 5531, 32, 32, 146000, 9),
    "TM32-tiles-per-workgroup": ((4, 2, 10, 16), 652, 32, 32, 43296, 128), "TM8-tiles-per-workgroup": ((128, 5, 50, 64), 18420, 8, 8, 126976, 128),
    "smallest-M1": ((1, 1, 2, 1), 16, 32, 8, 2064, 1), "smallest-M33": ((1, 1, 2, 1), 16, 32, 8, 2064, 5),
    "masked-tiles-nan": ((5, 3, 7, 12), 405, 32, 8, 9760, 13), "logits-in-the-hundreds": ((2, 5, 25, 64), 5531, 32, 16, 84304, 13),
}


def test_tile_sizes_and_lds_of_the_named_edges():
    assert set(EDGE_PLANS) == {c.name for c in K.EDGES}
    for name, (dims, P, tm_lds, TM, lds, wg) in EDGE_PLANS.items():
        c = K.CASES[name]
        p = K.homer_plan(c.dims, c.M)
        assert (c.dims, p.P, p.tm_lds, p.TM, p.lds, p.workgroups) == (dims, P, tm_lds, TM, lds, wg), name
        assert p.P == HH.n_params(*c.dims) <= K.MAX_FLOATS and not p.refused
    plans = {c.name: K.homer_plan(c.dims, c.M) for c in K.MATRIX + K.EDGES}
    assert {p.tm_lds for p in plans.values()} == {4, 8, 16, 32}                          # every TM is reached from LDS ...
    assert {p.TM for p in plans.values() if p.TM == p.tm_lds} == {4, 8, 16, 32}          # ... and launched as such
    assert {(p.tm_lds, p.TM) for p in plans.values() if p.TM < p.tm_lds} >= {(32, 16), (32, 8), (16, 8)}  # 16 and 8 are also reached from M
    assert any(p.lds <= 64 * 1024 for p in plans.values()) and any(p.lds > 64 * 1024 for p in plans.values())
    assert {p.TM for p in plans.values() if p.lds == K.LDS_MAX} == {8, 16, 32}           # three shapes at exactly 160 KiB
    # the DESIGN table's rows
    for dims, P, w_floats, per_record, tm_lds in (((2, 5, 25, 64), 5531, 5652, 964, 32), ((4, 5, 10, 16), 700, 764, 328, 32), ((128, 5, 50, 64), 18420, 18784, 1620, 8)):
        p = K.homer_plan(dims, 10 ** 6)
        assert (p.P, p.w_floats, p.per_record, p.tm_lds, p.TM) == (P, w_floats, per_record, tm_lds, tm_lds)
    # ownership and reduction edges
    p = plans["P-20480-M86"]
    assert p.P == K.THREADS * K.OWN and p.slots == K.OWN and p.nred == 80 and p.P % K.RED_BLOCK == 0
    assert plans["smallest-M1"].P == 16 and plans["smallest-M1"].nred == 1 and plans["TM4-H256-M5"].slots == 39
    # tiles per workgroup: 130 tiles on 128 workgroups (workgroups 0 and 1 take two), the last tile short
    for name, TM, tail in (("TM32-tiles-per-workgroup", 32, 5), ("TM8-tiles-per-workgroup", 8, 3)):
        p, c = plans[name], K.CASES[name]
        assert p.TM == TM and p.tiles == K.MAX_BLOCKS + 2 and p.workgroups == K.MAX_BLOCKS and c.M % TM == tail and c.pattern == "det"
    assert K.CASES["TM8-tiles-per-workgroup"].xdt == "f16"
    # TM = 4: 3 TM = 12 encoder rows are three HT_RB blocks, 2 TM = 8 classifier rows two; M = 21 leaves a last tile of one record
    assert [plans[f"TM4-H256-M{M}"].tiles for M in (1, 3, 4, 5, 21)] == [1, 1, 1, 2, 6]
    # nZ at its maximum: the D column of the encoder's last layer goes up to H + 255
    assert K.CASES["TM4-nZ256-M5"].dims[2] == 256
    for _, f32, f16 in K.FORWARD_CASES:
        assert K.CASES[f32].xdt == "f32" and K.CASES[f16].xdt == "f16" and K.CASES[f32].dims == K.CASES[f16].dims and K.CASES[f32].M == K.CASES[f16].M
    assert [plans[f32].TM for _, f32, _ in K.FORWARD_CASES] == [tm for tm, _, _ in K.FORWARD_CASES] == [4, 16, 32]


def test_homer_plan_agrees_with_the_library():
    """offsim_homer_work_doubles_pop sizes a learner's scratch by the workgroups ht_prepare gives the batch: the library's own TM rule"""
    from rl_offline_simulation_amd import _lib as L
    lib = L.load()  # (loads without a device, as in tests/test_homer_population_host.py)
    f = 0x1000
    seen = set()
    for c in K.MATRIX + K.EDGES:
        net = L.HomerNet(f, f, f, f, f, f, f, f, *c.dims, 0.01, 0)
        for M in (c.M, 1, 63, 64, 127, 128, 255, 256, 4096, 4097):
            p = K.homer_plan(c.dims, M)
            assert lib.offsim_homer_work_doubles_pop(ctypes.byref(net), 3, M) == 3 * L.homer_work_doubles_nb(p.P, p.workgroups), (c.name, M)
            seen.add((p.tm_lds, p.TM))
    assert seen == {(32, 32), (32, 16), (32, 8), (16, 16), (16, 8), (8, 8), (4, 4)}


def test_no_net_under_the_float_cap_is_refused_for_lds():
    """Over dO in {1, 4, 12, 64, 128}, nA in {1, 2, 16}, every nZ in 2..256 and every H in 1..256: no net with P <= 20480 needs more than
    160 KiB at TM = 4, so TM = 4 is the lowest path and ht_prepare's LDS refusal cannot be reached under the cap."""
    H = np.arange(1, 257, dtype=np.int64)[None, :]
    nZ = np.arange(2, 257, dtype=np.int64)[:, None]
    worst, arg, reached = 0, None, set()
    for dO in (1, 4, 12, 64, 128):
        for nA in (1, 2, 16):
            Kk = 2 * nZ + nA
            P = dO * H + H + H * nZ + nZ + Kk * H + H + 2 * H + 2
            wf = (dO * (H | 1) + H + H * (nZ | 1) + nZ + Kk * (H | 1) + H + H * 3 + 2 + 3) & ~3
            per = 3 * (((dO + H + 1) | 1) + ((H + nZ) | 1)) + 2 * (((Kk + H + 1) | 1) + ((H + 2 + Kk) | 1)) + 12
            ok = P <= K.MAX_FLOATS
            lds4 = np.where(ok, 4 * (wf + 4 * per), 0)
            if lds4.max() > worst:
                worst = int(lds4.max())
                a, b = np.unravel_index(int(lds4.argmax()), lds4.shape)
                arg = (dO, nA, int(nZ[a, 0]), int(H[0, b]))
            for TM in (4, 8, 16, 32):
                fits = ok & (4 * (wf + TM * per) <= K.LDS_MAX)
                if TM < 32:
                    fits &= 4 * (wf + 2 * TM * per) > K.LDS_MAX
                if fits.any():
                    reached.add(TM)
    assert worst == 140608 and arg == (128, 16, 256, 22) and worst <= K.LDS_MAX
    assert reached == {4, 8, 16, 32}
    p = K.homer_plan(arg, 100)  # the vectorised arithmetic above is homer_plan's
    assert p.lds_at_4 == worst and p.tm_lds == 4 and not p.refused
    for dims in ((12, 4, 19, 256), (4, 2, 256, 24), (1, 16, 190, 34)):
        p = K.homer_plan(dims, 100)
        dO, nA, z, h = dims
        assert p.P == dO * h + h + h * z + z + (2 * z + nA) * h + h + 2 * h + 2


# ---- the comparator ----
@pytest.mark.parametrize("name", ALL)
def test_comparator_accepts_f32_and_rejects_wrong_gradients(name):
    b = K.build(name)
    c, g = b.case, b.g64
    assert np.array_equal(K.mutant_grad(b), g), "the restated pass is the reference's"
    assert K.passes(b.g32, b), "torch's own f32 gradient"
    assert max(K.tensor_errors(b.g32, b)) <= K.REL_TENSOR_F32, K.tensor_errors(b.g32, b)
    assert K.scalar_bound(b.l64, b.l32) == b.loss_bound and abs(b.l32 - b.l64) <= b.loss_bound
    z = g.copy()
    z[-1] = 0.0
    assert not K.passes(z, b), "the last parameter zeroed"
    for s in b.slices[1::2]:
        z = g.copy()
        z[s] = 0.0
        assert not K.passes(z, b), "a layer's bias gradient dropped"
    last = int(np.flatnonzero(b.ok)[-1])  # the last valid record: the tail of the last tile that has one
    assert not K.passes(K.mutant_grad(b, drop=last), b), "one record left out, the divisor kept"
    assert not K.passes(K.mutant_grad(b, "slope"), b), "leaky_relu's slope off by 0.05 in the backward pass"
    if c.tau != 1.0:
        assert not K.passes(K.mutant_grad(b, "tau"), b), "the / tau of the softmax backward dropped"
    assert not K.passes(K.mutant_grad(b, "z2"), b), "z2's share of the obs[i] row's de dropped"
    differ = (b.nxt[b.i[b.ok]] != b.nxt[b.j[b.ok]]).any()
    assert differ, "some record has next_obs[j] != next_obs[i]"
    assert not K.passes(K.mutant_grad(b, "impostor"), b), "next_obs[j] replaced by next_obs[i]"
    if b.noise is not None:
        assert not K.passes(K.mutant_grad(b, "noise"), b), "the noise of q = 1 and q = 3 swapped"


@pytest.mark.parametrize("name", ALL)
def test_parameters_carry_signal(name):
    b = K.build(name)
    sig = np.abs(b.g64) > 10.0 * b.bound
    assert float(sig.mean()) >= 0.9, float(sig.mean())
    for t, s in zip(K.TENSORS, b.slices):
        assert float(sig[s].mean()) >= 0.5, (t, float(sig[s].mean()))
    assert b.n == int(b.ok.sum()) > 0
    if b.case.mask is None:
        assert b.n == b.case.M


def test_the_masked_case_has_every_kind_of_invalid_record():
    b = K.build("masked-tiles-nan")
    c, bad = b.case, ~b.ok
    n, nA = c.n_rows, c.dims[1]
    assert bad[16:32].all() and bad[48:64].all() and bad[96:].all() and 0 < b.ok[:16].sum() < 16  # whole tiles of 8 and of 16, the tail, scattered
    i, j = b.i.astype(np.int64), b.j.astype(np.int64)
    rows_ok = (i >= 0) & (i < n)
    a = b.act[np.where(rows_ok, i, 0)]
    assert (i < 0).any() and (i >= n).any() and (j < 0).any() and (j >= n).any() and (rows_ok & (a < 0)).any() and (rows_ok & (a >= nA)).any()
    assert np.isnan(b.noise[bad]).all() and np.isfinite(b.noise[b.ok]).all()
    assert np.isfinite(b.g64).all() and b.n == int(b.ok.sum()) == 57


# ---- no decision within rounding ----
@pytest.mark.parametrize("name", ALL)
def test_no_pre_activation_within_rounding_of_zero(name):
    b = K.build(name)
    assert b.pre_margin >= K.PRE_MARGIN and b.attempt < 50


@pytest.mark.parametrize("name", [n for _, f32, f16 in K.FORWARD_CASES for n in (f32, f16)])
def test_hard_cases_keep_every_argmax_clear(name):
    """Records whose top-two gap of any of the four perturbed logit vectors is below 1e-4 are dropped (at most a tenth).  On the rest an f32
    ulp of a logit (at most 2^-23 x 32 here) cannot flip an argmax, so torch's f32 hard loss differs from the f64 one by rounding alone: a
    flipped argmax would move one of 2 n terms of order 1, at least 1e-4 for these n, while rounding stays below 64 ulps."""
    h = K.build_hard(name)
    assert h.dropped <= 0.1 * h.case.M and h.n == h.case.M - h.dropped
    assert abs(h.l32 - h.l64) <= 64 * K.ULP * max(1.0, abs(h.l64)), (h.l32, h.l64)
    assert abs(h.l32 - h.l64) <= h.loss_bound
    assert h.l64 != h.base.l64  # the discretized forward is another function
