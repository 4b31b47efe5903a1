"""What the k_ppo_grad / k_ppo_adam matrix (tests/test_gpu_ppo_update_matrix.py) rests on, checked without a device: the case list covers
every instance and layout, the comparator with each case's bound accepts torch's f32 gradient and rejects subtly wrong ones, nearly every
parameter of every case carries a gradient far above the bound, no decision of a case sits within rounding of its threshold, and
ppou_prepare's tile-size arithmetic gives the TM and LDS sizes the cases are named for."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_update_cases as K  # noqa: E402
import ppo_update_host as U  # noqa: E402

GRAD_CASES = [c.name for c in K.MATRIX + K.EDGES if not c.zero_grad]


def test_the_matrix_covers_every_instance_and_layout():
    for kind in ("actor", "critic"):
        for xdt in ("f32", "f16"):
            cs = [c for c in K.MATRIX if c.kind == kind and c.xdt == xdt]
            assert {(c.act, c.slope) for c in cs if c.act == "leaky_relu"} == {("leaky_relu", 0.2), ("leaky_relu", 0.0)}
            assert {c.act for c in cs} == {"identity", "tanh", "relu", "leaky_relu"}
            assert {len(c.sizes) - 1 for c in cs} == {1, 2, 3, 4}
            assert {c.bias for c in cs} == {"all", "none", "mixed"}
            flags = [K.bias_flags(c.bias, len(c.sizes) - 1, c.seed) for c in cs if c.bias == "mixed"]
            assert any(f[0] and not f[-1] for f in flags) and any(f[-1] and not f[0] for f in flags)
            # a derivative that is not 1 needs a hidden layer to show
            assert all(len(c.sizes) > 2 for c in cs if c.act in ("tanh", "leaky_relu"))
        assert any(c.xdt == "f16" and c.sizes[0] % 2 for c in K.MATRIX if c.kind == kind)
    for c in K.MATRIX:
        assert 200 <= c.M <= 220 and all(3 <= w <= 24 for w in c.sizes[:-1])


def test_tile_sizes_and_lds_of_the_named_nets():
    plan = lambda name: K.lds_plan(K.CASES[name].sizes, K.bias_flags(K.CASES[name].bias, len(K.CASES[name].sizes) - 1, K.CASES[name].seed))  # noqa: E731
    TM, lds, P, lda, ldd = plan("actor-lds-above-64k-TM16")
    assert (TM, P, lds, lda, ldd) == (16, 15904, 136944, 557, 545)  # 133.7 KiB; at TM = 32 it would be 203.2 KiB
    assert (P + K.THREADS - 1) // K.THREADS == 32
    TM, lds, P, _, _ = plan("critic-lds-above-64k-TM16")
    assert TM == 16 and 64 * 1024 < lds <= 160 * 1024
    for name, want_P in (("actor-P-16384", 16384), ("critic-P-16384", 16384), ("actor-P-above-15872", 16272), ("critic-P-above-15872", 16129)):
        TM, lds, P, _, _ = plan(name)
        assert P == want_P and 512 * 31 < P <= K.MAX_FLOATS and TM == 32 and lds > 64 * 1024, name  # TM = 32 through the big-LDS path
    for name in ("actor-P-below-512", "critic-P-below-512"):
        TM, lds, P, _, _ = plan(name)
        assert P < K.THREADS and TM == 32 and lds < 64 * 1024
    for c in K.MATRIX:
        TM, lds, P, _, _ = K.lds_plan(c.sizes, K.bias_flags(c.bias, len(c.sizes) - 1, c.seed))
        assert TM == 32 and lds < 64 * 1024 and P < 1024
    c = K.CASES["actor-tiles-per-workgroup"]
    tiles = -(-c.M // 32)
    assert tiles == 2 * K.MAX_BLOCKS + 4 and c.M % 32 == 5  # workgroups 0-3 take three tiles, the others two; the last tile holds 5 records


def test_no_admissible_net_goes_below_tm_16():
    """TM = 8, TM = 4 and the 160 KiB refusal cannot be reached under the float cap.

    At TM = 16 the LDS holds, in floats, w_floats + 16 lda + 16 ldd + 160 (the f64 sums).  With S the sum of all layers' outputs:
    w_floats <= P + (dO + S) + 3 (W^T pads each of its rows, one per input unit, by at most one float), lda <= dO + S + 2, ldd <= S + 1, so
    the total is at most P + 17 dO + 33 S + 211, which must stay within 40960.  P <= 16384 and dO <= 128 leave S <= 672.  S itself is
    bounded by the cap: a hidden chain h1, h2, h3 costs at least dO h1 + h1 h2 + h2 h3 + h3 nA >= h1 + h1 h2 + h2 h3 + h3 parameters.
    The largest S over all chains within the cap is enumerated here; the networks found are then laid out exactly."""
    h = np.arange(1, 257, dtype=np.int64)
    best, arg = 0, None
    for h1 in h:  # depth 4 contains the shallower nets' sums (a width-1 layer costs less than it adds)
        h2, h3 = h[:, None], h[None, :]
        cost = h1 + h1 * h2 + h2 * h3 + h3
        s = np.where(cost <= K.MAX_FLOATS, h1 + h2 + h3, 0)
        if s.max() > best:
            best = int(s.max())
            i, j = np.unravel_index(int(s.argmax()), s.shape)
            arg = (int(h1), int(h[i]), int(h[j]))
    for depth3 in h:  # (and the shallower chains, for the record: two hidden layers)
        assert depth3 + min(256, (K.MAX_FLOATS - depth3) // (depth3 + 1)) <= best
    S = best + 16
    assert K.MAX_FLOATS + 17 * 128 + 33 * S + 211 <= 160 * 1024 // 4, (best, arg)
    # the widest chains, laid out exactly, with and without biases, narrow and wide ends: TM = 16, and far from the refusal
    seen = set()
    for dO in (1, 12, 128):
        for nA in (1, 16):
            for hid in (arg, (256, 16, 256), (256, 24, 256), (256, 30, 256), (128, 60, 128)):
                for hb in (True, False):
                    sizes = (dO,) + tuple(hid) + (nA,)
                    TM, lds, P, _, _ = K.lds_plan(sizes, (hb,) * 4)
                    if P <= K.MAX_FLOATS:
                        seen.add(TM)
                        assert TM >= 16 and lds <= 160 * 1024, sizes
    assert seen == {16, 32}


@pytest.mark.parametrize("name", GRAD_CASES)
def test_comparator_accepts_f32_and_rejects_wrong_gradients(name):
    b = K.build(name)
    c, g = b.case, b.ref["g"]
    assert K.passes(b.g32, b), "torch's own f32 gradient"
    z = g.copy()
    z[-1] = 0.0
    assert not K.passes(z, b), "the last parameter zeroed"
    for ws, bs in K.layer_slices(c):
        if bs is not None:
            z = g.copy()
            z[bs] = 0.0
            assert not K.passes(z, b), "a layer's bias gradient dropped"
    # one record left out of the sum (the last one that adds to it: the tail of the last tile), the divisor unchanged
    n = b.ref["n"]
    keep = np.ones(c.M, bool) if b.keep is None else b.keep.copy()
    last = next(m for m in np.flatnonzero(keep)[::-1] if np.any(K.reference(c, b.net, b.data, np.arange(c.M) == m)["g"]))  # (not clipped away)
    keep[last] = False
    less = K.reference(c, b.net, b.data, keep)["g"] * (n - 1) / n if n > 1 else np.zeros_like(g)
    assert not K.passes(less, b), "one record left out"
    if len(c.sizes) > 2 and c.act == "leaky_relu":
        wrong = K.reference(c, b.net, b.data, b.keep, dact=lambda x, h, kind, slope: np.where(x > 0, 1.0, slope + 0.05))["g"]
        assert not K.passes(wrong, b), "leaky_relu's slope off by 0.05"
    if len(c.sizes) > 2 and c.act == "tanh":
        wrong = K.reference(c, b.net, b.data, b.keep, dact=lambda x, h, kind, slope: np.ones_like(x))["g"]
        assert not K.passes(wrong, b), "tanh's derivative taken as 1"


@pytest.mark.parametrize("name", GRAD_CASES)
def test_parameters_carry_signal(name):
    b = K.build(name)
    share = float((np.abs(b.ref["g"]) > 10.0 * b.bound).mean())
    assert share >= 0.9, share
    assert b.ref["n"] == (b.case.M if b.keep is None else int(b.keep.sum()))


@pytest.mark.parametrize("name", [c.name for c in K.MATRIX + K.EDGES if c.kind == "actor"])
def test_no_ratio_within_rounding_of_a_clip_edge(name):
    """A ratio that f32 puts on the other side of 1 +- clip would change the gradient by a whole record.  The f32 ratio is off by about
    an ulp per unit of |logit| and of |log ratio|; no f64 ratio of a case comes within 64 times that of an edge."""
    b = K.build(name)
    r = K.clip_ratios(b)
    z = np.abs(U.forward(K.net64(b.net), b.data["obs"].astype(np.float64)[slice(None) if b.keep is None else b.keep], b.case.act, b.case.slope)[0]).max()
    gap = np.minimum(np.abs(r - (1 - K.CLIP)), np.abs(r - (1 + K.CLIP))).min()
    assert gap > 64 * K.ULP * (2.0 + z), (gap, z)
    if not b.case.zero_grad and b.case.M >= 31:
        assert 0.02 < b.ref["cf"] < 0.6  # both sides of the clip are there


def test_the_zero_gradient_case_is_zero():
    b = K.build("actor-nA1")
    assert not np.any(b.ref["g"]) and b.bound == 0.0 and b.ref["ent"] == 0.0


def test_adam_calls_stay_clear_of_the_kl_limit():
    """The three calls of the Adam test: the middle one stops early, the others run all their passes, and no host kl comes within 5 % of
    the limit, so that ulps cannot move StopIter on the device (or in the f32 torch loop that sets the bounds)."""
    A, R = K.ADAM, K.adam_calls()
    lim = 1.5 * A.target_kl
    stops = [x.a["stop_iter"] for x in R.calls]
    for x in R.calls:
        kl = x.a["trace"][:, 1]
        assert np.all(np.abs(kl - lim) >= K.MARGIN * lim), kl
    assert stops[0] == A.iters - 1 and stops[2] == A.iters - 1 and 2 <= stops[1] <= A.iters - 3, stops
    assert len(R.calls[1].a["trace"]) == stops[1] + 1 and R.calls[1].a["trace"][-1, 1] > lim
    steps = [A.iters, stops[1], A.iters]
    assert [x.pi_t for x in R.calls] == list(np.cumsum(steps)) and [x.v_t for x in R.calls] == [A.iters, 2 * A.iters, 3 * A.iters]
    for x in R.calls:  # the f32 loop took the same decisions: its state is that of the same number of steps
        for x64, x32 in ((x.pi, x.t32_pi[0]), (x.v, x.t32_v[0]), (x.pi_m, x.t32_pi[1]), (x.v_v, x.t32_v[2])):
            assert K.state_bound(x64, x32) <= 1e-3 * float(np.abs(x64).max())
