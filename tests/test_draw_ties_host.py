"""CPU tests of tests/draw_tie_host.py: the restated draw against NumPy's Generator.choice and the existing mirrors on the BUILT tables,
the census every case of tests/test_gpu_draw_ties.py has to meet -- as a condition (at least draw_tie_host.NEED = 32 steered meetings
of every class a case names), with the counts recorded --, and the discriminating power: four wrong draws, each of which changes the
trace of the mirror in every case that names a class it should be caught by.

Every class reaches the bar in every form.  The f32 exact ties (f32tie, f32tie0) have totals p_0 / u, within 2^-24 of 1 and not within
1e-12: such rows meet only the row-policy and collect mirrors, whose draw is the rule written out (Generator.choice itself refuses
widened f32 rows); every f64 built row is within 1e-12 of 1 and goes through Generator.choice in queue_host.run.  A state of the
tabular forms is steered once, so those cases name at most four classes each; the nA = 70 pi cases are two (the learner's LDS carve
holds at most 95 states of 70 actions)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import draw_tie_host as D  # noqa: E402

# name -> (steered meetings per class, unsteered meetings): the builder is deterministic
CENSUS = {
    "pi-nA4": ({"last": 64, "tie": 64, "tie0": 64, "tie0-end": 64}, 5239),
    "pi-nA3": ({"above": 64, "below": 64, "div-down": 64, "div-up": 64}, 6903),
    "pi-nA16": ({"last": 42, "tie": 43, "tie0": 43}, 1025),
    "pi-nA70-a": ({"chunk62": 40, "chunk63": 40}, 6476),
    "pi-nA70-b": ({"chunk64": 40, "chunk68": 40}, 8817),
    "rows-f64-nA4": ({"above": 325, "below": 325, "div-down": 325, "div-up": 325, "last": 326, "tie": 326, "tie0": 326, "tie0-end": 326}, 4665),
    "rows-f64-nA4-b": ({"above": 317, "below": 317, "div-down": 317, "div-up": 316, "last": 316, "tie": 316, "tie0": 316, "tie0-end": 316}, 3851),
    "rows-f64-nA3": ({"above": 381, "below": 381, "div-down": 381, "div-up": 381, "last": 382, "tie": 382, "tie0": 382}, 5356),
    "rows-f32-nA4": ({"f32dec": 766, "f32tie": 766}, 2401),
    "rows-f32-nA16": ({"f32dec": 656, "f32tie": 656, "f32tie0": 656}, 898),
    "rows-f32-nA16-b": ({"f32dec": 670, "f32tie": 669, "f32tie0": 669}, 1107),
    "rows-f64-nA70": ({"chunk62": 173, "chunk63": 193, "chunk64": 238, "chunk68": 205}, 357),
    "collect-rows-f64-nA4": ({"above": 111, "below": 111, "div-down": 111, "div-up": 111, "last": 111, "tie": 112, "tie0": 112, "tie0-end": 111}, 190),
    "collect-rows-f32-nA16": ({"f32dec": 272, "f32tie": 273, "f32tie0": 272}, 263),
    "collect-pi-f64-nA4": ({"last": 60, "tie": 60, "tie0": 60, "tie0-end": 60}, 840),
    "collect-pi-f64-nA3": ({"above": 63, "below": 63, "div-down": 62, "div-up": 62}, 830),
    "collect-pi-f32-nA16": ({"f32dec": 41, "f32tie": 41, "f32tie0": 41}, 474),
}
NAMES = [c.name for c in D.CASES]
TRACE = {"pi": ("trace_pop", "trace_row"), "rows": ("trace_pop", "trace_row"), "collect-rows": ("action", "row"), "collect-pi": ("action", "row")}


def _equal(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(a, b)
    return a == b


def _same_outputs(xs, ys, tag, skip=()):
    assert len(xs) == len(ys)
    for i, (x, y) in enumerate(zip(xs, ys)):
        assert x.keys() == y.keys()
        for k in x:
            assert k in skip or _equal(x[k], y[k]), (tag, i, k)


@pytest.mark.parametrize("name", NAMES)
def test_the_restated_draw_is_the_mirrors(name):
    """On the built tables: the mirrors as they are (queue_host.run draws with Generator.choice, which has to accept every built row)
    equal the mirrors with the restated draw in place of theirs, and equal the walk that fixed the rows, on every output the mirror
    returns (the walk's record of the row drawn from, `p` of collect, is taken before a first meeting rewrites the row)."""
    c = D.BY_NAME[name]
    b = D.build(c)
    plain, envs = D.mirror(c, b["tables"])
    restated, envs2 = D.mirror(c, b["tables"], D.with_gen(D.draw))
    _same_outputs(plain, restated, name)
    _same_outputs(plain, b["walk"], name, skip=("p",))
    for e, e2 in zip(envs, envs2):
        _same_outputs([e.state()], [e2.state()], name)
    assert sum(len(o[TRACE[c.walk][0]]) for o in plain) > 0


@pytest.mark.parametrize("name", NAMES)
def test_built_rows_are_distributions(name):
    c = D.BY_NAME[name]
    b = D.build(c)
    for r in b["records"]:
        p = b["tables"][r.table][r.row]
        assert p.dtype == c.dtype and np.isfinite(p).all() and (p >= 0).all(), r
        tot = np.cumsum(p.astype(np.float64))[-1]
        assert abs(tot - 1) <= (2.0 ** -23 if c.dtype == np.float32 else 1e-12), (r, tot)


@pytest.mark.parametrize("name", NAMES)
def test_census_is_met(name):
    c = D.BY_NAME[name]
    b = D.build(c)
    want, unsteered = CENSUS[name]
    assert set(want) == set(c.classes)
    for cls in c.classes:
        assert b["count"].get(cls, 0) >= D.NEED, (cls, b["count"])
    assert b["count"] == want and b["unsteered"] == unsteered
    assert c.log.N <= 4100 and c.R <= 16 and len(b["records"]) == sum(want.values())
    # every steered meeting is what its class says, re-derived from the built tables and default_rng alone
    us = [np.random.default_rng(sa).random(max(r.draw for r in b["records"]) + 1) for sa in c.action_seeds]
    for r in b["records"]:
        u = us[r.rollout][r.draw]
        p = b["tables"][r.table][r.row]
        assert u == r.u and r.cls in D.classify(p, u, r.k) and D.draw(p, u) == r.A, r
    if c.nA == 70:
        assert {r.k for r in b["records"]} == {D.CHUNK[cls] for cls in c.classes}
    else:
        feasible = set().union(*(D._ks(cls, c.nA)[0] for cls in c.classes))  # (an f32 tie needs three entries behind it: nA = 4 has k = 0 only)
        assert {r.k for r in b["records"]} == feasible  # boundaries across the row, not one


@pytest.mark.parametrize("name", NAMES)
def test_wrong_draws_change_the_trace(name):
    """(a) side='left', (b) no division by the total, (c) the comparison in f32, (d) k + 1 unchecked after a tie: each changes the trace
    of at least one rollout in every case that names a class it should be caught by, and decides every single meeting of such a class
    differently (c on `below` apart: there both comparisons pass the boundary) -- so a kernel wrong in one of these ways fails the
    bit-for-bit comparison of tests/test_gpu_draw_ties.py."""
    c = D.BY_NAME[name]
    b = D.build(c)
    plain, _ = D.mirror(c, b["tables"])
    hit = False
    for m, fn in D.MUTANTS.items():
        if not set(D.CAUGHT_BY[m]) & set(c.classes):
            continue
        hit = True
        wrong, _ = D.mirror(c, b["tables"], D.with_gen(fn))
        changed = [i for i, (x, y) in enumerate(zip(plain, wrong)) if any(not np.array_equal(x[k], y[k]) for k in TRACE[c.walk])]
        assert changed, (name, m)
        for r in b["records"]:
            if r.cls in D.CAUGHT_BY[m] and (m, r.cls) != ("f32", "below"):
                assert fn(b["tables"][r.table][r.row], r.u) != r.A, (m, r)
    assert hit


def test_every_mutant_and_every_class_has_a_case():
    named = {cls for c in D.CASES for cls in c.classes}
    assert named == {"tie", "last", "tie0", "tie0-end", "above", "below", "div-down", "div-up", "f32tie", "f32tie0", "f32dec"} | set(D.CHUNK)
    assert all(set(v) & named for v in D.CAUGHT_BY.values()) and set(D.CAUGHT_BY) == set(D.MUTANTS)
    assert {c.nA for c in D.CASES} == {3, 4, 16, 70}


def test_building_twice_gives_the_same_bytes():
    c = D.BY_NAME["rows-f32-nA16"]
    first = D.build(c)
    D.build.cache_clear()
    second = D.build(c)
    assert first is not second and first["records"] == second["records"]
    for k, t in first["tables"].items():
        assert t.tobytes() == second["tables"][k].tobytes()
