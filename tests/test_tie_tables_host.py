"""CPU tests of tests/tie_host.py: the restated threshold arithmetic against the pinned oracle, the built tables' host simulation against
the oracle's evalMC, and the census every table of tests/test_gpu_scan_ties.py has to meet -- as a condition, with the counts recorded."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tie_host as H  # noqa: E402
from oracle import oracle as O  # noqa: E402

# name -> (table, classes every one of which needs `need` realised meetings, recorded census)
A_CLASSES = H.A_ACCEPTS + H.A_REJECTS + H.A_SPECIAL
TABLES = {
    "a_every3": (lambda: H.table_a(3), A_CLASSES, 8, dict(planned=2000, skipped=0, positions={"1": 739, "2": 481, ">=3": 780, ">=9": 53})),
    "a_all": (lambda: H.table_a(1), A_CLASSES, 8, dict(planned=5968, skipped=0, positions={"1": 2292, "2": 1321, ">=3": 2355, ">=9": 346})),
    "a_every3_philox": (lambda: H.table_a(3, "philox"), A_CLASSES, 8, dict(planned=2000, skipped=0, positions={"1": 750, "2": 426, ">=3": 824, ">=9": 58})),
    "bc_70k": (lambda: H.table_bc(), H.BC_ACCEPTS + H.BC_REJECTS, 4, dict(planned=9528, skipped=5, positions={"1": 3330, "2": 2181, ">=3": 4012, ">=9": 292})),
    "c_131k": (lambda: H.table_bc(131072), H.BC_ACCEPTS + H.BC_REJECTS + H.C_LOC, 4,
               dict(planned=17563, skipped=8, positions={"1": 6220, "2": 3952, ">=3": 7383, ">=9": 581})),
}
# the fewest realised meetings of any class, per table (every class's count is asserted against `need`; this is the recorded minimum)
MIN_CLASS = {"a_every3": 61, "a_all": 188, "a_every3_philox": 62, "bc_70k": 396, "c_131k": 63}


def _oracle(log):
    return O.OraclePSRS(log["z"], log["actions"], log["rewards"], log["z_next"], log["terminals"], log["action_distributions"], log["steps"] == 0)


@pytest.mark.parametrize("name", list(TABLES))
def test_the_builders_simulation_is_the_oracles(name):
    """Rows, candidates per step, Gs, lengths and counts of the oracle's evalMC on the BUILT log equal the builder's own trace for every
    seed: the builder's queue orders, draws and decisions (k53 <= threshold) are the pinned oracle's, not its own invention."""
    b = TABLES[name][0]()
    ora = _oracle(b["log"])
    N = len(b["log"]["z"])
    for s in b["seeds"]:
        ora.reset_sampler(s)
        if name.endswith("philox"):
            ora.set_rejection_philox(s)
        ref = ora.evalmc(10 ** 9, b["pi"], b["gamma"], trace_cap=N + 1)
        mine = b["trace"][s]
        assert ref["steps"] == mine["steps"] and ref["candidates"] == mine["candidates"], s
        for k in ("trace_rows", "trace_popped", "Gs", "lengths"):
            assert np.array_equal(ref[k], mine[k]), (s, k)


@pytest.mark.parametrize("name", list(TABLES))
def test_census_is_met(name):
    make, classes, need, recorded = TABLES[name]
    b = make()
    c = H.census(b)
    for cls in classes:
        assert c["classes"].get(cls, 0) >= need, (cls, c["classes"].get(cls, 0))
    assert set(c["classes"]) == set(classes)
    assert c["skipped"] * 10 <= c["planned"]
    assert all(c["positions"][p] > 0 for p in ("1", "2", ">=3", ">=9")), c["positions"]
    assert {k: c[k] for k in recorded} == recorded
    assert min(c["classes"].values()) == MIN_CLASS[name]
    # every realised meeting is what its class says, re-derived from the built log alone
    log, pi = b["log"], b["pi"]
    for r in b["records"]:
        T = H.threshold(pi[log["z"][r.row]], log["action_distributions"][r.row], int(log["actions"][r.row]))
        kind = r.cls.split(":")[1] if r.cls[1:2] == ":" else r.cls
        if kind in ("thr>1", "thr=1", "nan"):
            assert T == H.T_MAX
        elif kind == "T=0":
            assert T == 0
        elif kind.startswith("t="):
            assert T >> 32 == int(kind[2:])
        if r.cls.endswith(":hi") or r.cls.endswith(":loc"):
            assert log["terminals"][r.row] and log["z_next"][r.row] == 254
    if name.startswith("a_"):  # the payload bits of the accepts around the clear-accept edge: both done values, z_next 0 and n_states - 1
        for cls in H.A_PAYLOAD:
            seen = {(bool(log["terminals"][r.row]), int(log["z_next"][r.row])) for r in b["records"] if r.cls == cls}
            assert seen == {(False, 0), (False, 5), (True, 0), (True, 5)}, (cls, seen)
    if name == "c_131k":
        order = np.argsort(log["z"], kind="stable")
        local = {int(g): i for i, g in enumerate(order[: 131072])}
        assert all(local[r.row] >= 0x1FF00 for r in b["records"] if r.cls.endswith(":loc"))


def test_ties_are_ties():
    """The delta of every realised format-A meeting against the draw it met, re-derived from default_rng: the classes are where they claim."""
    b = H.table_a(1)
    log, pi = b["log"], b["pi"]
    order = np.argsort(log["z"], kind="stable")
    seg = np.searchsorted(log["z"][order], np.arange(7))
    for s in b["seeds"]:
        k53 = H.draws("pcg64", s, len(log["z"]) + 1)
        # draw index of (step, position): candidates before the step + position - 1
        before = np.concatenate([[0], np.cumsum(b["trace"][s]["trace_popped"])])
        for r in (r for r in b["records"] if r.seed == s):
            k = k53[int(before[r.step]) + r.position - 1]
            T = H.threshold(pi[log["z"][r.row]], log["action_distributions"][r.row], int(log["actions"][r.row]))
            assert (k <= T) == r.accept
            d = (k >> 32) - (T >> 32)
            if r.cls in ("eq", "eq-1", "eq+1"):
                assert d == 0 and T - k == {"eq": 0, "eq-1": -1, "eq+1": 1}[r.cls]
            elif r.cls in ("far_acc", "far_rej"):
                assert d == 0 and abs(T - k) >= 1 << 16
            elif r.cls[0] == "d":
                assert d == int(r.cls[1:])
    assert seg[-1] == len(log["z"])


def test_threshold_decides_as_the_oracle_steps():
    """One state, every row a candidate in queue order: candidate i meets draw i, and `k53 <= threshold` picks exactly the rows
    OraclePSRS.step accepts -- with zeros in pi and p_log, NaN, f16 / f32 / f64 logs, one to five actions."""
    g = np.random.default_rng(7)
    for nA, dt in ((1, np.float64), (2, np.float32), (5, np.float16), (3, np.float64), (5, np.float32)):
        N = 400
        p = g.dirichlet(np.ones(nA), N).astype(dt)
        p[g.random((N, nA)) < 0.1] = 0
        pi = g.dirichlet(np.ones(nA), 1)
        if nA > 1:
            pi[0, g.integers(nA)] = 0.0
        a = g.integers(0, nA, N)
        zeros = np.zeros(N, np.int64)
        ora = O.OraclePSRS(zeros, a, np.zeros(N), zeros, np.zeros(N, bool), p.astype(np.float64), np.ones(N, bool))
        for seed in (0, 5):
            ora.reset_sampler(seed)
            assert ora.reset() is not None
            got = []
            while True:
                row, _ = ora.step(pi[0])
                if row is None:
                    break
                got.append(row)
            q = O.permutation(seed, N)
            k53 = H.draws("pcg64", seed, N)
            want = [int(r) for i, r in enumerate(q) if k53[i] <= H.threshold(pi[0], p[r], int(a[r]))]
            assert got == want, (nA, dt, seed)


def test_threshold_rules():
    assert H.threshold([0.5, 0.5], [0.5, 0.5], 0) == H.T_MAX            # thr == 1
    assert H.threshold([0.5, 0.5], [-0.5, -1.0], 0) == H.T_MAX          # thr == 2
    assert H.threshold([1.0, 0.0], [0.5, 0.0], 0) == H.T_MAX            # 0 / 0: NaN
    assert H.threshold([1.0, 0.0], [0.5, 0.5], 1) == 0                  # pi[a] == 0
    assert H.threshold([0.5, 0.5], [-0.5, 0.5], 0) == 0                 # thr < 0
    assert H.threshold([0.5, 0.5], [1.0, 0.5], 0) == 1 << 52            # thr == 0.5
    assert H.threshold([0.5, 0.5], [0.5, 0.0], 0) == 0                  # M == inf
    assert H.threshold([0.5, 0.5], np.array([2.0 ** -14, 1.0], np.float16), 1) == 1 << 39  # f16 widened exactly: thr == 2^-14


def test_key_and_digest_fields():
    T = (0x155555 << 32) | 0x89ABCDEF
    assert H.key(T, 0, 0) == (0x155555 << 43) | 0x89ABCDEF
    assert H.key(T, 1, 0) == (0x155555 << 43) | (1 << 42) | 0x89ABCDEF
    assert H.key(T, 0, 1023) == (0x155555 << 43) | (0x3FF << 32) | 0x89ABCDEF
    assert H.key(H.T_MAX, 1, 1023) == (1 << 64) - 1
    assert H.key(0, 0, 0) == 0 and H.key(1 << 32, 0, 0) == 1 << 43 and H.key((1 << 32) - 1, 0, 0) == (1 << 32) - 1
    k = H.key(T, 1, 254)
    assert H.digest(k, "A") == (0x155555 << 11) | 0x400 | 254
    assert H.digest(k, "B") == ((0x155555 >> 5) << 16) | 0x400 | 254
    assert H.digest(k, "C") == ((0x155555 >> 7) << 18) | 0x400 | 254
    # the local row's upper bits: B carries bits 16..22 (hi 1..0 in bits 8, 9; hi 6..2 in bits 11..15), C bits 8..16 (hi 8..2 in bits 11..17)
    assert H.digest(0, "B", 1 << 16) == 1 << 8 and H.digest(0, "B", 1 << 17) == 1 << 9 and H.digest(0, "B", 1 << 18) == 1 << 11
    assert H.digest(0, "B", (1 << 23) - 1) == 0xFB00 and H.digest(0, "B", 0xFFFF) == 0
    assert H.digest(0, "C", 1 << 8) == 1 << 8 and H.digest(0, "C", 1 << 9) == 1 << 9 and H.digest(0, "C", 1 << 10) == 1 << 11
    assert H.digest(0, "C", (1 << 17) - 1) == 0x3FB00 and H.digest(0, "C", 0xFF) == 0 and H.digest(0, "C", 0x1FF00) == 0x3FB00
    # the payload closest to all ones: done, z_next 254, every local-row bit -- one short of the mask a draw is laid down with
    assert H.digest(H.key(0, 1, 254), "C", 0x1FF00) == 0x3FFFE and H.digest(H.key(0, 1, 254), "B", (1 << 23) - 1) == 0xFFFE


def test_building_twice_gives_the_same_bytes():
    first = H.table_a(3)
    H._CACHE.clear()
    second = H.table_a(3)
    assert first is not second
    for k, v in first["log"].items():
        assert v.tobytes() == second["log"][k].tobytes() and v.dtype == second["log"][k].dtype, k
    assert first["records"] == second["records"] and first["skipped"] == second["skipped"]
    H._CACHE[("a", 3, "pcg64")] = first
