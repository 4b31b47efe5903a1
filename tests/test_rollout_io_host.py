"""The host plumbing every rollout launch and seed-tile driver shares (evaluators/rollout_io.py, and the tile default in batched.py),
checked without a device: CPU tensors only, the library is never loaded.  What the launches compute with these pieces is pinned by the
GPU tests of the six launch sites and five drivers."""
import os
import sys
import types
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rl_offline_simulation_amd import _lib as L  # noqa: E402
from rl_offline_simulation_amd.evaluators import batched as B  # noqa: E402
from rl_offline_simulation_amd.evaluators import rollout_io as IO  # noqa: E402

CPU = torch.device("cpu")
REQUIRED = {"sum_g": torch.float64, "n_ep": torch.int64, "steps": torch.int64, "cand": torch.int64, "n_len": torch.int64, "status": torch.int32}
OPTIONAL = ("ep_g", "ep_len", "trace_row", "trace_pop", "dbg")


def test_ptr_of_a_cpu_tensor_is_its_data_ptr():
    """What the struct comparisons below rest on."""
    x = torch.zeros(3)
    assert L.ptr(x) == x.data_ptr() and L.ptr(None) is None


def test_module_is_a_leaf():
    src = open(IO.__file__).read()
    assert not any(f"from .{m}" in src or f"import {m}" in src for m in ("batched", "psrs", "psrs_exo", "obs_policy"))


def test_rollout_outputs_with_every_optional_output():
    o, oc = IO.rollout_outputs(3, CPU, ep_cap=2, trace_cap=4)
    assert set(o) == set(REQUIRED) | {"ep_g", "ep_len", "trace_row", "trace_pop"}
    for k, dt in REQUIRED.items():
        assert o[k].shape == (3,) and o[k].dtype == dt
    assert o["ep_g"].shape == (3, 2) and o["ep_g"].dtype == torch.float64 and not o["ep_g"].any()
    assert o["ep_len"].shape == (3, 3) and o["ep_len"].dtype == torch.int32 and not o["ep_len"].any()
    assert o["trace_row"].shape == (3, 4) and o["trace_row"].dtype == torch.int32 and (o["trace_row"] == -1).all()
    assert o["trace_pop"].shape == (3, 4) and o["trace_pop"].dtype == torch.int32 and not o["trace_pop"].any()
    for k in o:
        assert getattr(oc, k) == o[k].data_ptr(), k
    assert oc.dbg is None
    assert (oc.ep_cap, oc.trace_cap) == (2, 4)
    assert {f for f, _ in L.EvalMCOut._fields_} == set(REQUIRED) | set(OPTIONAL) | {"ep_cap", "trace_cap"}  # (no field the builder could miss)


def test_rollout_outputs_without_caps():
    o, oc = IO.rollout_outputs(3, CPU)
    assert set(o) == set(REQUIRED)
    assert all(getattr(oc, k) is None for k in OPTIONAL)
    assert (oc.ep_cap, oc.trace_cap) == (0, 0)
    assert all(getattr(oc, k) == o[k].data_ptr() for k in REQUIRED)


def test_rollout_outputs_reuses_the_callers_required_tensors():
    mine = {"sum_g": torch.full((3,), 7.0, dtype=torch.float64), "status": torch.full((3,), 5, dtype=torch.int32)}
    given = dict(mine)
    o, oc = IO.rollout_outputs(3, CPU, ep_cap=1, out=given)
    assert o["sum_g"] is mine["sum_g"] and o["status"] is mine["status"]
    assert float(o["sum_g"][0]) == 7.0 and int(o["status"][2]) == 5  # (not refilled)
    assert oc.sum_g == mine["sum_g"].data_ptr() and oc.status == mine["status"].data_ptr()
    theirs = {x.data_ptr() for x in mine.values()}
    for k in ("n_ep", "steps", "cand", "n_len"):
        assert o[k].shape == (3,) and o[k].dtype == REQUIRED[k] and o[k].data_ptr() not in theirs
    # the optional ones are allocated afresh even when the dict holds one from an earlier call
    o2, _ = IO.rollout_outputs(3, CPU, ep_cap=1, out=o)
    assert o2 is o and not o2["ep_g"].any()


def test_rollout_outputs_dbg():
    o, oc = IO.rollout_outputs(3, CPU, dbg=True)
    assert o["dbg"].shape == (3, 4) and o["dbg"].dtype == torch.int64 and not o["dbg"].any()
    assert oc.dbg == o["dbg"].data_ptr()
    assert "dbg" not in IO.rollout_outputs(3, CPU)[0]


def test_td_outputs():
    q = torch.zeros((3, 5, 2), dtype=torch.float64)
    o = {}
    IO.td_outputs(o, q, trace_cap=4, snap_cap=2, beh_arg=True)
    assert set(o) == {"td_err", "beh_arg", "q_snap"}
    assert o["td_err"].shape == (3, 4) and o["td_err"].dtype == torch.float64 and not o["td_err"].any()
    assert o["beh_arg"].shape == (3, 4) and o["beh_arg"].dtype == torch.int32 and not o["beh_arg"].any()
    assert o["q_snap"].shape == (3, 2, 5, 2) and o["q_snap"].dtype == torch.float64 and not o["q_snap"].any()
    o = {}
    IO.td_outputs(o, q, trace_cap=4, snap_cap=0)
    assert set(o) == {"td_err"}
    o = {}
    IO.td_outputs(o, q, trace_cap=0, snap_cap=0, beh_arg=True)  # (no trace: no beh_arg either)
    assert o == {}


def test_episode_bound():
    assert IO.episode_bound(None) == 1 << 62 and IO.episode_bound(np.int64(7)) == 7 and type(IO.episode_bound(np.int64(7))) is int


def _state():
    S, n_slots = 2, 3
    return types.SimpleNamespace(
        R=S, rng=torch.arange(S * 4, dtype=torch.int64).reshape(S, 4) + 100, cursor=torch.arange(S * n_slots, dtype=torch.int32).reshape(S, n_slots) + 10,
        init_cursor=torch.tensor([5, 6], dtype=torch.int32), cur_slot=torch.tensor([2, -1], dtype=torch.int32),
        perm=torch.arange(S * 7, dtype=torch.int32).reshape(S, 7), perm_stride=7, init_perm=torch.arange(S * 4, dtype=torch.int32).reshape(S, 4),
        init_stride=4, rng_kind=L.STREAM_PHILOX)


def test_population_state_copies():
    st = _state()
    before = {k: getattr(st, k).clone() for k in ("rng", "cursor", "init_cursor", "cur_slot", "perm", "init_perm")}
    ro, cp = IO.population_state(st, 3)
    assert list(cp) == ["rng", "cursor", "init_cursor", "cur_slot"]
    for k, v in cp.items():
        src = getattr(st, k)
        assert torch.equal(v, src.repeat(3, 1) if src.dim() == 2 else src.repeat(3)) and v.dtype == src.dtype
        assert v.data_ptr() != src.data_ptr()
        assert getattr(ro, k) == v.data_ptr()
        v.add_(1)  # a launch advances its copies ...
    for k, v in before.items():
        assert torch.equal(getattr(st, k), v), k  # ... and the originals stay
    assert ro.R == 6
    assert ro.perm == st.perm.data_ptr() and ro.init_perm == st.init_perm.data_ptr()
    assert (ro.perm_stride, ro.init_stride, ro.rng_kind) == (7, 4, L.STREAM_PHILOX)
    st.perm = st.init_perm = None  # table order
    ro, _ = IO.population_state(st, 3)
    assert ro.perm is None and ro.init_perm is None


def test_population_result():
    st = _state()
    _, cp = IO.population_state(st, 3)
    flat = {"x": torch.arange(30).reshape(6, 5), "n": torch.arange(6)}
    keep = (object(), None)
    o = IO.population_result(dict(flat), 3, 2, cp, keep, "k_name")
    assert set(o) == {"x", "n", "_keepalive", "_kernel"}
    assert o["x"].shape == (3, 2, 5) and o["n"].shape == (3, 2)
    assert torch.equal(o["x"][1, 1], flat["x"][3]) and int(o["n"][2, 0]) == 4  # member l's rollout j was row l * S + j
    assert o["_kernel"] == "k_name"
    assert o["_keepalive"][:2] == keep and all(a is b for a, b in zip(o["_keepalive"][2:], cp.values())) and len(o["_keepalive"]) == 6
    assert flat["x"].shape == (6, 5) and cp["rng"].shape == (6, 4)  # (views: nothing reshaped in place)
    o = IO.population_result(dict(flat), 3, 2, cp, keep, "k_name", state=True)
    assert set(o["_state"]) == set(cp)
    assert {k: tuple(v.shape) for k, v in o["_state"].items()} == {"rng": (3, 2, 4), "cursor": (3, 2, 3), "init_cursor": (3, 2), "cur_slot": (3, 2)}
    assert o["_state"]["rng"].data_ptr() == cp["rng"].data_ptr()


def test_seed_tiles():
    seeds = np.arange(5, dtype=np.uint64) + 40
    made = []

    def make(n):
        made.append(n)
        return ("env", n, len(made))
    tiles = list(IO.seed_tiles(seeds, 2, make))
    assert [b for b, _, _ in tiles] == [0, 2, 4]
    assert [sd.tolist() for _, sd, _ in tiles] == [[40, 41], [42, 43], [44]]
    assert made == [2, 1]
    assert tiles[0][2] is tiles[1][2] and tiles[2][2] == ("env", 1, 2)
    for tile in (5, 9):
        made.clear()
        tiles = list(IO.seed_tiles(seeds, tile, make))
        assert len(tiles) == 1 and tiles[0][0] == 0 and tiles[0][1].tolist() == seeds.tolist() and made == [5]
    made.clear()
    assert list(IO.seed_tiles(seeds[:0], 2, make)) == [] and made == []


def test_default_tile():
    def never(table, keyed):
        raise AssertionError("the free memory is nobody's business when the rollouts share their queue orders")
    assert B.default_tile(None, 9, B.SHUFFLE_SHARED, keyed=True, resident=never) == 9
    assert B.default_tile(None, 9, B.SHUFFLE_NONE, keyed=False, resident=never) == 9
    asked = []

    def fit(n):
        def resident(table, keyed):
            asked.append((table, keyed))
            return n, 1, 2, 3
        return resident
    assert B.default_tile("t", 9, B.SHUFFLE_PER_ROLLOUT, keyed=True, resident=fit(4)) == 4
    assert B.default_tile("t", 9, B.SHUFFLE_PER_ROLLOUT, keyed=False, resident=fit(100)) == 9
    assert B.default_tile("t", 9, B.SHUFFLE_PER_ROLLOUT, keyed=False, resident=fit(0)) == 1
    assert B.default_tile("t", 0, B.SHUFFLE_PER_ROLLOUT, keyed=False, resident=fit(100)) == 1
    assert asked == [("t", True), ("t", False), ("t", False), ("t", False)]
    assert type(B.default_tile("t", 9, B.SHUFFLE_PER_ROLLOUT, keyed=True, resident=fit(np.int64(4)))) is int


def test_host_result():
    parts = {"sum_g": [np.array([1.0, 0.0]), np.array([3.0])], "n_ep": [np.array([2, 0]), np.array([4])]}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = IO.host_result(parts)
    assert set(res) == {"sum_g", "n_ep", "value"}
    assert res["sum_g"].tolist() == [1.0, 0.0, 3.0] and res["n_ep"].tolist() == [2, 0, 4]
    assert res["value"][0] == 0.5 and np.isnan(res["value"][1]) and res["value"][2] == 0.75
    cols = {"sum_g": [np.ones((2, 1)), np.ones((2, 2))], "n_ep": [np.ones((2, 1)), np.zeros((2, 2))]}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = IO.host_result(cols, axis=1, empty=(2, 0))
    assert res["value"].shape == (2, 3) and res["value"][:, 0].tolist() == [1.0, 1.0] and np.isinf(res["value"][:, 1:]).all()
    none = IO.host_result({"sum_g": [], "n_ep": []}, axis=1, empty=(2, 0))
    assert none["sum_g"].shape == none["value"].shape == (2, 0)
    with pytest.raises(ValueError):
        IO.host_result({"sum_g": [], "n_ep": []})  # (a driver without an empty form: NumPy's refusal, as before)


def test_tie_stream():
    words = np.random.default_rng(0).integers(0, 1 << 32, (2, 625), dtype=np.uint32)
    words[0, 0] = 0xFFFFFFFF
    mt = IO.tie_stream(words)
    assert mt.dtype == torch.int32 and mt.shape == (2, 625)
    assert np.array_equal(mt.numpy().view(np.uint32), words)
    assert IO.tie_stream(words[:, ::-1]).numpy().view(np.uint32).tolist() == words[:, ::-1].tolist()  # (a strided array)
    assert IO.tie_stream(mt) is mt and IO.tie_stream(mt, CPU) is mt
