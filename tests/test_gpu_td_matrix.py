"""k_eval_mc<PL, double, TD = true> (offsim_eval_td through BatchedPSRS.eval_td) against the plain Python learner loop of tests/td_host.py,
bit for bit, over the case list of tests/td_cases.py: every p_log instance under both updates, every launch shape (4 / 2 / 1 learners per
workgroup, the path above 64 KiB, the last size that fits 160 KiB and the first that does not), several learners per launch with their own
Q tables, tie streams and samplers, Philox and REJECT_NEVER, schedules and their clamp, snapshot strides, caps smaller than the run, every
way a run ends, and a second call that resumes from what the first wrote back.  tests/test_td_matrix_host.py checks, without a device,
that the host loop reproduces the reference's recorded runs and that the case list covers what it claims."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import td_cases as K  # noqa: E402
import td_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch.device("cuda", 0)


_TABLES = {}


def table_of(spec, gpu):
    from rl_offline_simulation_amd.table import TransitionTable
    if spec not in _TABLES:
        a, log = K.arrays(spec), K.log_of(spec)
        t = TransitionTable(a["z"], a["a"], a["r"], a["z_next"], a["done"], a["p_log"], a["t0"], device=gpu)
        assert t.n_slots == log.n_slots == spec.nS and np.array_equal(t.slot_z, log.slot_z)  # the dense map the host loop restates
        assert str(t.p_log.dtype) == {"f64": "torch.float64", "f32": "torch.float32", "f16": "torch.float16"}[spec.pl]
        _TABLES[spec] = t
    return _TABLES[spec]


def fresh_env(case, gpu):
    from rl_offline_simulation_amd.evaluators import BatchedPSRS
    table = table_of(case.table, gpu)
    env = BatchedPSRS(table, case.R, reject_mode=case.reject)
    kw = dict(rejection=case.stream)
    if case.reset == "keyed":
        env.reset_sampler(case.seeds, policy=K.pi_of(case), **kw)
        # keyed: the orders exist as candidate streams only and eval_td rebuilds the permutations (unless the variant matrix of
        # test_gpu_edges.py has switched the row-packed scan off)
        assert env.state.perm is None or os.environ.get("OFFSIM_SCAN_ROWS", "1") in ("0", "auto")
    elif case.reset == "shared":
        env.reset_sampler(case.seeds, shuffle="shared", shuffle_seed=K.SHUFFLE_SEED, **kw)
    else:
        env.reset_sampler(case.seeds, **kw)
    return env


def launch(case, env, q, mt, n_episodes):
    from rl_offline_simulation_amd import _lib as L
    kw = K.run_args(case)
    o = env.eval_td(K.pi_of(case), kw.pop("gamma"), kw.pop("mode"), kw.pop("alpha"), q_slots=q, n_episodes=n_episodes, n_gamma_pow=case.n_gamma_pow,
                    tie_mt=mt, **kw)
    torch.cuda.synchronize()
    L.check_async_faults()
    return {k: v.cpu().numpy() for k, v in o.items() if not k.startswith("_")}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype == np.float64:
        return b.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    return np.array_equal(a.astype(np.int64), b.astype(np.int64))


def first_difference(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape:
        return f"shapes {a.shape} / {b.shape}"
    ne = (a.view(np.uint64) != b.view(np.uint64)) if a.dtype == np.float64 else (a.astype(np.int64) != b.astype(np.int64))
    i = tuple(int(x[0]) for x in np.nonzero(ne))
    return f"{int(ne.sum())} of {ne.size} differ, first at {i}: device {a[i]!r}, host {b[i]!r}"


def compare(case, o, ref, what):
    trace_cap, ep_cap = K.caps_of(case)
    keys = ["q", "sum_g", "n_ep", "steps", "cand", "n_len", "status"]
    if trace_cap:
        keys += ["trace_row", "trace_pop", "td_err"] + (["beh_arg"] if case.behaviour == H.EPS_GREEDY else [])
    if ep_cap:
        keys += ["ep_g", "ep_len"]
    if case.snap_cap:
        keys.append("q_snap")
    assert set(keys) | ({"tie_mt"} if case.mt != "none" else set()) == set(o), (what, sorted(o))
    for k in keys:  # every returned tensor, every learner, bit for bit
        dev = o[k]
        print(f"{case.name} {what} {k}: {'equal' if same_bits(dev, ref[k]) else first_difference(dev, ref[k])}")
        assert same_bits(dev, ref[k]), (case.name, what, k, first_difference(dev, ref[k]))
    if case.mt != "none":
        dev = o["tie_mt"].view(np.uint32)
        assert same_bits(dev, ref["tie_mt"]), (case.name, what, "tie_mt", first_difference(dev, ref["tie_mt"]))


def compare_state(case, env, ref):
    st = env.state
    assert same_bits(st.init_cursor.cpu().numpy(), ref["init_cursor"]), (case.name, "init_cursor")
    assert same_bits(st.cur_slot.cpu().numpy(), ref["cur_slot"]), (case.name, "cur_slot", st.cur_slot.cpu().numpy(), ref["cur_slot"])
    assert same_bits(st.cursor.cpu().numpy(), ref["cursor"]), (case.name, "cursor", first_difference(st.cursor.cpu().numpy(), ref["cursor"]))


def run_case(case, gpu):
    """All calls of the case on a fresh environment: [(outputs of the call, host outputs)], and the environment afterwards."""
    refs = K.host(case)
    env = fresh_env(case, gpu)
    q, mt = K.q_init_of(case), K.mt_of(case)
    outs = []
    for i, ref in enumerate(refs):
        n_ep = case.n_episodes if case.resume_k is None else (case.resume_k if i == 0 else None)
        o = launch(case, env, q, mt, n_ep)
        compare(case, o, ref, f"call {i}")
        compare_state(case, env, ref)
        outs.append(o)
        q, mt = torch.from_numpy(o["q"]).to(gpu), (None if mt is None else torch.from_numpy(o["tie_mt"]).to(gpu))  # the resume path
    return env, outs, refs


RUNNABLE = [c for c in K.CASES if not c.refused]


@pytest.mark.parametrize("name", [c.name for c in RUNNABLE])
def test_learner_kernel_equals_the_host_loop(name, gpu):
    from rl_offline_simulation_amd import _lib as L
    case = K.BY_NAME[name]
    waves, lds, refused = case.shape
    assert not refused
    env, outs, refs = run_case(case, gpu)
    # where the sampler stands: one more reset and one more step serve what the oracle serves from the same cursors and stream position
    init_row = env.reset().cpu().numpy().copy()
    p = np.full((case.R, case.table.nA), 1.0 / case.table.nA)
    row, status, popped = (x.cpu().numpy().copy() for x in env.step(p))
    L.check_async_faults()
    after = refs[-1]["after"]
    assert np.array_equal(init_row, after[:, 0]), (name, "initial row after the run", init_row, after[:, 0])
    assert np.array_equal(status, after[:, 2]), (name, "status of the next step", status, after[:, 2])
    ok = after[:, 2] == H.ST_OK
    assert np.array_equal(row[ok], after[ok, 1]) and np.array_equal(popped, after[:, 3]), (name, "next step", row, popped, after)
    # the same inputs once more: the same bits
    if case.resume_k is None:
        _, again, _ = run_case(case, gpu)
        for k in outs[0]:
            assert same_bits(outs[0][k], again[0][k]), (name, "second run", k)


def test_one_size_class_above_160_kib_is_refused_and_nothing_runs(gpu):
    from rl_offline_simulation_amd import _lib as L
    case = K.BY_NAME["lds-160k-first-refused"]
    assert case.shape[2] and not K.BY_NAME["lds-160k-last-that-fits-R2"].shape[2]
    env = fresh_env(case, gpu)
    kw = K.run_args(case)
    with pytest.raises(L.OffsimError, match=f"offsim error {L.EUNSUPPORTED}: eval_td: .*160 KiB"):
        env.eval_td(K.pi_of(case), kw.pop("gamma"), kw.pop("mode"), kw.pop("alpha"), q_slots=K.q_init_of(case), **kw)
    torch.cuda.synchronize()
    L.check_async_faults()
    st = env.state
    assert not st.cursor.any() and not st.init_cursor.any() and bool((st.cur_slot == -1).all())


def test_no_learners_no_launch(gpu):
    """R = 0: OFFSIM_OK, and the buffers of a three-learner environment handed over with it stay as they were."""
    from rl_offline_simulation_amd import _lib as L
    case = K.BY_NAME["pl-f32-qlearn-soft-R5"]
    env = fresh_env(case, gpu)
    t, st = env.table, env.state
    i64 = lambda: torch.full((case.R,), -7, dtype=torch.int64, device=gpu)  # noqa: E731
    o = dict(sum_g=torch.full((case.R,), -7.0, dtype=torch.float64, device=gpu), n_ep=i64(), steps=i64(), cand=i64(), n_len=i64(),
             status=torch.full((case.R,), -7, dtype=torch.int32, device=gpu))
    q = torch.full((case.R, t.n_slots, t.nA), 0.5, dtype=torch.float64, device=gpu)
    pi = torch.from_numpy(K.pi_of(case)).to(gpu)
    ro = L.Rollouts(R=0, rng=L.ptr(st.rng), cursor=L.ptr(st.cursor), init_cursor=L.ptr(st.init_cursor), cur_slot=L.ptr(st.cur_slot), perm=L.ptr(st.perm),
                    perm_stride=st.perm_stride, init_perm=L.ptr(st.init_perm), init_stride=st.init_stride, rng_kind=st.rng_kind)
    oc = L.EvalMCOut(**{k: L.ptr(v) for k, v in o.items()})
    td = L.TD(mode=L.TD_QLEARN, alpha=0.1, q=L.ptr(q), behaviour=L.BEHAVIOUR_SOFT_GREEDY, snap_stride=1)
    before = [x.clone() for x in (st.rng, st.cursor, st.init_cursor, st.cur_slot)]
    rc = L.load().offsim_eval_td(C.byref(t.c), C.byref(ro), L.ptr(pi), L.REJECT_DEFAULT, 0.9, None, 0, 1 << 62, C.byref(oc), C.byref(td), L.stream_ptr())
    torch.cuda.synchronize()
    L.check_async_faults()
    assert rc == L.OK
    assert all(bool((v == -7).all()) for v in o.values()) and bool((q == 0.5).all())
    for a, b in zip(before, (st.rng, st.cursor, st.init_cursor, st.cur_slot)):
        assert torch.equal(a, b)
