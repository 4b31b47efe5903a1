"""What the row-policy queue tests (tests/test_gpu_queue_rows_policy.py) rest on, checked without a device: the plain Python loop of
tests/queue_rows_policy_host.py reproduces what the reference's own evalMC returned on its own QueueEvaluator_impl for a policy over
observations (tests/golden/queue_obs_policy/*.npz); with tables built from a [nZ, nA] policy it is queue_host.run's evalMC; the C ABI of
offsim_eval_queue_rows_policy / _pop refuses every bad argument before any HIP call (the pointers are fake addresses: a launch would fault);
and the case list reaches what it names."""
import ctypes
import glob
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import queue_host as H  # noqa: E402
import queue_rows_policy_host as Q  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "queue_obs_policy", "*.npz")))
F = 0x1000
NAMES = ("offsim_eval_queue_rows_policy", "offsim_eval_queue_rows_policy_pop")


def golden_log(path):
    d = np.load(os.path.join(ROOT, "tests", "golden", os.path.basename(path)))  # the inputs live beside the folder
    return H.Log(d["in_z"], d["in_a"], d["in_r"], d["in_z_next"], d["in_done"], d["in_p_log"], d["in_t0"])


def test_two_fixtures_with_every_run():
    assert len(FIXTURES) == 2
    for f in FIXTURES:
        d = np.load(f)
        assert all(f"{tag}_s{s}_Gs" in d.files and len(d[f"{tag}_s{s}_Gs"]) == int(d["n_episodes"]) >= 3 for s in d["seeds"] for tag in ("f64", "f32"))
        assert os.path.getsize(f) < 512 * 1024


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(f)[:-4] for f in FIXTURES])
def test_host_loop_replays_the_reference(path):
    d, log = np.load(path), golden_log(path)
    cap, n = log.N + 1, int(d["n_episodes"])
    for tag, cast in (("f64", np.float64), ("f32", np.float32)):
        pn, p0 = d["P_next"].astype(cast), d["P_init"].astype(cast)
        for s in (int(v) for v in d["seeds"]):
            k = f"{tag}_s{s}_"
            gen = np.random.default_rng(1000 + s)
            o = Q.run(H.Sampler(log, s), gen, pn, p0, float(d["gamma"]), n_episodes=n, trace_cap=cap, ep_cap=cap)
            m = o["steps"]
            assert o["status"] == H.ST_OK and o["n_ep"] == n == o["n_len"] and m == len(d[k + "rows"]), k
            assert np.array_equal(o["ep_g"][:n], d[k + "Gs"]) and np.array_equal(o["ep_len"][:n], d[k + "lengths"]), k
            assert np.array_equal(o["trace_row"][:m], d[k + "rows"]) and np.array_equal(o["trace_pop"][:m], d[k + "actions"]), k
            assert o["cur_slot"] == (int(d[k + "z"]) - log.z_lo) * log.nA and o["obs_row"] == d[k + "rows"][-1], k
            # exactly one draw per step: the stream stands where the reference's rng.choice calls left it
            ref = np.random.default_rng(1000 + s)
            ref.random(m)
            assert np.array_equal(o["rng"], H.rng_words(ref)), k


@pytest.mark.parametrize("name", ["evalmc-R5", "evalmc-neg-state-zeros-R5", "evalmc-short-rows-R5", "evalmc-holes-R9", "evalmc-max-episodes-R5"])
def test_tables_of_a_tabular_policy_give_queue_hosts_evalmc(name):
    """p_next[i] = pi[z_next[i]], p_init[i] = pi[z[i]]: every output and the state left behind equal queue_host.run(mode=EVALMC)."""
    c = H.BY_NAME[name]
    lg, pi = c.log, c.pi()
    pn, p0 = pi[lg.z_next - lg.z_lo], pi[lg.z - lg.z_lo]
    for i, (s, sa) in enumerate(zip(c.seeds, c.action_seeds)):
        want = c.host()[i]
        got = Q.run(H.Sampler(lg, s), np.random.default_rng(sa), pn, p0, H.GAMMA, **{k: v for k, v in c.kw().items() if k in ("n_episodes", "trace_cap", "ep_cap")})
        for k in ("sum_g", "n_ep", "steps", "cand", "n_len", "status", "ep_g", "ep_len", "trace_row", "trace_pop", "obs_row", "cursor", "init_cursor",
                  "cur_slot", "rng"):
            assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (name, i, k)


def test_grouped_order_and_cur_row():
    c = Q.BY_NAME["base-f64"]
    lg, order = c.log, Q.grouped_order(c.log)
    comp = (lg.z - lg.z_lo) * lg.nA + lg.a
    assert np.all(np.diff(comp[order]) >= 0) and all(np.all(np.diff(order[comp[order] == v]) > 0) for v in np.unique(comp))
    for o in c.host():
        m = o["steps"]
        assert o["cur_row"] == (np.flatnonzero(order == o["trace_row"][m - 1])[0] if o["obs_row"] >= 0 else -2 - list(np.flatnonzero(lg.t0)).index(-2 - o["obs_row"]))


@pytest.mark.parametrize("case", Q.CASES, ids=[c.name for c in Q.CASES])
def test_every_case_reaches_the_branch_it_names(case):
    outs = case.host()
    assert len(outs) == 5 and case.reaches <= set().union(*(o["branches"] for o in outs)), case.name
    lg = case.log
    if case.n_slots:  # the stretched logs keep dense slots (TransitionTable's rule), or the one-launch drivers refuse them
        comp = np.concatenate([(lg.z - lg.z_lo) * lg.nA + lg.a, (lg.z_next - lg.z_lo) * lg.nA])
        assert lg.n_slots == case.n_slots <= max(1024, 4 * len(np.unique(comp)))
    if case.bad_rows:
        pn = case.tables()[0]
        assert np.isnan(pn[0]).all() and (pn[3] == 0).all()
        stopped = [pn[o["trace_row"][o["steps"] - 1]] for o in outs if o["status"] == H.ST_KEYERROR and o["steps"]]
        assert any(np.isnan(r).all() for r in stopped) and any((r == 0).all() for r in stopped)
        assert all(o["trace_pop"][o["steps"]] == lg.nA for o in outs if o["status"] == H.ST_KEYERROR)
    if case.name == "holes":
        assert all(o["trace_pop"][o["steps"]] < lg.nA for o in outs if o["status"] == H.ST_KEYERROR)
    if case.n_episodes is not None:
        assert all(o["n_ep"] == case.n_episodes and o["n_len"] == case.n_episodes and o["status"] == H.ST_OK for o in outs)
    if case.name == "episodes-0":
        assert all(o["cur_row"] is None and o["obs_row"] == -(1 << 31) and o["steps"] == 0 for o in outs)


def test_the_cases_cover_the_launch_shapes():
    shape = {c.name: Q.launch_shape(c.log.n_slots, c.log.nA) for c in Q.CASES}
    assert shape["base-f64"][0] == 4 and shape["waves2"][0] == 2 and shape["waves2"][1] <= 65536
    assert shape["waves1-big"][0] == 1 and 65536 < shape["waves1-big"][1] <= 160 * 1024 and not any(s[2] for s in shape.values())
    assert Q.lds_bytes(4, 25, 5) == (26 + 100) * 4 + 4 * 5 * 8 == 664 and Q.lds_bytes(1, 10, 3) == 88 + 24  # (21 words padded to 22)
    assert {c.nA for c in Q.CASES} >= {2, 5, 16} and any(c.f32 for c in Q.CASES) and any(c.r32 for c in Q.CASES) and any(c.neg_state for c in Q.CASES)
    assert all(c.R == 5 for c in Q.CASES)


# ---- the C ABI ----
@pytest.mark.parametrize("n", NAMES)
def test_symbols_exported_bound_and_documented(n):
    from rl_offline_simulation_amd import _lib
    src = open(os.path.join(ROOT, "include", "offsim.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert "int " + n + "(" in src and hasattr(lib, n) and n in _lib.SIGNATURES
    doc = src[src.index("/* " + n + ":"):src.index("int " + n + "(")]
    for word in ("Identity", "cur_row", "OFFSIM_EINVAL"):
        assert word in doc, word
    if n.endswith("_pop"):
        assert "policy-major" in doc and "r % S" in doc and "1..65535" in doc
    else:
        for word in ("rgument validation happens before any HIP call", "OFFSIM_STREAM_PHILOX", "OFFSIM_EUNSUPPORTED", "160 KiB", "tabular.py:",
                     "queue_evaluator.py:", "ppo.py:", "never read", "env.reset()"):
            assert word in doc, word


def _call(pop=False, R=6, t=None, ro=True, nA=2, p_next=F, p_init=F, dt=0, kind=0, out=True, gp=None, n_gp=0, rng=F, L_=2, S=3, cur_row=None, **outkw):
    """the entry point on fake pointers; t: table fields to change (False: NULL)."""
    from rl_offline_simulation_amd import _lib as L
    tc = L.Table(N=10, n_slots=6, nA=2, plog_dtype=L.F32, r_dtype=L.F32, seg_off=F, p_log=F, a=F, r=F, z_next=F, done=F, orig_idx=F, N0=2,
                 init_slot=F, init_orig=F)
    for k, v in (t or {}).items():
        setattr(tc, k, v)
    roc = L.Rollouts(R=R, rng=rng, cursor=F, init_cursor=F, cur_slot=F, rng_kind=kind)
    okw = dict(sum_g=F, n_ep=F, steps=F, cand=F, n_len=F, status=F)
    okw.update(outkw)
    oc = L.EvalMCOut(**okw)
    head = (None if t is False else ctypes.byref(tc), ctypes.byref(roc) if ro else None, nA, p_next, p_init, dt)
    tail = (0.9, gp, n_gp, 10, ctypes.byref(oc) if out else None, cur_row, None, None)
    if pop:
        return L.load().offsim_eval_queue_rows_policy_pop(*head, L_, S, *tail)
    return L.load().offsim_eval_queue_rows_policy(*head, *tail)


@pytest.mark.parametrize("pop", [False, True], ids=["single", "pop"])
def test_validation_before_any_hip_call(pop):
    from rl_offline_simulation_amd import _lib as L
    err = L.load().offsim_last_error
    call = lambda **kw: _call(pop=pop, **kw)  # noqa: E731
    assert _call(pop=False, R=0) == L.OK, err()  # R = 0 validates and launches nothing
    assert _call(pop=False, R=0, dt=L.F64, cur_row=F) == L.OK
    # the action stream: Philox is refused, nothing is stepped
    assert call(kind=L.STREAM_PHILOX) == L.EUNSUPPORTED and b"(0, 1]" in err()
    assert call(kind=5) == L.EINVAL
    # the table and its key
    assert call(t=False) == L.EINVAL and call(t=dict(seg_off=None)) == L.EINVAL and call(t=dict(init_slot=None)) == L.EINVAL
    assert call(t=dict(n_slots=7)) == L.EINVAL and b"multiple of nA" in err()
    assert call(nA=3) == L.EINVAL and b"table's nA" in err()
    assert call(nA=0) == L.EINVAL
    # NULLs
    assert call(ro=False) == L.EINVAL and call(R=-1) == L.EINVAL and call(rng=None) == L.EINVAL
    assert call(out=False) == L.EINVAL and call(status=None) == L.EINVAL and call(sum_g=None) == L.EINVAL
    assert call(p_next=None) == L.EINVAL and b"p_next / p_init" in err() and call(p_init=None) == L.EINVAL
    assert _call(pop=False, R=0, p_next=None, t=dict(N=0)) == L.OK and _call(pop=False, R=0, p_init=None, t=dict(N0=0)) == L.OK
    assert call(n_gp=4) == L.EINVAL and b"gamma_pow" in err()
    assert call(ep_cap=-1) == L.EINVAL and call(trace_cap=-1) == L.EINVAL
    # the element type
    assert call(dt=L.F16) == L.EINVAL and b"p_dtype" in err() and call(dt=-1) == L.EINVAL and call(dt=3) == L.EINVAL
    if pop:  # the population
        for bad in (dict(L_=0, S=3, R=0), dict(L_=65536, S=1, R=65536), dict(L_=2, S=0, R=0), dict(L_=2, S=3, R=5), dict(L_=-1, S=-6)):
            assert _call(pop=True, **bad) == L.EINVAL and b"1..65535" in err(), bad
        assert _call(pop=True, R=0, L_=1, S=0) == L.EINVAL  # (S >= 1 even where R = 0)
    # the LDS size: refused when one rollout does not fit 160 KiB (queue_rows_policy_host.lds_bytes restates the carve)
    big = lambda n, **kw: call(t=dict(n_slots=n, nA=5), nA=5, **kw)  # noqa: E731
    n_ref = next(n for n in range(5, 1 << 20, 5) if Q.launch_shape(n, 5)[2])
    assert n_ref == 20475 and Q.lds_bytes(1, n_ref - 5, 5) == 163808
    if not pop:
        assert big(n_ref - 5, R=0) == L.OK
    assert big(n_ref) == L.EUNSUPPORTED and b"160 KiB" in err()
    assert big(5 << 20) == L.EUNSUPPORTED
