"""The learner's collection on QueueEvaluator without a GPU: the mirror (tests/queue_collect_host.py) against what the reference's own
QueueEvaluator_impl produced (tests/golden/queue_collect/*.npz), its draw rule against Generator.choice, every case of the kernel matrix
shown to reach the branch it names, and the C ABI of offsim_queue_collect / _ppo / _ppo_pop refusing bad arguments before any HIP call
(the pointers are fake)."""
import ctypes
import glob
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import queue_collect_host as H  # noqa: E402
import queue_host as Q  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "queue_collect", "*.npz")))


def test_draw_rule_is_generator_choice_on_f32_rows():
    """draw(p32, gen) == gen.choice(nA, p=p32) with the f32 array passed, on aligned streams, and both consume one double per draw."""
    g = np.random.default_rng(11)
    a, b = np.random.default_rng(5), np.random.default_rng(5)
    n = 0
    for nA in (2, 3, 5, 16):
        x = g.standard_normal((1000, nA)) * 3
        e = np.exp(x - x.max(1, keepdims=True)).astype(np.float32)
        P = (e / e.sum(1, keepdims=True, dtype=np.float32)).astype(np.float32)
        for p in P:
            assert H.draw(p, a)[0] == int(b.choice(nA, p=p))
            n += 1
    assert n == 4000 and a.bit_generator.state == b.bit_generator.state
    # a row of NaN or zeros draws nothing and still consumes its double
    assert H.draw(np.full(3, np.nan, np.float32), a)[0] == 3 and H.draw(np.zeros(4), a)[0] == 4
    b.random(2)
    assert a.bit_generator.state == b.bit_generator.state


def test_fixtures_exist():
    assert len(FIXTURES) == 2


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_mirror_equals_the_reference(path):
    d = np.load(path)
    i = np.load(os.path.join(ROOT, "tests", "golden", os.path.basename(path)))
    log = Q.Log(*(i["in_" + k] for k in ("z", "a", "r", "z_next", "done", "p_log", "t0")))
    T = int(d["T"])
    for s in d["seeds"]:
        for cap in d["caps"]:
            env = H.Env(log, int(s), 500 + int(s))
            assert env.reset() is not None
            o = H.collect(env, T, int(cap), P_next=d["P_next"], P_init=d["P_init"])
            k = f"s{s}_cap{cap}_"
            assert np.array_equal(o["row"], d[k + "rows"]) and np.array_equal(o["action"], d[k + "actions"]), k
            assert np.array_equal(o["flags"], d[k + "flags"]) and o["status"] == int(d[k + "status"]), k
            assert np.array_equal(env.state()["rng"][:2], d[k + "rng"]), k
            assert (o["row"] >= 0).sum() > 0
    # the cap matters in the fixture: some step is truncated with it, none without
    assert any((d[f"s{s}_cap8_flags"] & H.TRUNCATED).any() for s in d["seeds"]) and not any((d[f"s{s}_cap0_flags"] & H.TRUNCATED).any() for s in d["seeds"])


def _mirror(c):
    lg = c.log
    pn, p0 = H.row_tables(lg, c.log_seed, c.ptype if c.form == "rows" else np.float32, c.nan_rows)
    outs, envs = [], c.envs()
    for e in envs:
        outs.append(H.collect(e, c.T, c.cap, pi=c.pi()) if c.form == "tabular" else H.collect(e, c.T, c.cap, P_next=pn, P_init=p0))
    return outs, envs


@pytest.mark.parametrize("c", H.CASES, ids=[c.name for c in H.CASES])
def test_case_reaches_its_branch(c):
    outs, envs = _mirror(c)
    status = [o["status"] for o in outs]
    flags = np.stack([o["flags"] for o in outs]) if c.T else np.zeros((len(outs), 0), np.uint8)
    for want in c.expect:
        if want in (H.TRUNCATED, H.TERMINATED, H.RESET):
            assert (flags & want).any(), (c.name, want)
        else:
            assert want in status, (c.name, want, status)
    if c.T:
        assert (flags & H.SERVED).any()
    if c.name == "exhausted":  # the stopped environment keeps its state and has drawn the unserved action
        k = status.index(H.ST_EXHAUSTED)
        i = int(np.flatnonzero(outs[k]["action"] >= 0)[-1])
        assert outs[k]["row"][i] == -1 and envs[k].sm.cur is not None and (outs[k]["action"][i + 1:] == -1).all()
    if c.name == "nan-rows-keyerror":  # a row from which no action can be drawn
        assert any((o["action"] == c.nA).any() for o in outs)
    if c.name == "holes-keyerror":  # a drawn pair that was never logged
        assert any(o["status"] == H.ST_KEYERROR and (o["action"] < c.nA).all() for o in outs)
    if c.name == "inactive":
        assert sum(s == H.ST_INACTIVE for s in status) == c.E - len(c.reset_envs)
        assert all((o["row"] == -1).all() and (o["action"] == -1).all() for o, s in zip(outs, status) if s == H.ST_INACTIVE)
    if c.name == "neg-state":
        assert c.log.z_lo == -1 and any(e.sm.cur == -1 or (c.log.z[o["row"][o["row"] >= 0]] == -1).any() for o, e in zip(outs, envs))
    if c.name == "no-init":
        assert all(e.obs_row == -1 and e.state()["cur_slot"] == -1 for e, s in zip(envs, status) if s == H.ST_NO_INIT)


def test_case_list_covers_the_matrix():
    forms = {(c.form, np.dtype(c.ptype).name if c.form != "mlp" else np.dtype(c.xtype).name) for c in H.CASES}
    assert {("mlp", "float32"), ("mlp", "float16"), ("rows", "float32"), ("rows", "float64"), ("tabular", "float64")} <= forms
    assert {(c.vf, c.bootstrap) for c in H.CASES if c.vf} == {("mlp", "reference"), ("mlp", "spinup"), ("rows", "reference"), ("rows", "spinup")}
    assert {2, 16} <= {c.nA for c in H.CASES} and any(c.act == "relu" for c in H.CASES)
    base = H.BY_NAME["mlp-f32"]
    assert (base.log.N, base.nZ, base.nA, base.E, base.T, base.cap) == (2000, 25, 5, 9, 40, 8)


# ---- the C ABI on fake pointers -------------------------------------------------------------------------------------------------
F = 0x1000


def _args(R=2, nA=2, n_slots=6, kind=None):
    from rl_offline_simulation_amd import _lib as L
    t = L.Table(N=10, n_slots=n_slots, nA=nA, plog_dtype=L.F32, r_dtype=L.F32, seg_off=F, p_log=F, a=F, r=F, z_next=F, done=F, orig_idx=F, N0=2,
                init_slot=F, init_orig=F)
    ro = L.Rollouts(R=R, rng=F, cursor=F, init_cursor=F, cur_slot=F, rng_kind=L.STREAM_PCG64 if kind is None else kind)
    st = L.CollectState(ep_t=F, obs_row=F, alive=F, obs=F, obs_next=F, obs_init=F, obs_bytes=16)
    out = L.CollectOut(row=F, flags=F)
    ppo = L.CollectPPOOut(value=F, logp=F, final_value=F)
    return t, ro, st, out, ppo


def _net(widths, bias=True, cls=None, form=0):
    from rl_offline_simulation_amd import _lib as L
    layers = (L.MLPLayer * (len(widths) - 1))()
    for l, (i, o) in enumerate(zip(widths[:-1], widths[1:])):
        layers[l].W, layers[l].b, layers[l].out = F, (F if bias else None), o
        setattr(layers[l], "in", i)
    c = (cls or L.CollectPolicy)(form=form, n_layers=len(layers), layers_host=ctypes.cast(layers, ctypes.POINTER(L.MLPLayer)), activation=L.ACT_TANH,
                                 x_dtype=L.F32, dO=widths[0], x_start=F, x_next=F, x_init=F)
    return c, layers


def _collect(t, ro, pol, st, out, T=4, cap=0, nA=None, action=F):
    from rl_offline_simulation_amd import _lib as L
    return L.load().offsim_queue_collect(ctypes.byref(t), ctypes.byref(ro), t.nA if nA is None else nA, None if pol is None else ctypes.byref(pol), T, cap,
                                         None if st is None else ctypes.byref(st), None if out is None else ctypes.byref(out), action, None)


def _ppo(t, ro, pol, val, st, out, ppo, T=4, pop=None):
    from rl_offline_simulation_amd import _lib as L
    lib, b = L.load(), ctypes.byref
    if pop is None:
        return lib.offsim_queue_collect_ppo(b(t), b(ro), t.nA, b(pol), None if val is None else b(val), T, 0, b(st), b(out), F, None if ppo is None else b(ppo),
                                            None)
    return lib.offsim_queue_collect_ppo_pop(b(t), b(ro), t.nA, b(pol), b(val), pop[0], pop[1], T, 0, b(st), b(out), F, b(ppo), None)


def test_symbols_and_header():
    from rl_offline_simulation_amd import _lib as L
    src = open(os.path.join(ROOT, "include", "offsim.h")).read()
    for name in ("offsim_queue_collect", "offsim_queue_collect_ppo", "offsim_queue_collect_ppo_pop"):
        assert name in L.SIGNATURES and f"int {name}(" in src
        assert getattr(L.load(), name) is not None


def test_refusals_before_any_hip_call():
    from rl_offline_simulation_amd import _lib as L
    lib = L.load()
    t, ro, st, out, ppo = _args()
    pol, _k1 = _net((4, 8, 2))
    assert _collect(t, ro, pol, st, out, T=0) == L.OK
    # NULLs
    assert lib.offsim_queue_collect(None, ctypes.byref(ro), 2, ctypes.byref(pol), 0, 0, ctypes.byref(st), ctypes.byref(out), F, None) == L.EINVAL
    assert lib.offsim_queue_collect(ctypes.byref(t), None, 2, ctypes.byref(pol), 0, 0, ctypes.byref(st), ctypes.byref(out), F, None) == L.EINVAL
    assert _collect(t, ro, None, st, out, T=0) == L.EINVAL and _collect(t, ro, pol, None, out, T=0) == L.EINVAL
    assert _collect(t, ro, pol, st, None, T=0) == L.EINVAL
    assert _collect(t, ro, pol, st, out, T=1, action=None) == L.EINVAL and b"out_action" in lib.offsim_last_error()
    assert _collect(t, ro, pol, st, out, T=0, action=None) == L.OK
    assert _collect(t, ro, pol, st, out, T=-1) == L.EINVAL and _collect(t, ro, pol, st, out, cap=-1, T=0) == L.EINVAL
    ro.rng = None
    assert _collect(t, ro, pol, st, out, T=0) == L.EINVAL
    ro.rng = F
    # the key: nA_actions is the table's, n_slots a multiple of it
    assert _collect(t, ro, pol, st, out, T=0, nA=3) == L.EINVAL
    t.n_slots = 7
    assert _collect(t, ro, pol, st, out, T=0) == L.EINVAL and b"multiple" in lib.offsim_last_error()
    t.n_slots = 6
    # a Philox row
    ro.rng_kind = L.STREAM_PHILOX
    assert _collect(t, ro, pol, st, out, T=0) == L.EUNSUPPORTED and b"PCG64" in lib.offsim_last_error()
    ro.rng_kind = 7
    assert _collect(t, ro, pol, st, out, T=0) == L.EINVAL
    ro.rng_kind = L.STREAM_PCG64
    # nA = 17, for every form
    t17, ro17, _, _, _ = _args(nA=17, n_slots=34)
    for p17 in (_net((4, 8, 17))[0], L.CollectPolicy(form=L.COLLECT_ROWS, p_next=F, p_init=F, x_dtype=L.F64),
                L.CollectPolicy(form=L.COLLECT_TABULAR, pi=F, x_dtype=L.F64)):
        assert _collect(t17, ro17, p17, st, out, T=0) == L.EUNSUPPORTED and b"16 actions" in lib.offsim_last_error()
    t16, ro16, _, _, _ = _args(nA=16, n_slots=32)
    assert _collect(t16, ro16, L.CollectPolicy(form=L.COLLECT_TABULAR, pi=F, x_dtype=L.F64), st, out, T=0) == L.OK
    # tables: their element type, their pointers
    assert _collect(t, ro, L.CollectPolicy(form=L.COLLECT_ROWS, p_next=F, p_init=F, x_dtype=L.F16), st, out, T=0) == L.EINVAL
    assert _collect(t, ro, L.CollectPolicy(form=L.COLLECT_ROWS, x_dtype=L.F32), st, out, T=0) == L.EINVAL
    assert _collect(t, ro, L.CollectPolicy(form=L.COLLECT_ROWS, p_next=F, p_init=F, x_dtype=L.F32), st, out, T=0) == L.OK
    assert _collect(t, ro, L.CollectPolicy(form=L.COLLECT_TABULAR, x_dtype=L.F64), st, out, T=0) == L.EINVAL
    assert _collect(t, ro, L.CollectPolicy(form=9), st, out, T=0) == L.EINVAL
    # the float cap: 126 -> 128 -> 2 without biases is exactly OFFSIM_COLLECT_MLP_MAX_FLOATS
    big, bl = _net((126, 128, 2), bias=False)
    assert 126 * 128 + 128 * 2 == L.COLLECT_MLP_MAX_FLOATS
    assert _collect(t, ro, big, st, out, T=0) == L.OK
    bl[1].b = F
    assert _collect(t, ro, big, st, out, T=0) == L.EUNSUPPORTED and b"MAX_FLOATS" in lib.offsim_last_error()
    # R = 0 launches nothing
    ro.R = 0
    assert _collect(t, ro, pol, st, out, T=3) == L.OK
    ro.R = 2


def test_ppo_refusals_before_any_hip_call():
    from rl_offline_simulation_amd import _lib as L
    lib = L.load()
    t, ro, st, out, ppo = _args(R=6)
    pol, _k1 = _net((4, 8, 2))
    val, _k2 = _net((4, 8, 1), cls=L.CollectValue, form=L.VALUE_MLP)
    assert _ppo(t, ro, pol, val, st, out, ppo, T=0) == L.OK
    assert _ppo(t, ro, pol, None, st, out, ppo, T=0) == L.EINVAL and _ppo(t, ro, pol, val, st, out, None, T=0) == L.EINVAL
    ppo.logp = None
    ro.R = 0
    assert _ppo(t, ro, pol, val, st, out, ppo, T=1) == L.EINVAL
    ppo.logp, ro.R = F, 6
    assert _ppo(t, ro, pol, L.CollectValue(form=L.VALUE_ROWS), st, out, ppo, T=0) == L.EINVAL
    assert _ppo(t, ro, pol, L.CollectValue(form=L.VALUE_ROWS, v_next=F, v_init=F), st, out, ppo, T=0) == L.OK
    # actor plus critic of one learner: exactly the cap, then one bias more
    a, al = _net((62, 128, 2), bias=False)           # 62 * 128 + 256 = 8192
    c, cl = _net((62, 128, 1), bias=False, cls=L.CollectValue, form=L.VALUE_MLP)   # 62 * 128 + 128 = 8064
    assert 62 * 128 + 256 + 62 * 128 + 128 == L.COLLECT_MLP_MAX_FLOATS - 128
    cl[0].b = F                                        # + 128: exactly the cap
    assert _ppo(t, ro, a, c, st, out, ppo, T=0) == L.OK
    cl[1].b = F                                        # one float more
    assert _ppo(t, ro, a, c, st, out, ppo, T=0) == L.EUNSUPPORTED and b"MAX_FLOATS" in lib.offsim_last_error()
    # the population: L * E = R, MLP actors with MLP critics
    assert _ppo(t, ro, pol, val, st, out, ppo, T=0, pop=(3, 2)) == L.OK
    assert _ppo(t, ro, pol, val, st, out, ppo, T=0, pop=(2, 2)) == L.EINVAL and b"L * E" in lib.offsim_last_error()
    assert _ppo(t, ro, pol, val, st, out, ppo, T=0, pop=(0, 6)) == L.EINVAL
    rows = L.CollectPolicy(form=L.COLLECT_ROWS, p_next=F, p_init=F, x_dtype=L.F32)
    assert _ppo(t, ro, rows, val, st, out, ppo, T=0, pop=(3, 2)) == L.EUNSUPPORTED
    assert _ppo(t, ro, pol, L.CollectValue(form=L.VALUE_ROWS, v_next=F, v_init=F), st, out, ppo, T=0, pop=(3, 2)) == L.EUNSUPPORTED
    ro.rng_kind = L.STREAM_PHILOX
    assert _ppo(t, ro, pol, val, st, out, ppo, T=0, pop=(3, 2)) == L.EUNSUPPORTED and _ppo(t, ro, pol, val, st, out, ppo, T=0) == L.EUNSUPPORTED
