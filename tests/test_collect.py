"""CPU side of VectorPSRS.collect: the C ABI (offsim_vector_collect and its structs) and the NumPy restatement (tests/collect_host.py) pinned
on the reference's fixtures (tests/golden/collect/*.npz, made by tests/golden/make_golden_collect.py)."""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import collect_host as H  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "collect", "*.npz")))


def test_fixtures_present():
    names = {os.path.basename(p)[:-4] for p in FIXTURES}
    assert {"collect_cartpole_f32_cap500", "collect_cartpole_f32_cap8", "collect_grid_f64", "collect_grid_exhaust", "collect_grid_no_init",
            "collect_grid_keyerror"} <= names


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_host_restatement_matches_reference(path):
    d = np.load(path)
    for s in d["seeds"]:
        o = H.collect_rows(d["z"], d["a"], d["z_next"], d["done"], d["p_log"], d["t0"], d["P_next"], d["P_init"], int(s), int(d["T"]),
                           int(d["cap"]))
        assert np.array_equal(o["rows"], d[f"rows_{s}"]), s
        assert np.array_equal(o["obs_row"], d[f"obs_row_{s}"]), s
        assert np.array_equal(o["terminated"], d[f"terminated_{s}"]) and np.array_equal(o["truncated"], d[f"truncated_{s}"]), s
        assert o["status"] == str(d[f"status_{s}"]), s


def test_collect_struct_layout(tmp_path):
    """sizeof / offsetof of the new structs of include/offsim.h as gcc lays them out, against the ctypes mirrors in _lib.py."""
    from rl_offline_simulation_amd import _lib
    pairs = {"offsim_collect_policy": _lib.CollectPolicy, "offsim_collect_state": _lib.CollectState, "offsim_collect_out": _lib.CollectOut,
             "offsim_mlp_layer": _lib.MLPLayer}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "offsim.h"', "int main(void) {"]
    for c_name, cls in pairs.items():
        lines.append(f'  printf("{c_name} %zu\\n", sizeof({c_name}));')
        for f, _ in cls._fields_:
            lines.append(f'  printf("{c_name}.{f} %zu\\n", offsetof({c_name}, {f}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for c_name, cls in pairs.items():
        assert int(got[c_name]) == ctypes.sizeof(cls), c_name
        for f, _ in cls._fields_:
            assert int(got[f"{c_name}.{f}"]) == getattr(cls, f).offset, (c_name, f)


def test_collect_constants_match_header():
    from rl_offline_simulation_amd import _lib
    src = open(os.path.join(ROOT, "include", "offsim.h")).read()
    for name, v in (("OFFSIM_COLLECT_MLP", _lib.COLLECT_MLP), ("OFFSIM_COLLECT_ROWS", _lib.COLLECT_ROWS), ("OFFSIM_COLLECT_TABULAR", _lib.COLLECT_TABULAR),
                    ("OFFSIM_COLLECT_MLP_MAX_FLOATS", _lib.COLLECT_MLP_MAX_FLOATS), ("OFFSIM_COLLECT_SERVED", _lib.COLLECT_SERVED),
                    ("OFFSIM_COLLECT_TERMINATED", _lib.COLLECT_TERMINATED), ("OFFSIM_COLLECT_TRUNCATED", _lib.COLLECT_TRUNCATED),
                    ("OFFSIM_COLLECT_RESET", _lib.COLLECT_RESET), ("OFFSIM_COLLECT_ALIVE", _lib.COLLECT_ALIVE)):
        assert f"#define {name} {v}" in src, name
    assert "offsim_vector_collect" in _lib.SIGNATURES


def _args(T=4, R=2):
    """A table / rollouts / policy / state / out set whose pointers are never dereferenced (validation fails first)."""
    from rl_offline_simulation_amd import _lib as L
    fake = 0x1000
    t = L.Table(N=10, n_slots=3, nA=2, plog_dtype=L.F32, r_dtype=L.F32, seg_off=fake, p_log=fake, a=fake, r=fake, z_next=fake, done=fake,
                orig_idx=fake, N0=2, init_slot=fake, init_orig=fake)
    ro = L.Rollouts(R=R, rng=fake, cursor=fake, init_cursor=fake, cur_slot=fake)
    layers = (L.MLPLayer * 2)()
    layers[0].W, layers[0].b, layers[0].out = fake, fake, 8
    setattr(layers[0], "in", 4)
    layers[1].W, layers[1].b, layers[1].out = fake, fake, 2
    setattr(layers[1], "in", 8)
    pol = L.CollectPolicy(form=L.COLLECT_MLP, n_layers=2, layers_host=ctypes.cast(layers, ctypes.POINTER(L.MLPLayer)), activation=L.ACT_TANH,
                          x_dtype=L.F32, dO=4, x_start=fake, x_next=fake, x_init=fake)
    st = L.CollectState(ep_t=fake, obs_row=fake, alive=fake, obs=fake, obs_next=fake, obs_init=fake, obs_bytes=16)
    out = L.CollectOut(row=fake, flags=fake)
    return t, ro, pol, st, out, layers


def _call(t, ro, pol, st, out, T=4, prob_mode=0, cap=0):
    from rl_offline_simulation_amd import _lib as L
    lib = L.load()
    return lib.offsim_vector_collect(ctypes.byref(t), ctypes.byref(ro), ctypes.byref(pol), prob_mode, L.REJECT_DEFAULT, T, cap,
                                     ctypes.byref(st), ctypes.byref(out), None)


def test_collect_argument_validation_before_any_hip_call():
    """Every refusal below happens before a HIP call (the arguments are fake pointers; no device is needed).  T = 0 validates and launches
    nothing."""
    from rl_offline_simulation_amd import _lib as L
    lib = L.load()
    t, ro, pol, st, out, layers = _args()
    assert _call(t, ro, pol, st, out, T=0) == L.OK
    assert _call(t, ro, pol, st, out, T=-1) == L.EINVAL
    assert _call(t, ro, pol, st, out, cap=-1) == L.EINVAL
    assert _call(t, ro, pol, st, out, T=0, prob_mode=L.PROB_F32) == L.OK  # f32 p_log
    t.plog_dtype = L.F64
    assert _call(t, ro, pol, st, out, T=0, prob_mode=L.PROB_F32) == L.EINVAL
    assert b"PROB_F32" in lib.offsim_last_error()
    t.plog_dtype = L.F32
    for field, bad in (("form", 7), ("x_dtype", L.F64), ("activation", 9), ("dO", 129), ("n_layers", 5)):
        old = getattr(pol, field)
        setattr(pol, field, bad)
        assert _call(t, ro, pol, st, out, T=0) == L.EINVAL, field
        setattr(pol, field, old)
    layers[1].out = 3  # the network's outputs differ from nA
    assert _call(t, ro, pol, st, out, T=0) == L.EINVAL and b"nA" in lib.offsim_last_error()
    layers[1].out = 2
    layers[0].out = 300  # hidden width above 256
    assert _call(t, ro, pol, st, out, T=0) == L.EINVAL
    layers[0].out = 8
    big = (L.MLPLayer * 2)()  # 126 -> 128 -> 2 without biases: exactly OFFSIM_COLLECT_MLP_MAX_FLOATS floats
    big[0].W, big[0].out = 0x1000, 128
    setattr(big[0], "in", 126)
    big[1].W, big[1].out = 0x1000, 2
    setattr(big[1], "in", 128)
    pol2 = L.CollectPolicy(form=L.COLLECT_MLP, n_layers=2, layers_host=ctypes.cast(big, ctypes.POINTER(L.MLPLayer)), activation=L.ACT_TANH,
                           x_dtype=L.F32, dO=126, x_start=0x1000, x_next=0x1000, x_init=0x1000)
    assert _call(t, ro, pol2, st, out, T=0) == L.OK
    big[1].b = 0x1000  # two floats more
    assert _call(t, ro, pol2, st, out, T=0) == L.EUNSUPPORTED and b"MAX_FLOATS" in lib.offsim_last_error()
    st.obs_bytes = 0
    assert _call(t, ro, pol, st, out, T=0) == L.EINVAL
    st.obs_bytes = 16
    out.flags = None  # records are needed when T > 0 (R = 0 here: nothing would launch even past the check)
    ro.R = 0
    assert _call(t, ro, pol, st, out, T=1) == L.EINVAL and b"flags" in lib.offsim_last_error()
    assert _call(t, ro, pol, st, out, T=0) == L.OK
    ro.R = 2
    out.flags = 0x1000
    rows = L.CollectPolicy(form=L.COLLECT_ROWS)
    assert _call(t, ro, rows, st, out, T=0) == L.EINVAL  # p_next / p_init NULL
    tab = L.CollectPolicy(form=L.COLLECT_TABULAR, pi=0x1000)
    assert _call(t, ro, tab, st, out, T=0) == L.OK
    t.n_slots = 20000  # pi [n_slots, nA] f64 beyond the LDS budget
    assert _call(t, ro, tab, st, out, T=0) == L.EUNSUPPORTED
