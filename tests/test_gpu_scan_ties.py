"""Every form of the evalMC scan on BUILT tables (tests/tie_host.py): logs in which thousands of candidates meet their rejection draw
exactly at, one unit beside, and at every edge of the band around their compiled threshold -- where the scans' compressed compare
(top 21 / 16 / 14 bits, biased window entries, the exact 53-bit look) could be off by one without any statistical check noticing.
Against OraclePSRS, bit for bit: accepted rows and candidates per step where the form has a trace, and counts, every episode's return
and length and the in-order sum of returns everywhere.  tests/test_tie_tables_host.py holds the tables' census (which classes, how many
meetings, at which candidate positions) as a condition on the CPU.

Targeted meetings per table (all rollouts; R = 5 runs the first five seeds): a_every3 2000, a_all 5968, a_every3_philox 2000,
bc_70k 9523, c_131k 17555 -- each run through the forms below and decided as the oracle decides."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tie_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_TABLES = {}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch.device("cuda", 0)


def _built(name):
    return {"a_every3": lambda: H.table_a(3), "a_all": lambda: H.table_a(1), "a_every3_philox": lambda: H.table_a(3, "philox"),
            "bc_70k": lambda: H.table_bc(), "c_131k": lambda: H.table_bc(131072)}[name]()


def _table(name, gpu):
    from rl_offline_simulation_amd.table import TransitionTable
    if name not in _TABLES:
        e = _built(name)["log"]
        _TABLES[name] = TransitionTable(e["z"], e["actions"], e["rewards"], e["z_next"], e["terminals"], e["action_distributions"], e["steps"] == 0, device=gpu)
    return _TABLES[name]


def _oracle_runs(name, seeds, cuts):
    """ref[seed] = the oracle's evalMC results of the consecutive calls (n_episodes = each of `cuts`, None = to the end)."""
    from oracle import oracle as O
    b = _built(name)
    e, N = b["log"], len(b["log"]["z"])
    ora = O.OraclePSRS(e["z"], e["actions"], e["rewards"], e["z_next"], e["terminals"], e["action_distributions"], e["steps"] == 0)
    ref = {}
    for s in seeds:
        ora.reset_sampler(s)
        if name.endswith("philox"):
            ora.set_rejection_philox(s)
        ref[s] = [ora.evalmc(10 ** 9 if c is None else c, b["pi"], b["gamma"], trace_cap=N + 1) for c in cuts]
    return ref


def _run(name, gpu, R, traced, fast=None, keyed=False, cuts=(None,), kernel="k_eval_mc_rows", fmt=None):
    """eval_mc on the built table `name` for its first R seeds, call after call, each compared with the oracle's (the comparisons of
    test_gpu_edges._compare and _compare_untraced); returns the number of targeted meetings those rollouts ran through."""
    from rl_offline_simulation_amd import _lib as L
    from rl_offline_simulation_amd.evaluators import BatchedPSRS
    b = _built(name)
    table, seeds, N = _table(name, gpu), b["seeds"][:R], len(b["log"]["z"])
    pi = table.policy_slots(b["pi"])
    env = BatchedPSRS(table, R)
    env.reset_sampler(seeds, policy=pi if keyed else None, rejection="philox" if name.endswith("philox") else "pcg64")
    ref = _oracle_runs(name, seeds, cuts)
    for ci, cut in enumerate(cuts):
        o = env.eval_mc(pi, b["gamma"], n_episodes=cut, ep_cap=table.N0 + 1, trace_cap=N + 1 if traced else 0, fast=fast)
        torch.cuda.synchronize()
        L.check_async_faults()
        if fast is False:
            assert o["_kernel"] == "k_eval_mc" == kernel
        else:
            assert env.scan_variant() == kernel
        if fmt is not None:
            assert env._stream_format() == fmt
        for i, s in enumerate(seeds):
            r = ref[s][ci]
            assert int(o["status"][i]) != L.ST_PROTOCOL
            assert int(o["steps"][i]) == r["steps"] and int(o["cand"][i]) == r["candidates"], (s, ci)
            ne = int(o["n_ep"][i])
            assert ne == len(r["Gs"])
            assert np.array_equal(o["ep_g"][i, :ne].cpu().numpy(), r["Gs"]), (s, ci)
            assert np.array_equal(o["ep_len"][i, : int(o["n_len"][i])].cpu().numpy(), r["lengths"]), (s, ci)
            acc = 0.0
            for g in r["Gs"]:
                acc += float(g)
            assert float(o["sum_g"][i]) == acc, (s, ci)
            if traced:
                n = r["steps"]
                assert np.array_equal(o["trace_row"][i, :n].cpu().numpy(), r["trace_rows"]), (s, ci)
                assert np.array_equal(o["trace_pop"][i, :n].cpu().numpy(), r["trace_popped"]), (s, ci)
    if cuts[-1] is None and len(cuts) == 1:  # the oracle's whole run is the builder's own simulation: every recorded meeting was run
        for s in seeds:
            assert ref[s][0]["steps"] == b["trace"][s]["steps"] and ref[s][0]["candidates"] == b["trace"][s]["candidates"]
    return sum(r.seed in seeds for r in b["records"])


A_CASES = [("a_every3", 8), ("a_all", 8), ("a_every3", 5), ("a_all", 5)]


@pytest.mark.parametrize("name,R", A_CASES)
def test_format_a_rows_with_helpers(name, R, gpu):
    """The headline form: keyed sampler reset (candidate streams written by the reset) + the row-packed scan with helper wavefronts."""
    assert _run(name, gpu, R, traced=False, keyed=True, fmt=0) > 1000


@pytest.mark.parametrize("name,R", A_CASES)
def test_format_a_rows_traced(name, R, gpu):
    """The traced build of the row-packed scan (single wavefront), streams derived from permutations."""
    assert _run(name, gpu, R, traced=True, fmt=0) > 1000


@pytest.mark.parametrize("traced", [True, False])
@pytest.mark.parametrize("name", ["a_every3", "a_all"])
def test_format_a_window_kernel(name, traced, gpu, monkeypatch):
    monkeypatch.setenv("OFFSIM_SCAN_ROWS", "0")
    assert _run(name, gpu, 8, traced=traced, kernel="k_eval_mc_win") > 1000


@pytest.mark.parametrize("name", ["a_every3", "a_all"])
def test_format_a_generic_kernel(name, gpu):
    """k_eval_mc evaluates the f64 expression itself per candidate: the same decisions without any compiled threshold."""
    assert _run(name, gpu, 8, traced=True, fast=False, kernel="k_eval_mc") > 1000


@pytest.mark.parametrize("form", ["helpers", "traced", "win", "generic"])
def test_format_a_philox(form, gpu, monkeypatch):
    """The table built from oracle.philox_doubles, the rejection stream rocRAND's Philox4x32-10 in every kernel."""
    if form == "win":
        monkeypatch.setenv("OFFSIM_SCAN_ROWS", "0")
    kw = dict(helpers=dict(traced=False, keyed=True), traced=dict(traced=True), win=dict(traced=True, kernel="k_eval_mc_win"),
              generic=dict(traced=True, fast=False, kernel="k_eval_mc"))[form]
    assert _run("a_every3_philox", gpu, 8, **kw) > 1000


@pytest.mark.parametrize("form", ["helpers", "traced", "win"])
def test_format_a_calls_that_continue(form, gpu, monkeypatch):
    """40 episodes, then the rest in a second call: the exact look recomputes its draw from the stream position a call starts with, and
    most targeted meetings of the table come after the cut."""
    if form == "win":
        monkeypatch.setenv("OFFSIM_SCAN_ROWS", "0")
    b = H.table_a(1)
    first = _oracle_runs("a_all", [0, 4], (40,))
    for s in (0, 4):
        assert sum(r.seed == s and r.step >= first[s][0]["steps"] for r in b["records"]) > 500
    _run("a_all", gpu, 8, traced=form != "helpers", keyed=form == "helpers", cuts=(40, None), kernel="k_eval_mc_win" if form == "win" else "k_eval_mc_rows")


@pytest.mark.parametrize("variant", ["OFFSIM_ROWS_HELPER=0", "OFFSIM_ROWS_WAVES=1", "OFFSIM_ROWS_PER_WAVE=1"])
def test_format_a_in_a_child_process_per_launch_shape(variant, gpu):
    """These switches are read once per process: the format-A cases of this file run again in a fresh child for each."""
    k, v = variant.split("=")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k", "format_a and not child_process"],
                       env=dict(os.environ, **{k: v}), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("form", ["helpers", "traced", "continued"])
@pytest.mark.parametrize("fmt", ["C", "B"])
def test_formats_c_and_b(fmt, form, gpu, monkeypatch):
    """One state of 70000 rows and 254 small ones: format C by default, B on request; ties on 14 and on 16 bits, each with a plain
    payload and with done = 1, z_next = 254."""
    from rl_offline_simulation_amd import _lib as L
    if fmt == "B":
        monkeypatch.setenv("OFFSIM_STREAMS_FORMAT", "B")
    kw = dict(helpers=dict(traced=False, keyed=True), traced=dict(traced=True), continued=dict(traced=False, keyed=True, cuts=(300, None)))[form]
    assert _run("bc_70k", gpu, 4, fmt=L.STREAMS_C if fmt == "C" else L.STREAMS_B, **kw) > 9000


@pytest.mark.parametrize("traced", [False, True])
def test_format_c_high_local_rows(traced, gpu):
    """A state of 131072 rows: the 256 rows whose local row is >= 0x1ff00 set every local-row bit of a format-C digest; with done = 1 and
    z_next = 254 the payload is one short of the all-ones mask a draw is laid down with."""
    from rl_offline_simulation_amd import _lib as L
    assert _run("c_131k", gpu, 4, traced=traced, keyed=not traced, fmt=L.STREAMS_C) > 17000
