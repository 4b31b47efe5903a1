"""Round-6 GPU tests: the rocRAND provider of the rejection stream (OFFSIM_STREAM_PHILOX) in the ROW-PACKED scan (csrc/scan_rows.hpp:
the helper wavefront fills the draw ring from philox4x32_10_engine::ten_rounds) -- against the reference's own PSRS with a replayed
Philox stream (tests/golden/philox_*.npz), against the oracle fed the same stream, and against the generic kernel (the literal
rocrand_init / rocrand device API) at stream positions of either parity."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from common import load

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu():
    from rl_offline_simulation_amd import _lib
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    _lib.load()
    return torch.device("cuda", 0)


def _table(d, gpu):
    from rl_offline_simulation_amd.table import TransitionTable
    src = load(str(d["inputs_of"])) if "inputs_of" in d.files else d
    return TransitionTable(src["in_z"], src["in_a"], src["in_r"], src["in_z_next"], src["in_done"], src["in_p_log"], src["in_t0"], device=gpu)


@pytest.mark.parametrize("name", ["philox_iid_2k", "philox_iid_50k"])
def test_philox_in_the_row_packed_scan_against_the_reference_with_a_replayed_stream(name, gpu):
    """reset_sampler(policy=pi, rejection="philox") writes the candidate streams and hands the rollouts rocRAND's stream; eval_mc then
    runs k_eval_mc_rows<.., OFFSIM_STREAM_PHILOX>.  Traced launch (single wavefront): accepted rows and candidates popped per step, every
    episode's return (bit-exact f64) and length as the reference served them under the replayed stream.  Untraced launch (helper
    wavefronts: the product's form): the same counts and the in-order sum of returns."""
    from rl_offline_simulation_amd.evaluators import BatchedPSRS
    d = load(name)
    table = _table(d, gpu)
    seeds = [int(s) for s in d["seeds"]]
    pi = table.policy_slots(d["pi"])
    env = BatchedPSRS(table, len(seeds))
    for traced in (True, False):
        env.reset_sampler(seeds, policy=pi, rejection="philox")
        assert env.scan_variant() == "k_eval_mc_rows"
        o = env.eval_mc(pi, float(d["gamma"]), ep_cap=table.N0 + 1, trace_cap=(table.N + 1) if traced else 0)
        torch.cuda.synchronize()
        assert "_kernel" not in o  # (not the generic kernel)
        for i, s in enumerate(seeds):
            rows, pops = d[f"s{s}_mc_rows"], d[f"s{s}_mc_popped"]
            n = int(o["steps"][i])
            assert n == len(rows) and int(o["cand"][i]) == int(pops.sum()), (s, traced)
            if traced:
                assert np.array_equal(o["trace_row"][i, :n].cpu().numpy(), rows)
                assert np.array_equal(o["trace_pop"][i, :n].cpu().numpy(), pops[:n])
            ne, nl = int(o["n_ep"][i]), int(o["n_len"][i])
            assert np.array_equal(o["ep_g"][i, :ne].cpu().numpy(), d[f"s{s}_mc_Gs"])
            assert np.array_equal(o["ep_len"][i, :nl].cpu().numpy(), d[f"s{s}_mc_lengths"])
            acc = 0.0
            for g in d[f"s{s}_mc_Gs"]:
                acc += float(g)
            assert float(o["sum_g"][i]) == acc
            # the stream state written back: (seed, draws consumed so far, 0, 0)
            assert [int(x) for x in env.state.rng[i].cpu().numpy().view(np.uint64)] == [s, int(pops.sum()), 0, 0]


@pytest.mark.parametrize("name", ["philox_iid_2k", "philox_iid_50k"])
def test_philox_in_the_window_kernel_against_the_reference_with_a_replayed_stream(name, gpu, monkeypatch):
    """The same fixtures through csrc/scan_win.hpp on permutations (OFFSIM_SCAN_ROWS=0: the scan a table with a hot state gets), whose
    ring is filled from the same engine: k_eval_mc_win<.., OFFSIM_STREAM_PHILOX>, traced and untraced."""
    from rl_offline_simulation_amd.evaluators import BatchedPSRS
    monkeypatch.setenv("OFFSIM_SCAN_ROWS", "0")
    d = load(name)
    table = _table(d, gpu)
    seeds = [int(s) for s in d["seeds"]]
    pi = table.policy_slots(d["pi"])
    env = BatchedPSRS(table, len(seeds))
    for traced in (True, False):
        env.reset_sampler(seeds, policy=pi, rejection="philox")
        assert env._streams is None and env.scan_variant().startswith("k_eval_mc_win")
        o = env.eval_mc(pi, float(d["gamma"]), ep_cap=table.N0 + 1, trace_cap=(table.N + 1) if traced else 0)
        torch.cuda.synchronize()
        assert "_kernel" not in o
        for i, s in enumerate(seeds):
            rows, pops = d[f"s{s}_mc_rows"], d[f"s{s}_mc_popped"]
            n = int(o["steps"][i])
            assert n == len(rows) and int(o["cand"][i]) == int(pops.sum()), (s, traced)
            if traced:
                assert np.array_equal(o["trace_row"][i, :n].cpu().numpy(), rows)
                assert np.array_equal(o["trace_pop"][i, :n].cpu().numpy(), pops[:n])
            ne, nl = int(o["n_ep"][i]), int(o["n_len"][i])
            assert np.array_equal(o["ep_g"][i, :ne].cpu().numpy(), d[f"s{s}_mc_Gs"])
            assert np.array_equal(o["ep_len"][i, :nl].cpu().numpy(), d[f"s{s}_mc_lengths"])
            assert [int(x) for x in env.state.rng[i].cpu().numpy().view(np.uint64)] == [s, int(pops.sum()), 0, 0]


def test_philox_window_kernel_equals_the_generic_kernel_from_either_parity(gpu, monkeypatch):
    """k_eval_mc_win under Philox against k_eval_mc (the literal rocrand_init / rocrand API) on a 100 k-row table with a hot state, the
    rollouts entering the scan at stream positions of either parity."""
    monkeypatch.setenv("OFFSIM_SCAN_ROWS", "0")
    a = _philox_rows_vs_generic(gpu, 100000, 40, 3, 32, 3, seed=9, kernel="win")
    assert a["steps"].min() > 100


def _philox_rows_vs_generic(gpu, N, nS, nA, R, pre_steps, seed, want_format=None, kernel="rows"):
    from rl_offline_simulation_amd import synth
    from rl_offline_simulation_amd.table import TransitionTable
    from rl_offline_simulation_amd.evaluators import BatchedPSRS
    e = synth.synth_iid(N, nS, nA, seed=seed)
    table = TransitionTable(e["z"], e["actions"], e["rewards"], e["z_next"], e["terminals"], e["action_distributions"], e["steps"] == 0, device=gpu)
    pi_np = synth.dirichlet_policy(nS, nA)
    pi = table.policy_slots(pi_np)
    seeds = [1000 + 3 * i for i in range(R)]
    outs = []
    for rows in (True, False):
        env = BatchedPSRS(table, R)
        env.reset_sampler(seeds, policy=pi if rows else None, rejection="philox")
        if pre_steps:  # a few steps through the generic kernel first: the rollouts enter the scan at stream positions of either parity
            env.reset()
            p = np.tile(np.full(nA, 1.0 / nA), (R, 1))
            for _ in range(pre_steps):
                env.step(p)
            assert len(set((env.state.rng[:, 1].cpu().numpy() & 1).tolist())) == 2
        o = env.eval_mc(pi, 0.97, ep_cap=64, fast=None if rows else False)
        torch.cuda.synchronize()
        assert ("_kernel" not in o and env.scan_variant() == ("k_eval_mc_rows" if kernel == "rows" else "k_eval_mc_win")) if rows else True
        if rows and want_format is not None:
            assert env._streams["format"] == want_format
        outs.append({k: o[k].cpu().numpy() for k in ("steps", "cand", "n_ep", "n_len", "sum_g", "status", "ep_g", "ep_len")} |
                    {"rng": env.state.rng.cpu().numpy()})
    a, b = outs
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["steps"].min() > 100
    return a


def test_philox_rows_kernel_equals_the_generic_kernel(gpu):
    """block(seed, m) of csrc/scan_rows.hpp (the engine's ten_rounds through a derived class) against philox_k53 (rocrand_init /
    rocrand, the literal device API, in k_eval_mc): 64 rollouts on a 200 k-row table, every count, episode and sum equal, and the
    stream positions written back."""
    _philox_rows_vs_generic(gpu, 200000, 162, 2, 64, 0, seed=5)


def test_philox_rows_kernel_from_odd_and_even_stream_positions(gpu):
    """A rollout that was stepped before enters the scan at any stream position: an odd one pairs the draws across Philox blocks."""
    _philox_rows_vs_generic(gpu, 60000, 30, 3, 32, 3, seed=6)


@pytest.mark.parametrize("N,pre", [(200000, 0), (300000, 2)])
def test_philox_rows_kernel_in_stream_formats_c_and_b(N, pre, gpu):
    """Two states of 100 k rows (stream format C: 14-bit thresholds, written by the chunked shuffle) and of 150 k rows (format B: 16-bit
    thresholds): the draw's top bits are laid down in the ring at the format's resolution whatever the provider; every count, episode
    and sum as the generic kernel's (windows run dry all the time on such a table: the exact path and the dry-row handler do the work)."""
    from rl_offline_simulation_amd import _lib as L
    a = _philox_rows_vs_generic(gpu, N, 2, 3, 8, pre, seed=7 + pre, want_format=L.STREAMS_C if N == 200000 else L.STREAMS_B)
    assert a["cand"].min() > 1000


def test_philox_against_the_oracle_with_the_same_stream_at_a_million_rows(gpu):
    """What bench.py --rng philox checks on four seeds, at a size the oracle finishes in seconds: 1 M rows, 162 states, 2 actions."""
    from oracle import oracle as O
    from rl_offline_simulation_amd import synth
    from rl_offline_simulation_amd.table import TransitionTable
    from rl_offline_simulation_amd.evaluators import BatchedPSRS
    e = synth.synth_iid(1000000, 162, 2, seed=20221107)
    t0 = e["steps"] == 0
    table = TransitionTable(e["z"], e["actions"], e["rewards"], e["z_next"], e["terminals"], e["action_distributions"], t0, device=gpu)
    pi_np = synth.dirichlet_policy(162, 2)
    pi = table.policy_slots(pi_np)
    seeds = list(range(16))
    env = BatchedPSRS(table, len(seeds))
    env.reset_sampler(seeds, policy=pi, rejection="philox")
    o = env.eval_mc(pi, 0.99)
    torch.cuda.synchronize()
    assert env.scan_variant() == "k_eval_mc_rows" and "_kernel" not in o
    ora = O.OraclePSRS(e["z"], e["actions"], e["rewards"], e["z_next"], e["terminals"], e["action_distributions"], t0)
    for i in (0, 5, 15):
        ora.reset_sampler(seeds[i])
        ora.set_rejection_philox(seeds[i])
        ref = ora.evalmc(10 ** 9, pi_np, 0.99)
        assert int(o["steps"][i]) == ref["steps"] and int(o["cand"][i]) == ref["candidates"] and int(o["n_ep"][i]) == len(ref["Gs"])
        acc = 0.0
        for g in ref["Gs"]:
            acc += float(g)
        assert float(o["sum_g"][i]) == acc


@pytest.mark.parametrize("variant", ["rows_single", "waves1", "rpw2", "auto"])
def test_philox_tests_under_the_other_launch_shapes(variant):
    """The Philox tests of this file again with the single-wavefront form of the kernel, one chain wavefront per workgroup, two
    rollouts per chain wavefront, and the launcher's own choice (switches read once per process: child processes)."""
    env = dict(os.environ)
    if variant == "rows_single":
        env["OFFSIM_ROWS_HELPER"] = "0"
    elif variant == "waves1":
        env["OFFSIM_ROWS_WAVES"] = "1"
    elif variant == "rpw2":
        env["OFFSIM_ROWS_PER_WAVE"] = "2"
    else:
        env.pop("OFFSIM_ROWS_WAVES", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k", "philox and not other_launch_shapes and not bench"],
                       env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def _bench(args, env_extra=None, timeout=900):
    import json
    env = dict(os.environ, **(env_extra or {}))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), r.stderr


@pytest.mark.timeout(900)
def test_bench_philox_runs_the_row_packed_scan_with_its_own_parity_check(gpu):
    """`bench.py --rng philox`: rocRAND's stream in k_eval_mc_rows (not the generic kernel), checked on four seeds against the oracle fed
    the replayed stream."""
    out, _ = _bench(["--rng", "philox", "--transitions", "400000", "--rollouts", "256", "--steps", "1", "--warmup", "1", "--no-cpu-baseline", "--full"])
    assert out["config"]["rng"] == "philox" and out["roofline"]["kernel"] == "k_eval_mc_rows"
    assert out["parity_check"]["ok"] and out["parity_check"]["seeds"] == [0, 1]
    pcg, _ = _bench(["--transitions", "400000", "--rollouts", "256", "--steps", "1", "--warmup", "1", "--no-cpu-baseline", "--no-configs", "--full"])
    assert pcg["parity_check"]["ok"] and pcg["value_estimate_mean"] != out["value_estimate_mean"]  # another sample path


@pytest.mark.timeout(900)
def test_bench_c4_shard_as_two_episode_disjoint_parts_and_the_phase_trace(gpu):
    """The default line's C4 shard is evaluated as two episode-disjoint halves (each with its own oracle check, run on host threads beside
    the timed passes); OFFSIM_BENCH_TRACE stamps the command's phases on stderr."""
    out, err = _bench(["--steps", "1", "--warmup", "0", "--cpu-sample-seconds", "1", "--full"], env_extra={"OFFSIM_BENCH_TEST_SCALE": "50", "OFFSIM_BENCH_TRACE": "1"})
    c4 = out["configs"]["C4_shard"]
    assert c4["parity_ok"] is True and "2 episode-disjoint parts" in c4["sharding"] and c4["kernel"] == "k_eval_mc_rows"
    assert c4["segment_rows_min_max"][1] <= 65536 and c4["reset_s"] > 0 and c4["scan_s"] > 0
    assert "estimator" not in out and out["cpu_baseline"]["value"] > 0 and "the timed passes" in out["parity_check"]["checked"]
    assert "configuration C4_shard: parity checked" in err and "CPU baseline done" in err


@pytest.mark.timeout(900)
def test_plain_bench_line_is_the_headline_alone_and_dumps_what_the_full_run_checks(gpu, tmp_path):
    """A plain `bench.py` run reports the headline and what its timed passes measured, nothing of what --full adds; --dump-outputs
    writes the last timed pass's per-seed results as float64, the same in a plain and a --full run of the same arguments, and equal
    to the oracle on the seeds the --full run's parity check replays."""
    args = ["--transitions", "400000", "--rollouts", "256", "--steps", "2", "--warmup", "1"]
    plain, _ = _bench(args + ["--dump-outputs", str(tmp_path / "plain")])
    assert plain["steps"] == 2 and plain["warmup"] == 1 and plain["ms_per_step"] > 0 and plain["value"] > 0
    assert plain["unit"] == "simulated steps/s" and plain["higher_is_better"] is True and plain["dtype"] == "f64"
    assert not {"parity_check", "cpu_baseline", "configs", "collective", "rollout_sharded"} & set(plain) and "chain" not in plain["roofline"]
    full, _ = _bench(args + ["--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full")])
    assert full["parity_check"]["ok"]
    names = ("sum_g", "n_ep", "steps", "cand", "value_estimate")
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(k + ".npy" for k in names)
    got = {}
    for k in names:
        got[k] = np.load(tmp_path / "plain" / f"{k}.npy")
        assert got[k].dtype == np.float64 and got[k].shape == (256,), k
        assert np.array_equal(got[k], np.load(tmp_path / "full" / f"{k}.npy"), equal_nan=True), k
    for row in full["parity_check"]["oracle"]:
        s = row["seed"]
        assert (got["steps"][s], got["cand"][s], got["n_ep"][s]) == (row["steps"], row["candidates"], row["episodes"]), s
        assert abs(got["value_estimate"][s] - row["value"]) <= 1e-5, s
