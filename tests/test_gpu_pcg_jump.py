"""Where a chain of the sampler reset starts its draw stream (csrc/shuffle_wave.hpp, chain_start; the build-time jump tables of
csrc/pcg64_jump_tab.hpp), on the device:
  - offsim_pcg_jump_probe: the 64 lane states of both G wavefronts and the block jump, from the tables, against pcg_jump's squaring loop
    on the device and against numpy.random.PCG64.advance on the host, over composed counts (digit ends, skipped levels, 2^31 - 1,
    2^32 - 1) and over odd and even 32-bit draw counts;
  - the orders themselves: keyed resets of states of 2047 .. 65536 rows (every size class, every cut launch started from odd AND even
    draw counts -- asserted on NumPy's own stream) and of a table the chunked kernel takes, bit for bit np.random.default_rng(seed).shuffle."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pcg_jump_host as H  # noqa: E402

torch = pytest.importorskip("torch")

PROBE_SEEDS = [7, 2 ** 40 + 3]
# 32-bit draw counts as a cut launch finds them: odd and even, around the digit ends of count >> 1, and the counts the cut launches see
DRAW_COUNTS = [0, 1, 2, 3, 127, 128, 129, 8190, 8191, 65537, 131072, 2 ** 19 - 1, 2 ** 19, 2 ** 32 - 1]
SEEDS = [0, 7, 2 ** 40 + 3]
CUTS = (32768, 8192, 2048)  # SHUF_CUT_LIST of csrc/shuffle_wave.hpp: chains of more than 32768 rows run one launch per cut and one more
TABLES = [(2047, 2048, 2049), (8191, 8193, 32767), (32769, 40000, 65536)]
CHUNKED = (70001, 5000)  # a state beyond the LDS-resident classes: the chunked kernel (csrc/shuffle_chunk.hpp)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    from rl_offline_simulation_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def run_probe(counts, halve, gpu):
    from rl_offline_simulation_amd import _lib as L
    sd = torch.tensor(np.asarray(PROBE_SEEDS, dtype=np.uint64).view(np.int64), device=gpu)
    cn = torch.tensor(np.asarray(counts, dtype=np.uint32).view(np.int32), device=gpu)
    shape = (len(PROBE_SEEDS), len(counts), 2, 132)
    out_tab = torch.zeros(shape, dtype=torch.int64, device=gpu)
    out_ref = torch.zeros(shape, dtype=torch.int64, device=gpu)
    L.check(L.load().offsim_pcg_jump_probe(L.ptr(sd), len(PROBE_SEEDS), L.ptr(cn), len(counts), halve, L.ptr(out_tab), L.ptr(out_ref), L.stream_ptr()))
    torch.cuda.synchronize()
    return out_tab.cpu().numpy().view(np.uint64), out_ref.cpu().numpy().view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("halve", [0, 1])
def test_probe_equals_the_squaring_loop_and_numpy_advance(halve, gpu):
    counts = DRAW_COUNTS if halve else H.COUNTS
    tab, ref = run_probe(counts, halve, gpu)
    assert np.array_equal(tab, ref)  # the tables against pcg_jump on the device, every word
    for si, seed in enumerate(PROBE_SEEDS):
        st0, inc = H.pcg_state(seed)
        bg = np.random.PCG64(seed)
        base = bg.state
        for ci, cnt in enumerate(counts):
            q = cnt >> 1 if halve else cnt
            for g in (0, 1):
                w = tab[si, ci, g]
                bg.state = base
                bg.advance(q + 64 * g)
                for lane in range(64):
                    bg.advance(1)
                    assert (int(w[2 * lane]) << 64) | int(w[2 * lane + 1]) == int(bg.state["state"]["state"]), (seed, cnt, g, lane)
                mult, plus = (int(w[128]) << 64) | int(w[129]), (int(w[130]) << 64) | int(w[131])
                assert mult == pow(H.PCG_MULT, 128, 1 << 128)
                assert (mult * st0 + plus) & H.M128 == H.advanced(seed, 128)


def keyed_orders(lengths, gpu):
    """A table whose states have exactly these lengths, its keyed reset for SEEDS, and every chain's order as local rows."""
    from rl_offline_simulation_amd import synth, _lib
    from rl_offline_simulation_amd.table import TransitionTable
    from rl_offline_simulation_amd.evaluators import BatchedPSRS
    N, nS = sum(lengths), len(lengths)
    e = synth.synth_iid(N, nS, 2, seed=N + nS)
    e["z"] = np.random.default_rng(11).permutation(np.repeat(np.arange(nS), lengths)).astype(e["z"].dtype)
    table = TransitionTable(e["z"], e["actions"], e["rewards"], e["z_next"], e["terminals"], e["action_distributions"], e["steps"] == 0, device=gpu)
    pi = table.policy_slots(synth.dirichlet_policy(nS, 2))
    keyed = BatchedPSRS(table, len(SEEDS))
    keyed.reset_sampler(SEEDS, policy=pi)
    assert keyed._streams is not None
    so = table.seg_off.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    assert tuple(np.diff(so)) == tuple(lengths)
    kperm = (keyed.perm.to(torch.int64) & 0xFFFFFFFF).cpu().numpy()
    torch.cuda.synchronize()
    _lib.check_async_faults()
    return so, kperm


def check_orders(lengths, gpu):
    so, kperm = keyed_orders(lengths, gpu)
    for s, n in enumerate(lengths):
        for k, seed in enumerate(SEEDS):
            q = list(range(n))
            np.random.default_rng(seed=seed).shuffle(q)
            assert np.array_equal(kperm[k, so[s]:so[s + 1]], so[s] + np.asarray(q, dtype=np.int64)), (seed, n)


def test_cut_launches_start_from_odd_and_even_draw_counts():
    """The chains of TABLES that run cut launches (more than 32768 rows), on NumPy's own stream: the launch from every cut is started
    from an odd draw count (the buffered high half of a 64-bit output comes first) by at least one chain and from an even one by another."""
    parities = {c: set() for c in CUTS}
    for n in (n for t in TABLES for n in t if n > CUTS[0]):
        for seed in SEEDS:
            for cut, c in H.draws_at_cuts(seed, n, set(CUTS)).items():
                parities[cut].add(c & 1)
    assert all(parities[c] == {0, 1} for c in CUTS), parities


@pytest.mark.gpu
@pytest.mark.parametrize("lengths", TABLES, ids=lambda t: "-".join(map(str, t)))
def test_keyed_orders_equal_numpy_shuffle(lengths, gpu):
    check_orders(lengths, gpu)


@pytest.mark.gpu
def test_chunked_orders_equal_numpy_shuffle(gpu):
    check_orders(CHUNKED, gpu)
