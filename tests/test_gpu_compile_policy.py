"""offsim_compile_policy and offsim_compile_digests, called through the C ABI, bit for bit against the documented arithmetic restated in
tests/tie_host.py (threshold / key / digest): every p_log type, one to sixteen actions, zeros, NaN, thr == 1, subnormal thr, an all-ones
low word, row counts around the 256-thread block, empty segments in front of, between and behind the used ones, the 10-bit next-state
field at its limit, the refusals -- and nothing written outside the output buffers."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tie_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PAD, SENT = 64, 0x5A5A5A5A5A5A5A5A
ALL_ONES_T = (0x12345 << 32) | 0xFFFFFFFF


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    return torch.device("cuda", 0)


def _case(N, nA, dt, states, n_slots, seed, zn_max=None):
    """Rows over `states` (the other slots stay empty); pi [n_slots, nA].  states[0] is the all-ones state, states[-1] the subnormal one."""
    g = np.random.default_rng(seed)
    z = np.asarray(states)[g.integers(0, len(states), N)]
    zn = g.integers(0, n_slots, N)
    zn[-1] = n_slots - 1 if zn_max is None else zn_max
    p = g.dirichlet(np.ones(nA), N)
    p[g.random((N, nA)) < 0.08] = 0.0                       # zeros in p_log: infinite ratios, 0 / 0 where pi is zero too
    pi = g.dirichlet(np.ones(nA), n_slots)
    pi[g.random((n_slots, nA)) < 0.15] = 0.0                # zeros in pi
    ratio = np.divide(pi[z], p, out=np.full((N, nA), -1.0), where=p > 0)
    a = np.where(g.random(N) < 0.3, ratio.argmax(axis=1), g.integers(0, nA, N))   # thr == 1 exactly: the arg-max action
    if nA >= 2:
        pi[states[0]] = 0.0
        pi[states[0], 0], pi[states[0], 1] = ALL_ONES_T / 2.0 ** 53, 1.0          # thr = pi[0] exactly where p_log is all ones
        z[0], p[0], a[0] = states[0], 1.0, 0
        if N > 1:
            pi[states[-1]] = 0.0
            pi[states[-1], 0], pi[states[-1], 1] = 1.0, 1e-310                    # subnormal thr
            z[1], p[1], a[1] = states[-1], 1.0, 1
    return dict(z=z, z_next=zn, a=a, done=g.random(N) < 0.5, p=p.astype(dt), pi=pi)


def _table(c, gpu):
    from rl_offline_simulation_amd.table import TransitionTable
    N = len(c["z"])
    t = TransitionTable(c["z"], c["a"], np.zeros(N, np.float32), c["z_next"], c["done"], c["p"], None, device=gpu)
    order = np.argsort(c["z"], kind="stable")
    assert np.array_equal(t.order.cpu().numpy(), order)
    assert t.p_log.cpu().numpy().dtype == c["p"].dtype and np.array_equal(t.p_log.cpu().numpy(), c["p"][order], equal_nan=True)
    return t, order


def _expected_keys(c, order):
    return np.array([H.key(H.threshold(c["pi"][c["z"][i]], c["p"][i], int(c["a"][i])), c["done"][i], c["z_next"][i]) for i in order], np.uint64)


def _compile(t, pi, gpu):
    """offsim_compile_policy into a sentinel-framed buffer: (rc, keys [N] uint64)."""
    from rl_offline_simulation_amd import _lib as L
    pi_d = torch.as_tensor(np.ascontiguousarray(pi, np.float64)).to(gpu)
    buf = torch.full((t.N + 2 * PAD,), SENT, dtype=torch.int64, device=gpu)
    rc = L.load().offsim_compile_policy(C.byref(t.c), L.ptr(pi_d), buf.data_ptr() + 8 * PAD, L.stream_ptr())
    torch.cuda.synchronize()
    h = buf.cpu().numpy().view(np.uint64)
    assert (h[:PAD] == SENT).all() and (h[PAD + t.N:] == SENT).all(), "written outside keys_out"
    return rc, h[PAD:PAD + t.N], buf


@pytest.mark.parametrize("nA", [1, 2, 5, 16])
@pytest.mark.parametrize("dt", [np.float16, np.float32, np.float64])
def test_compile_policy_keys(dt, nA, gpu):
    """Slots 0, 3, 6 and 7 of 8 are empty: the kernel's binary search over seg_off has to step over leading, inner and trailing ones."""
    for N in (1, 255, 256, 257):
        c = _case(N, nA, dt, [1, 2, 4, 5], 8, seed=1000 * nA + N)
        t, order = _table(c, gpu)
        assert t.n_slots == 8 and t.segment_lengths()[[0, 3, 6, 7]].tolist() == [0, 0, 0, 0]
        rc, keys, _ = _compile(t, c["pi"], gpu)
        want = _expected_keys(c, order)
        assert rc == 0
        bad = np.flatnonzero(keys != want)
        assert bad.size == 0, (N, bad[:5], [hex(int(keys[i])) for i in bad[:5]], [hex(int(want[i])) for i in bad[:5]])
        if N >= 255:  # the case holds what it is meant to hold
            T = ((want >> np.uint64(43)) << np.uint64(32)) | (want & np.uint64(0xFFFFFFFF))
            assert (T == H.T_MAX).any()  # (one action: thr is 1 or NaN, every key is this one)
            if nA >= 2:
                assert (T == 0).any() and (T == ALL_ONES_T).any() and ((T > 0) & (T < H.T_MAX)).any()
                assert ((c["pi"][c["z"]] == 0) & (c["p"] == 0)).any()  # 0 / 0: a NaN row


def test_subnormal_threshold_is_subnormal():
    c = _case(2, 2, np.float32, [1, 2, 4, 5], 8, seed=1)
    thr = c["pi"][c["z"][1]][1] / np.float64(c["p"][1][1]) / (c["pi"][c["z"][1]] / c["p"][1].astype(np.float64)).max()
    assert 0 < thr < np.finfo(np.float64).tiny


@pytest.mark.parametrize("n_slots", [1, 1024])
def test_state_count_limits(n_slots, gpu):
    """One state; and 1024 states with z_next == 1023, the last value of the key's 10-bit field."""
    c = _case(257, 2, np.float32, [0] if n_slots == 1 else [0, 511, 1023], n_slots, seed=n_slots)
    t, order = _table(c, gpu)
    assert t.n_slots == n_slots and int(c["z_next"].max()) == n_slots - 1
    rc, keys, _ = _compile(t, c["pi"], gpu)
    assert rc == 0 and np.array_equal(keys, _expected_keys(c, order))


def test_1025_states_are_refused(gpu):
    from rl_offline_simulation_amd import _lib as L
    c = _case(600, 2, np.float32, [0, 1024], 1025, seed=3)
    c["z_next"][:] = np.arange(600) * 1024 // 599         # enough distinct ids that the table keeps them dense
    t, _ = _table(c, gpu)
    assert t.n_slots == 1025
    rc, keys, _ = _compile(t, c["pi"], gpu)
    assert rc == L.EUNSUPPORTED and (keys == SENT).all()


def _digests(t, keys_dev, fmt, gpu):
    from rl_offline_simulation_amd import _lib as L
    buf = torch.full((t.N + 2 * PAD,), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
    rc = L.load().offsim_compile_digests(C.byref(t.c), keys_dev.data_ptr(), fmt, buf.data_ptr() + 4 * PAD, L.stream_ptr())
    torch.cuda.synchronize()
    h = buf.cpu().numpy().view(np.uint32)
    assert (h[:PAD] == 0x5A5A5A5A).all() and (h[PAD + t.N:] == 0x5A5A5A5A).all(), "written outside dig32_out"
    return rc, h[PAD:PAD + t.N]


def test_compile_digests(gpu):
    """The three layouts from compiled keys and from arbitrary 64-bit words; 255 states run in B and C, 256 are refused there; a format
    that does not exist is refused."""
    from rl_offline_simulation_amd import _lib as L
    for n_slots in (255, 256):
        c = _case(257, 2, np.float64, [0, 100, n_slots - 1], n_slots, seed=n_slots)
        t, order = _table(c, gpu)
        rc, keys, buf = _compile(t, c["pi"], gpu)
        assert rc == 0 and np.array_equal(keys, _expected_keys(c, order))
        rnd = np.random.default_rng(n_slots).integers(0, 2 ** 64, t.N, dtype=np.uint64)
        rnd[0], rnd[1], rnd[2] = np.uint64(0), np.uint64(2 ** 64 - 1), np.uint64(0xFFFFFBFE00000000)
        for words in (keys, rnd):
            kd = torch.from_numpy(words.view(np.int64).copy()).to(gpu)
            for name, fmt in (("A", L.STREAMS_A), ("B", L.STREAMS_B), ("C", L.STREAMS_C)):
                rc, dig = _digests(t, kd, fmt, gpu)
                if n_slots == 256 and name != "A":
                    assert rc == L.EUNSUPPORTED and (dig == 0x5A5A5A5A).all()
                    continue
                assert rc == 0
                assert np.array_equal(dig, np.array([H.digest(int(k), name) for k in words], np.uint32)), name
        for fmt in (-1, 3):
            rc, dig = _digests(t, kd, fmt, gpu)
            assert rc == L.EINVAL and (dig == 0x5A5A5A5A).all()
