"""CPU side of the encoder population (HOMERPopulation.encode / latent_report / evaluators): the restated grid rule of
offsim_encode_mlp_pop and offsim_latent_counts against hand-computed values, the C ABI of both -- exported, bound, documented, every
refusal before any HIP call (the pointers are fake addresses: a launch would fault) --, latent_report's arithmetic on hand-made counts, and
PerStateRejectionSampling.from_latents against the constructor with a table-lookup encoder."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import encoder_host as E  # noqa: E402
import encoder_pop_host as P  # noqa: E402

ENTRIES = ("offsim_encode_mlp_pop", "offsim_latent_counts")
F = 0x1000


# ---- the grid rule ----
def test_grid_rule_hand_computed():
    S128, S2, G, V = ("S", (128, 2)), ("S", (2, 1)), ("G", (1, 1)), ("V", ())
    # L = 1 is the single call's grid, whatever the rows fill
    for path, inst in (S128, S2, ("R", (4, 2)), G, V):
        for N in (1, 33, 129, 16384, 1_000_000):
            assert P.pop_grid(path, inst, N, 1) == (P.single_grid(path, inst, N), 1), (path, inst, N)
    # the single call: S at dO = 128 (WPE 1) ceil(N / 128) up to 256; at dO = 2 (WPE 2) twice that; G up to 1024; V ceil(N / 256) up to 2048
    assert [P.single_grid(*S128, N) for N in (1, 129, 16384, 32768, 1_000_000)] == [1, 2, 128, 256, 256]
    assert [P.single_grid(*S2, N) for N in (1, 129, 16384, 1_000_000)] == [2, 4, 256, 512]
    assert [P.single_grid(*G, N) for N in (1, 129, 131072, 1_000_000)] == [1, 2, 1024, 1024]
    assert [P.single_grid(*V, N) for N in (1, 300, 1_000_000)] == [1, 2, 2048]
    # dO = 2: a workgroup takes 256 rows a pass, so 16384 rows fill 64 workgroups where the single call starts 256
    assert P.rows_per_wg(*S2) == 256 and P.rows_per_wg(*S128) == 128 and P.rows_per_wg(*G) == 128 and P.rows_per_wg(*V) == 256
    assert P.pop_grid(*S2, 16384, 2) == (128, 2)   # ceil(256 / 2): the total stays at the single call's 256
    assert P.pop_grid(*S2, 16384, 8) == (64, 8)    # capped by the rows: 512 in all
    assert P.pop_grid(*S2, 16384, 64) == (64, 64)  # 4096 in all, not 64 x 256
    assert P.pop_grid(*S2, 129, 3) == (2, 3) and P.pop_grid(*S2, 1, 3) == (1, 3)
    assert P.pop_grid(*S2, 1_000_000, 64) == (512, 64)
    # dO = 128, G and V: the single call's count is already what the rows fill
    assert P.pop_grid(*S128, 16384, 8) == (128, 8) and P.pop_grid(*S128, 1_000_000, 64) == (256, 64) and P.pop_grid(*S128, 33, 3) == (1, 3)
    assert P.pop_grid(*G, 129, 3) == (2, 3) and P.pop_grid(*G, 1_000_000, 2) == (1024, 2)
    assert P.pop_grid(*V, 300, 3) == (2, 3) and P.pop_grid(*V, 1_000_000, 2) == (2048, 2)
    # the total never shrinks below the single call's, and a learner never starts more than the single call
    for path, inst in (S128, S2, ("S", (4, 2)), G, V):
        for N in (1, 33, 129, 4097, 16384, 1_000_000):
            for L_ in (1, 2, 3, 8, 64, 65535):
                g, y = P.pop_grid(path, inst, N, L_)
                assert y == L_ and 1 <= g <= P.single_grid(path, inst, N) <= g * L_, (path, inst, N, L_)


def test_stride_rows_send_every_learner_round_the_loop():
    for (path, inst), want in ((("S", (128, 2)), 2 * 32768 + 39), (("S", (2, 1)), 2 * 131072 + 39), (("G", (1, 1)), 2 * 131072 + 39),
                               (("V", ()), 2 * 524288 + 39)):
        assert P.stride_N(path, inst, 2) == want
        assert P.pop_sweep_rows(path, inst, want, 2) == E.sweep_rows(path, inst)


def test_latent_grid_rule():
    assert [P.latent_grid(N, 3) for N in (1, 4096, 4097, 4096 * 1024, 10 ** 8)] == [(1, 3), (1, 3), (2, 3), (1024, 3), (1024, 3)]
    assert P.latent_lds_bytes(25, 0) == 200 and P.latent_lds_bytes(64, 25) == 12800 and P.latent_lds_bytes(128, 64) == 65536


# ---- the C ABI ----
def test_symbols_exported_bound_and_documented():
    from rl_offline_simulation_amd import _lib
    src = open(os.path.join(ROOT, "include", "offsim.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ENTRIES:
        assert "int " + n + "(" in src, n
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
        assert "rgument validation happens before any HIP call" in src[src.index("/* " + n + ":"):src.index("int " + n + "(")], n
    assert len(_lib.SIGNATURES["offsim_encode_mlp_pop"][1]) == len(_lib.SIGNATURES["offsim_encode_mlp"][1]) + 1
    assert len(_lib.SIGNATURES["offsim_latent_counts"][1]) == 10


def _encode_pop(L_=3, N=33, dO=4, H=64, nZ=25, x_dtype=None, x=F, W1=F, b1=F, W2=F, b2=F, z=F, logits=F):
    from rl_offline_simulation_amd import _lib as L
    return L.load().offsim_encode_mlp_pop(x, L.F32 if x_dtype is None else x_dtype, N, dO, W1, b1, H, W2, b2, nZ, L_, z, logits, None)


def test_encode_mlp_pop_validation_before_any_hip_call():
    from rl_offline_simulation_amd import _lib as L
    lib = L.load()
    assert _encode_pop(N=0) == L.OK, lib.offsim_last_error()  # N = 0 validates and launches nothing
    assert _encode_pop(1, N=0) == L.OK and _encode_pop(65535, N=0) == L.OK
    for l_ in (0, -1, 65536):
        for n in (0, 33):
            assert _encode_pop(l_, N=n) == L.EINVAL and lib.offsim_last_error().startswith(b"encode_mlp_pop") and b"65535" in lib.offsim_last_error(), l_
    assert _encode_pop(H=129) == L.EUNSUPPORTED and lib.offsim_last_error().startswith(b"encode_mlp_pop") and b"128" in lib.offsim_last_error()
    for kw in (dict(W1=None), dict(b1=None), dict(W2=None), dict(b2=None)):
        for n in (0, 33):
            assert _encode_pop(N=n, **kw) == L.EINVAL and lib.offsim_last_error().startswith(b"encode_mlp_pop"), kw
    for kw in (dict(x=None), dict(z=None), dict(N=-1), dict(dO=0), dict(H=0), dict(nZ=0)):
        assert _encode_pop(**kw) == L.EINVAL and lib.offsim_last_error().startswith(b"encode_mlp_pop"), kw
    # the LDS limit of the kernel the shape lands on (G at HT = 4, ZT = 2: 4 (128 x 301 + 64 x 129 + 192) bytes; V at nZ = 65)
    assert E.dispatch(300, 128, 64)[0] == "refused" and E.dispatch(300, 128, 65)[0] == "refused"
    for nZ in (64, 65):
        assert _encode_pop(dO=300, H=128, nZ=nZ) == L.EUNSUPPORTED and b"LDS" in lib.offsim_last_error() and lib.offsim_last_error().startswith(b"encode_mlp_pop")
    # neither f32 nor f16, on a shape of the VALU kernel (the MFMA paths do not take it either)
    assert _encode_pop(dO=4, H=96, nZ=5, x_dtype=L.F64) == L.EINVAL and b"x_dtype" in lib.offsim_last_error()
    # the single entry point keeps its own name in its messages
    assert lib.offsim_encode_mlp(F, L.F32, 33, 4, F, F, 129, F, F, 5, F, F, None) == L.EUNSUPPORTED and lib.offsim_last_error().startswith(b"encode_mlp:")


def _counts(L_=3, N=0, nZ=25, labels=None, nY=0, z=F, counts=F, joint=None, skipped=F):
    from rl_offline_simulation_amd import _lib as L
    return L.load().offsim_latent_counts(z, L_, N, nZ, labels, nY, counts, joint, skipped, None)


def test_latent_counts_validation_before_any_hip_call():
    from rl_offline_simulation_amd import _lib as L
    lib = L.load()
    for l_ in (0, -1, 65536):
        assert _counts(l_, N=10) == L.EINVAL and lib.offsim_last_error().startswith(b"latent_counts") and b"65535" in lib.offsim_last_error(), l_
    for kw in (dict(N=-1), dict(nZ=0), dict(N=10, z=None), dict(N=10, counts=None), dict(N=10, skipped=None)):
        assert _counts(**kw) == L.EINVAL and lib.offsim_last_error().startswith(b"latent_counts"), kw
    assert _counts(N=10, joint=F, nY=5) == L.EINVAL and b"out_joint without labels" in lib.offsim_last_error()
    assert _counts(N=10, labels=F, nY=0) == L.EINVAL and _counts(N=10, labels=F, nY=-3, joint=F) == L.EINVAL
    # the LDS limit: nZ * max(nY, 1) * 8 bytes, at most 64 KiB (nY counts only with out_joint)
    assert _counts(N=10, nZ=8193) == L.EUNSUPPORTED and b"64 KiB" in lib.offsim_last_error()
    assert _counts(N=10, nZ=128, labels=F, nY=65, joint=F) == L.EUNSUPPORTED
    assert _counts(N=10, nZ=129, labels=F, nY=64, joint=F) == L.EUNSUPPORTED


# ---- latent_report's arithmetic ----
def test_latent_stats_on_hand_made_counts():
    from rl_offline_simulation_amd.encoders.homer_population import LatentReport, latent_stats
    joint = torch.tensor([[[3, 0, 0], [0, 2, 1], [0, 0, 0], [0, 0, 4]],   # learner 0: 3 + 2 + 0 + 4 of 10 rows
                          [[1, 1, 1], [1, 1, 1], [1, 1, 1], [0, 0, 1]],   # learner 1: 1 + 1 + 1 + 1
                          [[0, 0, 0], [0, 0, 0], [4, 3, 3], [0, 0, 0]]],  # learner 2: one latent state holds everything
                         dtype=torch.int64)
    counts = joint.sum(2)
    used, purity = latent_stats(counts, joint, 10)
    assert used.tolist() == [3, 4, 1] and used.dtype == torch.int64
    assert purity.dtype == torch.float64 and purity.tolist() == [9 / 10, 4 / 10, 4 / 10]
    used, purity = latent_stats(counts, None, 10)
    assert used.tolist() == [3, 4, 1] and purity is None
    # exact in f64 where f32 would round: 2^24 + 1 rows in one bin
    big = torch.tensor([[[2 ** 24 + 1, 0]]], dtype=torch.int64)
    assert latent_stats(big.sum(2), big, 2 ** 24 + 1)[1].tolist() == [1.0]
    assert latent_stats(big.sum(2), big, 2 ** 25)[1].item() == (2 ** 24 + 1) / 2 ** 25
    assert latent_stats(torch.zeros((2, 5), dtype=torch.int64), torch.zeros((2, 5, 3), dtype=torch.int64), 0)[1].tolist() == [0.0, 0.0]
    assert LatentReport._fields == ("z", "counts", "used", "joint", "purity", "skipped")


def test_population_has_the_entry_points():
    from rl_offline_simulation_amd.encoders import HOMERPopulation
    for n in ("encode", "encode_device", "latent_report", "latent_counts", "evaluators"):
        assert callable(getattr(HOMERPopulation, n)), n


# ---- from_latents ----
class _Lookup:
    """a table-lookup encoder: observation k of the discrete grid log is latent state table[k]"""

    def __init__(self, table):
        self.table = np.asarray(table)

    def encode(self, observations):
        return self.table[np.asarray(observations)]


def _grid_dataset():
    from rl_offline_simulation_amd import OfflineDataset, ProbDistribution, spaces, synth
    e = synth.grid_log(10, 5, 10, (4, 4), seed=0)
    keys = ("observations", "actions", "rewards", "next_observations", "terminals", "action_distributions", "steps")
    return OfflineDataset(spaces.Discrete(25), spaces.Discrete(5), ProbDistribution.Discrete, **{k: e[k] for k in keys}), e


def test_from_latents_hands_the_constructors_table_to_psrs(monkeypatch):
    """PSRS.from_arrays builds the device table: replaced by a recorder, so that what the two routes hand it is compared with no device."""
    from rl_offline_simulation_amd.evaluators import per_state_rejection as M
    from rl_offline_simulation_amd.evaluators import PerStateRejectionSampling
    calls = []

    def record(*args, **kw):
        calls.append((args, kw))
        return object()
    monkeypatch.setattr(M.PSRS, "from_arrays", staticmethod(record))
    ds, e = _grid_dataset()
    enc = _Lookup(np.random.default_rng(3).permutation(25))
    a = PerStateRejectionSampling(ds, 25, encoder=enc)
    b = PerStateRejectionSampling.from_latents(ds, enc.encode(e["observations"]), enc.encode(e["next_observations"]), 25)
    assert isinstance(b, PerStateRejectionSampling) and b._dataset is ds and b.new_step_api is False and a.new_step_api is False
    assert b.observation_space is ds.observation_space and b.action_space is ds.action_space
    (args_a, kw_a), (args_b, kw_b) = calls
    assert len(args_a) == len(args_b) == 6 and sorted(kw_a) == sorted(kw_b)
    for x, y in zip(args_a, args_b):
        assert np.array_equal(np.asarray(x), np.asarray(y)) and np.asarray(x).dtype == np.asarray(y).dtype
    assert not np.array_equal(np.asarray(args_b[0]), e["observations"])  # the latents, not the observations
    for k in kw_a:
        x, y = kw_a[k], kw_b[k]
        assert (x is None and y is None) or np.array_equal(np.asarray(x), np.asarray(y)), k
    assert kw_b["nS"] == 25 and kw_b["nA"] == 5 and kw_b["reject_func"] is None and kw_b["reject_mode"] is None
    assert PerStateRejectionSampling.from_latents(ds, e["z"], e["z_next"], 25, new_step_api=True).new_step_api is True


def test_from_latents_keeps_a_subclass_rule_and_the_errors(monkeypatch):
    from rl_offline_simulation_amd import OfflineDataset, ProbDistribution, spaces
    from rl_offline_simulation_amd.evaluators import per_state_rejection as M
    from rl_offline_simulation_amd.evaluators import PerStateRejectionSampling
    calls = []
    monkeypatch.setattr(M.PSRS, "from_arrays", staticmethod(lambda *a, **kw: calls.append(kw) or object()))
    ds, e = _grid_dataset()

    class Hooked(PerStateRejectionSampling):
        def _reject(self, p_new, p_log, a):
            return False

    class Ruled(PerStateRejectionSampling):
        _device_reject_mode = 1
    for cls in (Hooked, Ruled):
        cls(ds, 25, encoder=_Lookup(np.arange(25)))
        ev = cls.from_latents(ds, e["z"], e["z_next"], 25)
        assert type(ev) is cls
        ctor, lat = calls[-2:]
        assert ctor["reject_mode"] == lat["reject_mode"] and (ctor["reject_func"] is None) == (lat["reject_func"] is None)
    assert calls[1]["reject_func"] is not None and calls[3]["reject_mode"] == 1
    with pytest.raises(ValueError, match="one latent state per transition"):
        PerStateRejectionSampling.from_latents(ds, e["z"][:-1], e["z_next"][:-1], 25)
    with pytest.raises(ValueError, match="num_states"):
        PerStateRejectionSampling.from_latents(ds, e["z"], e["z_next"], None)
    kw = {k: e[k] for k in ("observations", "rewards", "next_observations", "terminals", "action_distributions", "steps")}
    cont = OfflineDataset(spaces.Discrete(25), spaces.Box(0, 1, (1,)), ProbDistribution.Discrete, actions=np.zeros((len(e["z"]), 1), np.float32), **kw)
    with pytest.raises(ValueError, match="discrete action spaces"):
        PerStateRejectionSampling.from_latents(cont, e["z"], e["z_next"], 25)
