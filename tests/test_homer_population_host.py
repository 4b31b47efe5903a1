"""CPU side of HOMERPopulation: epoch_draws on a CPU generator, the per-learner hyperparameters, and the C ABI of
offsim_homer_grad_pop / offsim_homer_step_pop (struct layouts, the per-learner scratch size, argument validation before any HIP call)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import homer_train_host as HH  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT64_MAX = 2 ** 63 - 1


def test_epoch_draws_on_a_cpu_generator():
    from rl_offline_simulation_amd.encoders import epoch_draws
    L, n, nZ = 5, 37, 3
    g = torch.Generator()
    g.manual_seed(11)
    ir, ii, nz = epoch_draws(g, L, n, nZ)
    assert ir.shape == ii.shape == (L, n) and ir.dtype == ii.dtype == torch.int32
    assert nz.shape == (L, n, 4, nZ) and nz.dtype == torch.float32 and bool(torch.isfinite(nz).all())
    for idx in (ir, ii):
        assert torch.equal(idx.sort(dim=1)[0], torch.arange(n, dtype=torch.int32).expand(L, n))  # every row a permutation
        assert len({tuple(r.tolist()) for r in idx}) == L                                       # the learners' draws differ
    assert not torch.equal(ir, ii)
    assert len({tuple(r.reshape(-1).tolist()) for r in nz}) == L
    # the same seed gives the same draws, the next call of the same generator other ones, and nothing else is consumed
    state = torch.get_rng_state()
    g2 = torch.Generator()
    g2.manual_seed(11)
    again = epoch_draws(g2, L, n, nZ)
    assert all(torch.equal(x, y) for x, y in zip((ir, ii, nz), again))
    nxt = epoch_draws(g2, L, n, nZ)
    assert not torch.equal(nxt[0], ir) and not torch.equal(nxt[2], nz)
    assert torch.equal(torch.get_rng_state(), state)  # torch's global generator is untouched
    # standard Gumbel: mean = Euler's constant, variance = pi^2 / 6 (60 000 draws: 5 standard errors)
    big = epoch_draws(g, 4, 1500, 10)[2].double()
    assert abs(float(big.mean()) - 0.5772156649) < 5 * 1.2825 / np.sqrt(big.numel())
    assert abs(float(big.var()) - np.pi ** 2 / 6) < 0.06
    assert epoch_draws(g, 1, 0, 2)[0].shape == (1, 0)


def test_initial_weights_and_per_learner_arguments():
    from rl_offline_simulation_amd.encoders import HOMEREncoder, HOMERPopulation
    from rl_offline_simulation_amd.encoders.homer_population import _per_learner
    dims = (3, 4, 6, 8)
    pop = HOMERPopulation(*dims, seeds=[3, 9, 3])
    assert pop.L == 3 and pop.n_params == HH.n_params(*dims)
    for l, seed in enumerate((3, 9, 3)):
        torch.manual_seed(seed)
        want, got = HOMEREncoder(*dims).state_dict(), pop.state_dict(l)
        assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want), l
    assert not torch.equal(pop.state_dict(0)["obs_encoder.0.weight"], pop.state_dict(1)["obs_encoder.0.weight"])
    # state_dicts and from_encoders stack what they are given
    sds = [pop.state_dict(l) for l in (1, 0)]
    pop2 = HOMERPopulation(*dims, state_dicts=sds)
    assert pop2.L == 2 and all(torch.equal(pop2.state_dict(0)[k], sds[0][k]) for k in sds[0])
    with pytest.raises(IndexError):
        pop2.state_dict(2)
    with pytest.raises(ValueError):
        HOMERPopulation(*dims, L=3, seeds=[1, 2])
    with pytest.raises(ValueError):
        HOMERPopulation(*dims)
    with pytest.raises(ValueError):
        HOMERPopulation(*dims, seeds=[])
    with pytest.raises(ValueError):
        HOMERPopulation(4, 4, 6, 8, state_dicts=sds)  # another architecture
    with pytest.raises(ValueError):
        pop.best()
    # a scalar or one value per learner
    assert pop.lr == [1e-3] * 3 and pop.weight_decay == [0.0] * 3 and pop.max_grad_norm == [40.0] * 3
    pop.lr, pop.weight_decay = [1e-3, 1e-2, 0.0], 0.01
    assert pop.lr == [1e-3, 1e-2, 0.0] and pop.weight_decay == [0.01] * 3
    for name in ("lr", "weight_decay", "max_grad_norm"):
        for bad in ([1e-3, 1e-2], [1e-3] * 4, [], -1.0, [1.0, -1.0, 1.0], float("nan")):
            with pytest.raises(ValueError):
                setattr(pop, name, bad)
    assert pop.lr == [1e-3, 1e-2, 0.0]  # a refused value changes nothing
    assert _per_learner(np.float32(2.0), 2, "lr") == [2.0, 2.0] and _per_learner(np.array([1.0, 2.0]), 2, "lr") == [1.0, 2.0]


# ---- the C ABI ----
def test_population_struct_layout_and_signatures(tmp_path):
    from rl_offline_simulation_amd import _lib
    pairs = {"offsim_homer_batch_pop": _lib.HomerBatchPop, "offsim_homer_adam_pop": _lib.HomerAdamPop}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "offsim.h"', "int main(void) {"]
    for c_name, cls in pairs.items():
        lines.append(f'  printf("{c_name} %zu\\n", sizeof({c_name}));')
        for f, _ in cls._fields_:
            lines.append(f'  printf("{c_name}.{f} %zu\\n", offsetof({c_name}, {f}));')
    lines.append('  printf("work %lld\\n", (long long)OFFSIM_HOMER_WORK_DOUBLES_NB(18420, 8));')
    lines.append('  printf("full %d\\n", OFFSIM_HOMER_WORK_DOUBLES_NB(5531, OFFSIM_HOMER_MAX_BLOCKS) == OFFSIM_HOMER_WORK_DOUBLES(5531));')
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
    assert int(got["work"]) == _lib.homer_work_doubles_nb(18420, 8) == 8 * 2 + 8 + 72 + 9210 + 8 * 9210
    assert int(got["full"]) == 1 and _lib.homer_work_doubles_nb(5531, _lib.HOMER_MAX_BLOCKS) == _lib.homer_work_doubles(5531)
    for n in ("offsim_homer_work_doubles_pop", "offsim_homer_grad_pop", "offsim_homer_step_pop"):
        assert n in _lib.SIGNATURES, n


def _net(dO=4, nA=2, nZ=10, H=16, slope=0.01, **ptrs):
    from rl_offline_simulation_amd import _lib as L
    f = 0x1000
    n = L.HomerNet(f, f, f, f, f, f, f, f, dO, nA, nZ, H, slope, 0)
    for k, v in ptrs.items():
        setattr(n, k, v)
    return n


# (dims, TM from the LDS budget): DESIGN section 14's table, and the smallest net
WORK_SHAPES = [((2, 5, 25, 64), 32), ((128, 5, 50, 64), 8), ((3, 3, 2, 5), 32)]


def _nb(tm_lds, M):
    """ht_prepare's rule: the tile from the LDS budget, halved down to 8 while the batch has fewer than 8 tiles; at most 128 workgroups"""
    TM = tm_lds
    while TM > 8 and M < TM * 8:
        TM //= 2
    return max(1, min(-(-M // TM), 128))


@pytest.mark.parametrize("dims,tm_lds", WORK_SHAPES, ids=["2_5_25_64", "128_5_50_64", "3_3_2_5"])
def test_work_doubles_pop_is_per_learner_for_its_workgroups(dims, tm_lds):
    from rl_offline_simulation_amd import _lib as L
    lib = L.load()
    dO, nA, nZ, H = dims
    net, P = _net(dO=dO, nA=nA, nZ=nZ, H=H), L.homer_params(*dims)
    want_nb = {1: 1, 64: 8, 4500: 128, INT64_MAX: 128}
    for M in (1, 64, 4500, INT64_MAX):
        nb = _nb(tm_lds, M)
        assert nb == want_nb[M]
        for n_learners in (1, 3, 64):
            assert lib.offsim_homer_work_doubles_pop(ctypes.byref(net), n_learners, M) == n_learners * L.homer_work_doubles_nb(P, nb), (M, n_learners)
    # between the thresholds of the tile rule: 255 records are 16 tiles of 16, 256 are 8 tiles of 32 (where the LDS budget allows 32)
    for M in (0, 8, 9, 127, 128, 255, 256, 1000, 4096, 4097, 10 ** 12):
        assert lib.offsim_homer_work_doubles_pop(ctypes.byref(net), 2, M) == 2 * L.homer_work_doubles_nb(P, _nb(tm_lds, M)), M
    # the single call's reservation is the population's at 128 workgroups
    assert lib.offsim_homer_work_doubles_pop(ctypes.byref(net), 1, INT64_MAX) == lib.offsim_homer_work_doubles(ctypes.byref(net))
    assert lib.offsim_homer_work_doubles_pop(ctypes.byref(net), 0, 64) == L.EINVAL
    assert lib.offsim_homer_work_doubles_pop(ctypes.byref(net), 2, -1) == L.EINVAL
    assert lib.offsim_homer_work_doubles_pop(None, 2, 64) == L.EINVAL
    if dims == (2, 5, 25, 64):  # the reference's configuration, batch 64: 8 workgroups per learner, not the 128 of the single call
        assert L.homer_work_doubles_nb(P, 8) * 8 == 199_520 and L.homer_work_doubles(P) * 8 == 2_856_800


def test_population_validation_before_any_hip_call():
    from rl_offline_simulation_amd import _lib as L
    lib, f = L.load(), 0x1000

    def batch(M=0, stride=None, **kw):
        b = L.HomerBatchPop(obs=f, next_obs=f, x_dtype=L.F32, act=f, n_rows=10, idx_real=f, idx_impo=f, noise=None, M=M,
                            idx_stride=M if stride is None else stride)
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    def grad(n=None, b=None, n_learners=2, tau=1.0, hard=0, g=f, stats=f, work=f, null_net=False, null_batch=False):
        n, b = n or _net(), b or batch()
        return lib.offsim_homer_grad_pop(None if null_net else ctypes.byref(n), None if null_batch else ctypes.byref(b), n_learners, tau, hard, None, g,
                                         stats, work, None)

    def step(n=None, b=None, n_learners=2, tau=1.0, opt=-1, stats=f, work=f):
        n, b = n or _net(), b or batch()
        o = L.HomerAdamPop(m=f, v=f, t=f, lr=f, weight_decay=f, max_grad_norm=f) if opt == -1 else opt
        return lib.offsim_homer_step_pop(ctypes.byref(n), ctypes.byref(b), n_learners, tau, ctypes.byref(o) if o is not None else None, None, stats, work, None)

    # M = 0 launches nothing (every pointer here is a fake address: a launch would fault)
    assert grad() == L.OK and step() == L.OK and grad(n_learners=65535) == L.OK and step(n_learners=1) == L.OK
    for call in (grad, step):
        for bad in (0, -1, 65536):
            assert call(n_learners=bad) == L.EINVAL and b"L must be in 1..65535" in lib.offsim_last_error(), bad
        assert call(b=batch(M=5, stride=4)) == L.EINVAL and b"idx_stride" in lib.offsim_last_error()
        assert call(b=batch(M=0, stride=7)) == L.OK
        assert call(n=_net(nZ=1)) == L.EINVAL and b"nZ" in lib.offsim_last_error()
        assert call(n=_net(nZ=2)) == L.OK
        for bad in (0.0, -1.0, float("nan")):
            assert call(tau=bad) == L.EINVAL and b"tau" in lib.offsim_last_error()
        assert call(n=_net(slope=-0.1)) == L.EINVAL
        assert call(n=_net(dO=0)) == L.EINVAL and call(n=_net(dO=129)) == L.EINVAL and call(n=_net(H=257)) == L.EINVAL
        assert call(n=_net(nA=0)) == L.EINVAL and call(n=_net(nA=17)) == L.EINVAL and call(n=_net(nZ=257)) == L.EINVAL
        for k in ("enc_W1", "enc_b1", "enc_W2", "enc_b2", "cls_W1", "cls_b1", "cls_W2", "cls_b2"):
            assert call(n=_net(**{k: None})) == L.EINVAL and b"NULL" in lib.offsim_last_error(), k
        assert call(b=batch(x_dtype=L.F64)) == L.EINVAL and b"x_dtype" in lib.offsim_last_error()
        assert call(b=batch(M=-1)) == L.EINVAL
        for k in ("obs", "next_obs", "act", "idx_real", "idx_impo"):
            assert call(b=batch(M=3, **{k: None})) == L.EINVAL and b"NULL" in lib.offsim_last_error(), k
        assert call(b=batch(M=3), stats=None) == L.EINVAL and call(b=batch(M=3), work=None) == L.EINVAL
        assert call(n=_net(dO=128, nA=5, nZ=50, H=128)) == L.EUNSUPPORTED and b"MAX_FLOATS" in lib.offsim_last_error()
    assert grad(null_net=True) == L.EINVAL and b"homer_grad_pop" in lib.offsim_last_error()
    assert grad(null_batch=True) == L.EINVAL and b"batch is NULL" in lib.offsim_last_error()
    assert grad(hard=1) == L.EINVAL and b"forward only" in lib.offsim_last_error()
    assert grad(hard=1, g=None) == L.OK and grad(hard=0, g=None) == L.OK
    assert step(opt=None) == L.EINVAL and b"homer_step_pop" in lib.offsim_last_error()
    for k in ("m", "v", "t", "lr", "weight_decay", "max_grad_norm"):
        o = L.HomerAdamPop(m=f, v=f, t=f, lr=f, weight_decay=f, max_grad_norm=f)
        setattr(o, k, None)
        assert step(b=batch(M=3), opt=o) == L.EINVAL and b"adam->" in lib.offsim_last_error(), k
