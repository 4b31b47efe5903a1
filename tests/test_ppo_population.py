"""CPU side of PPOPopulation: the C ABI of the population entry points (offsim_vector_collect_ppo_pop, offsim_ppo_advantages_pop,
offsim_ppo_grad_pop, offsim_ppo_update_pop, offsim_ppo_update_work_doubles_pop) -- exported, bound, struct layouts, every refusal before
any HIP call (the pointers are fake addresses: a launch would fault), zero-size calls -- and the argument checks of the Python surface."""
import ctypes
import os
import subprocess
import sys
import types

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_collect import _args  # noqa: E402
from test_ppo_update import _layers, _net  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POP_ENTRIES = ("offsim_vector_collect_ppo_pop", "offsim_ppo_advantages_pop", "offsim_ppo_update_work_doubles_pop", "offsim_ppo_grad_pop",
               "offsim_ppo_update_pop")
F = 0x1000


def test_population_symbols_exported_and_bound():
    from rl_offline_simulation_amd import _lib
    src = open(os.path.join(ROOT, "include", "offsim.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in POP_ENTRIES:
        assert n + "(" in src, n
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
    # each is documented like its single-learner sibling
    for doc, decl in (("/* offsim_vector_collect_ppo_pop:", "int offsim_vector_collect_ppo_pop("), ("/* offsim_ppo_advantages_pop:", "int offsim_ppo_advantages_pop("),
                      ("/* offsim_ppo_grad_pop / offsim_ppo_update_pop:", "int offsim_ppo_update_pop(")):
        assert "rgument validation happens before any HIP call" in src[src.index(doc):src.index(decl)], decl


def test_population_struct_layout_and_macros(tmp_path):
    from rl_offline_simulation_amd import _lib
    cls = _lib.PPOAdamPop
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "offsim.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(offsim_ppo_adam_pop));']
    for f, _ in cls._fields_:
        lines.append(f'  printf("{f} %zu\\n", offsetof(offsim_ppo_adam_pop, {f}));')
    lines.append('  printf("nb %lld\\n", (long long)OFFSIM_PPO_UPDATE_WORK_DOUBLES_NB(4611, 125));')
    lines.append('  printf("full %d\\n", OFFSIM_PPO_UPDATE_WORK_DOUBLES_NB(4611, OFFSIM_PPO_MAX_BLOCKS) == OFFSIM_PPO_UPDATE_WORK_DOUBLES(4611));')
    lines.append('  printf("adv %lld\\n", (long long)OFFSIM_PPO_WORK_DOUBLES_POP(3, 300));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f
    assert int(got["nb"]) == _lib.ppo_update_work_doubles_nb(4611, 125) and int(got["full"]) == 1
    assert int(got["adv"]) == 3 * _lib.ppo_work_doubles(300)


def _collect_pop(L_, E_, T=0, pol_form=None, val_form=None, R=None, critic_sizes=(4, 8, 1), pol=None):
    from rl_offline_simulation_amd import _lib as L
    t, ro, p, st, out, layers = _args(R=L_ * E_ if R is None else R)
    p = p if pol is None else pol
    if pol_form is not None:
        p.form, p.p_next, p.p_init, p.pi = pol_form, F, F, F
    good = _layers(list(critic_sizes))
    val = L.CollectValue(form=L.VALUE_MLP if val_form is None else val_form, n_layers=len(critic_sizes) - 1,
                         layers_host=ctypes.cast(good, ctypes.POINTER(L.MLPLayer)), activation=1, x_dtype=L.F32, dO=critic_sizes[0], x_start=F, x_next=F,
                         x_init=F, v_next=F, v_init=F)
    ppo = L.CollectPPOOut(value=F, logp=F, final_value=F)
    return L.load().offsim_vector_collect_ppo_pop(ctypes.byref(t), ctypes.byref(ro), ctypes.byref(p), ctypes.byref(val), L_, E_, L.PROB_F64,
                                                  L.REJECT_DEFAULT, T, 0, ctypes.byref(st), ctypes.byref(out), ctypes.byref(ppo), None)


def test_collect_pop_validation_before_any_hip_call():
    from rl_offline_simulation_amd import _lib as L
    lib = L.load()
    assert _collect_pop(3, 5) == L.OK, lib.offsim_last_error()  # T = 0 validates and launches nothing
    for l_, e_ in ((0, 5), (-1, 5), (3, 0), (3, -2), (65536, 1)):
        assert _collect_pop(l_, e_, R=15) == L.EINVAL and lib.offsim_last_error().startswith(b"vector_collect_ppo_pop"), (l_, e_)
    assert _collect_pop(3, 5, R=16) == L.EINVAL and b"L * E" in lib.offsim_last_error()
    # only the in-kernel networks
    for form in (L.COLLECT_ROWS, L.COLLECT_TABULAR):
        assert _collect_pop(3, 5, pol_form=form) == L.EUNSUPPORTED, form
    assert _collect_pop(3, 5, val_form=L.VALUE_ROWS) == L.EUNSUPPORTED and b"OFFSIM_COLLECT_MLP" in lib.offsim_last_error()
    # NULL arguments
    t, ro, p, st, out, _ = _args(R=15)
    ppo = L.CollectPPOOut(value=F, logp=F, final_value=F)
    assert lib.offsim_vector_collect_ppo_pop(ctypes.byref(t), ctypes.byref(ro), ctypes.byref(p), None, 3, 5, L.PROB_F64, L.REJECT_DEFAULT, 0, 0,
                                             ctypes.byref(st), ctypes.byref(out), ctypes.byref(ppo), None) == L.EINVAL
    assert lib.offsim_vector_collect_ppo_pop(ctypes.byref(t), None, ctypes.byref(p), None, 3, 5, L.PROB_F64, L.REJECT_DEFAULT, 0, 0,
                                             ctypes.byref(st), ctypes.byref(out), ctypes.byref(ppo), None) == L.EINVAL
    # the budget is per learner: the actor's 4*8+8+8*2+2 = 58 floats and a critic of 4*128+128+128*122+122+122+1 = 16501 together exceed it
    assert _collect_pop(3, 5, critic_sizes=(4, 128, 122, 1)) == L.EUNSUPPORTED and b"MAX_FLOATS" in lib.offsim_last_error()
    assert lib.offsim_last_error().startswith(b"vector_collect_ppo_pop")
    assert _collect_pop(3, 5, critic_sizes=(4, 120, 120, 1)) == L.OK
    # a bad network comes back with the population entry's own prefix
    assert _collect_pop(3, 5, critic_sizes=(4, 8, 2)) == L.EINVAL and lib.offsim_last_error().startswith(b"vector_collect_ppo_pop critic: ")


def test_advantages_pop_validation_before_any_hip_call():
    from rl_offline_simulation_amd import _lib as L
    lib = L.load()

    def adv(T=0, L_=3, E_=5, gamma=0.99, lam=0.97, boot=L.PPO_BOOT_REFERENCE, rew=F, v_trunc=None, adv_norm=None, stats=None, work=None):
        return lib.offsim_ppo_advantages_pop(rew, F, F, F, v_trunc, T, L_, E_, gamma, lam, boot, F, F, adv_norm, stats, work, None)

    assert adv() == L.OK  # T = 0 without adv_norm: nothing to do, nothing launched
    for l_, e_ in ((0, 5), (-3, 5), (3, 0), (3, -1), (65536, 5)):
        assert adv(L_=l_, E_=e_) == L.EINVAL and lib.offsim_last_error().startswith(b"ppo_advantages_pop"), (l_, e_)
    assert adv(T=-1) == L.EINVAL and adv(gamma=1.5) == L.EINVAL and adv(lam=-0.1) == L.EINVAL and adv(boot=7) == L.EINVAL
    assert adv(T=4, rew=None) == L.EINVAL and b"NULL" in lib.offsim_last_error()
    assert adv(T=4, boot=L.PPO_BOOT_SPINUP) == L.EINVAL and b"v_trunc" in lib.offsim_last_error()
    assert adv(T=4, adv_norm=F) == L.EINVAL and b"stats and work" in lib.offsim_last_error()


def _batch(M=0, **kw):
    from rl_offline_simulation_amd import _lib as L
    b = L.PPOBatchC(obs=F, x_dtype=L.F32, dO=4, act=F, adv=F, logp=F, ret=F, valid=None, M=M)
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def _dbl(xs):
    return None if xs is None else (ctypes.c_double * len(xs))(*xs)


def test_grad_and_update_pop_validation_before_any_hip_call():
    from rl_offline_simulation_amd import _lib as L
    lib = L.load()
    net = _net([4, 8, 2])

    def grad(n=net, kind=L.PPO_ACTOR, b=None, L_=3, E_=5, clip=(0.2, 0.1, 0.3), g=F, stats=F, work=F):
        b = _batch() if b is None else b
        return lib.offsim_ppo_grad_pop(ctypes.byref(n) if n is not None else None, kind, ctypes.byref(b) if b != "null" else None, L_, E_, _dbl(clip), g,
                                       stats, work, None)

    def upd(n=net, kind=L.PPO_ACTOR, b=None, L_=3, E_=5, clip=(0.2, 0.1, 0.3), kl=(0.01, 0.0, 1.0), iters=3, lr=(1e-3, 0.0, 1e-2), opt=-1, stats=F,
            trace=F, work=F, m=F):
        b = _batch() if b is None else b
        o = L.PPOAdamPop(m=m, v=F, t=F, lr=_dbl(lr)) if opt == -1 else opt
        return lib.offsim_ppo_update_pop(ctypes.byref(n) if n is not None else None, kind, ctypes.byref(b) if b != "null" else None, L_, E_, _dbl(clip),
                                         _dbl(kl), iters, ctypes.byref(o) if o is not None else None, stats, trace, work, None)

    # zero-size calls launch nothing: T = 0 (M = 0), and iters = 0 with records
    assert grad() == L.OK and upd() == L.OK and upd(b=_batch(M=30), iters=0) == L.OK
    for l_, e_ in ((0, 5), (-1, 5), (3, 0), (3, -5), (65536, 5)):
        assert grad(L_=l_, E_=e_) == L.EINVAL and lib.offsim_last_error().startswith(b"ppo_grad_pop: "), (l_, e_)
        assert upd(L_=l_, E_=e_) == L.EINVAL and lib.offsim_last_error().startswith(b"ppo_update_pop: "), (l_, e_)
    assert grad(n=None) == L.EINVAL and b"ppo_grad_pop" in lib.offsim_last_error()
    assert upd(n=None) == L.EINVAL and b"ppo_update_pop" in lib.offsim_last_error()
    assert grad(b="null") == L.EINVAL and upd(b="null") == L.EINVAL
    assert grad(kind=2) == L.EINVAL and upd(kind=-1) == L.EINVAL
    assert grad(b=_batch(M=31)) == L.EINVAL and b"T * L * E" in lib.offsim_last_error()  # not a multiple of L * E = 15
    assert upd(b=_batch(M=-15)) == L.EINVAL
    # any learner's hyperparameter out of range refuses the call
    for bad in (-0.1, 1.0, float("nan")):
        for i in range(3):
            clip = [0.2, 0.2, 0.2]
            clip[i] = bad
            assert grad(clip=clip) == L.EINVAL and b"clip_ratio" in lib.offsim_last_error(), (bad, i)
            assert upd(clip=clip) == L.EINVAL and b"clip_ratio" in lib.offsim_last_error(), (bad, i)
    assert upd(kl=(0.01, 0.01, -1e-9)) == L.EINVAL and b"target_kl" in lib.offsim_last_error()
    assert upd(kl=(float("nan"), 0.01, 0.01)) == L.EINVAL
    assert upd(lr=(1e-3, -1e-3, 1e-3)) == L.EINVAL and b"lr" in lib.offsim_last_error()
    assert upd(iters=-1) == L.EINVAL and upd(opt=None) == L.EINVAL and upd(clip=None) == L.EINVAL and upd(kl=None) == L.EINVAL and upd(lr=None) == L.EINVAL
    assert grad(clip=None) == L.EINVAL
    # the float cap is a learner's
    big = _net([4, 128, 124, 1])  # 16761 floats
    assert grad(n=big, kind=L.PPO_CRITIC) == L.EUNSUPPORTED and b"MAX_FLOATS" in lib.offsim_last_error()
    assert upd(n=big, kind=L.PPO_CRITIC) == L.EUNSUPPORTED
    assert grad(n=_net([4, 8, 2]), kind=L.PPO_CRITIC) == L.EINVAL and b"one output" in lib.offsim_last_error()
    # with records, the columns and the outputs must be there
    assert grad(b=_batch(M=30, obs=None)) == L.EINVAL and grad(b=_batch(M=30, adv=None)) == L.EINVAL
    assert grad(b=_batch(M=30), g=None) == L.EINVAL and grad(b=_batch(M=30), work=None) == L.EINVAL
    assert upd(b=_batch(M=30), m=None) == L.EINVAL and b"opt->m" in lib.offsim_last_error()
    assert upd(b=_batch(M=30), trace=None) == L.EINVAL and upd(b=_batch(M=30), stats=None) == L.EINVAL and upd(b=_batch(M=30), work=None) == L.EINVAL


def test_work_doubles_pop_sizes_by_the_learners_workgroups():
    from rl_offline_simulation_amd import _lib as L
    lib = L.load()
    ref = _net([4, 64, 64, 2])  # the reference agent's actor: 4610 parameters, tiles of 32 records
    P = 4 * 64 + 64 + 64 * 64 + 64 + 64 * 2 + 2
    size = lambda n, nl, M: lib.offsim_ppo_update_work_doubles_pop(ctypes.byref(n), nl, M)  # noqa: E731
    assert size(ref, 1, 4000) == L.ppo_update_work_doubles_nb(P, 125)
    assert size(ref, 64, 4000) == 64 * L.ppo_update_work_doubles_nb(P, 125)
    assert size(ref, 3, 35) == 3 * L.ppo_update_work_doubles_nb(P, 2) and size(ref, 3, 1) == 3 * L.ppo_update_work_doubles_nb(P, 1)
    assert size(ref, 3, 0) == 3 * L.ppo_update_work_doubles_nb(P, 1)
    # past OFFSIM_PPO_MAX_BLOCKS tiles, and for a caller that does not know M: the single learner's size per learner
    assert size(ref, 2, 32 * 256 + 1) == 2 * L.ppo_update_work_doubles(P) == size(ref, 2, 2 ** 63 - 1)
    assert size(ref, 0, 10) == L.EINVAL and size(ref, 2, -1) == L.EINVAL
    assert lib.offsim_ppo_update_work_doubles_pop(None, 2, 10) == L.EINVAL
    assert size(_net([4, 128, 124, 1]), 2, 10) == L.EUNSUPPORTED


def _pair(hidden=8, nA=2, act="tanh", dO=4, seed=0):
    import torch
    from rl_offline_simulation_amd.evaluators import MLPPolicy, MLPValue
    g = torch.Generator().manual_seed(seed)
    w = lambda o, i: (torch.randn(o, i, generator=g), torch.randn(o, generator=g))  # noqa: E731
    return MLPPolicy([w(hidden, dO), w(nA, hidden)], act), MLPValue([w(hidden, dO), w(1, hidden)], act)


def test_population_python_surface():
    """What needs no device: the exports, PPOPopulation's argument checks, the per-learner export of the host copy."""
    import torch
    import rl_offline_simulation_amd as P
    from rl_offline_simulation_amd.evaluators import PPOPopulation, VectorPSRS, ppo_grad_population  # noqa: F401
    assert P.PPOPopulation is PPOPopulation and "PPOPopulation" in P.__all__
    pairs = [_pair(seed=s) for s in range(3)]
    actors, critics = [a for a, _ in pairs], [c for _, c in pairs]
    pop = PPOPopulation(actors, critics)
    assert pop.L == 3 and pop.pi_lr == [3e-4] * 3 and pop.vf_lr == [1e-3] * 3 and pop.clip_ratio == [0.2] * 3 and pop.target_kl == [0.01] * 3
    assert (pop.train_pi_iters, pop.train_v_iters) == (80, 80)
    pop = PPOPopulation(actors, critics, pi_lr=[1e-4, 2e-4, 3e-4], target_kl=(0.0, 0.01, 1.0), clip_ratio=[0.1, 0.2, 0.3], vf_lr=2e-3)
    assert pop.pi_lr == [1e-4, 2e-4, 3e-4] and pop.target_kl == [0.0, 0.01, 1.0] and pop.vf_lr == [2e-3] * 3
    for l in range(3):
        for (W, b), (W0, b0) in zip(pop.actor(l).weights, actors[l].weights):
            assert torch.equal(W, W0) and torch.equal(b, b0)
        assert torch.equal(pop.state_dict(l)["critic"]["2.weight"], critics[l].weights[1][0])
        a, c = pop.to_torch(l)
        x = torch.randn(5, 4)
        assert torch.equal(a(x), actors[l].to_torch()(x)) and c(x).shape == (5, 1)
    with pytest.raises(IndexError):
        pop.actor(3)
    # mixed architectures
    other_a, other_c = _pair(hidden=9)
    relu_a, relu_c = _pair(act="relu")
    for bad_a, bad_c in (([actors[0], other_a], critics[:2]), (actors[:2], [critics[0], other_c]), ([actors[0], relu_a], critics[:2]),
                         (actors[:2], [critics[0], relu_c]), (actors, critics[:2]), ([], []), (critics, actors), ([actors[0], "net"], critics[:2])):
        with pytest.raises(ValueError):
            PPOPopulation(bad_a, bad_c)
    with pytest.raises(ValueError):
        PPOPopulation(actors, [_pair(dO=5)[1]] * 3)
    # a hyperparameter sequence of the wrong length, or out of range for one learner
    for kw in (dict(pi_lr=[1e-3, 1e-3]), dict(vf_lr=[1e-3] * 4), dict(clip_ratio=[0.2]), dict(target_kl=[0.01, 0.01]),
               dict(clip_ratio=[0.2, 1.0, 0.2]), dict(target_kl=[0.01, -1.0, 0.01]), dict(pi_lr=[1e-3, 1e-3, -1e-3]), dict(train_pi_iters=-1)):
        with pytest.raises(ValueError):
            PPOPopulation(actors, critics, **kw)
    # the environments must divide among the learners (checked before anything touches the device)
    for n in (7, 2, 0):
        with pytest.raises(ValueError, match="multiple"):
            VectorPSRS.collect_ppo_population(types.SimpleNamespace(num_envs=n), pop, 4)
    with pytest.raises(TypeError):
        VectorPSRS.collect_ppo_population(types.SimpleNamespace(num_envs=6), actors[0], 4)
