"""k_ppo_grad / k_ppo_adam (csrc/ppo_update.hpp) over every dispatched instance, activation, depth, bias layout and tile path, each case
against the NumPy f64 host reference (tests/ppo_update_host.py) and never against the device's own output:

  * the instance and layout matrix and the named edges of tests/ppo_update_cases.py, one ppo_grad pass each: the flat gradient in max norm
    within 4 x the error of torch's own f32 autograd on the CPU (floor: 4 ulps of the gradient's max norm), n, loss, kl, entropy, clipfrac;
  * an all-invalid batch: n = 0, a zero gradient, a stop at pass 0 and not a bit of the weights or the Adam state changed;
  * one Adam step from a zero state in closed form;
  * three update() calls on one learner, the middle one stopping early, against the host run that carries its optimiser across them.

tests/test_ppo_update_matrix_host.py checks, without a device, that each case's bound tells a subtly wrong gradient from a right one."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_update_cases as K  # noqa: E402
from test_gpu_ppo_update import _flat_dev  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from rl_offline_simulation_amd import _lib
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    _lib.load()
    return torch.device("cuda", 0)


def _dev_batch(d, valid, dev):
    out = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items()}
    if valid is not None:
        out["valid"] = torch.from_numpy(np.ascontiguousarray(valid)).to(dev)
    return out


def _group(c):
    return "matrix" if c in K.MATRIX else "edges"


@pytest.mark.parametrize("name", [c.name for c in K.MATRIX + K.EDGES])
def test_grad_case(gpu, name):
    from rl_offline_simulation_amd.evaluators import ppo_grad
    b = K.build(name)
    c, ref = b.case, b.ref
    TM, lds, P, _, _ = K.lds_plan(c.sizes, K.bias_flags(c.bias, len(c.sizes) - 1, c.seed))
    got = ppo_grad(K.model(c), _dev_batch(b.data, b.valid, gpu), c.kind, K.CLIP)
    g = got.grad.cpu().numpy().astype(np.float64)
    assert g.shape == (P,) == ref["g"].shape
    diff = np.abs(g - ref["g"])
    err = float(diff.max())
    per_layer = [tuple(float(diff[s].max()) for s in sl if s is not None) for sl in K.layer_slices(c)]
    print(f"{_group(c)} {name}: P {P} TM {TM} lds {lds} n {int(got.n)} err {err:.3e} bound {b.bound:.3e} ratio {err / b.bound if b.bound else 0.0:.3f} "
          f"max|g| {float(np.abs(ref['g']).max()):.3e}")
    assert np.isfinite(g).all()
    assert err <= b.bound, (err, b.bound, per_layer)  # per layer (W, b): where an excess sits
    assert int(got.n) == ref["n"]
    for key, x in (("loss", got.loss), ("kl", got.kl), ("ent", got.entropy)):
        e, bd = abs(float(x) - ref[key]), K.scalar_bound(ref[key], b.ref32[key])
        print(f"  {key}: err {e:.3e} bound {bd:.3e}")
        assert e <= bd, key
    assert abs(float(got.clipfrac) - ref["cf"]) <= 2.0 / ref["n"]  # (test_gpu_ppo_update.py's rule; the cases keep every ratio clear of the edges)


def _small_pair(seed=3):
    from rl_offline_simulation_amd.evaluators import MLPPolicy, MLPValue
    rng = np.random.default_rng(seed)
    pi, v = K.make_net((5, 12, 3), (True, True), rng), K.make_net((5, 12, 1), (True, False), rng)
    c = K._c("pair", "actor", (5, 12, 3), M=70, seed=seed)
    d = K.make_batch(pi, c, rng)
    return pi, v, d, MLPPolicy(pi, "tanh"), MLPValue(v, "tanh")


def _state(lrn, actor, critic, dev):
    (am, av, at), (cm, cv, ct) = lrn.adam_state()
    return [_flat_dev(actor, dev), _flat_dev(critic, dev)] + [x.cpu().numpy().copy() for x in (am, av, at, cm, cv, ct)]


def test_all_invalid_batch_changes_nothing(gpu):
    """valid = 0 everywhere (NaN in every float column): n = 0 and a zero gradient from ppo_grad; update() stops at pass 0 for the actor and
    for the critic and leaves weights, m, v and t bit for bit, here on a learner whose Adam state is not zero.  The next update() runs as
    if the empty one had not happened."""
    from rl_offline_simulation_amd.evaluators import PPOLearner, ppo_grad
    _, _, d, actor, critic = _small_pair()
    _, _, _, actor2, critic2 = _small_pair()
    good = _dev_batch(d, None, gpu)
    nan = {k: (np.full_like(v, np.nan) if v.dtype.kind == "f" else v) for k, v in d.items()}
    empty = _dev_batch(nan, np.zeros(len(d["adv"]), np.uint8), gpu)
    kw = dict(pi_lr=1e-3, vf_lr=1e-3, train_pi_iters=3, train_v_iters=3, target_kl=1e9)
    lrn, lrn2 = PPOLearner(actor, critic, **kw), PPOLearner(actor2, critic2, **kw)
    lrn.update(good)
    before = _state(lrn, actor, critic, gpu)
    assert int(before[4][0]) == 3 and int(before[7][0]) == 3 and np.any(before[2]) and np.any(before[6])
    for net, kind in ((actor, "actor"), (critic, "critic")):
        got = ppo_grad(net, empty, kind)
        assert float(got.n) == 0.0 and not bool(got.grad.any()) and float(got.loss) == 0.0 and float(got.kl) == 0.0
    info = lrn.update(empty)
    assert int(info.StopIter) == 0
    for x, y in zip(before, _state(lrn, actor, critic, gpu)):
        assert x.tobytes() == y.tobytes()
    for tr in (lrn.pi_trace, lrn.v_trace):
        assert bool(torch.isnan(tr[1:]).all()) and not bool(torch.isnan(tr[0]).any())
    # the stop of the empty call is gone with it: the next call steps both networks, and ends where a learner that never saw the empty
    # batch ends (two identical calls give identical bits: test_gpu_ppo_update.py)
    lrn.update(good)
    lrn2.update(good)
    lrn2.update(good)
    after, want = _state(lrn, actor, critic, gpu), _state(lrn2, actor2, critic2, gpu)
    assert int(after[4][0]) == 6 and int(after[7][0]) == 6 and not np.array_equal(after[0], before[0]) and not np.array_equal(after[1], before[1])
    for x, y in zip(after, want):
        assert x.tobytes() == y.tobytes()


def test_one_adam_step_in_closed_form(gpu):
    """From a zero state, one step on the device's own ppo_grad gradient g (f32): m = 0.1 g, v = 0.001 g^2, t = 1, and
    w' = w - (lr / (1 - 0.9)) * m / (sqrt(v) / sqrt(1 - 0.999) + 1e-8), torch.optim.Adam's line, evaluated here in f64.

    The bound.  The kernel steps on the f64 mean gd, of which g is the rounding: gd = g (1 + d), |d| <= 2^-24.  So the f32 state m differs
    from 0.1 g by that and its own rounding, at most 2^-23 relative, which is within 2 ulps; v = 0.001 gd^2 by 2 d and its rounding.  The
    step's quotient m / (sqrt(v) / sqrt(0.001) + eps) is at most 1 in size and inherits at most 2^-23 (m) + 2^-24 + 2^-25 (sqrt v) < 1e-6
    relative, so the step is off by less than 1e-6 * lr; the final rounding of w' to f32 adds half an ulp of w', at most one ulp of w."""
    from rl_offline_simulation_amd.evaluators import PPOLearner, ppo_grad
    pi, v, d, actor, critic = _small_pair(seed=5)
    batch = _dev_batch(d, None, gpu)
    lrs = dict(actor=3e-3, critic=1e-2)
    g = {k: ppo_grad(net, batch, k).grad.cpu().numpy().astype(np.float64) for k, net in (("actor", actor), ("critic", critic))}
    w0 = dict(actor=_flat_dev(actor, gpu).astype(np.float64), critic=_flat_dev(critic, gpu).astype(np.float64))
    lrn = PPOLearner(actor, critic, pi_lr=lrs["actor"], vf_lr=lrs["critic"], train_pi_iters=1, train_v_iters=1, target_kl=1e9)
    info = lrn.update(batch)
    assert int(info.StopIter) == 0
    ulp = lambda x: np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)  # noqa: E731
    for (m, vv, t), kind, net in zip(lrn.adam_state(), ("actor", "critic"), (actor, critic)):
        gk, lr = g[kind], lrs[kind]
        assert np.all(np.abs(gk) > 1e-12)  # (v stays a normal f32 number)
        m, vv = m.cpu().numpy().astype(np.float64), vv.cpu().numpy().astype(np.float64)
        m_e, v_e = 0.1 * gk, 0.001 * gk * gk
        em, ev = float((np.abs(m - m_e) / ulp(m_e)).max()), float((np.abs(vv - v_e) / ulp(v_e)).max())
        w_e = w0[kind] - (lr / (1.0 - 0.9 ** 1)) * m_e / (np.sqrt(v_e) / np.sqrt(1.0 - 0.999 ** 1) + 1e-8)
        w = _flat_dev(net, gpu).astype(np.float64)
        ew = float(((np.abs(w - w_e)) / (ulp(w) + 1e-6 * lr)).max())
        print(f"{kind}: m off by {em:.2f} ulps, v by {ev:.2f} ulps, w by {ew:.3f} of (1 ulp + 1e-6 lr); |step| {float(np.abs(w - w0[kind]).min()):.3e}..{float(np.abs(w - w0[kind]).max()):.3e}")
        assert int(t) == 1 and em <= 2.0 and ev <= 2.0 and ew <= 1.0
        assert np.all(np.abs(w - w0[kind]) > 0.5 * lr)  # every weight moved by about lr, towards -sign(g)
        assert np.all(np.sign(w0[kind] - w) == np.sign(gk))


def test_adam_state_across_three_calls(gpu):
    """One learner, three update() calls on three batches, the second stopping early: StopIter, t (the steps actually taken), the traces
    (NaN after the stop), weights, m and v after every call against the host f64 run that carries its optimiser.  Bounds: 4 x the deviation
    of the f32 torch loop (autograd + torch.optim.Adam, the same stop rule) from the host run, floor 4 ulps of the largest entry."""
    from rl_offline_simulation_amd.evaluators import MLPPolicy, MLPValue, PPOLearner
    A, R = K.ADAM, K.adam_calls()
    lim = 1.5 * A.target_kl
    actor, critic = MLPPolicy(R.pi0, A.act), MLPValue(R.v0, A.act)
    lrn = PPOLearner(actor, critic, pi_lr=A.pi_lr, vf_lr=A.vf_lr, clip_ratio=K.CLIP, train_pi_iters=A.iters, train_v_iters=A.iters, target_kl=A.target_kl)
    steps = 0
    for i, x in enumerate(R.calls):
        kl = x.a["trace"][:, 1]
        assert np.all(np.abs(kl - lim) >= K.MARGIN * lim)  # ulps cannot move StopIter
        info = lrn.update(_dev_batch(x.data, None, gpu))
        stop = x.a["stop_iter"]
        stopped = kl[-1] > lim
        assert stopped == (i == 1) and int(info.StopIter) == stop
        steps += stop if stopped else A.iters
        (am, av, at), (cm, cv, ct) = lrn.adam_state()
        assert int(at) == steps == x.pi_t and int(ct) == (i + 1) * A.iters == x.v_t  # the critic steps on, whatever the actor's call did
        for nm, got, host, t32 in (("pi", lrn.pi_trace.cpu().numpy(), x.a["trace"], x.tr32_pi), ("v", lrn.v_trace.cpu().numpy(), x.c["trace"], x.tr32_v)):
            k = len(host)
            assert k == (stop + 1 if nm == "pi" else A.iters) and np.isnan(got[k:]).all() and not np.isnan(got[:k]).any(), nm
            for col in ((0, 1) if nm == "pi" else (0,)):
                bound = max(4.0 * float(np.abs(t32[:, col] - host[:, col]).max()), 4.0 * K.ULP * max(1.0, float(np.abs(host[:, col]).max())))
                err = float(np.abs(got[:k, col] - host[:, col]).max())
                print(f"call {i} {nm} trace col {col}: err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
                assert err <= bound, (i, nm, col)
        for nm, got, host, t32 in (("pi w", _flat_dev(actor, gpu), x.pi, x.t32_pi[0]), ("pi m", am.cpu().numpy(), x.pi_m, x.t32_pi[1]),
                                   ("pi v", av.cpu().numpy(), x.pi_v, x.t32_pi[2]), ("v w", _flat_dev(critic, gpu), x.v, x.t32_v[0]),
                                   ("v m", cm.cpu().numpy(), x.v_m, x.t32_v[1]), ("v v", cv.cpu().numpy(), x.v_v, x.t32_v[2])):
            err, bound = float(np.abs(got.astype(np.float64) - host).max()), K.state_bound(host, t32)
            print(f"adam call {i} {nm}: err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
            assert err <= bound, (i, nm)
        assert abs(float(info.KL) - x.a["last"]["kl"]) <= 1e-5 and abs(float(info.LossPi) - x.a["first"]["loss"]) <= 1e-5
