"""k_homer_grad / k_homer_reduce / k_homer_adam (csrc/homer_train.hpp) over every dispatched instance, every tile size ht_prepare can
choose (TM 4, 8, 16 and 32, from the LDS budget and from M), LDS at exactly 160 KiB, P = 20480 and the population on top, each case against
the NumPy f64 host reference (tests/homer_train_host.py) and never against the device's own output:

  * the matrix and the named edges of tests/homer_cases.py, one offsim_homer_grad pass each: n, the loss and the flat gradient in max norm
    within 4 x the error of torch's own f32 autograd on the CPU (floor: 4 ulps of the max norm), and every one of the eight tensors within
    1e-3 in relative 2-norm;
  * the forward-only instances (grad == NULL soft, and hard) over f32 and f16 observations at TM 4, 16 and 32;
  * two calls of a case give the same bits;
  * one offsim_homer_step in closed form from the device's own gradient at P = 20480, at TM = 4 and on the 16-parameter net;
  * a population of three learners, the middle one inactive, bit for bit against the single encoder at TM 4, 16 and 32.

A case goes through HOMEREncoder where it can express it, and through the C API (ctypes) where it cannot: a slope other than 0.01, or the
soft forward-only call.  tests/test_homer_matrix_host.py checks, without a device, that each case's bound tells a subtly wrong gradient from
a right one.  OFFSIM_HOMER_ERROR_JSONL=<file>: test_grad_case appends one JSON line per case (tools/homer_error_table.py prints them)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import homer_cases as K  # noqa: E402
import homer_train_host as HH  # noqa: E402
import test_gpu_homer_population as PT  # noqa: E402
import test_gpu_homer_train as T  # noqa: E402

pytestmark = pytest.mark.gpu
ULP = K.ULP


@pytest.fixture(scope="module")
def gpu():
    from rl_offline_simulation_amd import _lib
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    _lib.load()
    return torch.device("cuda", 0)


def _capi_grad(gpu, b, i, j, noise, hard, want_grad):
    """offsim_homer_grad through ctypes, the case's slope in the net: (n, loss, flat gradient or None) on the host"""
    from rl_offline_simulation_amd import _lib as L
    c = b.case
    on = lambda a: torch.from_numpy(np.array(a)).to(gpu)  # noqa: E731  (a copy: the case's arrays are read-only)
    params = [on(t) for t in b.model]
    x, a, xn, di, dj = on(b.obs), on(b.act), on(b.nxt), on(i), on(j)
    dg = None if noise is None else on(noise)
    P, M = K.homer_plan(c.dims, len(i)).P, len(i)
    net = L.HomerNet(*[L.ptr(t) for t in params], *c.dims, float(c.slope), 0)
    bt = L.HomerBatch(L.ptr(x), L.ptr(xn), L.F16 if c.xdt == "f16" else L.F32, 0, L.ptr(a), x.shape[0], L.ptr(di), L.ptr(dj), L.ptr(dg), M)
    stats = torch.zeros(2, dtype=torch.float64, device=gpu)
    grad = torch.zeros(P, dtype=torch.float32, device=gpu) if want_grad else None
    work = torch.empty(L.homer_work_doubles(P), dtype=torch.float64, device=gpu)
    L.check(L.load().offsim_homer_grad(net, bt, float(c.tau), int(hard), L.ptr(grad), L.ptr(stats), L.ptr(work), L.stream_ptr()))
    s = stats.cpu().numpy()
    return int(s[0]), float(s[1]), None if grad is None else grad.cpu().numpy()


def _copies(*arrays):
    """writable copies of a case's read-only arrays (torch.from_numpy wants them writable)"""
    return [None if a is None else np.array(a) for a in arrays]


def _run(gpu, b, i=None, j=None, noise=None, hard=False, want_grad=True):
    """one pass of a case (or of other records over its model and dataset): (n, loss, gradient or None)"""
    c = b.case
    if i is None:
        i, j, noise = b.i, b.j, b.noise
    if c.slope != HH.SLOPE or (not hard and not want_grad):
        return _capi_grad(gpu, b, i, j, noise, hard, want_grad and not hard)
    enc = T.encoder(_copies(*b.model), c.dims)
    loss, grad = enc.loss_grad(*_copies(b.obs, b.act, b.nxt, i, j, noise), c.tau, hard)
    return int(enc.last_n), float(loss), None if grad is None else grad.cpu().numpy()


# ---- 1. every case ----
@pytest.mark.parametrize("name", [c.name for c in K.MATRIX + K.EDGES])
def test_grad_case(gpu, name):
    b = K.build(name)
    c, p = b.case, b.plan
    n, loss, g = _run(gpu, b)
    assert g.shape == (p.P,) == b.g64.shape and np.isfinite(g).all()
    err, e_l = K.max_error(g, b), abs(loss - b.l64)
    per = K.tensor_errors(g, b)
    print(f"{c.group} {name}: P {p.P} TM {p.TM} lds {p.lds} wg {p.workgroups} n {n} err {err:.3e} bound {b.bound:.3e} ratio {err / b.bound:.3f} "
          f"loss err {e_l:.3e} bound {b.loss_bound:.3e} worst tensor {max(per):.2e}")
    out = os.environ.get("OFFSIM_HOMER_ERROR_JSONL")
    if out:
        with open(out, "a") as f:
            f.write(json.dumps({"case": name, "group": c.group, "dims": list(c.dims), "x_dtype": c.xdt, "slope": c.slope, "tau": c.tau, "M": c.M, "P": p.P,
                                "TM": p.TM, "TM_lds": p.tm_lds, "lds_bytes": p.lds, "workgroups": p.workgroups, "n": n, "err": err, "bound": b.bound,
                                "ratio": err / b.bound, "loss_err": e_l, "loss_bound": b.loss_bound, "worst_tensor_rel": max(per),
                                "worst_tensor": K.TENSORS[int(np.argmax(per))]}) + "\n")
    assert n == b.n
    assert e_l <= b.loss_bound, (e_l, b.loss_bound)
    assert err <= b.bound, (err, b.bound, [float(np.abs(g[s] - b.g64[s]).max()) for s in b.slices])  # per tensor: where an excess sits
    assert max(per) <= K.REL_TENSOR, dict(zip(K.TENSORS, per))


# ---- 2. the forward-only instances ----
FWD = [(tm, xdt, (f32, f16)[xdt == "f16"]) for tm, f32, f16 in K.FORWARD_CASES for xdt in ("f32", "f16")]
FWD_IDS = [f"TM{tm}-{xdt}" for tm, xdt, _ in FWD]


@pytest.mark.parametrize("tm,xdt,name", FWD, ids=FWD_IDS)
def test_soft_forward_only(gpu, tm, xdt, name):
    """grad == NULL, hard == 0: k_homer_grad<XT, false> on the soft z"""
    b = K.build(name)
    assert b.plan.TM == tm and b.case.xdt == xdt
    n, loss, g = _run(gpu, b, want_grad=False)
    e = abs(loss - b.l64)
    print(f"soft forward {name}: loss err {e:.3e} bound {b.loss_bound:.3e}")
    assert g is None and n == b.n and e <= b.loss_bound


@pytest.mark.parametrize("tm,xdt,name", FWD, ids=FWD_IDS)
def test_hard_forward(gpu, tm, xdt, name):
    """hard == 1 on the records whose argmax an ulp cannot flip (tests/test_homer_matrix_host.py)"""
    h = K.build_hard(name)
    b = h.base
    assert K.homer_plan(b.case.dims, len(h.i)).TM == tm
    n, loss, g = _run(gpu, b, h.i, h.j, h.noise, hard=True)
    e = abs(loss - h.l64)
    print(f"hard forward {name}: dropped {h.dropped} loss err {e:.3e} bound {h.loss_bound:.3e}")
    assert g is None and n == h.n and e <= h.loss_bound


# ---- 3. the same bits twice ----
@pytest.mark.parametrize("name", ["TM4-H256-M21", "TM4-nZ256-M21", "TM32-tiles-per-workgroup", "TM8-tiles-per-workgroup"])
def test_two_calls_give_the_same_bits(gpu, name):
    b = K.build(name)
    n1, l1, g1 = _run(gpu, b)
    n2, l2, g2 = _run(gpu, b)
    assert n1 == n2 and np.float64(l1).tobytes() == np.float64(l2).tobytes() and g1.tobytes() == g2.tobytes() and np.any(g1)


# ---- 4. the step at the new edges ----
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("clip", ["active", "inactive"])
@pytest.mark.parametrize("name", ["P-20480-M9", "TM4-H256-M5", "smallest-M33"])
def test_one_step_in_closed_form_from_the_device_gradient(gpu, name, clip, wd):
    """one offsim_homer_step from a zero Adam state, as tests/test_gpu_homer_train.py checks it on 4/2/10/16: m and v within 2 ulps, the
    weights within 1 ulp + 1e-6 lr, stats[2] against the norm of the device's own gradient to 1e-12"""
    b = K.build(name)
    c = b.case
    assert c.slope == HH.SLOPE and c.xdt == "f32"
    host_norm = float(np.sqrt((b.g64 ** 2).sum()))
    max_norm = 0.5 * host_norm if clip == "active" else 40.0
    assert (host_norm > max_norm) == (clip == "active")
    enc = T.encoder(_copies(*b.model), c.dims)
    obs, act, nxt, i, j, noise = _copies(b.obs, b.act, b.nxt, b.i, b.j, b.noise)
    loss, grad = enc.loss_grad(obs, act, nxt, i, j, noise, c.tau)
    gd = grad.cpu().numpy().astype(np.float64)
    lr = 1e-3
    enc.lr, enc.weight_decay, enc.max_grad_norm = lr, wd, max_norm
    enc.reset_optimizer()
    p0 = T.flat_dev(enc)
    stats = T._one_step(enc, enc.upload((obs, act, nxt)), i, j, noise, c.tau)
    total, coef = HH.clip_coef(gd, max_norm)
    assert stats[0] == b.n and stats[1] == float(loss) and abs(stats[2] - total) <= 1e-12 * total
    assert abs(stats[2] - host_norm) <= np.sqrt(gd.size) * b.bound
    assert (coef < 1.0) == (clip == "active")
    gg = gd * coef + wd * p0
    m = (0.1 * gg).astype(np.float32).astype(np.float64)
    v = (0.001 * gg * gg).astype(np.float32).astype(np.float64)
    want = p0 - (lr / (1 - 0.9)) * m / (np.sqrt(v) / np.sqrt(1 - 0.999) + 1e-8)
    dm, dv, dt = enc.adam_state()
    assert int(dt) == 1
    tiny = 2.0 ** -126
    assert np.all(np.abs(dm.cpu().numpy() - m) <= 2 * ULP * np.abs(m) + tiny) and np.all(np.abs(dv.cpu().numpy() - v) <= 2 * ULP * np.abs(v) + tiny)
    assert np.all(np.abs(T.flat_dev(enc) - want) <= ULP * np.abs(want) + 1e-6 * lr)
    assert not np.array_equal(T.flat_dev(enc), p0)


# ---- 5. the population at the new tile sizes ----
@pytest.mark.parametrize("name,tm", [("TM4-H256-M5", 4), ("TM16-by-M-M129", 16), ("LDS-160K-TM32-M300", 32)])
def test_population_equals_the_single_encoder(gpu, name, tm):
    """three learners, the middle one inactive, the records a column slice with idx_stride > M: loss, n, gradient and one step bit for bit
    the single encoder's per learner; the inactive learner's weights, m, v and t untouched"""
    c = K.CASES[name]
    p = K.homer_plan(c.dims, c.M)
    assert p.TM == tm and c.slope == HH.SLOPE
    models, obs, act, nxt, i, j, g, cols = PT.make_learners(c.dims, 3, c.M, 900 + tm, n_rows=c.n_rows, scale=0.3)
    assert i.shape[1] > c.M == cols.stop - cols.start
    pop, loss, grad = PT.check_pass(gpu, c.dims, models, obs, act, nxt, i, j, g, cols, tau=0.7)
    assert pop.last_n.tolist() == [float(c.M)] * 3 and bool(torch.isfinite(grad).all()) and len({float(x) for x in loss}) == 3
    pop = PT.population(models, c.dims)
    pop.weight_decay, pop.lr = 0.01, [1e-3, 2e-3, 3e-3]
    pop.reset_optimizer()
    data = pop.upload((obs, act, nxt))
    encs = [T.encoder(m, c.dims) for m in models]
    for l, enc in enumerate(encs):
        enc.weight_decay, enc.lr = 0.01, pop.lr[l]
        enc.reset_optimizer()
    quiet = PT._snapshot(pop, 1)
    stats = PT._step_both(pop, encs, data, i, j, g, cols, gpu, tau=0.7, active=[1, 0, 1], stepped=(0, 2))
    assert stats[1].tolist() == [0.0, 0.0, 0.0] and stats[0, 0] == c.M and stats[2, 0] == c.M
    assert all(PT.same(a, b) for a, b in zip(quiet, PT._snapshot(pop, 1)))
    assert pop.adam_state()[2].tolist() == [1, 0, 1]
    assert PT._state_equal(pop, 0, encs[0]) and PT._state_equal(pop, 2, encs[2]) and PT._state_equal(pop, 1, encs[1])
    assert not PT.same(pop._params()[0][0], torch.from_numpy(models[0][0]).to(gpu))  # learner 0 moved
