"""k_policy_mlp (csrc/policy_mlp.hpp, launched by mlp_forward in csrc/offsim_hip.hip) over its six instances -- f32 / f16 observations x
policy / value / population --, each case of tests/policy_mlp_host.py against the NumPy f64 forward through the C ABI, into output buffers
the test owns, framed by 64 sentinel rows on either side:

  * every output within the case's own propagated bound elementwise (tests/policy_mlp_host.py derives it), the integer cases with ==, NaN in
    exactly the rows whose index lies outside x, policy rows summing to 1 within (nA + 2) u, nA = 1 giving exactly 1.0f;
  * the same bits on a second call, with rows = arange(M) as without rows, for every learner of a population as from the single call on its
    weights, and from MLPPolicy.forward / MLPValue.forward / PolicyPopulation.forward as from the C ABI.

tests/test_policy_mlp_matrix_host.py checks, without a device, that the bound tells a wrong kernel from a right one."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_mlp_host as P  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64  # sentinel rows before and after the output
SENTINEL = np.float32(-7.25e30)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    from rl_offline_simulation_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _upload(b, dev, learners=None):
    """x, rows and the weights of the given learners (stacked [L, ...]) on the device, with the offsim_mlp_layer array of the first of them"""
    from rl_offline_simulation_amd import _lib as L
    learners = list(range(len(b.weights))) if learners is None else learners
    keep = [torch.from_numpy(np.array(b.x)).to(dev), None if b.rows is None else torch.from_numpy(np.array(b.rows)).to(dev)]
    n = len(b.weights[0])
    arr = (L.MLPLayer * n)()
    for l in range(n):
        W = torch.from_numpy(np.stack([b.weights[i][l][0] for i in learners])).to(dev).contiguous()
        bias = None if b.weights[0][l][1] is None else torch.from_numpy(np.stack([b.weights[i][l][1] for i in learners])).to(dev).contiguous()
        keep += [W, bias]
        arr[l].W, arr[l].b, arr[l].out = L.ptr(W), L.ptr(bias), int(W.shape[1])
        setattr(arr[l], "in", int(W.shape[2]))
    return keep, arr


def _call(b, dev, form, learners=None, rows="case"):
    """One launch through the C ABI into a sentinel-framed buffer -> the output as NumPy ([M], [M, nA] or [L, M, nA]); form: "policy",
    "value" or "pop".  The frame is asserted, the stream synchronised and the async fault word checked."""
    from rl_offline_simulation_amd import _lib as L
    c = b.case
    keep, arr = _upload(b, dev, learners)
    xd, rd = keep[0], keep[1]
    if rows == "arange":
        rd = torch.arange(c.M, dtype=torch.int32, device=dev)
    elif rows == "none":
        rd = None
    n_l = len(learners) if learners is not None else len(b.weights)
    width = 1 if form == "value" else c.sizes[-1] * (n_l if form == "pop" else 1)
    # the frame is 64 rows of the widest row this case writes, on either side of [L * M * nA] floats
    row = c.sizes[-1]
    buf = torch.full((2 * GUARD * row + c.M * width,), float(SENTINEL), dtype=torch.float32, device=dev)
    out = buf[GUARD * row:]
    args = (L.ptr(xd), L.F16 if c.xdt == "f16" else L.F32, c.n_x, c.sizes[0], L.ptr(rd), c.M, arr, len(arr), P.ACT[c.act], ctypes.c_float(c.slope))
    lib = L.load()
    if form == "pop":
        rc = lib.offsim_policy_mlp_pop(*args, n_l, out.data_ptr(), L.stream_ptr())
    else:
        rc = (lib.offsim_value_mlp if form == "value" else lib.offsim_policy_mlp)(*args, out.data_ptr(), L.stream_ptr())
    torch.cuda.synchronize()
    L.check_async_faults()
    assert rc == L.OK, lib.offsim_last_error()
    h = buf.cpu().numpy()
    sent = SENTINEL.view(np.uint32)
    assert (_bits(h[:GUARD * row]) == sent).all() and (_bits(h[GUARD * row + c.M * width:]) == sent).all(), "written outside the output"
    got = h[GUARD * row:GUARD * row + c.M * width]
    if form == "value":
        return got.copy()
    return got.reshape((n_l, c.M, c.sizes[-1]) if form == "pop" else (c.M, c.sizes[-1])).copy()


def _check(got, b, l, name):
    """got against learner l's f64 reference: NaN exactly on the rows outside x, everything else within the bound; prints the share used"""
    c = b.case
    bad = ~b.valid
    assert np.isnan(got[bad]).all(), f"{name}: a row with an index outside x is not all NaN"
    assert np.isfinite(got[b.valid]).all(), name
    r = P.ratio(got, b.ref[l], b.bound[l], b.valid)
    print(f"{name} learner {l} {c.inst} chunks {b.shape.chunks} lds {b.shape.lds_bytes}: {r:.4f} of the bound")
    assert (np.abs(got[b.valid].astype(np.float64) - b.ref[l][b.valid]) <= b.bound[l][b.valid]).all(), (name, l, r)
    if not c.value:
        rows = got[b.valid].astype(np.float64).sum(axis=1)
        # every p_a is rounded once (the division) off e_a / s, and s is off sum(e) by at most (nA - 1) u relative: (nA + 2) u covers both
        assert (np.abs(rows - 1.0) <= (c.sizes[-1] + 2) * P.U).all(), (name, float(np.abs(rows - 1.0).max()))
        if c.sizes[-1] == 1:
            assert (got[b.valid] == np.float32(1.0)).all()
    return r


@pytest.mark.parametrize("name", [c.name for c in P.CASE_LIST])
def test_case(gpu, name):
    b = P.build(name)
    c = b.case
    if c.L:
        got = _call(b, gpu, "pop")
        assert got.shape == (c.L, c.M, c.sizes[-1])
        for l in range(c.L):
            _check(got[l], b, l, name)
            single = _call(b, gpu, "policy", learners=[l])
            assert np.array_equal(_bits(single), _bits(got[l])), (name, l)  # the single call on that learner's weights, bit for bit
            if c.fam == "exact":  # nA = 1 reads back 1.0 from the policy; the integers through a value call per learner
                v = _call(b, gpu, "value", learners=[l])
                assert np.array_equal(v.astype(np.float64), b.logits[l][:, 0]), (name, l)
        again = _call(b, gpu, "pop")
    else:
        form = "value" if c.value else "policy"
        got = _call(b, gpu, form)
        _check(got, b, 0, name)
        if c.fam == "exact":
            assert np.array_equal(got.astype(np.float64), b.ref[0]), name
        again = _call(b, gpu, form)
    assert np.array_equal(_bits(again), _bits(got)), name
    if c.rows in ("none", "arange"):
        other = _call(b, gpu, "pop" if c.L else "value" if c.value else "policy", rows="arange" if c.rows == "none" else "none")
        assert np.array_equal(_bits(other), _bits(got)), name


def _net(b, l, cls):
    return cls([(torch.from_numpy(np.array(W)), None if bias is None else torch.from_numpy(np.array(bias))) for W, bias in b.weights[l]],
               b.case.act, b.case.slope)


@pytest.mark.parametrize("name", ["chunk-128x256-pol16", "chunk-128x256-val", "oob-policy-relu", "oob-value-tanh", "inst-f16-policy-M65",
                                  "inst-f16-value-M1", "nobias-mid-policy", "act-leaky15-val"])
def test_python_surface_returns_the_c_abi_bits(gpu, name):
    from rl_offline_simulation_amd import _lib as L
    from rl_offline_simulation_amd.evaluators import MLPPolicy, MLPValue
    b = P.build(name)
    c = b.case
    want = _call(b, gpu, "value" if c.value else "policy")
    net = _net(b, 0, MLPValue if c.value else MLPPolicy)
    x = torch.from_numpy(np.array(b.x)).to(gpu)
    rows = None if b.rows is None else torch.from_numpy(np.array(b.rows)).to(gpu)
    got = net.forward(x, rows)
    torch.cuda.synchronize()
    L.check_async_faults()
    assert got.shape == want.shape and np.array_equal(_bits(got.cpu().numpy()), _bits(want))


@pytest.mark.parametrize("name", ["pop-f32-bias", "pop-f16-nobias", "nobias-mid-pop", "oob-pop-f16", "inst-f32-pop-M1"])
def test_population_surface_returns_the_c_abi_bits(gpu, name):
    from rl_offline_simulation_amd import _lib as L
    from rl_offline_simulation_amd.evaluators import MLPPolicy, PolicyPopulation
    b = P.build(name)
    want = _call(b, gpu, "pop")
    pop = PolicyPopulation.from_policies([_net(b, l, MLPPolicy) for l in range(b.case.L)])
    x = torch.from_numpy(np.array(b.x)).to(gpu)
    rows = None if b.rows is None else torch.from_numpy(np.array(b.rows)).to(gpu)
    got = pop.forward(x, rows)
    part = pop.forward(x, rows, 1, 3)  # a tile of the population that starts past learner 0
    torch.cuda.synchronize()
    L.check_async_faults()
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)) and np.array_equal(_bits(part.cpu().numpy()), _bits(want[1:3]))
