"""The encoder population on the device: offsim_encode_mlp_pop against L calls of offsim_encode_mlp bit for bit on every dispatch path (and
once more in a child process under OFFSIM_ENCODER_F32=1, where the S cases run k_encode_mlp_mfma_reg), one learner of a population pinned
directly on the f64 forward, a NaN learner that leaves its neighbours alone, HOMERPopulation.encode / latent_report / evaluators against
the per-learner route, and offsim_latent_counts against NumPy.  Cases, grid rule and tolerance: tests/encoder_pop_host.py,
tests/encoder_host.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_host as E  # noqa: E402
import encoder_pop_host as P  # noqa: E402
from test_gpu_encoder_matrix import GUARD, L_SENTINEL, Z_SENTINEL, _bits, _run, _upload_x, _weights  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    from rl_offline_simulation_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def _run_pop(dev, xd, w, nZ, n, want_logits=True):
    """one population call through the C ABI into sentinel-framed buffers -> (rc, z [n, N], logits [n, N, nZ] or None)"""
    from rl_offline_simulation_amd import _lib as L
    W1, b1, W2, b2 = w
    assert W1.shape[0] == n and b1.shape[0] == n and W2.shape[0] == n and b2.shape[0] == n
    N, dO, H = xd.shape[0], xd.shape[1], W1.shape[1]
    zbuf = torch.full((n * N + 2 * GUARD,), Z_SENTINEL, dtype=torch.int32, device=dev)
    lbuf = torch.full((n * N + 2 * GUARD, nZ), float(L_SENTINEL), dtype=torch.float32, device=dev) if want_logits else None
    rc = L.load().offsim_encode_mlp_pop(xd.data_ptr(), L.F16 if xd.dtype == torch.float16 else L.F32, N, dO, W1.data_ptr(), b1.data_ptr(), H,
                                        W2.data_ptr(), b2.data_ptr(), nZ, n, zbuf[GUARD:].data_ptr(),
                                        lbuf[GUARD:].data_ptr() if want_logits else None, L.stream_ptr())
    torch.cuda.synchronize()
    z = zbuf.cpu().numpy()
    assert (z[:GUARD] == Z_SENTINEL).all() and (z[GUARD + n * N:] == Z_SENTINEL).all(), "out_z written outside its L N rows"
    lg = None
    if want_logits:
        lg = lbuf.cpu().numpy()
        sent = L_SENTINEL.view(np.uint32)
        assert (lg[:GUARD].view(np.uint32) == sent).all() and (lg[GUARD + n * N:].view(np.uint32) == sent).all(), "out_logits written outside its L N rows"
        lg = lg[GUARD:GUARD + n * N].reshape(n, N, nZ)
    return rc, z[GUARD:GUARD + n * N].reshape(n, N), lg


def _against_single_calls(dev, p):
    """the population call of case p against one offsim_encode_mlp per learner on the same device x: z and logits bit for bit"""
    c = p.case
    path, inst, _ = E.taken_path(c)
    xd = _upload_x(p.x, dev, c.unaligned)
    assert (xd.data_ptr() % 16 != 0) == c.unaligned
    w = _weights(dev, p.W1, p.b1, p.W2, p.b2)
    rc, z, lg = _run_pop(dev, xd, w, c.nZ, p.L)
    assert rc == 0
    assert not (lg.view(np.uint32) == L_SENTINEL.view(np.uint32)).any() and ((z >= 0) & (z < c.nZ)).all()  # every row of every learner written
    rc, z_only, _ = _run_pop(dev, xd, w, c.nZ, p.L, want_logits=False)
    assert rc == 0 and np.array_equal(z_only, z)
    for l in range(p.L):
        rc, z1, lg1 = _run(dev, xd, tuple(t[l] for t in w), c.nZ)
        assert rc == 0
        assert np.array_equal(z[l], z1), (path, inst, l)
        assert np.array_equal(_bits(lg[l]), _bits(lg1)), (path, inst, l)
    print(f"path {path} inst {inst} {c.name} L {p.L}: grid {P.pop_grid(path, inst, c.N, p.L)}")
    return z, lg


S_SHAPES = [f"S-{xdt}-d{dO}-H64-z{nZ}-N{N}" for xdt, dO, nZ in (("f32", 128, 50), ("f32", 2, 25), ("f16", 128, 64), ("f16", 2, 32))
            for N in (1, 33, 65, 129)]
OTHERS = ["G-f32-d3-H16-z10-N129", "G-f16-d1-H32-z32-N97", "G-f32-d128-H128-z64-N129-biglds", "V-f32-d4-H96-z5-N300", "V-f16-d4-H96-z5-N300",
          "G-f32-d2-H64-z25-N129-unaligned", "G-f16-d4-H64-z50-N65-unaligned"]
STRIDES = ["S-f32-d128-H64-z50-N65575-stride", "S-f16-d2-H64-z25-N262183-stride", "G-f32-d3-H32-z10-N262183-stride", "V-f32-d4-H96-z5-N1048615-stride"]


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("name", S_SHAPES + OTHERS)
def test_bit_equal_to_single_calls(gpu, name, n):
    _against_single_calls(gpu, P.population(name, n))


@pytest.mark.parametrize("name", STRIDES)
def test_bit_equal_round_the_grid_stride_loop(gpu, name):
    """N from the population's own grid rule: two sweeps of a learner's workgroups + 39 rows, two learners"""
    c = E.CASES[name]
    path, inst, _ = E.taken_path(c)
    N = P.stride_N(path, inst, 2)
    assert N > 2 * P.pop_sweep_rows(path, inst, N, 2) and P.pop_grid(path, inst, N, 2)[0] == P.single_grid(path, inst, N)
    _against_single_calls(gpu, P.population(name, 2, N))


@pytest.mark.parametrize("name", ["S-f32-d128-H64-z50-N129", "S-f16-d2-H64-z32-N129", "G-f32-d8-H64-z25-N129", "G-f16-d8-H64-z64-N129"])
def test_learner_one_against_f64(gpu, name):
    """a direct pin, not only a relative one: learner 1 of three within encoder_host's tolerance of the f64 forward of ITS weights"""
    p, b = P.population(name, 3), P.build_learner(name, 3, 1)
    path = E.taken_path(p.case)[0]
    tol = E.tolerance(b, path)
    rc, z, lg = _run_pop(gpu, _upload_x(p.x, gpu), _weights(gpu, p.W1, p.b1, p.W2, p.b2), p.case.nZ, 3)
    assert rc == 0
    ratio = float((np.abs(lg[1].astype(np.float64) - b.ref) / b.B).max())
    clear = E.clear_rows(b, tol)
    print(f"path {path} {name} learner 1 of 3: rho_ref {b.rho_ref:.3e} measured {ratio:.3e} tol {tol:.3e} used {ratio / tol:.3f} clear {clear.mean():.4f}")
    assert (np.abs(lg[1].astype(np.float64) - b.ref) <= tol * b.B).all(), (path, ratio, tol)
    assert np.array_equal(z[1], E.first_argmax(lg[1]))
    assert clear.mean() >= 0.9 and np.array_equal(z[1][clear], E.first_argmax(b.ref)[clear])
    for other in (0, 2):  # and it is not a neighbour's forward
        assert not (np.abs(lg[other].astype(np.float64) - b.ref) <= tol * b.B).all()


@pytest.mark.parametrize("name", ["S-f32-d2-H64-z25-N129", "S-f16-d128-H64-z64-N129", "G-f32-d3-H16-z10-N129", "V-f32-d4-H96-z5-N300"])
def test_nan_learner_encodes_zero_and_leaves_its_neighbours(gpu, name):
    p = P.population(name, 3)
    c = p.case
    xd = _upload_x(p.x, gpu)
    W2 = np.array(p.W2)
    W2[1] = np.nan
    w = _weights(gpu, p.W1, p.b1, W2, p.b2)
    rc, z, lg = _run_pop(gpu, xd, w, c.nZ, 3)
    assert rc == 0 and np.isnan(lg[1]).all() and not z[1].any()
    for l in (0, 2):
        rc, z1, lg1 = _run(gpu, xd, tuple(t[l] for t in w), c.nZ)
        assert rc == 0 and np.array_equal(z[l], z1) and np.array_equal(_bits(lg[l]), _bits(lg1))
        assert np.isfinite(lg[l]).all()


def test_refusals_launch_nothing(gpu):
    from rl_offline_simulation_amd import _lib as L
    p = P.population("G-f32-d3-H16-z10-N129", 2)
    xd, w = _upload_x(p.x, gpu), _weights(gpu, p.W1, p.b1, p.W2, p.b2)
    zbuf = torch.full((2 * 129,), Z_SENTINEL, dtype=torch.int32, device=gpu)
    for (n, H, N, want) in ((0, 16, 129, L.EINVAL), (65536, 16, 129, L.EINVAL), (2, 129, 129, L.EUNSUPPORTED), (2, 16, 0, L.OK)):
        rc = L.load().offsim_encode_mlp_pop(xd.data_ptr(), L.F32, N, 3, w[0].data_ptr(), w[1].data_ptr(), H, w[2].data_ptr(), w[3].data_ptr(), 10, n,
                                            zbuf.data_ptr(), None, L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == want and (zbuf.cpu().numpy() == Z_SENTINEL).all(), (n, H, N, rc)


def test_f32_products_child(gpu):
    """OFFSIM_ENCODER_F32 is read once per process: the bit-equality tests again in a fresh child with the switch on, where every S case runs
    k_encode_mlp_mfma_reg (encoder_host.taken_path asserts the path from the same switch)."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, OFFSIM_ENCODER_F32="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_gpu_encoder_population.py"), "-m", "gpu", "-x", "-q",
                        "-k", "bit_equal or learner_one or nan_learner"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


# ---- HOMERPopulation ----
DIMS = (2, 5, 25, 64)  # obs_dim, action_dim, latent_size, hidden_size: the continuous grid's


def _grid(n_episodes=20, seed=6):
    from rl_offline_simulation_amd import synth
    return synth.grid_coords_log(n_episodes, seed=seed)


def _cell_and_seeded():
    """two learners: the grid-cell encoder of synth and a seed-initialised one"""
    from rl_offline_simulation_amd import synth
    from rl_offline_simulation_amd.encoders import HOMEREncoder
    from rl_offline_simulation_amd.encoders.homer import ENC_KEYS
    torch.manual_seed(1)
    seeded = HOMEREncoder(*DIMS).state_dict()
    return [dict(zip(ENC_KEYS, synth.grid_cell_encoder_weights(5, 64, seed=7))), seeded]


@pytest.mark.parametrize("xdt", [np.float32, np.float16, np.float64])
def test_encode_equals_each_learners_encode(gpu, xdt):
    from rl_offline_simulation_amd.encoders import HOMERPopulation
    pop = HOMERPopulation(*DIMS, seeds=[3, 4, 5])
    obs = _grid()["observations"].astype(xdt)
    zs = pop.encode(obs)
    assert zs.dtype == np.int64 and zs.shape == (3, len(obs))
    assert pop.last_input_dtype == (torch.float16 if xdt == np.float16 else torch.float32)
    for l in range(3):
        enc = pop.encoder(l)
        assert np.array_equal(zs[l], enc.encode(obs)) and enc.last_input_dtype == pop.last_input_dtype
    assert len({zs[l].tobytes() for l in range(3)}) == 3  # the learners differ
    xd = torch.from_numpy(obs.astype(np.float32)).to(gpu)
    z, lg = pop.encode_device(xd, return_logits=True)
    assert z.dtype == torch.int32 and tuple(z.shape) == (3, len(obs)) and tuple(lg.shape) == (3, len(obs), 25) and z.device == xd.device
    for l in range(3):
        z1, lg1 = pop.encoder(l).encode_device(xd, return_logits=True)
        assert torch.equal(z[l], z1) and np.array_equal(_bits(lg[l].cpu().numpy()), _bits(lg1.cpu().numpy()))


def test_encode_best_after_train(gpu):
    from rl_offline_simulation_amd.encoders import HOMERPopulation
    e = _grid()
    x, a, xn = e["observations"], e["actions"], e["next_observations"]
    n = len(x) * 3 // 4
    pop = HOMERPopulation(*DIMS, seeds=[0, 1])
    xd = torch.from_numpy(x).to(gpu)
    assert np.array_equal(pop.encode(x, best=True), pop.encode(x))  # before train(): the current weights
    before = pop.encode_device(xd, return_logits=True)[1].clone()
    pop.train((x[:n], a[:n], xn[:n]), (x[n:], a[n:], xn[n:]), num_epochs=2, batch_size=64, lr=[1e-2, 3e-2], seed=5)
    cur, best = pop.encode(x), pop.encode(x, best=True)
    for l in range(2):
        assert np.array_equal(cur[l], pop.encoder(l).encode(x))
        assert np.array_equal(best[l], pop.encoder(l, best=True).encode(x))
    after = pop.encode_device(xd, return_logits=True)[1]
    assert all(not torch.equal(after[l], before[l]) for l in range(2))  # two epochs moved every learner's weights
    lb = pop.encode_device(xd, return_logits=True, best=True)[1]
    for l in range(2):
        assert torch.equal(lb[l], pop.encoder(l, best=True).encode_device(xd, return_logits=True)[1])


def test_latent_report_on_the_grid(gpu):
    from rl_offline_simulation_amd.encoders import HOMERPopulation
    e = _grid(40, seed=2)
    obs, cells = e["observations"], e["z"]
    N = len(obs)
    pop = HOMERPopulation(*DIMS, state_dicts=_cell_and_seeded())
    rep = pop.latent_report(obs, labels=cells, n_labels=25)
    for t in (rep.z, rep.counts, rep.used, rep.joint, rep.purity, rep.skipped):
        assert isinstance(t, torch.Tensor) and t.is_cuda
    assert tuple(rep.z.shape) == (2, N) and tuple(rep.counts.shape) == (2, 25) and tuple(rep.joint.shape) == (2, 25, 25)
    z = rep.z.cpu().numpy()
    assert np.array_equal(z, pop.encode(obs))
    for l in range(2):
        assert np.array_equal(rep.counts[l].cpu().numpy(), np.bincount(z[l], minlength=25))
        joint = np.zeros((25, 25), np.int64)
        np.add.at(joint, (z[l], cells), 1)
        assert np.array_equal(rep.joint[l].cpu().numpy(), joint)
        assert float(rep.purity[l]) == joint.max(1).sum() / N
    assert (rep.counts.sum(1) + rep.skipped).tolist() == [N, N] and rep.skipped.tolist() == [0, 0]
    assert rep.used.tolist() == [int((np.bincount(z[l], minlength=25) > 0).sum()) for l in range(2)]
    print(f"purity {rep.purity.tolist()} used {rep.used.tolist()} of 25, N {N}")
    assert float(rep.purity[0]) > float(rep.purity[1])
    # labels given on the host without n_labels: max + 1; labels outside n_labels are skipped for every learner
    assert torch.equal(pop.latent_report(obs, labels=cells).joint[:, :, :int(cells.max()) + 1], rep.joint[:, :, :int(cells.max()) + 1])
    few = pop.latent_report(obs, labels=cells, n_labels=10)
    assert few.skipped.tolist() == [int((cells >= 10).sum())] * 2 and (few.counts.sum(1) + few.skipped).tolist() == [N, N]
    plain = pop.latent_report(obs)
    assert plain.joint is None and plain.purity is None and torch.equal(plain.counts, rep.counts)


def _serve(ev, n_steps=50):
    ev.reset_sampler(0)
    obs = ev.reset()
    out = [None if obs is None else np.asarray(obs).tolist()]
    for _ in range(n_steps):
        if obs is None:
            break
        try:
            res = ev.step_dist(np.full(5, 0.2))
        except KeyError:
            out.append("keyerror")
            obs = ev.reset()
            continue
        if res[0] is None:
            out.append("exhausted")
            obs = ev.reset()
            continue
        a, obs, r, done, info = res
        out.append((int(a), np.asarray(obs).tolist(), float(r), bool(done)))
        if done:
            obs = ev.reset()
    return out


def test_evaluators_serve_what_the_per_learner_route_serves(gpu):
    from rl_offline_simulation_amd import OfflineDataset, ProbDistribution, spaces
    from rl_offline_simulation_amd.encoders import HOMERPopulation
    from rl_offline_simulation_amd.evaluators import PerStateRejectionSampling
    e = _grid(40, seed=2)
    keys = ("observations", "actions", "rewards", "next_observations", "terminals", "action_distributions", "steps")
    ds = OfflineDataset(spaces.Box(0, 1.2, (2,)), spaces.Discrete(5), ProbDistribution.Discrete, **{k: e[k] for k in keys})
    pop = HOMERPopulation(*DIMS, state_dicts=_cell_and_seeded() + [HOMERPopulation(*DIMS, seeds=[9]).state_dict(0)])
    evs = pop.evaluators(ds)
    assert len(evs) == 3 and all(type(ev) is PerStateRejectionSampling for ev in evs)
    served = []
    for l, ev in enumerate(evs):
        ref = PerStateRejectionSampling(ds, 25, encoder=pop.encoder(l))
        assert np.array_equal(ev._impl._z, ref._impl._z) and np.array_equal(ev._impl._zn, ref._impl._zn)
        got, want = _serve(ev), _serve(ref)
        assert got == want and len(got) > 10, l
        served.append(got)
    assert served[0] != served[1]  # another partition serves other rows
    only = pop.evaluators(ds, learners=[2])
    assert len(only) == 1 and _serve(only[0]) == served[2]
    with pytest.raises(IndexError):
        pop.evaluators(ds, learners=[3])


# ---- offsim_latent_counts ----
def _latent_case(N, nZ, nY, seed):
    g = np.random.default_rng(seed)
    z = g.integers(0, nZ, (3, N)).astype(np.int32)
    labels = None if nY is None else g.integers(0, nY, N).astype(np.int32)
    z[0, 0], z[2, N - 1] = nZ, -7  # outside the range, at the first and the last row
    if labels is not None:
        labels[N - 1] = nY
        if N > 2:
            labels[0], labels[1] = -1, nY - 1
    return z, labels


def _latent_reference(z, labels, nZ, nY):
    n = z.shape[0]
    counts, skipped = np.zeros((n, nZ), np.int64), np.zeros(n, np.int64)
    joint = None if labels is None else np.zeros((n, nZ, nY), np.int64)
    for l in range(n):
        ok = (z[l] >= 0) & (z[l] < nZ)
        if labels is not None:
            ok &= (labels >= 0) & (labels < nY)
            np.add.at(joint[l], (z[l][ok], labels[ok]), 1)
        counts[l] = np.bincount(z[l][ok], minlength=nZ)
        skipped[l] = (~ok).sum()
    return counts, joint, skipped


def _latent_call(dev, z, labels, nZ, nY, with_joint=True):
    from rl_offline_simulation_amd import _lib as L
    n, N = z.shape
    zd = torch.from_numpy(z).to(dev)
    ld = None if labels is None else torch.from_numpy(labels).to(dev)
    fill = -0x0123456789  # the call zeroes its outputs itself
    counts = torch.full((n + 2, nZ), fill, dtype=torch.int64, device=dev)
    skipped = torch.full((n + 2,), fill, dtype=torch.int64, device=dev)
    joint = torch.full((n + 2, nZ, nY), fill, dtype=torch.int64, device=dev) if (labels is not None and with_joint) else None
    rc = L.load().offsim_latent_counts(zd.data_ptr(), n, N, nZ, None if ld is None else ld.data_ptr(), nY or 0, counts[1:].data_ptr(),
                                       None if joint is None else joint[1:].data_ptr(), skipped[1:].data_ptr(), L.stream_ptr())
    torch.cuda.synchronize()
    for t in (counts, skipped) + (() if joint is None else (joint,)):
        assert (t[0] == fill).all() and (t[-1] == fill).all(), "written outside the L learners"
    return rc, counts[1:-1].cpu().numpy(), None if joint is None else joint[1:-1].cpu().numpy(), skipped[1:-1].cpu().numpy()


@pytest.mark.parametrize("nY", [None, 1, 25])
@pytest.mark.parametrize("nZ", [1, 25, 64])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 4097])
def test_latent_counts_against_numpy(gpu, N, nZ, nY):
    z, labels = _latent_case(N, nZ, nY, seed=N * 100 + nZ)
    assert P.latent_grid(N, 3)[0] == (2 if N == 4097 else 1)
    want = _latent_reference(z, labels, nZ, nY)
    rc, counts, joint, skipped = _latent_call(gpu, z, labels, nZ, nY)
    assert rc == 0
    assert np.array_equal(counts, want[0]) and np.array_equal(skipped, want[2])
    assert (joint is None) == (want[1] is None) and (joint is None or np.array_equal(joint, want[1]))
    assert ((counts.sum(1) + skipped) == N).all() and skipped[0] >= 1 and skipped[2] >= 1 and (labels is None or skipped[1] >= 1)
    rc, counts2, joint2, skipped2 = _latent_call(gpu, z, labels, nZ, nY)  # the same on a second call
    assert rc == 0 and np.array_equal(counts2, counts) and np.array_equal(skipped2, skipped) and (joint is None or np.array_equal(joint2, joint))
    if labels is not None:  # labels without out_joint: the same rows count
        rc, counts3, joint3, skipped3 = _latent_call(gpu, z, labels, nZ, nY, with_joint=False)
        assert rc == 0 and joint3 is None and np.array_equal(counts3, counts) and np.array_equal(skipped3, skipped)


def test_latent_counts_lds_limit(gpu):
    from rl_offline_simulation_amd import _lib as L
    g = np.random.default_rng(5)
    z, labels = g.integers(0, 128, (3, 300)).astype(np.int32), g.integers(0, 64, 300).astype(np.int32)
    assert P.latent_lds_bytes(128, 64) == P.LATENT_LDS_LIMIT  # exactly 64 KiB runs
    rc, counts, joint, skipped = _latent_call(gpu, z, labels, 128, 64)
    want = _latent_reference(z, labels, 128, 64)
    assert rc == 0 and np.array_equal(counts, want[0]) and np.array_equal(joint, want[1]) and not skipped.any()
    assert P.latent_lds_bytes(128, 65) > P.LATENT_LDS_LIMIT  # just over is refused, outputs untouched
    zd, ld = torch.from_numpy(z).to(gpu), torch.from_numpy(labels).to(gpu)
    out = [torch.full(s, -5, dtype=torch.int64, device=gpu) for s in ((3, 128), (3, 128, 65), (3,))]
    rc = L.load().offsim_latent_counts(zd.data_ptr(), 3, 300, 128, ld.data_ptr(), 65, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == L.EUNSUPPORTED and all((t == -5).all() for t in out)
