"""PPOLearner.update / ppo_grad (offsim_ppo_update, offsim_ppo_grad) on the device: gradients, traces, StopIter and final weights against the
NumPy f64 restatement (tests/ppo_update_host.py) with bounds set by the reference's own f32 error on the same fixtures
(tests/golden/ppo_update/*.npz), the early stop, determinism, masked against compacted input, the gradient at scale against torch autograd
in f64, and the hand-over of the updated weights to forward / collect_ppo."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_update_host as U  # noqa: E402
from test_gpu_collect import _cartpole, _env  # noqa: E402
from test_ppo_update import host_run, hyper, nets  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ppo_update", "*.npz")))
IDS = [os.path.basename(p)[:-4] for p in FIXTURES]
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def gpu():
    from rl_offline_simulation_amd import _lib
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    _lib.load()
    return torch.device("cuda", 0)


def _pair(d):
    from rl_offline_simulation_amd.evaluators import MLPPolicy, MLPValue
    pi, v = nets(d)
    act = str(d["activation"])
    return MLPPolicy(pi, act), MLPValue(v, act)


def _data(d, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(d[k])).to(dev) for k in ("obs", "act", "adv", "logp", "ret")}


def _learner(d, actor, critic):
    from rl_offline_simulation_amd.evaluators import PPOLearner
    h = hyper(d)
    return PPOLearner(actor, critic, pi_lr=h["pi_lr"], vf_lr=h["vf_lr"], clip_ratio=h["clip_ratio"], train_pi_iters=int(h["train_pi_iters"]),
                      train_v_iters=int(h["train_v_iters"]), target_kl=h["target_kl"])


def _grad_bound(g64, g_ref32):
    """4 x the reference's own f32 error against the f64 gradient, floored at 4 f32 ulps of the gradient's max norm"""
    return max(4.0 * float(np.abs(np.asarray(g_ref32, np.float64) - g64).max()), 4.0 * ULP * float(np.abs(g64).max()))


def _flat_dev(net, dev):
    ws, _ = net._device_weights(dev)
    return torch.cat([x.reshape(-1) for W, b in ws for x in ((W,) if b is None else (W, b))]).cpu().numpy()


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_grad_matches_host_f64_within_the_reference_error(gpu, path):
    from rl_offline_simulation_amd.evaluators import ppo_grad
    d = np.load(path)
    h, act = hyper(d), str(d["activation"])
    actor, critic = _pair(d)
    data = _data(d, gpu)
    pi, v = nets(d)
    loss, kl, ent, cf, g64, n = U.loss_pi(pi, d["obs"], d["act"], d["adv"], d["logp"], h["clip_ratio"], act)
    got = ppo_grad(actor, data, "actor", h["clip_ratio"])
    err, bound = float(np.abs(got.grad.cpu().numpy().astype(np.float64) - g64).max()), _grad_bound(g64, d["g_pi"])
    print(f"actor grad err {err:.3e} bound {bound:.3e}")
    assert err <= bound
    assert int(got.n) == n
    for name, x, want, ref in (("loss", got.loss, loss, d["pi_old"][0]), ("kl", got.kl, kl, d["pi_old"][1]), ("ent", got.entropy, ent, d["ent_old"])):
        assert abs(float(x) - want) <= max(4.0 * abs(float(ref) - want), 4.0 * ULP * max(1.0, abs(want))), name
    assert abs(float(got.clipfrac) - cf) <= 2.0 / n  # (a ratio within an ulp of the clip edge may fall on the other side in f32)
    lv, gv64, _ = U.loss_v(v, d["obs"], d["ret"], act)
    gotv = ppo_grad(critic, data, "critic")
    errv, boundv = float(np.abs(gotv.grad.cpu().numpy().astype(np.float64) - gv64).max()), _grad_bound(gv64, d["g_v"])
    print(f"critic grad err {errv:.3e} bound {boundv:.3e}")
    assert errv <= boundv
    assert abs(float(gotv.loss) - lv) <= max(4.0 * abs(float(d["v_old"]) - lv), 4.0 * ULP * max(1.0, lv))


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_update_matches_host_f64_within_the_reference_error(gpu, path):
    d = np.load(path)
    h = hyper(d)
    a, c = host_run(d)
    # the reference's own f32 error, measured on the CPU (tests/test_ppo_update.py prints the same figures): never from the device's output
    d_pi = float(np.abs(U.flatten(a["net"]) - d["pi_after"]).max())
    d_v = float(np.abs(U.flatten(c["net"]) - d["v_after"]).max())
    actor, critic = _pair(d)
    lrn = _learner(d, actor, critic)
    info = lrn.update(_data(d, gpu))
    assert int(info.StopIter) == a["stop_iter"] == int(d["log_StopIter"])
    for name, got, host, ref in (("pi", lrn.pi_trace.cpu().numpy(), a["trace"], d["pi_trace"]), ("v", lrn.v_trace.cpu().numpy(), c["trace"], d["v_trace"])):
        k = len(host)
        assert np.isnan(got[k:]).all() and not np.isnan(got[:k]).any(), name
        for col in ((0, 1) if name == "pi" else (0,)):
            bound = max(4.0 * float(np.abs(ref[:, col] - host[:, col]).max()), 4.0 * ULP * max(1.0, float(np.abs(host[:, col]).max())))
            err = float(np.abs(got[:k, col] - host[:, col]).max())
            print(f"{name} trace col {col}: err {err:.3e} bound {bound:.3e}")
            assert err <= bound, (name, col)
    e_pi = float(np.abs(_flat_dev(actor, gpu).astype(np.float64) - U.flatten(a["net"])).max())
    e_v = float(np.abs(_flat_dev(critic, gpu).astype(np.float64) - U.flatten(c["net"])).max())
    print(f"final weights: actor err {e_pi:.3e} (4 d_ref {4 * d_pi:.3e})  critic err {e_v:.3e} (4 d_ref {4 * d_v:.3e})")
    assert e_pi <= 4.0 * d_pi and e_v <= 4.0 * d_v
    # the logged values
    assert abs(float(info.LossPi) - a["first"]["loss"]) <= 1e-5 and abs(float(info.LossV) - c["first"]["loss"]) <= 1e-5 * max(1.0, c["first"]["loss"])
    assert abs(float(info.KL) - a["last"]["kl"]) <= 1e-5 and abs(float(info.Entropy) - a["first"]["ent"]) <= 1e-5
    assert abs(float(info.ClipFrac) - a["last"]["cf"]) <= 2.0 / len(d["adv"])
    assert abs(float(info.DeltaLossPi) - (a["last"]["loss"] - a["first"]["loss"])) <= 1e-5
    assert abs(float(info.DeltaLossV) - (c["last"]["loss"] - c["first"]["loss"])) <= 1e-5 * max(1.0, c["first"]["loss"])
    (am, av, at), (cm, cv, ct) = lrn.adam_state()
    assert int(at) == a["opt"].t and int(ct) == c["opt"].t == int(h["train_v_iters"])


def test_early_stop_leaves_the_state_of_iteration_stopiter(gpu):
    """After the stop at pass s the remaining launches change nothing: weights, m, v and t are those of s Adam steps -- the same bits as a
    run of exactly s iterations that never tests the KL (a target_kl nothing reaches)."""
    from rl_offline_simulation_amd.evaluators import PPOLearner
    d = np.load(os.path.join(ROOT, "tests", "golden", "ppo_update", "ppo_update_stop_tanh.npz"))
    h = hyper(d)
    s = int(d["log_StopIter"])
    assert 0 < s < int(h["train_pi_iters"]) - 1
    data = _data(d, gpu)
    a1, c1 = _pair(d)
    l1 = _learner(d, a1, c1)
    info = l1.update(data)
    assert int(info.StopIter) == s
    a2, c2 = _pair(d)
    l2 = PPOLearner(a2, c2, pi_lr=h["pi_lr"], vf_lr=h["vf_lr"], clip_ratio=h["clip_ratio"], train_pi_iters=s, train_v_iters=int(h["train_v_iters"]),
                    target_kl=1e9)
    l2.update(data)
    assert np.array_equal(_flat_dev(a1, gpu), _flat_dev(a2, gpu)) and np.array_equal(_flat_dev(c1, gpu), _flat_dev(c2, gpu))
    for x, y in zip(l1.adam_state()[0], l2.adam_state()[0]):
        assert torch.equal(x, y)
    assert int(l1.adam_state()[0][2]) == s
    assert torch.equal(l1.pi_trace[:s], l2.pi_trace[:s]) and bool(torch.isnan(l1.pi_trace[s + 1:]).all())
    assert float(l1.pi_trace[s, 1]) > 1.5 * h["target_kl"]


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_two_identical_calls_give_identical_bits(gpu, path):
    from rl_offline_simulation_amd.evaluators import ppo_grad
    d = np.load(path)
    data = _data(d, gpu)
    outs = []
    for _ in range(2):
        actor, critic = _pair(d)
        g = ppo_grad(actor, data, "actor", hyper(d)["clip_ratio"])
        lrn = _learner(d, actor, critic)
        info = lrn.update(data)
        outs.append((g.grad.clone(), g.loss.clone(), _flat_dev(actor, gpu), _flat_dev(critic, gpu), lrn.pi_trace.clone(), lrn.v_trace.clone(),
                     torch.stack([x.double() for x in info])))
    for x, y in zip(*outs):
        x, y = (torch.as_tensor(t) for t in (x, y))
        assert torch.equal(torch.nan_to_num(x, nan=-7.0), torch.nan_to_num(y, nan=-7.0))


def test_masked_records_equal_the_compacted_batch(gpu):
    """[T, E] records with invalid entries (a small log: environments run dry) against flat(): same n, gradients within the bound."""
    from rl_offline_simulation_amd.evaluators import MLPPolicy, MLPValue, ppo_grad
    d = _cartpole(400, 4, np.float32)
    E, T = 24, 64
    env = _env(**d, E=E)
    env.reset_sampler(np.arange(E))
    env.reset()
    torch.manual_seed(3)
    mk = lambda o: torch.nn.Sequential(torch.nn.Linear(4, 16), torch.nn.Tanh(), torch.nn.Linear(16, o))  # noqa: E731
    actor, critic = MLPPolicy.from_torch(mk(2)), MLPValue.from_torch(mk(1))
    b = env.collect_ppo(actor, critic, T, max_episode_steps=20)
    n_valid = int(b.valid.sum())
    assert 0 < n_valid < T * E  # some environments ran dry
    # garbage in the invalid entries must not matter
    b = b._replace(obs=torch.where(b.valid[..., None], b.obs, torch.full_like(b.obs, float("nan"))),
                   adv=torch.where(b.valid, b.adv, torch.full_like(b.adv, float("inf"))))
    flat = b.flat()
    for net, kind in ((actor, "actor"), (critic, "critic")):
        gm, gf = ppo_grad(net, b, kind), ppo_grad(net, flat, kind)
        assert int(gm.n) == int(gf.n) == n_valid
        g64, _, _ = _torch_grad(net, kind, flat, 0.2, torch.float64, "cpu")
        g32, _, _ = _torch_grad(net, kind, flat, 0.2, torch.float32, "cpu")
        bound = _grad_bound(g64, g32)  # the gradient bound of the fixture tests, torch's f32 autograd on the CPU setting the scale
        for g in (gm, gf):
            err = float(np.abs(g.grad.cpu().numpy() - g64).max())
            print(f"{kind}: err {err:.3e} bound {bound:.3e}")
            assert err <= bound, kind
        assert abs(float(gm.loss) - float(gf.loss)) <= 4.0 * ULP * max(1.0, abs(float(gf.loss)))


def _torch_grad(net, kind, f, clip, dtype, device):
    """torch autograd on a copy of the network in `dtype` on `device`: (flat gradient, loss, kl)"""
    m = net.to_torch().to(dtype).to(device)
    t = {k: (v.to(device).to(dtype) if v.is_floating_point() else v.to(device)) for k, v in f.items()}
    if kind == "actor":
        logp = torch.distributions.Categorical(logits=m(t["obs"])).log_prob(t["act"].long())
        ratio = torch.exp(logp - t["logp"])
        loss = -(torch.min(ratio * t["adv"], torch.clamp(ratio, 1 - clip, 1 + clip) * t["adv"])).mean()
        kl = (t["logp"] - logp).mean()
    else:
        loss = ((m(t["obs"])[:, 0] - t["ret"]) ** 2).mean()
        kl = torch.zeros((), dtype=dtype)
    loss.backward()
    g = torch.cat([p.grad.reshape(-1) for x in m if isinstance(x, torch.nn.Linear) for p in (x.weight, x.bias) if p is not None])
    return g.double().cpu().numpy(), float(loss), float(kl)


def test_gradients_at_scale_and_the_weights_hand_over(gpu):
    """4096 x 256 from collect_ppo on synth.cartpole_log with the C2 pair: both gradients against torch autograd in f64; then update(), and
    forward / collect_ppo run the new weights (compared with a torch net loaded through to_torch)."""
    from rl_offline_simulation_amd.evaluators import MLPPolicy, MLPValue, PPOLearner, ppo_grad
    d = _cartpole(1_000_000, 4, np.float32)
    E, T = 4096, 256
    env = _env(**d, E=E)
    env.reset_sampler(np.arange(E))
    env.reset()
    torch.manual_seed(0)
    mk = lambda o: torch.nn.Sequential(torch.nn.Linear(4, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, o))  # noqa: E731
    actor, critic = MLPPolicy.from_torch(mk(2)), MLPValue.from_torch(mk(1))
    b = env.collect_ppo(actor, critic, T, max_episode_steps=500)
    flat = b.flat()
    assert int(b.valid.sum()) > T * E // 2
    for net, kind in ((actor, "actor"), (critic, "critic")):
        g = ppo_grad(net, b, kind)
        g64, loss, kl = _torch_grad(net, kind, flat, 0.2, torch.float64, gpu)
        g32, _, _ = _torch_grad(net, kind, flat, 0.2, torch.float32, gpu)
        err, scale, bound = float(np.abs(g.grad.cpu().numpy() - g64).max()), float(np.abs(g64).max()), _grad_bound(g64, g32)
        print(f"{kind}: n {int(g.n)} grad err {err:.3e} bound {bound:.3e} max norm {scale:.3e}; loss {float(g.loss):.6f} / {loss:.6f}")
        assert err <= bound, kind  # 4 x the error of torch's own f32 autograd on the same data (floor: 4 ulps of the max norm)
        assert abs(float(g.loss) - loss) <= 1e-5 * max(1.0, abs(loss)) and abs(float(g.kl) - kl) <= 1e-6
    lrn = PPOLearner(actor, critic, train_pi_iters=5, train_v_iters=5)
    before = actor.forward(flat["obs"][:1000]).clone()
    info = lrn.update(b)
    assert 0 <= int(info.StopIter) <= 4 and float(info.DeltaLossV) < 0.0
    after = actor.forward(flat["obs"][:1000])
    assert not torch.equal(before, after)
    pi_t, v_t = actor.to_torch().double(), critic.to_torch().double()
    x = flat["obs"][:1000].cpu().double()
    with torch.no_grad():
        assert float((torch.softmax(pi_t(x), -1) - after.cpu().double()).abs().max()) <= 1e-5
        assert float((v_t(x)[:, 0] - critic.forward(flat["obs"][:1000]).cpu().double()).abs().max()) <= 1e-5 * float(v_t(x).abs().max() + 1)
    b2 = env.collect_ppo(actor, critic, 8, max_episode_steps=500)  # no from_torch, no copy: the kernel reads the updated tensors
    o2 = b2.obs[b2.valid][:1000]
    with torch.no_grad():
        want = torch.softmax(pi_t(o2.cpu().double()), -1)
        assert float((b2.collected.probs[b2.valid][:1000].cpu().double() - want).abs().max()) <= 1e-5
        assert float((b2.val[b2.valid][:1000].cpu().double() - v_t(o2.cpu().double())[:, 0]).abs().max()) <= 1e-5 * float(v_t(o2.cpu().double()).abs().max() + 1)
