"""The cases of the k_ppo_grad / k_ppo_adam matrix (tests/test_gpu_ppo_update_matrix.py on the device, tests/test_ppo_update_matrix_host.py
for what needs none): networks, batches, the NumPy f64 reference of each (tests/ppo_update_host.py), torch's own f32 autograd on the CPU,
which sets every bound, and ppou_prepare's LDS arithmetic (csrc/ppo_update.hpp) restated.

A case is built once per process and then only read."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_update_host as U  # noqa: E402
from test_gpu_ppo_update import _grad_bound, _torch_grad  # noqa: E402

ULP = 2.0 ** -23
CLIP = 0.2
MAX_FLOATS, MAX_BLOCKS, THREADS = 16384, 256, 512  # OFFSIM_COLLECT_MLP_MAX_FLOATS, OFFSIM_PPO_MAX_BLOCKS, PPOU_THREADS
BIG_NET = (12, 256, 16, 256, 16)  # biases on every layer: 15904 floats, 133.7 KiB of LDS at TM = 16 (203.2 KiB at TM = 32)


# ---- ppou_prepare's layout arithmetic ----
def lds_plan(sizes, has_bias):
    """(TM, LDS bytes, P, lda, ldd) of a network as ppou_prepare lays it out; TM = 0 where it refuses (more than 160 KiB at TM = 4)."""
    ins, outs = sizes[:-1], sizes[1:]
    P = sum(i * o + (o if hb else 0) for i, o, hb in zip(ins, outs, has_bias))
    wf = sum(i * (o | 1) + (o if hb else 0) for i, o, hb in zip(ins, outs, has_bias))
    w_floats = (wf + 3) & ~3
    lda = (sizes[0] + sum(outs) + 1) | 1  # observations, every layer's outputs, the column of ones
    ldd = sum(outs) | 1
    TM = 32
    while True:
        lds = 4 * (w_floats + TM * lda + ((TM * ldd + 1) & ~1)) + 8 * 5 * TM
        if lds <= 160 * 1024 or TM == 4:
            break
        TM //= 2
    return (TM if lds <= 160 * 1024 else 0), lds, P, lda, ldd


def bias_flags(bias, depth, seed=0):
    if bias == "mixed":  # every other layer; which half depends on the seed, so that both the first and the last layer come without one
        return tuple((l + seed) % 2 == 0 for l in range(depth))
    return (bias == "all",) * depth


# ---- the case table ----
def _c(name, kind, sizes, act="tanh", slope=0.01, bias="all", xdt="f32", M=200, seed=0, **kw):
    sizes = tuple(sizes[:-1]) + ((1,) if kind == "critic" else (sizes[-1],))
    opts = dict(pattern="iid", mask=None, bad_act=False, logit_scale=1.0, lp_noise=0.15, zero_grad=False)
    opts.update(kw)
    return SimpleNamespace(name=name, kind=kind, sizes=sizes, act=act, slope=slope, bias=bias, xdt=xdt, M=M, seed=seed, **opts)


def _matrix():
    """A covering list: every activation, depth 1-4 and bias layout, each with both kinds and both observation types."""
    nets = [  # (activation, slope, sizes, bias)
        ("identity", 0.01, (5, 3), "all"),
        ("tanh", 0.01, (7, 12, 4), "none"),
        ("relu", 0.01, (6, 16, 10, 3), "mixed"),
        ("leaky_relu", 0.2, (9, 24, 8, 12, 5), "all"),
        ("identity", 0.01, (11, 8, 9, 3), "none"),
        ("leaky_relu", 0.0, (8, 16, 2), "mixed"),
        ("tanh", 0.01, (5, 10, 16, 8, 2), "mixed"),
        ("relu", 0.01, (13, 4), "none"),
        ("leaky_relu", 0.2, (7, 20, 3), "none"),
        ("leaky_relu", 0.0, (6, 12, 12, 4), "all"),
        ("relu", 0.01, (10, 16, 3), "all"),
        ("tanh", 0.01, (8, 9, 7, 3), "all"),
    ]
    out = []
    for i, (act, slope, sizes, bias) in enumerate(nets):
        for xdt in ("f32", "f16"):
            for kind in ("actor", "critic"):
                tag = act if act != "leaky_relu" else f"leaky{slope}"
                out.append(_c(f"{kind}-{xdt}-{tag}-d{len(sizes) - 1}-{bias}-{i}", kind, sizes, act, slope, bias, xdt, M=200 + i, seed=i))
    return out


def _edges():
    out = []
    for kind in ("actor", "critic"):
        k = kind
        out += [
            _c(f"{k}-hidden256", k, (6, 256, 3), M=300, seed=20),
            _c(f"{k}-dO128", k, (128, 16, 4), "relu", xdt="f16", M=200, seed=21),
            # P in (512 * 31, 16384]: all 32 parameter slots of a thread are taken
            _c(f"{k}-P-above-15872", k, (110, 128, 16) if k == "actor" else (124, 128, 1), "leaky_relu", 0.2, M=300, seed=22),
            # P = 16384 exactly: 128 * (112 + 16) and 128 * (127 + 1), no biases
            _c(f"{k}-P-16384", k, (112, 128, 16) if k == "actor" else (127, 128, 1), bias="none", M=300, seed=23),
            _c(f"{k}-P-below-512", k, (4, 8, 3), M=200, seed=24),  # 67 / 49 parameters: most threads own nothing
            # above 64 KiB of LDS, TM = 16: three full tiles and a partial one
            _c(f"{k}-lds-above-64k-TM16", k, BIG_NET, M=16 * 3 + 5, seed=25),
            # more tiles than workgroups: tiles b, b + 256, ... per workgroup, the last tile partial; a pattern, not noise, so that no
            # two tiles look alike
            _c(f"{k}-tiles-per-workgroup", k, (4, 8, 3), M=MAX_BLOCKS * 32 * 2 + 32 * 3 + 5, seed=26, pattern="det"),
            # valid = 0 on whole tiles, on the tail and on scattered records, NaN / inf in every column of those
            _c(f"{k}-masked-tiles-nan", k, (5, 12, 3), "relu", M=32 * 6 + 7, seed=27, mask="tiles"),
        ]
        for M in (1, 3, 31, 32, 33):
            out.append(_c(f"{k}-M{M}", k, (4, 8, 3), M=M, seed=30 + M, lp_noise=0.05 if M <= 3 else 0.15))  # (M <= 3: no record clipped away)
    out += [
        _c("actor-nA16", "actor", (6, 16, 16), M=300, seed=40),
        # one action: log-softmax is 0 and the gradient is identically 0; the device has to give exactly that
        _c("actor-nA1", "actor", (6, 16, 1), M=200, seed=41, zero_grad=True),
        _c("actor-logits-in-the-hundreds", "actor", (6, 16, 4), M=300, seed=42, logit_scale=150.0),
        _c("actor-act-out-of-range", "actor", (5, 12, 3), M=200, seed=43, bad_act=True),
    ]
    return out


MATRIX = _matrix()
EDGES = _edges()
CASES = {c.name: c for c in MATRIX + EDGES}
assert len(CASES) == len(MATRIX) + len(EDGES)


# ---- building a case ----
def make_net(sizes, flags, rng, logit_scale=1.0):
    net = []
    for l, (i, o) in enumerate(zip(sizes[:-1], sizes[1:])):
        W = rng.normal(size=(o, i)) / np.sqrt(i)
        b = rng.normal(size=o) * 0.3 if flags[l] else None
        if l == len(sizes) - 2:
            W = W * logit_scale
        net.append((W.astype(np.float32), None if b is None else b.astype(np.float32)))
    return net


def net64(net):
    return [(W.astype(np.float64), None if b is None else b.astype(np.float64)) for W, b in net]


def model(c, net=None):
    """the MLPPolicy / MLPValue of a case (host copy only until something asks for a device)"""
    from rl_offline_simulation_amd.evaluators import MLPPolicy, MLPValue
    return (MLPPolicy if c.kind == "actor" else MLPValue)(net if net is not None else build(c.name).net, c.act, c.slope)


def _logp(net, obs64, act, activation, slope):
    z = U.forward(net64(net), obs64, activation, slope)[0]
    mx = z.max(1, keepdims=True)
    return (z - mx - np.log(np.exp(z - mx).sum(1, keepdims=True)))[np.arange(len(act)), act]


def make_batch(net, c, rng):
    M, dO, nA = c.M, c.sizes[0], c.sizes[-1]
    m = np.arange(M, dtype=np.float64)
    if c.pattern == "det":
        k = np.arange(dO, dtype=np.float64)
        obs = np.cos(m[:, None] * 0.0137 * (k + 1.0) + k) + 0.5 * np.sin(m[:, None] * 0.00091 * (k + 2.0))
        act = ((m.astype(np.int64) * 7 + m.astype(np.int64) // 32) % nA).astype(np.int32)
        adv = np.sin(0.11 * m) + 0.6 * np.cos(0.0173 * m + 1.0)
        noise = c.lp_noise * np.array([-2.0, -0.7, 0.0, 0.7, 2.0])[(m.astype(np.int64) * 3 + m.astype(np.int64) // 32) % 5]  # clear of the clip edges
        ret = np.cos(0.05 * m) + 0.3 * np.sin(0.0031 * m)
    else:
        obs = rng.normal(size=(M, dO))
        act = rng.integers(0, nA, size=M).astype(np.int32)
        adv = rng.normal(size=M)
        adv = np.where(np.abs(adv) < 0.05, 0.05, adv)
        noise = c.lp_noise * rng.normal(size=M)
        ret = rng.normal(size=M)
    obs = obs.astype(np.float16 if c.xdt == "f16" else np.float32)
    logp = (_logp(net, obs.astype(np.float64), act, c.act, c.slope) + noise).astype(np.float32) if c.kind == "actor" else np.zeros(M, np.float32)
    return dict(obs=obs, act=act, adv=adv.astype(np.float32), logp=logp, ret=ret.astype(np.float32))


def _mask(c, d, rng):
    """(valid as the device gets it or None, the records the reference keeps or None); plants the garbage"""
    M, nA = c.M, c.sizes[-1]
    valid = keep = None
    if c.mask == "tiles":
        valid = np.ones(M, np.uint8)
        valid[32:64] = 0
        valid[96:128] = 0
        valid[192:] = 0  # the tail: the partial last tile
        valid[rng.choice(M, size=M // 10, replace=False)] = 0
        bad = valid == 0
        garbage = np.array([np.nan, np.inf, -np.inf], np.float32)
        for key in ("obs", "adv", "logp", "ret"):
            x = d[key]
            g = garbage[rng.integers(0, 3, size=x.shape)].astype(x.dtype)
            d[key] = np.where(bad.reshape((-1,) + (1,) * (x.ndim - 1)), g, x)
        d["act"] = np.where(bad & (np.arange(M) % 3 == 0), 2 ** 30, d["act"]).astype(np.int32)
        keep = ~bad
    if c.bad_act:
        d["act"] = d["act"].copy()
        d["act"][[0, 33, 64, M - 1]] = -1
        d["act"][[5, 31, 100]] = nA
        d["act"][7] = -2 ** 31
        keep = (d["act"] >= 0) & (d["act"] < nA)
    return valid, keep


def reference(c, net, d, keep, dact=None):
    """the f64 host pass: dict(g, n, loss, kl, ent, cf)"""
    n64, x = net64(net), d["obs"].astype(np.float64)
    if c.kind == "actor":
        act = np.where(keep, d["act"], 0) if keep is not None else d["act"]
        loss, kl, ent, cf, g, n = U.loss_pi(n64, x, act, d["adv"], d["logp"], CLIP, c.act, c.slope, valid=keep, dact=dact)
        return dict(g=g, n=n, loss=loss, kl=kl, ent=ent, cf=cf)
    loss, g, n = U.loss_v(n64, x, d["ret"], c.act, c.slope, valid=keep, dact=dact)
    return dict(g=g, n=n, loss=loss, kl=0.0, ent=0.0, cf=0.0)


def compact(d, keep):
    """the kept records as CPU torch tensors (what torch's autograd gets: it knows no mask)"""
    sel = slice(None) if keep is None else keep
    return {k: torch.from_numpy(np.ascontiguousarray(v[sel])) for k, v in d.items()}


def torch_entropy(net, f, dtype):
    with torch.no_grad():
        return float(torch.distributions.Categorical(logits=net.to_torch().to(dtype)(f["obs"].to(dtype))).entropy().mean())


@functools.lru_cache(maxsize=None)
def build(name):
    c = CASES[name]
    rng = np.random.default_rng(1000 + c.seed)
    net = make_net(c.sizes, bias_flags(c.bias, len(c.sizes) - 1, c.seed), rng, c.logit_scale)
    d = make_batch(net, c, rng)
    valid, keep = _mask(c, d, rng)
    ref = reference(c, net, d, keep)
    f = compact(d, keep)
    g32, loss32, kl32 = _torch_grad(model(c, net), c.kind, f, CLIP, torch.float32, "cpu")
    ent32 = torch_entropy(model(c, net), f, torch.float32) if c.kind == "actor" else 0.0
    for v in d.values():
        v.setflags(write=False)
    return SimpleNamespace(case=c, net=net, data=d, valid=valid, keep=keep, ref=ref, g32=g32, ref32=dict(loss=loss32, kl=kl32, ent=ent32),
                           bound=_grad_bound(ref["g"], g32))


def passes(g, b):
    """the comparator of the device test: max norm of the difference against the f64 gradient within the case's bound"""
    return float(np.abs(np.asarray(g, np.float64) - b.ref["g"]).max()) <= b.bound


def scalar_bound(want, ref32):
    """test_gpu_ppo_update.py's rule for loss / kl / entropy: 4 x the f32 reference's own error, floored at 4 ulps of max(1, |value|)"""
    return max(4.0 * abs(float(ref32) - want), 4.0 * ULP * max(1.0, abs(want)))


def layer_slices(c):
    """[(W slice, b slice or None)] of the flat parameter vector"""
    out, o = [], 0
    for (i, w), hb in zip(zip(c.sizes[:-1], c.sizes[1:]), bias_flags(c.bias, len(c.sizes) - 1, c.seed)):
        ws = slice(o, o + i * w)
        o += i * w
        bs = None
        if hb:
            bs = slice(o, o + w)
            o += w
        out.append((ws, bs))
    return out


def clip_ratios(b):
    """the f64 ratios of an actor case's kept records"""
    c, d = b.case, b.data
    sel = slice(None) if b.keep is None else b.keep
    lp = _logp(b.net, d["obs"].astype(np.float64)[sel], d["act"][sel], c.act, c.slope)
    return np.exp(lp - d["logp"].astype(np.float64)[sel])


# ---- Adam across calls ----
ADAM = SimpleNamespace(sizes_pi=(4, 16, 3), sizes_v=(4, 16, 1), act="tanh", M=3000, iters=10, pi_lr=3e-3, vf_lr=1e-2, target_kl=0.01044, seed=7)
MARGIN = 0.05  # of test_ppo_update.py: no host kl within 5 % of the limit


def torch_update(model_, kind, f, iters, lr, target_kl, opt=None):
    """adapt()'s loop for one network in f32 on the CPU, autograd and torch.optim.Adam: (optimizer, trace [passes computed, 2])"""
    opt = opt or torch.optim.Adam(model_.parameters(), lr=lr)
    trace = []
    for i in range(iters):
        opt.zero_grad()
        if kind == "actor":
            logp = torch.distributions.Categorical(logits=model_(f["obs"])).log_prob(f["act"].long())
            ratio = torch.exp(logp - f["logp"])
            loss = -(torch.min(ratio * f["adv"], torch.clamp(ratio, 1 - CLIP, 1 + CLIP) * f["adv"])).mean()
            kl = float((f["logp"] - logp).mean().detach())
        else:
            loss, kl = ((model_(f["obs"])[:, 0] - f["ret"]) ** 2).mean(), 0.0
        trace.append((float(loss.detach()), kl))
        if kind == "actor" and kl > 1.5 * target_kl:
            break
        loss.backward()
        opt.step()
    return opt, np.asarray(trace, np.float64).reshape(-1, 2)


def torch_flat(model_, opt):
    """(weights, m, v) flat in the device's order, f64"""
    ps = [p for x in model_ if isinstance(x, torch.nn.Linear) for p in (x.weight, x.bias) if p is not None]
    cat = lambda xs: torch.cat([x.detach().reshape(-1) for x in xs]).double().numpy()  # noqa: E731
    return cat(ps), cat([opt.state[p]["exp_avg"] for p in ps]), cat([opt.state[p]["exp_avg_sq"] for p in ps])


@functools.lru_cache(maxsize=None)
def adam_calls():
    """Three batches for one learner and the f64 host run / the f32 torch run over them, the optimiser states carried.  Batches 1 and 2
    hold actions and log-probs of the initial policy, so the kl of call 2 goes on from where call 1 left it and passes the limit; batch 3
    is drawn from the policy the host run has after call 2."""
    A = ADAM
    rng = np.random.default_rng(A.seed)
    pi0 = make_net(A.sizes_pi, (True, True), rng)
    v0 = make_net(A.sizes_v, (True, True), rng)
    from rl_offline_simulation_amd.evaluators import MLPPolicy, MLPValue
    t_pi, t_v = MLPPolicy(pi0, A.act).to_torch(), MLPValue(v0, A.act).to_torch()
    pi, v, opt_pi, opt_v, o_pi, o_v = net64(pi0), net64(v0), None, None, None, None
    calls = []
    for call in range(3):
        obs = rng.normal(size=(A.M, A.sizes_pi[0])).astype(np.float32)
        sampler = pi0 if call < 2 else [(W.astype(np.float32), b.astype(np.float32)) for W, b in pi]
        z = U.forward(net64(sampler), obs.astype(np.float64), A.act)[0]
        p = np.exp(z - z.max(1, keepdims=True))
        p /= p.sum(1, keepdims=True)
        act = (p.cumsum(1) < rng.random(A.M)[:, None]).sum(1).clip(0, A.sizes_pi[-1] - 1).astype(np.int32)
        # the advantage is the same function of (obs, act) in every batch, plus noise: the calls push the policy the same way
        adv = np.where(act == 0, obs[:, 0], np.where(act == 1, -obs[:, 1], 0.5 * obs[:, 2])) + 0.5 * rng.normal(size=A.M)
        d = dict(obs=obs, act=act, adv=adv.astype(np.float32),
                 logp=np.log(p[np.arange(A.M), act]).astype(np.float32), ret=(obs[:, 0] + 0.5 * rng.normal(size=A.M)).astype(np.float32))
        a = U.update(pi, "actor", d, A.iters, A.pi_lr, CLIP, A.target_kl, A.act, opt=opt_pi)
        c = U.update(v, "critic", d, A.iters, A.vf_lr, CLIP, A.target_kl, A.act, opt=opt_v)
        pi, v, opt_pi, opt_v = a["net"], c["net"], a["opt"], c["opt"]
        f = {k: torch.from_numpy(x) for k, x in d.items()}
        o_pi, tr_pi = torch_update(t_pi, "actor", f, A.iters, A.pi_lr, A.target_kl, o_pi)
        o_v, tr_v = torch_update(t_v, "critic", f, A.iters, A.vf_lr, A.target_kl, o_v)
        calls.append(SimpleNamespace(data=d, a=a, c=c, pi=U.flatten(pi), v=U.flatten(v), pi_m=opt_pi.m.copy(), pi_v=opt_pi.v.copy(), pi_t=opt_pi.t,
                                     v_m=opt_v.m.copy(), v_v=opt_v.v.copy(), v_t=opt_v.t, t32_pi=torch_flat(t_pi, o_pi), t32_v=torch_flat(t_v, o_v), tr32_pi=tr_pi, tr32_v=tr_v))
    return SimpleNamespace(pi0=pi0, v0=v0, calls=calls)


def state_bound(x64, x32):
    """weights, m or v after several steps: 4 x the deviation of the f32 torch loop from the f64 host run, floored at 4 ulps of the largest"""
    return max(4.0 * float(np.abs(x32 - x64).max()), 4.0 * ULP * float(np.abs(x64).max()))
