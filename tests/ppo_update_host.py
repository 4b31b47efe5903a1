"""NumPy f64 restatement of the PPO update (offsim4rl/agents/ppo.py:162-223: _compute_loss_pi, _compute_loss_v, adapt's two Adam loops and
the KL early stop; torch.optim.Adam's default step), the host reference of offsim_ppo_grad / offsim_ppo_update.

A network is a list of (W [out, in], b [out] or None) with one activation kind between the layers; gradients are flat in layer order,
W then b of each layer (the layout of offsim_ppo_grad's `grad`)."""
import numpy as np


def _act(x, kind, slope):
    if kind == "tanh":
        return np.tanh(x)
    if kind == "relu":
        return np.maximum(x, 0.0)
    if kind == "leaky_relu":
        return np.where(x > 0, x, slope * x)
    return x


def _dact(x, h, kind, slope):
    """the activation's derivative at pre-activation x (output h), torch's conventions at 0"""
    if kind == "tanh":
        return 1.0 - h * h
    if kind == "relu":
        return (x > 0).astype(np.float64)
    if kind == "leaky_relu":
        return np.where(x > 0, 1.0, slope)
    return np.ones_like(x)


def forward(net, obs, activation="tanh", slope=0.01):
    """(outputs [M, out_last], the layers' inputs, the hidden layers' pre-activations)"""
    a = np.asarray(obs, np.float64)
    ins, pre = [], []
    for i, (W, b) in enumerate(net):
        ins.append(a)
        z = a @ np.asarray(W, np.float64).T + (0.0 if b is None else np.asarray(b, np.float64))
        pre.append(z)
        a = _act(z, activation, slope) if i < len(net) - 1 else z
    return a, ins, pre


def backward(net, ins, pre, d_out, activation="tanh", slope=0.01, dact=None):
    """flat gradient from d loss / d outputs [M, out_last]; dact: another derivative in _dact's place (tests of a comparator's sensitivity)"""
    dact = dact or _dact
    grads = [None] * len(net)
    d = d_out
    for i in range(len(net) - 1, -1, -1):
        W, b = net[i]
        grads[i] = (d.T @ ins[i], None if b is None else d.sum(0))
        if i > 0:
            d = (d @ np.asarray(W, np.float64)) * dact(pre[i - 1], ins[i], activation, slope)
    return flatten(grads)


def flatten(net):
    return np.concatenate([np.concatenate([np.asarray(W, np.float64).ravel()] + ([] if b is None else [np.asarray(b, np.float64).ravel()]))
                           for W, b in net])


def unflatten(flat, like):
    out, o = [], 0
    for W, b in like:
        w = flat[o:o + W.size].reshape(W.shape)
        o += W.size
        bb = None
        if b is not None:
            bb = flat[o:o + b.size].copy()
            o += b.size
        out.append((w.copy(), bb))
    return out


def loss_pi(net, obs, act, adv, logp_old, clip, activation="tanh", slope=0.01, valid=None, dact=None):
    """(loss, kl, entropy, clipfrac, flat gradient, n) of _compute_loss_pi over the valid entries"""
    obs, act, adv, logp_old = np.asarray(obs, np.float64), np.asarray(act).astype(np.int64), np.asarray(adv, np.float64), np.asarray(logp_old, np.float64)
    if valid is not None:
        v = np.asarray(valid).astype(bool).ravel()
        obs, act, adv, logp_old = obs.reshape(v.size, -1)[v], act.ravel()[v], adv.ravel()[v], logp_old.ravel()[v]
    n = len(act)
    z, ins, pre = forward(net, obs, activation, slope)
    mx = z.max(1, keepdims=True)
    lse = mx + np.log(np.exp(z - mx).sum(1, keepdims=True))
    logq = z - lse
    p = np.exp(logq)
    logp = logq[np.arange(n), act]
    ratio = np.exp(logp - logp_old)
    lo, hi = 1.0 - clip, 1.0 + clip
    x, y = ratio * adv, np.clip(ratio, lo, hi) * adv
    inside = (ratio >= lo) & (ratio <= hi)
    loss = -np.minimum(x, y).mean()
    kl = (logp_old - logp).mean()
    ent = (-(p * logq).sum(1)).mean()
    cf = (~inside).mean()
    dsurr = np.where(inside | (x < y), adv, 0.0)  # d min(x, y) / d ratio (torch: ties halve, and both halves reach ratio inside the range)
    dlogp = -dsurr * ratio / n
    onehot = np.zeros_like(z)
    onehot[np.arange(n), act] = 1.0
    g = backward(net, ins, pre, dlogp[:, None] * (onehot - p), activation, slope, dact)
    return loss, kl, ent, cf, g, n


def loss_v(net, obs, ret, activation="tanh", slope=0.01, valid=None, dact=None):
    """(loss, flat gradient, n) of _compute_loss_v over the valid entries"""
    obs, ret = np.asarray(obs, np.float64), np.asarray(ret, np.float64)
    if valid is not None:
        v = np.asarray(valid).astype(bool).ravel()
        obs, ret = obs.reshape(v.size, -1)[v], ret.ravel()[v]
    n = len(ret)
    z, ins, pre = forward(net, obs, activation, slope)
    e = z[:, 0] - ret
    return (e * e).mean(), backward(net, ins, pre, (2.0 * e / n)[:, None], activation, slope, dact), n


class Adam:
    """torch.optim.Adam, defaults (b1 0.9, b2 0.999, eps 1e-8, no weight decay), on a flat parameter vector"""

    def __init__(self, n, lr):
        self.lr, self.m, self.v, self.t = lr, np.zeros(n), np.zeros(n), 0

    def step(self, p, g):
        b1, b2, eps = 0.9, 0.999, 1e-8
        self.t += 1
        self.m = b1 * self.m + (1 - b1) * g
        self.v = b2 * self.v + (1 - b2) * g * g
        return p - (self.lr / (1 - b1 ** self.t)) * self.m / (np.sqrt(self.v) / np.sqrt(1 - b2 ** self.t) + eps)


def update(net, kind, data, iters, lr, clip=0.2, target_kl=0.01, activation="tanh", slope=0.01, opt=None):
    """adapt()'s loop for one network: returns dict(net, stop_iter, trace [passes computed, 2] of (loss, kl), first / last pass stats,
    opt).  kind: 'actor' | 'critic'.  The KL test comes before the step of pass i; StopIter is i at the break, else iters - 1."""
    flat = flatten(net)
    opt = opt or Adam(flat.size, lr)
    trace, first, last, stop = [], None, None, iters - 1
    for i in range(iters):
        cur = unflatten(flat, net)
        if kind == "actor":
            loss, kl, ent, cf, g, _ = loss_pi(cur, data["obs"], data["act"], data["adv"], data["logp"], clip, activation, slope, data.get("valid"))
        else:
            loss, g, _ = loss_v(cur, data["obs"], data["ret"], activation, slope, data.get("valid"))
            kl = ent = cf = 0.0
        last = dict(loss=loss, kl=kl, ent=ent, cf=cf)
        first = first or last
        trace.append((loss, kl))
        if kind == "actor" and kl > 1.5 * target_kl:
            stop = i
            break
        flat = opt.step(flat, g)
    return dict(net=unflatten(flat, net), stop_iter=stop, trace=np.asarray(trace, np.float64).reshape(-1, 2), first=first, last=last, opt=opt)
