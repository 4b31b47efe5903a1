"""NumPy f64 restatement of HOMER training (offsim4rl/encoders/homer.py:81-91 and 170-184, the model of offsim4rl/encoders/models.py): the loss
of _calc_loss with the Gumbel noise and the batch indices given, its gradient, the hard (discretized) forward, clip_grad_norm_ and
torch.optim.Adam with L2 weight decay -- the host reference of offsim_homer_grad / offsim_homer_step.

A model is a list of eight arrays in state_dict order (obs_encoder.0 W, b, .2 W, b, classifier.0 W, b, .2 W, b); gradients are flat in that
order (the layout of offsim_homer_grad's `grad`).  Conventions as tests/ppo_update_host.py."""
import numpy as np

KEYS = ("obs_encoder.0.weight", "obs_encoder.0.bias", "obs_encoder.2.weight", "obs_encoder.2.bias",
        "classifier.0.weight", "classifier.0.bias", "classifier.2.weight", "classifier.2.bias")
SLOPE = 0.01


def n_params(dO, nA, nZ, H):
    return dO * H + H + H * nZ + nZ + (2 * nZ + nA) * H + H + 2 * H + 2


def shapes(dO, nA, nZ, H):
    return [(H, dO), (H,), (nZ, H), (nZ,), (H, 2 * nZ + nA), (H,), (2, H), (2,)]


def flatten(model):
    return np.concatenate([np.asarray(t, np.float64).ravel() for t in model])


def unflatten(flat, like):
    out, o = [], 0
    for t in like:
        t = np.asarray(t)
        out.append(np.asarray(flat[o:o + t.size]).reshape(t.shape).copy())
        o += t.size
    return out


def _leaky(x, slope):
    return np.where(x > 0, x, slope * x)


def _mlp(x, W1, b1, W2, b2, slope):
    pre = x @ W1.T + b1
    h = _leaky(pre, slope)
    return h @ W2.T + b2, pre, h


def _mlp_back(d_out, x, pre, h, W2, slope):
    """(gW1, gb1, gW2, gb2, d_in) from d loss / d outputs"""
    gW2, gb2 = d_out.T @ h, d_out.sum(0)
    dpre = (d_out @ W2) * np.where(pre > 0, 1.0, slope)
    return dpre.T @ x, dpre.sum(0), gW2, gb2, dpre


def _softmax(u):
    e = np.exp(u - u.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def valid_records(act, idx_real, idx_impo, n_rows, nA):
    i, j = np.asarray(idx_real).astype(np.int64), np.asarray(idx_impo).astype(np.int64)
    ok = (i >= 0) & (i < n_rows) & (j >= 0) & (j < n_rows)
    a = np.asarray(act).astype(np.int64)[np.where(ok, i, 0)]
    return ok & (a >= 0) & (a < nA)


def loss_grad(model, obs, act, next_obs, idx_real, idx_impo, noise=None, tau=1.0, hard=False, slope=SLOPE, info=None):
    """(loss, flat gradient or None with hard, n) over the valid records.  noise [M, 4, nZ] (None: zeros), in the order prev, curr of
    the real call, prev, curr of the impostor call.  info: a dict that receives the perturbed logits u [4][n, nZ] and the hidden
    pre-activations (the fixture script's margins)."""
    W1, b1, W2, b2, V1, c1, V2, c2 = [np.asarray(t, np.float64) for t in model]
    nZ, nA = W2.shape[0], V1.shape[1] - 2 * W2.shape[0]
    obs, next_obs = np.asarray(obs, np.float64), np.asarray(next_obs, np.float64)
    obs, next_obs = obs.reshape(obs.shape[0], -1), next_obs.reshape(next_obs.shape[0], -1)
    ok = valid_records(act, idx_real, idx_impo, obs.shape[0], nA)
    i, j = np.asarray(idx_real).astype(np.int64)[ok], np.asarray(idx_impo).astype(np.int64)[ok]
    n = int(ok.sum())
    if n == 0:
        return 0.0, (None if hard else np.zeros(flatten(model).size)), 0
    g = np.zeros((n, 4, nZ)) if noise is None else np.asarray(noise, np.float64)[ok]
    a = np.asarray(act).astype(np.int64)[i]
    onehot = np.zeros((n, nA))
    onehot[np.arange(n), a] = 1.0
    xs = [obs[i], next_obs[i], next_obs[j]]
    enc = [_mlp(x, W1, b1, W2, b2, slope) for x in xs]
    src = (0, 1, 0, 2)  # which encoder pass feeds z_q
    us = [(enc[src[q]][0] + g[:, q]) / tau for q in range(4)]
    ys = [_softmax(u) for u in us]
    if hard:
        zs = []
        for u, y in zip(us, ys):
            oh = np.zeros_like(y)
            oh[np.arange(n), u.argmax(1)] = 1.0
            zs.append((oh - y) + y)
    else:
        zs = ys
    loss, cls = 0.0, []
    for c, target in ((0, 1), (1, 0)):
        x = np.concatenate([zs[2 * c], onehot, zs[2 * c + 1]], 1)
        logits, pre, h = _mlp(x, V1, c1, V2, c2, slope)
        mx = logits.max(1, keepdims=True)
        logp = logits - (mx + np.log(np.exp(logits - mx).sum(1, keepdims=True)))
        loss += -logp[:, target].mean() / 2.0
        cls.append((x, pre, h, logp, target))
    if info is not None:
        info.update(u=us, enc_pre=[e[1] for e in enc], cls_pre=[c[1] for c in cls])
    if hard:
        return float(loss), None, n
    gV = [0.0] * 4
    gW = [0.0] * 4
    d_enc = [np.zeros((n, nZ)) for _ in range(3)]
    for c, (x, pre, h, logp, target) in enumerate(cls):
        t = np.zeros_like(logp)
        t[:, target] = 1.0
        d_out = (np.exp(logp) - t) / (2.0 * n)
        *gs, dpre = _mlp_back(d_out, x, pre, h, V2, slope)
        gV = [p + q for p, q in zip(gV, gs)]
        dx = dpre @ V1
        for q, dz in ((2 * c, dx[:, :nZ]), (2 * c + 1, dx[:, nZ + nA:])):
            z = zs[q]
            d_enc[src[q]] += z * (dz - (dz * z).sum(1, keepdims=True)) / tau
    for s in range(3):
        _, pre, h = enc[s]
        *gs, _ = _mlp_back(d_enc[s], xs[s], pre, h, W2, slope)
        gW = [p + q for p, q in zip(gW, gs)]
    return float(loss), np.concatenate([np.asarray(t).ravel() for t in gW + gV]), n


def clip_coef(g, max_norm):
    """torch.nn.utils.clip_grad_norm_: (total_norm, the clamped coefficient every gradient is multiplied by)"""
    total = float(np.sqrt((np.asarray(g, np.float64) ** 2).sum()))
    return total, min(1.0, max_norm / (total + 1e-6))


class Adam:
    """torch.optim.Adam with L2 weight decay (g += wd * p before the moments; b1 0.9, b2 0.999, eps 1e-8) on a flat parameter vector"""

    def __init__(self, n, lr, weight_decay=0.0):
        self.lr, self.wd, self.m, self.v, self.t = lr, weight_decay, np.zeros(n), np.zeros(n), 0

    def step(self, p, g):
        b1, b2, eps = 0.9, 0.999, 1e-8
        self.t += 1
        g = g + self.wd * p
        self.m = b1 * self.m + (1 - b1) * g
        self.v = b2 * self.v + (1 - b2) * g * g
        return p - (self.lr / (1 - b1 ** self.t)) * self.m / (np.sqrt(self.v) / np.sqrt(1 - b2 ** self.t) + eps)


def step(model, opt, data, idx_real, idx_impo, noise, tau, max_norm=40.0):
    """one batch of homer.py:87-91: (new model, loss, total_norm, n); a batch without a valid record changes nothing"""
    obs, act, next_obs = data
    loss, g, n = loss_grad(model, obs, act, next_obs, idx_real, idx_impo, noise, tau)
    if n == 0:
        return model, 0.0, 0.0, 0
    total, coef = clip_coef(g, max_norm)
    return unflatten(opt.step(flatten(model), g * coef), model), loss, total, n


def train_epoch(model, opt, data, idx_real, idx_impo, noise, batch_size, tau, max_norm=40.0):
    """(new model, per-batch losses)"""
    losses = []
    for lo in range(0, len(idx_real), batch_size):
        hi = min(len(idx_real), lo + batch_size)
        model, loss, _, _ = step(model, opt, data, idx_real[lo:hi], idx_impo[lo:hi], None if noise is None else noise[lo:hi], tau, max_norm)
        losses.append(loss)
    return model, np.asarray(losses)


def eval_epoch(model, data, idx_real, idx_impo, noise, batch_size):
    obs, act, next_obs = data
    return np.asarray([loss_grad(model, obs, act, next_obs, idx_real[lo:lo + batch_size], idx_impo[lo:lo + batch_size],
                                 None if noise is None else noise[lo:lo + batch_size], 1.0, hard=True)[0]
                       for lo in range(0, len(idx_real), batch_size)])
