"""A population of independent HOMER encoders on the device: L seeds or (lr, weight_decay, max_grad_norm) settings per launch.

One encoder at the reference's sizes is three launches of 8 workgroups per batch of 64, and HOMER is run over many
seeds and a small grid of hyperparameters, the latent map chosen by best validation loss.  The learner is therefore a grid dimension of
the kernels HOMEREncoder uses (offsim_homer_grad_pop, offsim_homer_step_pop): all learners read the same dataset, each
has its own weights, Adam state, hyperparameters, batch indices, Gumbel noise and early stop.  Learners never interact: learner l's
numbers are, bit for bit, those of a HOMEREncoder fed learner l's indices and noise.

The population owns the stacked device weights (every tensor of the state_dict with a leading learner axis) and steps them in place;
encoder(l) / state_dict(l) / best_state_dict(l) export one learner.

The population is also used as one: encode / encode_device run every learner over the same observations in one launch
(offsim_encode_mlp_pop, the learner as a grid dimension of the encoder's kernels), latent_report counts what each learner makes of a log
(offsim_latent_counts), and evaluators builds each learner's PerStateRejectionSampling from two such launches."""
import math
import os
from collections import namedtuple

import numpy as np
import torch

from .. import _lib as L
from .homer import CLS_KEYS, ENC_KEYS, LEAKY_SLOPE, HOMEREncoder, HomerTrainResult


def _per_learner(x, n, name):
    """a scalar or a length-n sequence -> a list of n floats, none negative"""
    try:
        xs = [float(v) for v in x]
    except TypeError:
        xs = [float(x)] * n
    if len(xs) != n:
        raise ValueError(f"HOMERPopulation: {name} must be a scalar or a sequence of {n} values, got {len(xs)}")
    if not all(v >= 0.0 for v in xs):
        raise ValueError(f"HOMERPopulation: every {name} must be >= 0")
    return xs


def epoch_draws(generator, L, n, nZ):
    """One epoch's draws for L learners over n rows, from `generator` alone (a CPU or a device torch.Generator): (idx_real [L, n] i32,
    idx_impo [L, n] i32, noise [L, n, 4, nZ] f32) on the generator's device.  Every index row is a permutation of range(n) (the ranks of n
    uniform draws); the noise is standard Gumbel as gumbel_noise draws it, -log(Exponential(1))."""
    dev = generator.device
    perms = lambda: torch.rand((L, n), dtype=torch.float64, device=dev, generator=generator).argsort(dim=1).to(torch.int32)  # noqa: E731
    idx_real, idx_impo = perms(), perms()
    noise = -torch.empty((L, n, 4, nZ), dtype=torch.float32, device=dev).exponential_(generator=generator).log()
    return idx_real, idx_impo, noise


LatentReport = namedtuple("LatentReport", "z counts used joint purity skipped")


def latent_stats(counts, joint, n_rows):
    """(used [L] i64, purity [L] f64 or None) of counts [L, nZ] and joint [L, nZ, nY] (or None), exact integers: used = the non-empty
    latent states, purity = sum_z max_y joint[l, z, y] / n_rows in f64 (0 rows: 0).  torch on the tensors' device, nothing read back."""
    used = (counts > 0).sum(dim=1)
    if joint is None:
        return used, None
    hits = joint.max(dim=2).values.sum(dim=1).to(torch.float64)
    return used, hits / torch.full_like(hits, max(int(n_rows), 1))  # (tensor by tensor: a scalar divisor is multiplied by as its reciprocal on the device)


class HOMERPopulation:
    """L HOMEREncoder's of one architecture, trained together.  Initial weights: with `seeds`, learner l gets those of
    HOMEREncoder(...) constructed under torch.manual_seed(seeds[l]) (the reference's initialisation at that seed); with `state_dicts`,
    the given ones (the reference's keys; a dict without the classifier gets torch's default one); with `L` alone, L encoders drawn one
    after another from torch's current generator.  lr, weight_decay and max_grad_norm (attributes, each a scalar or one value per
    learner) are what train_epoch steps with; train() sets them from its arguments."""

    def __init__(self, obs_dim, action_dim, latent_size, hidden_size, L=None, seeds=None, state_dicts=None, device=None):
        self.obs_dim, self.action_dim, self.latent_size, self.hidden_size = obs_dim, action_dim, latent_size, hidden_size
        self.device = device
        if (seeds is not None) and (state_dicts is not None):
            raise ValueError("HOMERPopulation: give seeds or state_dicts, not both")
        given = seeds if seeds is not None else state_dicts
        if given is not None:
            given = list(given)
            if L is not None and L != len(given):
                raise ValueError(f"HOMERPopulation: L = {L} but {len(given)} seeds / state_dicts")
            L = len(given)
        if L is None or not 1 <= L <= 65535:
            raise ValueError("HOMERPopulation: the number of learners must be in 1..65535 (L, seeds or state_dicts)")
        self.L = L
        one = lambda: HOMEREncoder(obs_dim, action_dim, latent_size, hidden_size)  # noqa: E731
        if seeds is not None:
            host = []
            for s in given:
                torch.manual_seed(int(s))
                host.append(one()._host)
        elif state_dicts is not None:
            host = [self._host_of(sd, one) for sd in given]
        else:
            host = [one()._host for _ in range(L)]
        shapes = one()._shapes()
        for h in host:
            for t, shape in zip(h, shapes):
                if tuple(t.shape) != shape:
                    raise ValueError(f"HOMERPopulation: a tensor of shape {tuple(t.shape)} where the architecture has {shape}")
        self._host = [torch.stack([h[k] for h in host]).contiguous() for k in range(8)]  # per tensor [L, ...]
        self._p = self._best = self._opt = self._work = self._hyper_dev = None
        self._hyper = {"lr": [1e-3] * L, "weight_decay": [0.0] * L, "max_grad_norm": [40.0] * L}
        self.result = None

    @staticmethod
    def _host_of(sd, one):
        get = lambda k: torch.as_tensor(np.asarray(sd[k]) if not isinstance(sd[k], torch.Tensor) else sd[k]).detach().to("cpu", torch.float32)  # noqa: E731
        enc = [get(k) for k in ENC_KEYS]
        return enc + ([get(k) for k in CLS_KEYS] if all(k in sd for k in CLS_KEYS) else one()._host[4:])

    @classmethod
    def from_encoders(cls, encoders, device=None):
        """the population of these HOMEREncoder's current weights (copies), all of one architecture"""
        encoders = list(encoders)
        if not encoders:
            raise ValueError("HOMERPopulation.from_encoders: no encoder")
        dims = lambda e: (e.obs_dim, e.action_dim, e.latent_size, e.hidden_size)  # noqa: E731
        if any(dims(e) != dims(encoders[0]) for e in encoders):
            raise ValueError("HOMERPopulation.from_encoders: all learners share one architecture")
        return cls(*dims(encoders[0]), state_dicts=[e.state_dict() for e in encoders], device=device)

    # ---- hyperparameters: host lists, and [L] f64 device tensors once a device is known ----
    def _set_hyper(self, name, value):
        self._hyper[name] = _per_learner(value, self.L, name)
        self._hyper_dev = None

    lr = property(lambda self: self._hyper["lr"], lambda self, v: self._set_hyper("lr", v))
    weight_decay = property(lambda self: self._hyper["weight_decay"], lambda self, v: self._set_hyper("weight_decay", v))
    max_grad_norm = property(lambda self: self._hyper["max_grad_norm"], lambda self, v: self._set_hyper("max_grad_norm", v))

    def _hyper_on(self, dev):
        if self._hyper_dev is None or self._hyper_dev[0].device != dev:
            self._hyper_dev = tuple(torch.tensor(self._hyper[k], dtype=torch.float64, device=dev) for k in ("lr", "weight_decay", "max_grad_norm"))
        return self._hyper_dev

    # ---- the device side ----
    @property
    def n_params(self):
        return L.homer_params(self.obs_dim, self.action_dim, self.latent_size, self.hidden_size)

    def _params(self):
        """the eight stacked tensors on the device"""
        if self._p is None:
            dev = self.device or L.require_device()
            self._p = [t.to(dev, torch.float32).contiguous() for t in self._host]
        return self._p

    def _net(self):
        return L.HomerNet(*[L.ptr(t) for t in self._params()], self.obs_dim, self.action_dim, self.latent_size, self.hidden_size, LEAKY_SLOPE, 0)

    def _scratch(self, dev, sizes):
        """device scratch for launches of these record counts per learner (offsim_homer_work_doubles_pop), kept between calls"""
        net, need = self._net(), 0
        for M in set(sizes):
            n = L.load().offsim_homer_work_doubles_pop(net, self.L, M)
            if n < 0:
                L.check(n)
            need = max(need, n)
        if self._work is None or self._work.device != dev or self._work.numel() < need:
            self._work = torch.empty(need, dtype=torch.float64, device=dev)
        return self._work

    def reset_optimizer(self):
        """every learner's Adam state back to zero"""
        dev, P = self._params()[0].device, self.n_params
        self._opt = (torch.zeros((self.L, P), dtype=torch.float32, device=dev), torch.zeros((self.L, P), dtype=torch.float32, device=dev),
                     torch.zeros(self.L, dtype=torch.int64, device=dev))
        return self._opt

    def adam_state(self):
        """(m [L, P], v [L, P], t [L]): the device tensors of the optimiser state"""
        return self._opt or self.reset_optimizer()

    upload = HOMEREncoder.upload  # (obs, act, next_obs) on the device: the dataset all learners share

    def _records(self, idx_real, idx_impo, noise, dev):
        """the learners' records as the kernels read them: (idx_real, idx_impo, noise, M, idx_stride).  Column slices [:, lo:hi] of
        device arrays [L, n] i32 / [L, n, 4, nZ] f32 are taken as they are (idx_stride = n); anything else is copied."""
        nZ = self.latent_size

        def as_dev(t, dtype):
            t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
            return t.to(dev, dtype)
        ir, ii = as_dev(idx_real, torch.int32), as_dev(idx_impo, torch.int32)
        nz = None if noise is None else as_dev(noise, torch.float32)
        if ir.dim() != 2 or ir.shape[0] != self.L or ii.shape != ir.shape:
            raise ValueError(f"HOMERPopulation: idx_real and idx_impo must be [L = {self.L}, M], got {tuple(ir.shape)} and {tuple(ii.shape)}")
        M = int(ir.shape[1])
        if nz is not None and tuple(nz.shape) != (self.L, M, 4, nZ):
            raise ValueError(f"HOMERPopulation: noise must be [L, M, 4, nZ] = {(self.L, M, 4, nZ)}, got {tuple(nz.shape)}")
        if M == 0:
            return ir, ii, nz, 0, 0
        stride = max(int(ir.stride(0)), M) if self.L > 1 else M
        rows_ok = lambda t: t.stride(1) == 1 and (self.L == 1 or t.stride(0) == stride)  # noqa: E731
        noise_ok = nz is None or (nz[0].is_contiguous() and (self.L == 1 or nz.stride(0) == stride * 4 * nZ))
        if not (rows_ok(ir) and rows_ok(ii) and noise_ok):
            ir, ii, nz, stride = ir.contiguous(), ii.contiguous(), None if nz is None else nz.contiguous(), M
        return ir, ii, nz, M, stride

    def _batch(self, data, ir, ii, nz, M, stride):
        x, a, xn = data
        return L.HomerBatchPop(L.ptr(x), L.ptr(xn), L.F16 if x.dtype == torch.float16 else L.F32, 0, L.ptr(a), x.shape[0], ir.data_ptr(),
                               ii.data_ptr(), None if nz is None else nz.data_ptr(), M, stride)

    def _active(self, active, dev):
        if active is None:
            return None
        a = active if isinstance(active, torch.Tensor) else torch.as_tensor(np.asarray(active))
        if a.numel() != self.L:
            raise ValueError(f"HOMERPopulation: active must have one entry per learner ({self.L}), got {a.numel()}")
        return (a.reshape(-1) != 0).to(dev, torch.uint8).contiguous()

    def loss_grad(self, obs, act, next_obs, idx_real, idx_impo, noise=None, tau=1.0, hard=False):
        """One pass of _calc_loss per learner over its records (idx_real[l, m], idx_impo[l, m], noise[l, m]): (loss [L] f64, grad [L, P] f32
        unclipped and flat per learner in state_dict order; None with hard=True, which is forward only).  `last_n` [L] holds the number of
        valid records per learner."""
        data = self.upload((obs, act, next_obs))
        dev = data[0].device
        ir, ii, nz, M, stride = self._records(idx_real, idx_impo, noise, dev)
        stats = torch.zeros((self.L, 2), dtype=torch.float64, device=dev)
        grad = None if hard else torch.zeros((self.L, self.n_params), dtype=torch.float32, device=dev)
        L.check(L.load().offsim_homer_grad_pop(self._net(), self._batch(data, ir, ii, nz, M, stride), self.L, float(tau), int(bool(hard)), None,
                                               L.ptr(grad), L.ptr(stats), L.ptr(self._scratch(dev, [M])), L.stream_ptr()))
        self.last_n = stats[:, 0]
        return stats[:, 1], grad

    def _epoch(self, data, idx_real, idx_impo, batch_size, tau, noise, active, step):
        dev, nZ = data[0].device, self.latent_size
        ir, ii, nz, n, _ = self._records(idx_real, idx_impo, noise, dev)
        nb = (n + batch_size - 1) // batch_size
        stats = torch.zeros((max(nb, 1), self.L, 3 if step else 2), dtype=torch.float64, device=dev)
        if nb and nz is None:  # the epoch's noise in one draw: a batch's records are a column slice of it, as of the indices
            nz = -torch.empty((self.L, n, 4, nZ), dtype=torch.float32, device=dev).exponential_().log()
        lib, net, stream, act = L.load(), self._net(), L.stream_ptr(), self._active(active, dev)
        work = self._scratch(dev, [min(batch_size, n), n - (nb - 1) * batch_size]) if nb else None
        if step:
            m, v, t = self.adam_state()
            adam = L.HomerAdamPop(L.ptr(m), L.ptr(v), L.ptr(t), *[L.ptr(h) for h in self._hyper_on(dev)])
        for b in range(nb):
            lo, hi = b * batch_size, min(n, (b + 1) * batch_size)
            bt = self._batch(data, *self._records(ir[:, lo:hi], ii[:, lo:hi], nz[:, lo:hi], dev))
            if step:
                L.check(lib.offsim_homer_step_pop(net, bt, self.L, float(tau), adam, L.ptr(act), L.ptr(stats[b]), L.ptr(work), stream))
            else:
                L.check(lib.offsim_homer_grad_pop(net, bt, self.L, 1.0, 1, L.ptr(act), None, L.ptr(stats[b]), L.ptr(work), stream))
        self.last_stats = stats[:nb]
        return stats[:nb, :, 1]

    def train_epoch(self, data, idx_real, idx_impo, batch_size, tau, noise=None, active=None):
        """One offsim_homer_step_pop per batch of `batch_size` records per learner (the short last batch included) -- the column slice
        [:, lo:hi] of idx_real / idx_impo [L, n] and noise [L, n, 4, nZ], uncopied -- all enqueued with no synchronisation; returns the
        per-batch losses [batches, L] as one device tensor.  data: upload()'s triple; noise None: drawn for the epoch on the device;
        active: [L] or None; a learner whose entry is 0 is not stepped and its losses stay 0.  Adam's state carries over."""
        return self._epoch(data, idx_real, idx_impo, batch_size, tau, noise, active, True)

    def eval_epoch(self, data, idx_real, idx_impo, batch_size, noise=None, active=None):
        """The validation pass per learner (discretized, temperature 1.0, no step): per-batch losses [batches, L] as one device tensor."""
        return self._epoch(data, idx_real, idx_impo, batch_size, 1.0, noise, active, False)

    def train(self, train_dataset, val_dataset, lr=1e-3, weight_decay=0.0, num_epochs=1000, batch_size=64, patience_threshold=50,
              temperature_decay=False, max_grad_norm=40.0, seed=0, model_dir=None):
        """HOMEREncoder.train's loop for every learner at once, each with its own early stop.  One device generator seeded with `seed`
        gives, per epoch, epoch_draws for the training pass and then epoch_draws for the validation pass, so a run can be replayed.  A
        fresh Adam; tau = max(0.5, exp(-0.005 epoch)) with temperature_decay; a learner's epoch losses are the plain means of its per-batch
        losses; per learner best_val_loss starts at 0.69 and the learner stops at val_loss > 0.8 in a non-improving epoch or at the
        patience limit.  A stopped learner is never stepped again; the loop ends when all have stopped or at num_epochs.  One host
        synchronisation per epoch.  Returns HomerTrainResult of per-learner lists (train_losses[l], val_losses[l]) and [L] arrays
        (best_epoch, best_val_loss, epochs_run); with model_dir every learner's best weights are saved as encoder_model_{l}.pt."""
        self.lr, self.weight_decay, self.max_grad_norm = lr, weight_decay, max_grad_norm
        tr, va = self.upload(train_dataset), self.upload(val_dataset)
        dev, n, nZ = tr[0].device, self.L, self.latent_size
        self.reset_optimizer()
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed))
        n_tr, n_va = tr[0].shape[0], va[0].shape[0]
        best_val, best_epoch = np.full(n, 0.69), np.full(n, -1, np.int64)
        patience, epochs_run, running = np.zeros(n, np.int64), np.zeros(n, np.int64), np.ones(n, bool)
        self._best = [t.clone() for t in self._params()]
        train_losses, val_losses = [[] for _ in range(n)], [[] for _ in range(n)]
        active = torch.ones(n, dtype=torch.uint8, device=dev)
        mean = lambda x, l: x[:, l].mean() if x.shape[0] else x[:, l].sum()  # noqa: E731  (a learner's column reduced as HOMEREncoder.train reduces its own)
        for epoch in range(1, num_epochs + 1):
            tau = max(0.5, math.exp(-0.005 * epoch)) if temperature_decay else 1.0
            ir, ii, nz = epoch_draws(gen, n, n_tr, nZ)
            lt = self.train_epoch(tr, ir, ii, batch_size, tau, noise=nz, active=active)
            ir, ii, nz = epoch_draws(gen, n, n_va, nZ)
            lv = self.eval_epoch(va, ir, ii, batch_size, noise=nz, active=active)
            both = torch.stack([torch.stack([mean(x, l) for l in range(n)]) for x in (lt, lv)]).cpu()  # [2, L]: the epoch's one synchronisation
            improved = []
            for l in np.flatnonzero(running):
                train_loss, val_loss = float(both[0, l]), float(both[1, l])
                train_losses[l].append(train_loss)
                val_losses[l].append(val_loss)
                epochs_run[l] = epoch
                if val_loss < best_val[l]:
                    patience[l], best_val[l], best_epoch[l] = 0, val_loss, epoch
                    improved.append(int(l))
                else:
                    patience[l] += 1
                    if val_loss > 0.8 or patience[l] == patience_threshold:
                        running[l] = False
            if improved:  # the best weights: a masked copy of the stacked tensors
                rows = torch.tensor(improved, dtype=torch.int64, device=dev)
                for dst, src in zip(self._best, self._params()):
                    dst.index_copy_(0, rows, src.index_select(0, rows))
            if not running.any():
                break
            active = torch.from_numpy(running.astype(np.uint8)).to(dev)
        L.check_async_faults()
        self.result = HomerTrainResult(train_losses, val_losses, best_epoch, best_val, epochs_run)
        if model_dir is not None:
            os.makedirs(model_dir, exist_ok=True)
            for l in range(n):
                torch.save(self.best_state_dict(l), os.path.join(model_dir, f"encoder_model_{l}.pt"))
        return self.result

    # ---- one learner, exported ----
    def _sd(self, tensors, l):
        if not 0 <= l < self.L:
            raise IndexError(f"HOMERPopulation: learner {l} of {self.L}")
        t = [x[l].detach().cpu().clone() for x in tensors]
        out = dict(zip(ENC_KEYS, t[:4]))
        out["action_emb.weight"] = torch.eye(self.action_dim, dtype=torch.float32)
        out.update(zip(CLS_KEYS, t[4:]))
        return out

    def state_dict(self, l):
        """learner l's current weights under the reference's keys, on the host"""
        return self._sd(self._host if self._p is None else self._p, l)

    def best_state_dict(self, l):
        """learner l's weights of its best validation epoch in train(); before train(), the current ones"""
        return self._sd(self._best, l) if self._best is not None else self.state_dict(l)

    def encoder(self, l, best=False):
        """learner l as a HOMEREncoder holding a copy of its current (or best) weights, ready for encode"""
        return HOMEREncoder(self.obs_dim, self.action_dim, self.latent_size, self.hidden_size,
                            state_dict=self.best_state_dict(l) if best else self.state_dict(l), device=self.device)

    # ---- the population in use: all learners over a set of observations per launch ----
    def _enc_weights(self, best):
        """(W1 [L, H, dO], b1 [L, H], W2 [L, nZ, H], b2 [L, nZ]) on the device: the current weights, or with `best` those of the best
        validation epoch of the last train() (before train(), the current ones: best_state_dict's rule)"""
        if self._host is None and self._p is None:  # homer.py:160-161 (a population is constructed with weights, so this never fires)
            raise ValueError("Model not initialized. Either train a new model for the encoder or load an existing one.")
        return (self._best if best and self._best is not None else self._params())[:4]

    def encode_device(self, x, return_logits=False, best=False):
        """x [N, dO] f32 / f16 on the device -> z [L, N] i32, with return_logits also the logits [L, N, nZ] f32, in ONE launch
        (offsim_encode_mlp_pop).  z[l] and logits[l] are encoder(l, best).encode_device(x)'s bit for bit."""
        W1, b1, W2, b2 = self._enc_weights(best)
        if x.dtype not in (torch.float32, torch.float16):
            x = x.to(torch.float32)
        x = x.contiguous()
        if x.dim() != 2 or x.shape[1] != self.obs_dim:
            raise ValueError(f"HOMERPopulation.encode_device: x must be [N, {self.obs_dim}], got {tuple(x.shape)}")
        N = x.shape[0]
        z = torch.empty((self.L, N), dtype=torch.int32, device=x.device)
        logits = torch.empty((self.L, N, self.latent_size), dtype=torch.float32, device=x.device) if return_logits else None
        L.check(L.load().offsim_encode_mlp_pop(L.ptr(x), L.F16 if x.dtype == torch.float16 else L.F32, N, self.obs_dim, L.ptr(W1), L.ptr(b1),
                                               self.hidden_size, L.ptr(W2), L.ptr(b2), self.latent_size, self.L, L.ptr(z), L.ptr(logits),
                                               L.stream_ptr()))
        return (z, logits) if return_logits else z

    def _observations_on_device(self, observations):
        """HOMEREncoder.encode's rule: float16 observations stay float16, everything else goes to float32; [N, dO], uploaded once"""
        dev = self._params()[0].device
        obs = observations if isinstance(observations, torch.Tensor) else np.asarray(observations)
        half = obs.dtype in (np.float16, torch.float16)
        if isinstance(obs, torch.Tensor):
            x = obs.to(device=dev, dtype=torch.float16 if half else torch.float32)
        else:
            x = torch.from_numpy(np.ascontiguousarray(obs, dtype=np.float16 if half else np.float32)).to(dev)
        self.last_input_dtype = x.dtype
        return x.reshape(x.shape[0], -1)

    def encode(self, observations, best=False):
        """every learner's HOMEREncoder.encode of the same observations: np.int64 [L, N], one upload and one launch"""
        return self.encode_device(self._observations_on_device(observations), best=best).cpu().numpy().astype(np.int64)

    def latent_counts(self, z, labels=None, n_labels=None):
        """offsim_latent_counts of z [L, N] i32 on the device (and labels [N] i32 in [0, n_labels)): (counts [L, nZ], joint [L, nZ, nY] or
        None, skipped [L]), i64 device tensors"""
        z = z.to(torch.int32).contiguous()
        n, N = z.shape
        if (labels is None) != (n_labels is None):
            raise ValueError("HOMERPopulation.latent_counts: labels and n_labels go together")
        nZ, nY = self.latent_size, 0 if labels is None else int(n_labels)
        if labels is not None:
            labels = labels.to(z.device, torch.int32).contiguous()
            if labels.shape != (N,) or nY < 1:
                raise ValueError(f"HOMERPopulation.latent_counts: labels must be [{N}] with n_labels >= 1, got {tuple(labels.shape)}, {nY}")
        counts = torch.empty((n, nZ), dtype=torch.int64, device=z.device)
        joint = None if labels is None else torch.empty((n, nZ, nY), dtype=torch.int64, device=z.device)
        skipped = torch.empty(n, dtype=torch.int64, device=z.device)
        L.check(L.load().offsim_latent_counts(L.ptr(z), n, N, nZ, L.ptr(labels), nY, L.ptr(counts), L.ptr(joint), L.ptr(skipped), L.stream_ptr()))
        return counts, joint, skipped

    def latent_report(self, observations, labels=None, n_labels=None, best=False):
        """What the L encoders make of a log (the reference looks at this with _visualize): LatentReport of device tensors, nothing read
        back.  z [L, N] i32; counts [L, nZ] i64 rows per latent state; used [L] the number of non-empty latent states; skipped [L] rows
        counted nowhere (a label outside [0, n_labels)); with labels [N] (the true state, say; n_labels = their number, by default
        max + 1 of labels given on the host) also joint [L, nZ, nY] and purity [L] f64 = sum_z max_y joint[l, z, y] / N, the share of rows
        whose label is the most frequent one of their latent state (1.0: every latent state holds one true state)."""
        z = self.encode_device(self._observations_on_device(observations), best=best)
        if labels is not None:
            if n_labels is None:
                if isinstance(labels, torch.Tensor) and labels.device.type != "cpu":
                    raise ValueError("HOMERPopulation.latent_report: give n_labels with labels on the device (no host read in here)")
                n_labels = int(np.asarray(labels).max()) + 1 if len(labels) else 1
            labels = labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(labels))
            labels = labels.reshape(-1)
        counts, joint, skipped = self.latent_counts(z, labels, n_labels if labels is not None else None)
        used, purity = latent_stats(counts, joint, z.shape[1])
        return LatentReport(z, counts, used, joint, purity, skipped)

    def evaluators(self, dataset, learners=None, best=False, cls=None):
        """[cls.from_latents(dataset, ...) for the chosen learners (default: all)], cls = PerStateRejectionSampling or a subclass:
        observations and next_observations are each uploaded once and encoded by all learners in one launch, where building
        cls(dataset, num_states, encoder=population.encoder(l)) per learner uploads and encodes both 2 L times."""
        if cls is None:
            from ..evaluators.per_state_rejection import PerStateRejectionSampling as cls
        learners = list(range(self.L)) if learners is None else [int(l) for l in learners]
        for l in learners:
            if not 0 <= l < self.L:
                raise IndexError(f"HOMERPopulation: learner {l} of {self.L}")
        e = dataset.experience
        zs, next_zs = self.encode(e["observations"], best=best), self.encode(e["next_observations"], best=best)
        return [cls.from_latents(dataset, zs[l], next_zs[l], self.latent_size) for l in learners]

    def best(self):
        """the learner with the lowest best_val_loss of the last train()"""
        if self.result is None:
            raise ValueError("HOMERPopulation.best: train() has not run")
        return int(np.argmin(self.result.best_val_loss))


__all__ = ["HOMERPopulation", "HomerTrainResult", "LatentReport", "epoch_draws", "latent_stats"]
