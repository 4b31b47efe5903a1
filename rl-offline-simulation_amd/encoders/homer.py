"""HOMEREncoder on the device (offsim4rl/encoders/homer.py, the model of offsim4rl/encoders/models.py).

encode (homer.py:159-168): forward of EncoderModel.obs_encoder + argmax.
train (homer.py:35-157): the reference's loop -- per batch _calc_loss, backward, clip_grad_norm_ and Adam as one offsim_homer_step
(csrc/homer_train.hpp), a whole epoch enqueued without a host round trip, one synchronisation per epoch for the early-stopping rule.
The Gumbel noise and the permutations are drawn with torch on the device and handed to the kernels, so a recorded run can be replayed
(loss_grad, train_epoch and eval_epoch take indices and noise).  Weights come from a reference state_dict (keys obs_encoder.0.weight /
.0.bias / .2.weight / .2.bias, and classifier.* when present) or from torch's default nn.Linear initialisation; state_dict() returns the
reference's key set, so EncoderModel.load reads a file saved from it.  Tensorboard, the plots and the per-10-epoch checkpoints stay out."""
import math
import os
from collections import namedtuple

import numpy as np
import torch

from .. import _lib as L

ENC_KEYS = ("obs_encoder.0.weight", "obs_encoder.0.bias", "obs_encoder.2.weight", "obs_encoder.2.bias")
CLS_KEYS = ("classifier.0.weight", "classifier.0.bias", "classifier.2.weight", "classifier.2.bias")
LEAKY_SLOPE = 0.01  # nn.LeakyReLU's default

HomerTrainResult = namedtuple("HomerTrainResult", "train_losses val_losses best_epoch best_val_loss epochs_run")


def gumbel_noise(M, nZ, device):
    """[M, 4, nZ] standard Gumbel draws, as F.gumbel_softmax draws them: -log(Exponential(1))"""
    return -torch.empty((M, 4, nZ), dtype=torch.float32, device=device).exponential_().log()


class HOMEREncoder:
    def __init__(self, obs_dim, action_dim, latent_size, hidden_size, model_path=None, state_dict=None, device=None):
        self.obs_dim, self.action_dim, self.latent_size, self.hidden_size = obs_dim, action_dim, latent_size, hidden_size
        self.device = device
        self.lr, self.weight_decay, self.max_grad_norm = 1e-3, 0.0, 40.0
        self._w = None       # the encoder's four tensors once loaded or trained: what encode runs
        self._p = None       # all eight tensors on the device (ENC_KEYS + CLS_KEYS), stepped in place by train
        self._opt = None     # Adam's m, v [P] f32 and t [1] i64
        self._work = None
        self._best = None
        self._host = None
        if model_path:
            state_dict = torch.load(model_path, map_location="cpu")
        if state_dict is not None:
            self.load_state_dict(state_dict)
        else:
            self._host = self._init_host()

    # ---- weights ----
    def _shapes(self):
        dO, nA, nZ, H = self.obs_dim, self.action_dim, self.latent_size, self.hidden_size
        return [(H, dO), (H,), (nZ, H), (nZ,), (H, 2 * nZ + nA), (H,), (2, H), (2,)]

    def _init_host(self):
        """torch's default initialisation under the current torch.manual_seed, the modules built in EncoderModel's order (encoder,
        action embedding, classifier), so a seed gives the weights it gives the reference"""
        dO, nA, nZ, H = self.obs_dim, self.action_dim, self.latent_size, self.hidden_size
        enc = [torch.nn.Linear(dO, H), torch.nn.Linear(H, nZ)]
        torch.nn.Embedding(nA, nA)
        cls = [torch.nn.Linear(2 * nZ + nA, H), torch.nn.Linear(H, 2)]
        return [t.detach().clone() for lin in enc + cls for t in (lin.weight, lin.bias)]

    def _params(self):
        """all eight tensors on the device.  A model loaded from an encoder-only dict gets its classifier here, at the first use that
        needs one (loading and encoding draw nothing from torch's generator)"""
        if self._p is None:
            dev = self.device or L.require_device()
            if self._host is None:
                self._host = self._init_host()
            self._p = [t.to(dev, torch.float32).contiguous() for t in self._host]
            if self._w is not None:
                self._p[:4] = list(self._w)
        return self._p

    def load_state_dict(self, sd):
        dev = self.device or L.require_device()
        get = lambda k: torch.as_tensor(np.asarray(sd[k]) if not isinstance(sd[k], torch.Tensor) else sd[k]).to(dev, torch.float32).contiguous()
        W1, b1, W2, b2 = get("obs_encoder.0.weight"), get("obs_encoder.0.bias"), get("obs_encoder.2.weight"), get("obs_encoder.2.bias")
        assert W1.shape == (self.hidden_size, self.obs_dim) and W2.shape == (self.latent_size, self.hidden_size)
        self._w = (W1, b1, W2, b2)
        self._opt = None
        if all(k in sd for k in CLS_KEYS):
            self._p = [W1, b1, W2, b2] + [get(k) for k in CLS_KEYS]
            for t, shape in zip(self._p, self._shapes()):
                assert tuple(t.shape) == shape, (tuple(t.shape), shape)
        elif self._p is not None:
            self._p[:4] = [W1, b1, W2, b2]

    def _sd(self, tensors):
        t = [x.detach().cpu().clone() for x in tensors]
        out = dict(zip(ENC_KEYS, t[:4]))
        out["action_emb.weight"] = torch.eye(self.action_dim, dtype=torch.float32)
        out.update(zip(CLS_KEYS, t[4:]))
        return out

    def state_dict(self):
        """the reference's EncoderModel.state_dict(): obs_encoder.*, action_emb.weight = eye(nA), classifier.*, on the host"""
        if self._p is None and self._w is None:
            return self._sd(self._host)
        return self._sd(self._params())

    def best_state_dict(self):
        """the weights of train()'s best validation epoch (the reference's best_model); before train(), the current ones"""
        return self._sd(self._best) if self._best is not None else self.state_dict()

    def save(self, model_path, best=False):
        torch.save(self.best_state_dict() if best else self.state_dict(), model_path)

    # ---- encode ----
    def encode_device(self, x, return_logits=False):
        if self._w is None:  # homer.py:160-161
            raise ValueError("Model not initialized. Either train a new model for the encoder or load an existing one.")
        W1, b1, W2, b2 = self._w
        if x.dtype not in (torch.float32, torch.float16):
            x = x.to(torch.float32)
        x = x.contiguous()
        N = x.shape[0]
        z = torch.empty(N, dtype=torch.int32, device=x.device)
        logits = torch.empty((N, self.latent_size), dtype=torch.float32, device=x.device) if return_logits else None
        L.check(L.load().offsim_encode_mlp(L.ptr(x), L.F16 if x.dtype == torch.float16 else L.F32, N, self.obs_dim, L.ptr(W1), L.ptr(b1),
                                           self.hidden_size, L.ptr(W2), L.ptr(b2), self.latent_size, L.ptr(z), L.ptr(logits), L.stream_ptr()))
        return (z, logits) if return_logits else z

    def encode(self, observations):
        """homer.py:159-168.  float16 observations (config C5) cross the PCIe bus as float16 and are widened by the kernel -- the
        reference's `.float()` (homer.py:163) is a cast on the device side too, and exact; every other dtype is cast to float32 on the
        host as before.  `last_input_dtype` records which instance of the kernel ran."""
        dev = self.device or L.require_device()
        obs = observations if isinstance(observations, torch.Tensor) else np.asarray(observations)
        half = obs.dtype in (np.float16, torch.float16)
        if isinstance(obs, torch.Tensor):
            x = obs.to(device=dev, dtype=torch.float16 if half else torch.float32)
        else:
            x = torch.from_numpy(np.ascontiguousarray(obs, dtype=np.float16 if half else np.float32)).to(dev)
        self.last_input_dtype = x.dtype
        return self.encode_device(x.reshape(x.shape[0], -1)).cpu().numpy().astype(np.int64)

    # ---- training ----
    @property
    def n_params(self):
        return L.homer_params(self.obs_dim, self.action_dim, self.latent_size, self.hidden_size)

    def _net(self):
        p = self._params()
        return L.HomerNet(*[L.ptr(t) for t in p], self.obs_dim, self.action_dim, self.latent_size, self.hidden_size, LEAKY_SLOPE, 0)

    def _scratch(self, dev):
        if self._work is None or self._work.device != dev:
            self._work = torch.empty(L.homer_work_doubles(self.n_params), dtype=torch.float64, device=dev)
        return self._work

    def reset_optimizer(self):
        """Adam's state back to zero (a new optimizer, as the reference's train() makes one per call)"""
        dev = self._params()[0].device
        P = self.n_params
        self._opt = (torch.zeros(P, dtype=torch.float32, device=dev), torch.zeros(P, dtype=torch.float32, device=dev),
                     torch.zeros(1, dtype=torch.int64, device=dev))
        return self._opt

    def adam_state(self):
        return self._opt or self.reset_optimizer()

    def upload(self, dataset):
        """(obs [n, dO] f32 / f16, act [n] i32, next_obs [n, dO]) on the device, from an (x, a, x_next) triple or anything with
        .x / .a / .x_next; tensors already there are taken as they are"""
        dev = self._params()[0].device
        x, a, xn = (dataset.x, dataset.a, dataset.x_next) if hasattr(dataset, "x_next") else dataset
        half = all(getattr(t, "dtype", None) in (np.float16, torch.float16) for t in (x, xn))

        def to_dev(t, dtype):
            t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
            return t.to(dev, dtype).contiguous()
        fd = torch.float16 if half else torch.float32
        x, xn = to_dev(x, fd), to_dev(xn, fd)
        x, xn = x.reshape(x.shape[0], -1), xn.reshape(xn.shape[0], -1)
        a = to_dev(a, torch.int32).reshape(-1)
        assert x.shape == xn.shape and x.shape[1] == self.obs_dim and a.shape[0] == x.shape[0]
        return x, a, xn

    def _batch(self, data, idx_real, idx_impo, noise):
        x, a, xn = data
        M = idx_real.shape[0]
        assert idx_real.dtype == torch.int32 and idx_impo.dtype == torch.int32 and idx_impo.shape[0] == M
        if noise is not None:
            assert noise.dtype == torch.float32 and tuple(noise.shape) == (M, 4, self.latent_size)
        return L.HomerBatch(L.ptr(x), L.ptr(xn), L.F16 if x.dtype == torch.float16 else L.F32, 0, L.ptr(a), x.shape[0], L.ptr(idx_real),
                            L.ptr(idx_impo), L.ptr(noise), M)

    def _idx(self, idx, dev):
        idx = idx if isinstance(idx, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(idx))
        return idx.to(dev, torch.int32).contiguous()

    def loss_grad(self, obs, act, next_obs, idx_real, idx_impo, noise=None, tau=1.0, hard=False):
        """One pass of _calc_loss over the records (idx_real[m], idx_impo[m], noise[m]): (loss, grad) as device tensors, grad [P] f32
        unclipped and flat in state_dict order (None with hard=True, which is forward only).  `last_n` holds the number of valid records."""
        data = self.upload((obs, act, next_obs))
        dev = data[0].device
        idx_real, idx_impo = self._idx(idx_real, dev), self._idx(idx_impo, dev)
        if noise is not None:
            noise = (noise if isinstance(noise, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(noise))).to(dev, torch.float32).contiguous()
        stats = torch.zeros(2, dtype=torch.float64, device=dev)
        grad = None if hard else torch.zeros(self.n_params, dtype=torch.float32, device=dev)
        net, bt = self._net(), self._batch(data, idx_real, idx_impo, noise)
        L.check(L.load().offsim_homer_grad(net, bt, float(tau), int(bool(hard)), L.ptr(grad), L.ptr(stats), L.ptr(self._scratch(dev)), L.stream_ptr()))
        self.last_n = stats[0]
        return stats[1], grad

    def _epoch(self, data, idx_real, idx_impo, batch_size, tau, noise, step):
        dev = data[0].device
        idx_real, idx_impo = self._idx(idx_real, dev), self._idx(idx_impo, dev)
        M = idx_real.shape[0]
        nb = (M + batch_size - 1) // batch_size
        stats = torch.zeros((max(nb, 1), 3), dtype=torch.float64, device=dev)
        lib, net, work, stream = L.load(), self._net(), self._scratch(dev), L.stream_ptr()
        if step:
            m, v, t = self.adam_state()
            adam = L.HomerAdam(L.ptr(m), L.ptr(v), L.ptr(t), float(self.lr), float(self.weight_decay))
        for b in range(nb):
            lo, hi = b * batch_size, min(M, (b + 1) * batch_size)
            g = noise[lo:hi] if noise is not None else gumbel_noise(hi - lo, self.latent_size, dev)
            bt = self._batch(data, idx_real[lo:hi], idx_impo[lo:hi], g)
            if step:
                L.check(lib.offsim_homer_step(net, bt, float(tau), float(self.max_grad_norm), adam, L.ptr(stats[b]), L.ptr(work), stream))
            else:
                L.check(lib.offsim_homer_grad(net, bt, 1.0, 1, None, L.ptr(stats[b]), L.ptr(work), stream))
        self.last_stats = stats[:nb]
        return stats[:nb, 1]

    def train_epoch(self, data, idx_real, idx_impo, batch_size, tau, noise=None):
        """One offsim_homer_step per batch of `batch_size` records (the short last batch included), all enqueued with no synchronisation;
        returns the per-batch losses as one device tensor.  data: upload()'s triple; noise [M, 4, nZ] or None: drawn per batch on the
        device.  lr, weight_decay and max_grad_norm are the attributes of that name; Adam's state carries over (reset_optimizer)."""
        if noise is not None:
            noise = noise.to(data[0].device, torch.float32).contiguous()
        return self._epoch(data, idx_real, idx_impo, batch_size, tau, noise, True)

    def eval_epoch(self, data, idx_real, idx_impo, batch_size, noise=None):
        """The validation pass (homer.py:108-113): discretized=True, temperature 1.0, no step; per-batch losses as one device tensor."""
        if noise is not None:
            noise = noise.to(data[0].device, torch.float32).contiguous()
        return self._epoch(data, idx_real, idx_impo, batch_size, 1.0, noise, False)

    def train(self, train_dataset, val_dataset, lr=1e-3, weight_decay=0.0, num_epochs=1000, batch_size=64, patience_threshold=50,
              temperature_decay=False, model_dir=None, model_name="encoder_model.pt", max_grad_norm=40.0, seed=None):
        """homer.py:35-157 with a fresh Adam: four fresh permutations per epoch (train real / impostor, val real / impostor), tau =
        max(0.5, exp(-0.005 epoch)) with temperature_decay, epoch losses the plain mean of the per-batch losses (the reference weights
        every batch by len(batch) = 2), best_val_loss from 0.69, stop at val_loss > 0.8 in a non-improving epoch or at the patience
        limit.  One host synchronisation per epoch.  Afterwards encode uses the last weights (the reference's self.model);
        best_state_dict() returns the best ones, which are saved to model_dir/model_name when model_dir is given."""
        if seed is not None:
            torch.manual_seed(seed)
        self.lr, self.weight_decay, self.max_grad_norm = lr, weight_decay, max_grad_norm
        tr, va = self.upload(train_dataset), self.upload(val_dataset)
        dev = tr[0].device
        self.reset_optimizer()
        n_tr, n_va = tr[0].shape[0], va[0].shape[0]
        best_val, best_epoch, patience = 0.69, -1, 0
        self._best = [t.clone() for t in self._params()]
        train_losses, val_losses, epoch = [], [], 0
        perm = lambda n: torch.randperm(n, device=dev).to(torch.int32)  # noqa: E731
        for epoch in range(1, num_epochs + 1):
            tau = max(0.5, math.exp(-0.005 * epoch)) if temperature_decay else 1.0
            lt = self.train_epoch(tr, perm(n_tr), perm(n_tr), batch_size, tau)
            lv = self.eval_epoch(va, perm(n_va), perm(n_va), batch_size)
            both = torch.stack([lt.mean() if lt.numel() else lt.sum(), lv.mean() if lv.numel() else lv.sum()]).cpu()  # the epoch's one synchronisation
            train_loss, val_loss = float(both[0]), float(both[1])
            train_losses.append(train_loss)
            val_losses.append(val_loss)
            if val_loss < best_val:
                patience, best_val, best_epoch = 0, val_loss, epoch
                for dst, src in zip(self._best, self._params()):
                    dst.copy_(src)
            else:
                patience += 1
                if val_loss > 0.8 or patience == patience_threshold:
                    break
        self._w = tuple(self._params()[:4])
        L.check_async_faults()
        if model_dir is not None:
            os.makedirs(model_dir, exist_ok=True)
            self.save(os.path.join(model_dir, model_name), best=True)
        return HomerTrainResult(train_losses, val_losses, best_epoch, best_val, epoch)
