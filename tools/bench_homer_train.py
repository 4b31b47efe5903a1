"""One epoch of HOMER encoder training on the device (HOMEREncoder.train_epoch: offsim_homer_step per batch) against the reference-shaped
torch loop on the same device, in the same process.

The torch loop is the same model in torch (Linear -> LeakyReLU -> Linear encoder and classifier, a one-hot action), F.gumbel_softmax
twice per gen_log_prob as the reference calls it, autograd, clip_grad_norm_(40) and optim.Adam, over batches gathered from device tensors
by the same kind of permutations (no DataLoader: its host-side collation would only add to the torch side).  Both routes draw their own
noise on the device.  Per (shape, batch size) one JSON line: ms per epoch and per batch for both routes and their ratio.  Timing: one
warm-up epoch, then the median of `--reps` epochs, each bracketed by torch.cuda.synchronize().

usage: python tools/bench_homer_train.py [--rows 16384] [--reps 5] [--out profiles/homer_train_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rl_offline_simulation_amd.encoders import HOMEREncoder  # noqa: E402


def timed(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts), min(ts), max(ts)


class TorchModel(torch.nn.Module):
    def __init__(self, dO, nA, nZ, H):
        super().__init__()
        self.nA = nA
        self.obs_encoder = torch.nn.Sequential(torch.nn.Linear(dO, H), torch.nn.LeakyReLU(), torch.nn.Linear(H, nZ))
        self.classifier = torch.nn.Sequential(torch.nn.Linear(2 * nZ + nA, H), torch.nn.LeakyReLU(), torch.nn.Linear(H, 2))

    def log_prob(self, prev, act, cur, tau):
        pz = F.gumbel_softmax(self.obs_encoder(prev), tau=tau)
        cz = F.gumbel_softmax(self.obs_encoder(cur), tau=tau)
        return F.log_softmax(self.classifier(torch.cat([pz, F.one_hot(act, self.nA).float(), cz], dim=1)), dim=1)


def torch_epoch(model, opt, x, a, xn, batch):
    n = x.shape[0]
    pr, pi = torch.randperm(n, device=x.device), torch.randperm(n, device=x.device)
    for lo in range(0, n, batch):
        i, j = pr[lo:lo + batch], pi[lo:lo + batch]
        obs, act = x[i], a[i]
        ones = torch.ones(len(i), dtype=torch.long, device=x.device)
        loss = (F.nll_loss(model.log_prob(obs, act, xn[i], 1.0), ones) + F.nll_loss(model.log_prob(obs, act, xn[j], 1.0), 0 * ones)) / 2
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 40)
        opt.step()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []
    for dO, nA, nZ, H in ((2, 5, 25, 64), (128, 5, 50, 64)):
        rng = np.random.default_rng(0)
        x = torch.from_numpy(rng.random((a.rows, dO)).astype(np.float32)).to(dev)
        act = torch.from_numpy(rng.integers(0, nA, a.rows).astype(np.int32)).to(dev)
        xn = (x + 0.05 * torch.randn_like(x)).contiguous()
        for batch in (64, 4096):
            torch.manual_seed(0)
            enc = HOMEREncoder(dO, nA, nZ, H)
            enc.reset_optimizer()
            data = enc.upload((x, act, xn))
            perm = lambda: torch.randperm(a.rows, device=dev).to(torch.int32)  # noqa: E731
            dev_ms = timed(lambda: enc.train_epoch(data, perm(), perm(), batch, 1.0), a.reps)
            model = TorchModel(dO, nA, nZ, H).to(dev)
            opt = torch.optim.Adam(model.parameters(), lr=1e-3)
            act64 = act.long()
            torch_ms = timed(lambda: torch_epoch(model, opt, x, act64, xn, batch), a.reps)
            nb = (a.rows + batch - 1) // batch
            line = dict(bench="homer_train", dims=[dO, nA, nZ, H], rows=a.rows, batch=batch, batches=nb, reps=a.reps,
                        epoch_device_ms=round(dev_ms[0], 3), epoch_device_min_max_ms=[round(dev_ms[1], 3), round(dev_ms[2], 3)],
                        epoch_torch_ms=round(torch_ms[0], 3), epoch_torch_min_max_ms=[round(torch_ms[1], 3), round(torch_ms[2], 3)],
                        batch_device_ms=round(dev_ms[0] / nb, 4), batch_torch_ms=round(torch_ms[0] / nb, 4),
                        torch_over_device=round(torch_ms[0] / dev_ms[0], 2), device=torch.cuda.get_device_name(0))
            print(json.dumps(line), flush=True)
            lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
