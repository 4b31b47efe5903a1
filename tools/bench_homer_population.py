"""One epoch of HOMER encoder training for L encoders: HOMERPopulation.train_epoch (one offsim_homer_step_pop per batch for all learners)
against the same L encoders trained one after another through HOMEREncoder.train_epoch, the route of before, in the same process.

Both routes draw what they need inside the timed region: the population its epoch_draws (two [L, rows] index arrays and the epoch's
noise, from one device generator, as HOMERPopulation.train does), the loop two device permutations per encoder and the noise per batch
(as HOMEREncoder.train does).  One warm-up epoch of each route, then `--reps` epochs of each, alternating, each bracketed by
torch.cuda.synchronize(); median, min and max per route.  One JSON line per L, appended to --out.

One invocation measures one (shape, batch size); run each under its own time limit and chain them:

  timeout -k 10 400 python tools/bench_homer_population.py --dims 2 5 25 64 --batch 64 && \\
  timeout -k 10 400 python tools/bench_homer_population.py --dims 128 5 50 64 --batch 64 && \\
  timeout -k 10 400 python tools/bench_homer_population.py --dims 2 5 25 64 --batch 4096

--out defaults to profiles/homer_population_bench.jsonl."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rl_offline_simulation_amd.encoders import HOMEREncoder, HOMERPopulation, epoch_draws  # noqa: E402


def timed_once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def summary(ts):
    return round(statistics.median(ts), 3), [round(min(ts), 3), round(max(ts), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs=4, default=[2, 5, 25, 64], metavar=("dO", "nA", "nZ", "H"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--learners", type=int, nargs="+", default=[1, 8, 32, 64])
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "homer_population_bench.jsonl"),
                    help="the file the JSON lines are appended to")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    dO, nA, nZ, H = a.dims
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.random((a.rows, dO)).astype(np.float32)).to(dev)
    act = torch.from_numpy(rng.integers(0, nA, a.rows).astype(np.int32)).to(dev)
    xn = (x + 0.05 * torch.randn_like(x)).contiguous()
    nb = (a.rows + a.batch - 1) // a.batch
    for n in a.learners:
        seeds = list(range(n))
        pop = HOMERPopulation(dO, nA, nZ, H, seeds=seeds)
        pop.reset_optimizer()
        data = pop.upload((x, act, xn))
        gen = torch.Generator(device=dev)
        gen.manual_seed(0)
        encs = []
        for s in seeds:
            torch.manual_seed(s)
            encs.append(HOMEREncoder(dO, nA, nZ, H))
            encs[-1].reset_optimizer()
        perm = lambda: torch.randperm(a.rows, device=dev).to(torch.int32)  # noqa: E731

        def pop_epoch():
            ir, ii, nz = epoch_draws(gen, n, a.rows, nZ)
            pop.train_epoch(data, ir, ii, a.batch, 1.0, noise=nz)

        def loop_epoch():
            for enc in encs:
                enc.train_epoch(data, perm(), perm(), a.batch, 1.0)

        pop_epoch(), loop_epoch()  # warm-up
        tp, tl = [], []
        for _ in range(a.reps):
            tp.append(timed_once(pop_epoch))
            tl.append(timed_once(loop_epoch))
        (pm, pr), (lm, lr) = summary(tp), summary(tl)
        line = dict(bench="homer_population", dims=[dO, nA, nZ, H], rows=a.rows, batch=a.batch, batches=nb, L=n, reps=a.reps,
                    epoch_population_ms=pm, epoch_population_min_max_ms=pr, epoch_loop_ms=lm, epoch_loop_min_max_ms=lr,
                    batch_population_ms=round(pm / nb, 4), loop_over_population=round(lm / pm, 2), device=torch.cuda.get_device_name(0))
        print(json.dumps(line), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        del pop, encs


if __name__ == "__main__":
    main()
