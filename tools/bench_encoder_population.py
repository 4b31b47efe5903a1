#!/usr/bin/env python3
"""bench_encoder_population.py [--out profiles/encoder_population_bench.jsonl] -- one HOMERPopulation.encode_device call against the loop of
population.encoder(l).encode_device(x) per learner (the only route before offsim_encode_mlp_pop), on the same device observations.

L = 1 / 8 / 64; shapes 2-64-25 f32 (config C3) and 128-64-50 f16 (C5); N = 16 384 and 1 000 000.  Synchronised wall time of a whole route
(the loop's L launches, or the one population launch; the encoders of the loop are built beforehand, their weight copies are not timed),
medians of five after a warm-up, the two routes alternating.  One JSON line per configuration; the outputs of the two routes are compared
bit for bit before anything is timed."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("2-64-25 f32", 2, 64, 25, torch.float32), ("128-64-50 f16", 128, 64, 50, torch.float16))
LEARNERS = (1, 8, 64)
ROWS = (16_384, 1_000_000)
REPEATS = 5


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encoder_population_bench.jsonl"))
    args = ap.parse_args()
    from rl_offline_simulation_amd.encoders import HOMERPopulation
    dev = torch.device("cuda", 0)
    lines = []
    for name, dO, H, nZ, dtype in SHAPES:
        for N in ROWS:
            g = torch.Generator(device="cpu").manual_seed(N + dO)
            x = torch.randn((N, dO), generator=g).to(dev, dtype)
            for n in LEARNERS:
                pop = HOMERPopulation(dO, 5, nZ, H, seeds=list(range(n)), device=dev)
                encoders = [pop.encoder(l) for l in range(n)]
                one = lambda: pop.encode_device(x)  # noqa: E731
                loop = lambda: [e.encode_device(x) for e in encoders]  # noqa: E731
                assert torch.equal(one(), torch.stack(loop()))
                timed(one), timed(loop)
                t_pop, t_loop = [], []
                for _ in range(REPEATS):
                    t_loop.append(timed(loop))
                    t_pop.append(timed(one))
                rec = {"shape": name, "N": N, "L": n, "loop_ms": 1e3 * statistics.median(t_loop), "population_ms": 1e3 * statistics.median(t_pop),
                       "loop_ms_all": [1e3 * t for t in t_loop], "population_ms_all": [1e3 * t for t in t_pop]}
                rec["loop_over_population"] = rec["loop_ms"] / rec["population_ms"]
                rec["device"] = torch.cuda.get_device_name(0)
                print(json.dumps(rec), flush=True)
                lines.append(rec)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
