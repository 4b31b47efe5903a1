#!/usr/bin/env python3
"""The error table behind tests/test_gpu_true_env.py's CartPole tolerance: for every case of tests/true_env_host.py's CARTPOLE_CASES, run
VectorCartPole.collect on the device, redo every recorded step on the host in f64 from the device's own state and action
(true_env_host.cartpole_step), and write the largest deviation of the device's next_state, in units of eps * max(1, |value|), to
profiles/true_env_error.jsonl (one line per case).  The library is built without contraction, so only sin / cos (ocml on the device, libm
under NumPy) can differ.  The test allows 8 times the largest line, and never more than 1e-12 * max(1, |value|).

    python tools/true_env_error_table.py [--out profiles/true_env_error.jsonl]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import true_env_host as H  # noqa: E402
from test_gpu_true_env import run_cartpole_case  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "true_env_error.jsonl"))
    a = ap.parse_args()
    gpu = torch.device("cuda", 0)
    lines = []
    for case in H.CARTPOLE_CASES:
        env = run_cartpole_case(gpu, case)[0]
        rec = env.records
        dev = H.cartpole_deviation(rec.state.cpu().numpy(), env.drawn_action.cpu().numpy(), rec.next_state.cpu().numpy())
        lines.append({"what": "cartpole next_state", "case": {"E": case[0], "T": case[1], "max_episode_steps": case[2], "seed_base": case[3]},
                      "steps": case[0] * case[1], "max_dev_eps": dev, "unit": "eps(f64) * max(1, |value|)",
                      "device": torch.cuda.get_device_name(0)})
        print(lines[-1])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
