#!/usr/bin/env python3
"""The lines of profiles/true_env_error.jsonl behind tests/test_gpu_latent_env.py's CartPole tolerance, by tools/true_env_error_table.py's
method: for every traced case of that test (CartPole behind the box encoder, caps CARTPOLE_BOX_CAPS, the test's seeds, epsilon-greedy
Q-learners in k_eval_env_latent), redo every traced step on the host in f64 from the device's own traced state and action
(true_env_host.cartpole_step) and record the largest deviation of the device's next_state, in units of eps * max(1, |value|).  The kernel
calls the same env_step as VectorCartPole.collect, so the lines carry the same `what` and enter the same rule: the tests allow 8 times the
largest line, never more than 1e-12 * max(1, |value|).  The lines are APPENDED (earlier lines of this kernel are replaced; the other
tool's lines stay).

    python tools/latent_env_error_table.py [--out profiles/true_env_error.jsonl]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_gpu_latent_env import CARTPOLE_BOX_CAPS, SEEDS, case_deviation, run_cartpole_box_case  # noqa: E402

KERNEL = "k_eval_env_latent"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "true_env_error.jsonl"))
    a = ap.parse_args()
    gpu = torch.device("cuda", 0)
    kept = []
    if os.path.exists(a.out):
        kept = [x for x in (json.loads(ln) for ln in open(a.out) if ln.strip()) if x.get("kernel") != KERNEL]
    lines = []
    for cap in CARTPOLE_BOX_CAPS:
        host_o = run_cartpole_box_case(gpu, cap)[0]
        dev = max(case_deviation(host_o, i) for i in range(len(SEEDS)))
        lines.append({"what": "cartpole next_state", "kernel": KERNEL,
                      "case": {"S": len(SEEDS), "episodes": 4, "max_episode_steps": cap, "seeds": list(SEEDS), "encoder": "box"},
                      "steps": int(host_o["steps"].sum()), "max_dev_eps": dev, "unit": "eps(f64) * max(1, |value|)",
                      "device": torch.cuda.get_device_name(0)})
        print(lines[-1])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for ln in kept + lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
