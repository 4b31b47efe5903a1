#!/usr/bin/env python3
"""Row-policy evalMC (a policy over observations) on the device: one JSON line per shape.

  C2  cartpole_log 1 M rows x 4096 seeds, 162 box states (CartpoleBoxEncoder)
  C3  grid_coords_log_fast 10 M rows x 512 seeds, 25 states from the HOMER-shaped encoder weights of synth.grid_cell_encoder_weights

Policy: a 2 x 64 tanh MLP (nn.Linear's default init, seeded) over the raw observation -- spinup's MLPCategoricalActor shape.
Every line carries
  forward_s        both per-row tables (P_next at next_obs of every grouped row, P_init at obs of every initial row) by offsim_policy_mlp
  scan_s           the row-policy scan (offsim_eval_mc_rows_policy) over all seeds, summed over tiles (sampler resets not included)
  steps_per_s      accepted steps of that scan / scan_s
  tab_scan_s       the tabular generic kernel (offsim_eval_mc) on the same table and seeds with a tabular policy
  rows_tab_scan_s  the row-policy scan fed P built from that same tabular policy: the same work as tab_scan_s, so
                   rows_tab_scan_s / tab_scan_s is the cost of the mode itself
  parity_ok        the host restatement (tests/obs_policy_host.py) fed the device's own P tables reproduces the first seeds' returns,
                   episode counts and steps (2 seeds for C2, 1 for C3)

Usage: python tools/bench_obs_policy.py [--shapes C2,C3] [--seeds-c2 4096] [--seeds-c3 512] [--parity-seeds-c2 2] [--parity-seeds-c3 1]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_log(shape, dev):
    from rl_offline_simulation_amd import synth
    from rl_offline_simulation_amd.encoders import CartpoleBoxEncoder, HOMEREncoder
    if shape == "C2":
        e = synth.cartpole_log(1_000_000, seed=0)
        enc = CartpoleBoxEncoder()
        nS = 162
    else:
        e = synth.grid_coords_log_fast(10_000_000, seed=0)
        W1, b1, W2, b2 = (torch.from_numpy(w) for w in synth.grid_cell_encoder_weights(5, 64, seed=0))
        enc = HOMEREncoder(2, 5, 25, 64, state_dict={"obs_encoder.0.weight": W1, "obs_encoder.0.bias": b1,
                                                      "obs_encoder.2.weight": W2, "obs_encoder.2.bias": b2}, device=dev)
        nS = 25
    e["z"], e["z_next"] = enc.encode(e["observations"]), enc.encode(e["next_observations"])
    return e, nS


def sync():
    torch.cuda.synchronize()


def run_shape(shape, n_seeds, n_parity, dev):
    from rl_offline_simulation_amd import _lib as L, synth
    from rl_offline_simulation_amd.evaluators import BatchedPSRS, MLPPolicy
    from rl_offline_simulation_amd.evaluators.batched import resident_rollouts
    from rl_offline_simulation_amd.table import TransitionTable
    import obs_policy_host as H

    e, nS = make_log(shape, dev)
    t0 = e["steps"] == 0
    table = TransitionTable(e["z"], e["actions"], e["rewards"], e["z_next"], e["terminals"], e["action_distributions"], t0)
    dO, nA = e["observations"].shape[1], table.nA
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(dO, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, nA))
    pol = MLPPolicy.from_torch(net)
    obs_d = torch.from_numpy(e["observations"]).to(dev)
    nobs_d = torch.from_numpy(e["next_observations"]).to(dev)
    pol.row_tables(table, obs_d, nobs_d)  # (warm-up)
    sync()
    fw = []
    for _ in range(3):
        t = time.perf_counter()
        p_next, p_init = pol.row_tables(table, obs_d, nobs_d)
        sync()
        fw.append(time.perf_counter() - t)
    forward_s = float(np.median(fw))

    pi_tab = synth.dirichlet_policy(table.n_slots, nA, seed=9)
    pis = torch.from_numpy(table.policy_slots(pi_tab)).to(dev)
    tab_next, tab_init = pis[table.z_next.to(torch.int64)].contiguous(), pis[table.init_slot.to(torch.int64)].contiguous()

    seeds = np.arange(n_seeds, dtype=np.uint64)
    tile = int(max(1, min(n_seeds, resident_rollouts(table, keyed=False)[0])))
    res = {"rows": [0.0, 0, None], "rows_tab": [0.0, 0, None], "tab": [0.0, 0, None]}
    env = None
    for b in range(0, n_seeds, tile):
        sd = seeds[b:b + tile]
        if env is None or env.R != len(sd):
            env = BatchedPSRS(table, len(sd))
        for kind in ("rows", "rows_tab", "tab"):
            env.reset_sampler(sd)
            env._orders_for_generic()
            sync()
            t = time.perf_counter()
            if kind == "rows":
                o = env.eval_mc_rows_policy(p_next, p_init, 0.99)
            elif kind == "rows_tab":
                o = env.eval_mc_rows_policy(tab_next, tab_init, 0.99)
            else:
                o = env.eval_mc(pis, 0.99, fast=False)
            sync()
            res[kind][0] += time.perf_counter() - t
            res[kind][1] += int(o["steps"].sum())
            if res[kind][2] is None:
                res[kind][2] = {k: o[k][:n_parity].cpu().numpy() for k in ("sum_g", "n_ep", "steps", "status")}
            L.check_async_faults()
    if int(res["rows_tab"][1]) != int(res["tab"][1]):
        raise SystemExit("row mode fed the tabular policy took a different number of steps than the tabular kernel")

    # parity: the host restatement fed the device's own tables (caller order)
    order, init = table.order.cpu().numpy(), table.init_orig.cpu().numpy()
    P_next = np.zeros((table.N, nA), np.float32)
    P_init = np.zeros_like(P_next)
    P_next[order] = p_next.cpu().numpy()
    P_init[init] = p_init.cpu().numpy()
    first = res["rows"][2]
    ok = True
    for i in range(n_parity):
        h = H.evalmc_rows(e["z"], e["actions"], e["rewards"].astype(np.float64), e["z_next"], e["terminals"], e["action_distributions"], t0, P_next, P_init,
                          seed=int(seeds[i]), gamma=0.99)
        sg = 0.0
        for G in h["Gs"]:
            sg += G
        ok &= bool(first["sum_g"][i] == sg and first["n_ep"][i] == len(h["Gs"]) and first["steps"][i] == len(h["rows"]))
    scan_s, steps = res["rows"][0], res["rows"][1]
    return dict(shape=shape, N=int(table.N), seeds=int(n_seeds), tile=tile, n_states=int(table.n_slots), nA=int(nA), policy="mlp 2x64 tanh",
                forward_s=round(forward_s, 6), scan_s=round(scan_s, 4), steps=int(steps), steps_per_s=float(f"{steps / scan_s:.4g}"),
                tab_scan_s=round(res["tab"][0], 4), rows_tab_scan_s=round(res["rows_tab"][0], 4),
                mode_cost_ratio=round(res["rows_tab"][0] / res["tab"][0], 4), scan_ratio_vs_tab=round(scan_s / res["tab"][0], 4),
                forward_frac_of_scan=round(forward_s / scan_s, 6), parity_seeds=int(n_parity), parity_ok=bool(ok))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C2,C3")
    ap.add_argument("--seeds-c2", type=int, default=4096)
    ap.add_argument("--seeds-c3", type=int, default=512)
    ap.add_argument("--parity-seeds-c2", type=int, default=2)
    ap.add_argument("--parity-seeds-c3", type=int, default=1)
    a = ap.parse_args()
    from rl_offline_simulation_amd import _lib as L
    dev = L.require_device()
    for shape in a.shapes.split(","):
        n = a.seeds_c2 if shape == "C2" else a.seeds_c3
        p = a.parity_seeds_c2 if shape == "C2" else a.parity_seeds_c3
        print(json.dumps(run_shape(shape, n, p, dev)), flush=True)


if __name__ == "__main__":
    main()
