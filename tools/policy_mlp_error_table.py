"""How much of its bound every case of the k_policy_mlp matrix uses: runs the case table of tests/policy_mlp_host.py on the device through
the C ABI and writes one JSON line per case to profiles/policy_mlp_instances_error.jsonl -- the name and the instance, the chunk lists and
the LDS bytes, max |gpu - f64| / bound (the worst learner of a population), the same ratio for the NumPy f32 emulation, and for each mutant
of the emulation that is pinned on this case its ratio."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _gpu_ratio(P, L, b, dev):
    c = b.case
    n_l, n = len(b.weights), len(b.weights[0])
    x = torch.from_numpy(np.array(b.x)).to(dev)
    rows = None if b.rows is None else torch.from_numpy(np.array(b.rows)).to(dev)
    keep, arr = [], (L.MLPLayer * n)()
    for l in range(n):
        W = torch.from_numpy(np.stack([w[l][0] for w in b.weights])).to(dev).contiguous()
        bias = None if b.weights[0][l][1] is None else torch.from_numpy(np.stack([w[l][1] for w in b.weights])).to(dev).contiguous()
        keep += [W, bias]
        arr[l].W, arr[l].b, arr[l].out = L.ptr(W), L.ptr(bias), int(W.shape[1])
        setattr(arr[l], "in", int(W.shape[2]))
    out = torch.empty((n_l, c.M) if c.value else (n_l, c.M, c.sizes[-1]), dtype=torch.float32, device=dev)
    args = (L.ptr(x), L.F16 if c.xdt == "f16" else L.F32, c.n_x, c.sizes[0], L.ptr(rows), c.M, arr, n, P.ACT[c.act], c.slope)
    lib = L.load()
    if c.L:
        L.check(lib.offsim_policy_mlp_pop(*args, c.L, L.ptr(out), L.stream_ptr()))
    else:
        L.check((lib.offsim_value_mlp if c.value else lib.offsim_policy_mlp)(*args, L.ptr(out), L.stream_ptr()))
    torch.cuda.synchronize()
    L.check_async_faults()
    got = out.cpu().numpy()
    return max(P.ratio(got[l], b.ref[l], b.bound[l], b.valid) for l in range(n_l))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_mlp_instances_error.jsonl"))
    a = ap.parse_args()
    import policy_mlp_host as P
    from rl_offline_simulation_amd import _lib as L
    dev = torch.device("cuda", 0)
    lines = []
    for c in P.CASE_LIST:
        b = P.build(c.name)
        row = {"case": c.name, "instance": c.inst, "sizes": list(c.sizes), "activation": c.act, "M": c.M, "learners": max(c.L, 1),
               "chunks": b.shape.chunks, "lds_bytes": b.shape.lds_bytes, "gpu_over_bound": _gpu_ratio(P, L, b, dev),
               "emulation_over_bound": max(P.ratio(P.emulate_f32(b, None, l), b.ref[l], b.bound[l], b.valid) for l in range(max(c.L, 1))),
               "mutants_over_bound": {m: P.ratio(P.emulate_f32(b, m, l), b.ref[l], b.bound[l], b.valid)
                                      for m, (name, l) in P.MUTANT_CASE.items() if name == c.name}}
        lines.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in lines:
            f.write(json.dumps(r).replace("Infinity", '"inf"') + "\n")
    worst = max(lines, key=lambda r: r["gpu_over_bound"])
    print(f"{len(lines)} cases -> {a.out}; largest share of a bound used on the device: {worst['gpu_over_bound']:.4f} ({worst['case']})")


if __name__ == "__main__":
    main()
