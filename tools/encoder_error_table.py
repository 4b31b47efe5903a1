"""How much of the encoder matrix's tolerance each kernel instance of offsim_encode_mlp uses: runs the case table of tests/encoder_host.py on
the device and writes one JSON line per instance (path, instance, dtype) -- the case of that instance with the largest measured
max |gpu - f64| / B, its shape, rho_ref and tolerance -- to profiles/encoder_instances_error.jsonl.

OFFSIM_ENCODER_F32 is read once per process, so the R instances come from a child process with the switch on (--f32-products)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def measure():
    import encoder_host as E
    from rl_offline_simulation_amd import _lib as L
    dev = torch.device("cuda", 0)
    lib = L.load()
    rows = {}
    for c in E.CASE_LIST:
        path, inst, lds = E.taken_path(c)
        if E.F32_PRODUCTS and path != "R":
            continue
        b = E.build(c.name)
        t = torch.from_numpy(np.array(b.x))
        if c.unaligned:
            flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
            xd = flat[1:].view(t.shape)
            xd.copy_(t)
        else:
            xd = t.to(dev)
        W1, b1, W2, b2 = (torch.from_numpy(np.array(a)).to(dev) for a in (b.W1, b.b1, b.W2, b.b2))
        z = torch.empty(c.N, dtype=torch.int32, device=dev)
        lg = torch.empty((c.N, c.nZ), dtype=torch.float32, device=dev)
        L.check(lib.offsim_encode_mlp(xd.data_ptr(), L.F16 if c.xdt == "f16" else L.F32, c.N, c.dO, W1.data_ptr(), b1.data_ptr(), c.H, W2.data_ptr(),
                                      b2.data_ptr(), c.nZ, z.data_ptr(), lg.data_ptr(), L.stream_ptr()))
        torch.cuda.synchronize()
        measured = float((np.abs(lg.cpu().numpy().astype(np.float64) - b.ref) / b.B).max())
        tol = E.tolerance(b, path)
        row = {"path": path, "instance": list(inst), "x_dtype": c.xdt, "case": c.name, "N": c.N, "dO": c.dO, "H": c.H, "nZ": c.nZ,
               "lds_bytes": lds, "rho_ref": b.rho_ref, "measured": measured, "tolerance": tol, "used": measured / tol, "cases": 1}
        key = (path, tuple(inst), c.xdt)
        if key in rows:
            row["cases"] = rows[key]["cases"] + 1
            if rows[key]["used"] >= row["used"]:
                rows[key]["cases"] = row["cases"]
                continue
        rows[key] = row
    return [rows[k] for k in sorted(rows)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encoder_instances_error.jsonl"))
    ap.add_argument("--f32-products", action="store_true", help="(child) print the R instances' lines and exit")
    a = ap.parse_args()
    if a.f32_products:
        for r in measure():
            print("ROW " + json.dumps(r))
        return
    rows = measure()
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--f32-products"], env=dict(os.environ, OFFSIM_ENCODER_F32="1"),
                           capture_output=True, text=True, timeout=900)
    if child.returncode != 0:
        raise SystemExit(child.stdout[-2000:] + child.stderr[-2000:])
    rows += [json.loads(line[4:]) for line in child.stdout.splitlines() if line.startswith("ROW ")]
    rows.sort(key=lambda r: ("SRGV".index(r["path"]), r["instance"], r["x_dtype"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    print(f"{len(rows)} instances -> {a.out}; largest share of the tolerance used: {max(r['used'] for r in rows):.3f}")


if __name__ == "__main__":
    main()
