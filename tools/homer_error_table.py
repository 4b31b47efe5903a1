"""How much of its bound each group of the HOMER training matrix uses: prints the table of profiles/homer_instances_error.jsonl, the lines
tests/test_gpu_homer_matrix.py::test_grad_case writes on a device when OFFSIM_HOMER_ERROR_JSONL names a file:

    OFFSIM_HOMER_ERROR_JSONL=$PWD/profiles/homer_instances_error.jsonl python -m pytest tests/test_gpu_homer_matrix.py -k test_grad_case

(the test appends: remove the file first).  Per group -- the matrix, and the edges by what they pin -- the number of cases, the tile sizes
run, the worst err / bound with its case, and the worst per-tensor relative error; then the same per tile size."""
import argparse
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def group_of(row):
    if row["group"] == "matrix":
        return "matrix, " + row["x_dtype"]
    return re.sub(r"-M\d+(-f16)?$", "", row["case"])


def table(rows, key, title):
    groups = {}
    for r in rows:
        groups.setdefault(key(r), []).append(r)
    print(f"| {title} | cases | TM | LDS bytes | worst err / bound | case | worst tensor rel. err |")
    print("|---|---|---|---|---|---|---|")
    for g, rs in groups.items():
        w = max(rs, key=lambda r: r["ratio"])
        t = max(rs, key=lambda r: r["worst_tensor_rel"])
        tms = ", ".join(str(v) for v in sorted({r["TM"] for r in rs}))
        lds = sorted({r["lds_bytes"] for r in rs})
        lds = f"{lds[0]}" if len(lds) == 1 else f"{lds[0]}..{lds[-1]}"
        print(f"| {g} | {len(rs)} | {tms} | {lds} | {w['ratio']:.3f} | {w['case']} | {t['worst_tensor_rel']:.1e} ({t['worst_tensor']}) |")
    print()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--file", default=os.path.join(ROOT, "profiles", "homer_instances_error.jsonl"))
    a = ap.parse_args()
    with open(a.file) as f:
        rows = [json.loads(line) for line in f if line.strip()]
    table(rows, group_of, "group")
    table(sorted(rows, key=lambda r: r["TM"]), lambda r: f"TM = {r['TM']}", "tile")
    worst = max(rows, key=lambda r: r["ratio"])
    print(f"{len(rows)} cases; largest err / bound {worst['ratio']:.3f} ({worst['case']}); largest loss err / bound "
          f"{max(r['loss_err'] / r['loss_bound'] for r in rows):.3f}; every n exact")


if __name__ == "__main__":
    main()
