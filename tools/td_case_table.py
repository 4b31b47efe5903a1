"""Writes profiles/td_instances.jsonl: one line per case of the learner-kernel matrix (tests/td_cases.py) -- the p_log instance, the
launch the restated LDS arithmetic gives it, and what the plain Python loop (tests/td_host.py) does in it: per-learner steps, episodes,
status and MT words consumed.  Needs no GPU.

    python tools/td_case_table.py [out.jsonl]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import td_cases as K  # noqa: E402


def main(path):
    with open(path, "w") as f:
        for c in K.CASES:
            waves, lds, refused = c.shape
            rec = dict(case=c.name, PL=c.table.pl, r_dtype=c.table.rd, N=c.table.N, n_slots=c.table.nS, nA=c.table.nA, R=c.R, waves=waves, lds_bytes=lds,
                       above_64k=lds > 64 * 1024, refused=refused)
            if not refused:
                outs = K.host(c)
                tot = lambda k: [int(sum(o[k][i] for o in outs)) for i in range(c.R)]  # noqa: E731
                rec.update(calls=len(outs), steps=tot("steps"), episodes=tot("n_ep"), status=[int(s) for s in outs[-1]["status"]], mt_words=tot("mt_words"))
            f.write(json.dumps(rec) + "\n")
    print(f"{len(K.CASES)} cases -> {path}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "td_instances.jsonl"))
