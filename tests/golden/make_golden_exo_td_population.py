#!/usr/bin/env python3
"""Generate tests/golden/exo_td_pop/*.npz by RUNNING THE REFERENCE's qlearn_psrs on its own PSRS_Exo with the behaviour policies that look
at Q (offsim4rl/evaluators/psrs.py:59-190, offsim4rl/agents/tabular.py:4-32).

Run from the repo root:   python tests/golden/make_golden_exo_td_population.py
Needs /root/reference (read-only) and NumPy; nothing of it is copied -- the fixtures hold inputs and the outputs the reference produced for
them.  Imported from the reference, by file path: offsim4rl/evaluators/psrs.py (PSRS_Exo, qlearn_psrs) and offsim4rl/agents/tabular.py
(greedy_policy, epsilon_greedy_policy, soft_greedy_policy).

Logs: the layouts exo_a_mod4 and exo_c_skewed of tests/golden/exo_drivers (the 2000 rows of exo_iid_2k.npz; their inputs are read from
those fixtures), sampler seeds 0 and 5.  Per log and seed, four runs until the log ends, np.random.seed(1234) before each:
  greedy    greedy_policy
  eps       epsilon_greedy_policy at epsilon = 0.3
  sched     epsilon_greedy_policy with epsilon(episode) = 1 / (1 + episode) and alpha(episode) = 0.5 / (1 + 0.1 episode)
  soft      soft_greedy_policy
and kept per run: Q, Gs, TD_errors, env.o, and np.random.get_state() afterwards (624 words + position).
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
SRC = os.path.join(ROOT, "tests", "golden", "exo_drivers")
OUT = os.path.join(ROOT, "tests", "golden", "exo_td_pop")
SEEDS = (0, 5)
GAMMA, ALPHA, EPSILON, NP_SEED = 0.9, 0.1, 0.3, 1234
eps_of = lambda e: 1.0 / (1.0 + e)  # noqa: E731
alpha_of = lambda e: 0.5 / (1.0 + 0.1 * e)  # noqa: E731


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


ref_psrs = _load("ref_psrs", os.path.join(REF, "offsim4rl/evaluators/psrs.py"))
ref_tab = _load("ref_tabular", os.path.join(REF, "offsim4rl/agents/tabular.py"))
RUNS = {"greedy": (ref_tab.greedy_policy, dict(alpha=ALPHA)), "eps": (ref_tab.epsilon_greedy_policy, dict(alpha=ALPHA, epsilon=EPSILON)),
        "sched": (ref_tab.epsilon_greedy_policy, dict(alpha=alpha_of, epsilon=eps_of)), "soft": (ref_tab.soft_greedy_policy, dict(alpha=ALPHA))}


def fixture(name):
    d = np.load(os.path.join(SRC, name + ".npz"))
    span, N, nO = int(d["span"]), len(d["in_o"]), int(d["nO"])
    buf = [(int(d["in_o"][i]), int(d["in_a"][i]), float(d["in_r"][i]), int(d["in_o_next"][i]), bool(d["in_done"][i]), np.array(d["in_p_log"][i]),
            {"t": 0 if d["in_t0"][i] else 1}) for i in range(N)]
    kw = dict(o_split_func=lambda o: (o // span, o % span), o_combine_func=lambda s, x: s * span + x)
    n_sched = int(d["in_t0"].sum()) + 1
    out = {k: d[k] for k in ("in_o", "in_a", "in_r", "in_o_next", "in_done", "in_p_log", "in_t0", "span", "nO")}
    out.update(gamma=np.float64(GAMMA), alpha=np.float64(ALPHA), epsilon=np.float64(EPSILON), np_seed=np.int64(NP_SEED), seeds=np.array(SEEDS, np.int64),
               alpha_ep=np.array([alpha_of(e) for e in range(n_sched)]), epsilon_ep=np.array([eps_of(e) for e in range(n_sched)]))
    np.random.seed(NP_SEED)
    fresh = np.random.get_state()
    open_episode = False
    for seed in SEEDS:
        for run, (policy, pkw) in RUNS.items():
            env = ref_psrs.PSRS_Exo(buf, nO=nO, nA=5, **kw)
            env.reset_sampler(seed=seed)
            np.random.seed(NP_SEED)
            Q, info = ref_psrs.qlearn_psrs(env, 10 ** 9, policy, GAMMA, **pkw)
            st = np.random.get_state()
            moved = st[2] != fresh[2] or not np.array_equal(st[1], fresh[1])
            if run != "soft":  # a run from Q = 0 ties at its first step
                assert moved, (name, seed, run, "the global stream did not advance")
            # exhaustion with an open episode: the last return belongs to an episode that did not end (its last accepted row is not done)
            open_episode |= len(info["memory"]) > 0 and not bool(info["memory"][-1][4])
            k = f"s{seed}_{run}_"
            out.update({k + "Q": Q, k + "Gs": info["Gs"], k + "td": info["TD_errors"], k + "o": np.int64(env.o),
                        k + "mt": np.concatenate([np.asarray(st[1], np.uint32), np.array([st[2]], np.uint32)])})
            print(f"{name:14s} seed {seed} {run:6s} steps {len(info['TD_errors']):5d} episodes {len(info['Gs']):4d} mt position {st[2]}")
    assert open_episode, (name, "no run ends by exhaustion with an open episode")
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)


def main():
    for name in ("exo_a_mod4", "exo_c_skewed"):
        fixture(name)
    print("done")


if __name__ == "__main__":
    sys.exit(main())
