#!/usr/bin/env python3
"""Generate tests/golden/exo_drivers/*.npz by RUNNING THE REFERENCE's PSRS_Exo under its own drivers (offsim4rl/evaluators/psrs.py:59-271).

Run from the repo root:   python tests/golden/make_golden_exo_drivers.py
Needs /root/reference (read-only); nothing of it is copied -- the fixtures hold inputs and the outputs the reference produced for them.
Imported from the reference, by file path: offsim4rl/evaluators/psrs.py (PSRS_Exo, evalMC_psrs, qlearn_psrs, expSARSA_psrs) and
offsim4rl/agents/tabular.py (uniformly_random_policy).

Every fixture holds the 2000 rows of iid_2k (as tests/golden/exo_iid_2k.npz keeps them) with an exogenous x added:
  exo_a_mod4      o = 4 s + x, x uniform over 4 values -- the layout of exo_iid_2k.npz itself
  exo_b_default   the constructor's default split and combine: o = s, one x-queue
  exo_c_skewed    o = 3 s + x with a skewed x (a rare value with a short queue) and three initial rows
and, per sampler seed in (0, 5, 7): evalMC_psrs until exhaustion (Gs, lengths, accepted s-rows and x-rows, env.o, how it ended), evalMC_psrs
with n_episodes = 2, qlearn_psrs with uniformly_random_policy (Q, Gs, TD_errors, and Qs of a save_Q = 1 run for the first 8 steps) and
expSARSA_psrs (Q, Gs).  The endings the fixtures must cover between them are asserted below.
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "exo_drivers")
SEEDS = (0, 5, 7)
GAMMA, ALPHA = 0.9, 0.1
END_S_EMPTY, END_X_EMPTY, END_NO_INIT, END_EPISODES = 0, 1, 2, 3  # how evalMC_psrs ended: s-queue empty, x-queue empty with s rows left, no initial row


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


ref_psrs = _load("ref_psrs", os.path.join(REF, "offsim4rl/evaluators/psrs.py"))
ref_tab = _load("ref_tabular", os.path.join(REF, "offsim4rl/agents/tabular.py"))

SPLITS = {  # name -> (span, split, combine); span 0: the constructor's defaults
    "mod4": (4, lambda o: (o // 4, o % 4), lambda s, x: s * 4 + x),
    "mod3": (3, lambda o: (o // 3, o % 3), lambda s, x: s * 3 + x),
    "default": (0, None, None),
}


def fixture(name, split_name, s, s_next, x, x_next, a, r, done, p_log, t0, pi_s, write=True):
    span, split, combine = SPLITS[split_name]
    N = len(s)
    o = s * span + x if span else s.copy()
    o_next = s_next * span + x_next if span else s_next.copy()
    xs = x if span else np.zeros(N, np.int64)
    nO = 25 * max(span, 1)
    p_rows = [np.array(p_log[i]) for i in range(N)]
    pid = {(p_rows[i].tobytes(), int(a[i]), float(r[i])): i for i in range(N)}  # PSRS_Exo deep-copies its buffer: rows are known by content
    assert len(pid) == N
    buf = [(int(o[i]), int(a[i]), float(r[i]), int(o_next[i]), bool(done[i]), p_rows[i], {"t": 0 if t0[i] else 1}) for i in range(N)]
    kw = {} if not span else dict(o_split_func=split, o_combine_func=combine)
    sp = split if span else (lambda ob: (ob, 0))
    pi = np.repeat(pi_s, max(span, 1), axis=0)  # pi[o] = the policy of exo_iid_2k.npz at the s of o
    out = dict(in_o=o, in_a=a, in_r=r, in_o_next=o_next, in_done=done, in_p_log=p_log, in_t0=t0, split=np.array(split_name), span=np.int64(span),
               nO=np.int64(nO), pi=pi, gamma=np.float64(GAMMA), alpha=np.float64(ALPHA), seeds=np.array(SEEDS, np.int64))
    endings, episodes = [], []
    for seed in SEEDS:
        env = ref_psrs.PSRS_Exo(buf, nO=nO, nA=5, **kw)
        rows_s, rows_x = [], []
        orig_step = env.step

        def step(p_new):
            _, xv = sp(env.o)
            res = orig_step(p_new)
            if res[0] is not None:
                rows_s.append(pid[(np.asarray(res[3]["p"]).tobytes(), int(res[3]["a"]), float(res[1]))])
                rows_x.append(order_x[xv][len(order_x[xv]) - len(env.x_queues[xv]) - 1])  # the x-element popped with the accepted s-element
            return res
        env.step = step

        def fresh():
            env.reset_sampler(seed=seed)
            rows_s.clear()
            rows_x.clear()
        # the x-queues' row order: the rows of every x value in buffer order under the shuffle reset_sampler applies (psrs.py:83, :88-89)
        order_x = {}
        for v in np.unique(xs):
            rows = [int(i) for i in np.flatnonzero(xs == v)]
            np.random.default_rng(seed).shuffle(rows)
            order_x[int(v)] = rows
        k = f"s{seed}_"
        fresh()
        Gs, lengths = ref_psrs.evalMC_psrs(env, 10 ** 9, pi, GAMMA)
        if getattr(env, "s", 0) is None and len(env.init_queue) == 0 and len(lengths) == len(Gs):
            end = END_NO_INIT
        else:
            sv, xv = sp(env.o)
            end = END_S_EMPTY if len(env.s_queues[sv]) == 0 else END_X_EMPTY
            assert end == END_S_EMPTY or len(env.x_queues[xv]) == 0
        endings.append(end)
        episodes.append(len(Gs))
        out.update({k + "mc_Gs": Gs, k + "mc_len": lengths, k + "mc_rows_s": np.array(rows_s, np.int64), k + "mc_rows_x": np.array(rows_x, np.int64),
                    k + "mc_o": np.int64(env.o), k + "mc_end": np.int64(end)})
        fresh()
        Gs, lengths = ref_psrs.evalMC_psrs(env, 2, pi, GAMMA)
        out.update({k + "mc2_Gs": Gs, k + "mc2_len": lengths, k + "mc2_o": np.int64(env.o)})
        fresh()
        Q, info = ref_psrs.qlearn_psrs(env, 10 ** 9, ref_tab.uniformly_random_policy, GAMMA, alpha=ALPHA)
        out.update({k + "ql_Q": Q, k + "ql_Gs": info["Gs"], k + "ql_td": info["TD_errors"], k + "ql_rows_s": np.array(rows_s, np.int64),
                    k + "ql_o": np.int64(env.o)})
        fresh()
        Q2, info2 = ref_psrs.qlearn_psrs(env, 10 ** 9, ref_tab.uniformly_random_policy, GAMMA, alpha=ALPHA, save_Q=1)
        assert np.array_equal(Q, Q2)
        out[k + "ql_Qs8"] = info2["Qs"][:9]  # Q before the first step and after each of the first 8
        fresh()
        Q, info = ref_psrs.expSARSA_psrs(env, 10 ** 9, pi, GAMMA, alpha=ALPHA)
        out.update({k + "es_Q": Q, k + "es_Gs": info["Gs"], k + "es_rows_s": np.array(rows_s, np.int64), k + "es_o": np.int64(env.o)})
    if not write:
        return endings, episodes
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(f"{name:16s} endings {endings} episodes {episodes} steps {[len(out[f's{s}_mc_rows_s']) for s in SEEDS]}")
    return endings, episodes


def main():
    d = np.load(os.path.join(ROOT, "tests", "golden", "exo_iid_2k.npz"))
    s, s_next, x, x_next = d["in_o"] // 4, d["in_o_next"] // 4, d["in_o"] % 4, d["in_o_next"] % 4
    cols = (d["in_a"], d["in_r"], d["in_done"], d["in_p_log"])
    ends, eps = [], []
    e, n = fixture("exo_a_mod4", "mod4", s, s_next, x, x_next, *cols, d["in_t0"], d["pi"])
    ends += e
    eps += n
    e, n = fixture("exo_b_default", "default", s, s_next, np.zeros_like(x), np.zeros_like(x), *cols, d["in_t0"], d["pi"])
    ends += e
    eps += n
    # (c): x = 2 is rare as a from-value (a short queue) and not so rare as a next value; only the first three initial rows of the log stay
    # initial rows.  The generator's seed is the first whose three rollouts show both endings that (a) and (b) do not -- an empty x-queue
    # with rows left in the s-queue, no initial row left -- and complete two episodes each.
    N = len(s)
    t0 = np.zeros(N, bool)
    t0[np.flatnonzero(d["in_t0"])[:3]] = True
    for gen_seed in range(1000):
        g = np.random.default_rng(gen_seed)
        xc = g.choice(3, N, p=[0.80, 0.17, 0.03])
        xc_next = g.choice(3, N, p=[0.80, 0.17, 0.03])
        e, n = fixture("exo_c_skewed", "mod3", s, s_next, xc, xc_next, *cols, t0, d["pi"], write=False)
        if END_X_EMPTY in e and END_NO_INIT in e and min(n) >= 2:
            break
    print("exo_c_skewed: generator seed", gen_seed)
    e, n = fixture("exo_c_skewed", "mod3", s, s_next, xc, xc_next, *cols, t0, d["pi"])
    ends += e
    eps += n
    # what the fixtures must cover between them
    assert END_X_EMPTY in ends, "no rollout ends on an empty x-queue with rows left in its s-queue"
    assert END_S_EMPTY in ends, "no rollout ends on an empty s-queue"
    assert END_NO_INIT in ends, "no rollout ends with no initial row left"
    assert min(eps) >= 2, "a rollout completes fewer than 2 episodes"
    print("done")


if __name__ == "__main__":
    sys.exit(main())
