"""NumPy restatement of a population evaluation (test infrastructure): L policies over observations, as per-row tables in caller order,
on the same S sampler seeds -- tests/obs_policy_host.py looped over (l, j).  A population shares nothing but the seeds: rollout (l, j) is
evalMC with policy l after reset_sampler(seeds[j]), whatever the other policies do."""
import numpy as np

import obs_policy_host as H


def evalmc_rows_population(inp, P_next, P_init, seeds, gamma, n_episodes=10 ** 9):
    """inp: the log as H.fixture_inputs gives it (its own P_next / P_init are ignored); P_next / P_init: sequences of L caller-order
    tables.  Returns {(l, j): H.evalmc_rows's dict}."""
    base = {k: v for k, v in inp.items() if k not in ("P_next", "P_init")}
    return {(l, j): H.evalmc_rows(**base, P_next=P_next[l], P_init=P_init[l], seed=int(s), gamma=gamma, n_episodes=n_episodes)
            for l in range(len(P_next)) for j, s in enumerate(seeds)}


def fixture_policies(d):
    """The three policies the population tests run on a tests/golden/obs_policy fixture, as caller-order tables of the fixture's own
    element type: 0 the fixture's own tables, 1 uniform, 2 a Dirichlet draw per row.  Returns (P_next [3, N, nA], P_init [3, N, nA])."""
    pn, p0 = d["P_next"], d["P_init"]
    N, nA = pn.shape
    g = np.random.default_rng(17)
    uni = np.full((N, nA), 1.0 / nA, pn.dtype)
    return (np.stack([pn, uni, g.dirichlet(np.ones(nA), N).astype(pn.dtype)]),
            np.stack([p0, uni, g.dirichlet(np.ones(nA), N).astype(pn.dtype)]))


def sum_in_order(Gs):
    """sum of the completed episodes' returns in episode order (the device's sum_g)"""
    s = 0.0
    for G in Gs:
        s += G
    return s
