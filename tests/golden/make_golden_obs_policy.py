#!/usr/bin/env python3
"""Generate tests/golden/obs_policy/*.npz by RUNNING THE REFERENCE's evalMC_psrs with a policy over continuous observations.

Run from the repo root:   python tests/golden/make_golden_obs_policy.py
Needs /root/reference (read-only); nothing of it is copied -- the fixtures hold inputs and the outputs the reference produced for them.

Imported from the reference, by file path (as make_golden.py does):
  offsim4rl/evaluators/psrs.py       PSRS, evalMC_psrs          (numpy only)
  offsim4rl/encoders/heuristic.py    CartpoleBoxEncoder          (numpy, pandas)

The reference PSRS is fed legacy tuples (obs_i, a, r, next_obs_i, done, p_i, {'z', 'z_next', 't'}) whose obs_i / next_obs_i are the
CONTINUOUS observations, and evalMC_psrs calls pi[S] with S = such an observation (psrs.py:255).  `pi` is LinearSoftmax below:
softmax(W S + b) in NumPy, f64 or f32.  The per-row tables stored beside the results are obtained by calling that same __getitem__ on
every row's obs and next_obs, one row at a time (a vectorised matmul would not be bit-equal), so a consumer that takes p_new from the
tables sees exactly the probabilities the reference saw.

Every fixture: inputs (obs, next_obs, z, a, r, z_next, done, p_log, t0), tables P_next[i] = pi[next_obs[i]], P_init[i] = pi[obs[i]]
(caller order), and per seed the reference's Gs, lengths, accepted rows (caller indices, in step order) and status.
"""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "obs_policy")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


ref_psrs = _load("ref_psrs", os.path.join(REF, "offsim4rl/evaluators/psrs.py"))
ref_heur = _load("ref_heur", os.path.join(REF, "offsim4rl/encoders/heuristic.py"))
synth = _load("synth", os.path.join(ROOT, "rl-offline-simulation_amd", "synth.py"))


class LinearSoftmax:
    """pi[S] = softmax(W S + b) over an observation S, computed in NumPy in the dtype of W."""

    def __init__(self, dO, nA, seed, dtype):
        g = np.random.default_rng(seed)
        self.W = (g.standard_normal((nA, dO)) * 2.0).astype(dtype)
        self.b = (g.standard_normal(nA) * 0.5).astype(dtype)

    def __getitem__(self, S):
        logits = self.W @ np.asarray(S, self.W.dtype) + self.b
        e = np.exp(logits - logits.max())
        return e / e.sum()


def run_reference(inp, pi, seed):
    """reset_sampler(seed) + evalMC_psrs(env, 1e9, pi, 0.99) on the reference; the accepted rows are read off the p_log objects the
    reference hands back in info['p'] (one object per row)."""
    N = len(inp["z"])
    p_rows = [np.array(inp["p_log"][i]) for i in range(N)]
    id2row = {id(p): i for i, p in enumerate(p_rows)}
    buf = [(inp["obs"][i], int(inp["a"][i]), float(inp["r"][i]), inp["next_obs"][i], bool(inp["done"][i]), p_rows[i],
            {"z": int(inp["z"][i]), "z_next": int(inp["z_next"][i]), "t": 0 if inp["t0"][i] else 1}) for i in range(N)]
    env = ref_psrs.PSRS(buf, nS=int(max(inp["z"].max(), inp["z_next"].max())) + 1, nA=inp["p_log"].shape[1])
    env.reset_sampler(seed)
    rows = []
    orig_step = env.step

    def step(p_new):
        out = orig_step(p_new)
        if out[0] is not None:
            rows.append(id2row[id(out[3]["p"])])
        return out

    env.step = step
    status = "ok"
    try:
        Gs, lengths = ref_psrs.evalMC_psrs(env, 10 ** 9, pi, 0.99)
    except KeyError:
        status, Gs, lengths = "keyerror", np.zeros(0), np.zeros(0, np.int64)
    return np.asarray(Gs, np.float64), np.asarray(lengths, np.int64), np.asarray(rows, np.int64), status


def fixture(name, inp, pi, seeds):
    N = len(inp["z"])
    P_next = np.stack([pi[inp["next_obs"][i]] for i in range(N)])  # row by row: the reference's own pi[S]
    P_init = np.stack([pi[inp["obs"][i]] for i in range(N)])
    out = dict(inp, P_next=P_next, P_init=P_init, seeds=np.asarray(seeds, np.int64), gamma=np.float64(0.99))
    for s in seeds:
        Gs, lengths, rows, status = run_reference(inp, pi, s)
        out[f"Gs_{s}"], out[f"lengths_{s}"], out[f"rows_{s}"] = Gs, lengths, rows
        out[f"status_{s}"] = np.array(status)
        print(f"{name} seed {s}: {len(Gs)} episodes, {len(lengths)} lengths, {len(rows)} steps, {status}")
    np.savez_compressed(os.path.join(OUT, f"{name}.npz"), **out)
    return out


def main():
    enc = ref_heur.CartpoleBoxEncoder()
    cp = synth.cartpole_log(2000, seed=5)
    cp_inp = dict(obs=cp["observations"], next_obs=cp["next_observations"], z=np.asarray(enc.encode(cp["observations"]), np.int64),
                  z_next=np.asarray(enc.encode(cp["next_observations"]), np.int64), a=cp["actions"], r=cp["rewards"].astype(np.float64),
                  done=cp["terminals"], p_log=cp["action_distributions"], t0=cp["steps"] == 0)
    fixture("obs_policy_cartpole_f64", cp_inp, LinearSoftmax(4, 2, 1, np.float64), [0, 1, 2])
    fixture("obs_policy_cartpole_f32", cp_inp, LinearSoftmax(4, 2, 1, np.float32), [0, 1, 2])  # f32 p_log and f32 p_new: f32 division

    gr = synth.grid_coords_log(140, seed=6)
    gr_inp = dict(obs=gr["observations"], next_obs=gr["next_observations"], z=gr["z"], z_next=gr["z_next"], a=gr["actions"],
                  r=gr["rewards"], done=gr["terminals"], p_log=gr["action_distributions"], t0=gr["steps"] == 0)
    fixture("obs_policy_grid_f64", gr_inp, LinearSoftmax(2, 5, 2, np.float64), [0, 1, 2])
    fixture("obs_policy_grid_f32", gr_inp, LinearSoftmax(2, 5, 2, np.float32), [0, 1])  # f64 p_log: p_new widened, f64 division

    # exhaustion in the middle of an episode: a log whose initial rows outnumber what its queues can serve (every row initial)
    ex = dict(gr_inp, t0=np.ones(len(gr_inp["z"]), bool))
    o = fixture("obs_policy_grid_exhaust", ex, LinearSoftmax(2, 5, 3, np.float64), [0, 1])
    assert all(len(o[f"lengths_{s}"]) > len(o[f"Gs_{s}"]) for s in (0, 1)), "expected an episode cut short by exhaustion"

    # KeyError: some rows lead to a state that never occurs as a from-state (psrs.py:44)
    ke = dict(gr_inp, z_next=gr_inp["z_next"].copy())
    ke["z_next"][gr_inp["z_next"] == 1] = 30
    o = fixture("obs_policy_grid_keyerror", ke, LinearSoftmax(2, 5, 4, np.float64), [0, 1])
    assert str(o["status_0"]) == "keyerror"


if __name__ == "__main__":
    main()
