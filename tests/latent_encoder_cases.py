"""The case table of the in-kernel latent encoder (latent_encode<ENV, OFFSIM_LATENT_MLP> of csrc/eval_env_latent.hpp), read by
tests/test_latent_encoder_matrix_host.py (CPU) and tests/test_gpu_latent_encoder_matrix.py (GPU).  Host only: no HIP import.

The reference of every case is the oracle's f32 encoder (oracle_mlp_encode, oracle/psrs_oracle.c: per unit one k-ordered fmaf chain from 0,
then the bias, 0.01f * acc, the first strict maximum), which is the arithmetic the kernel's header claims: the kernel's z is held to it on
every observation, exactly -- no top-2 gap, no clear-row rule.

A case: the environment ("grid_coords": dO = 2, nA = 5; "cartpole": dO = 4, nA = 2), (H, nZ), the weights (a seed through latent_env_host.mlp_weights, a
power of two on W1 and W2, optionally zero biases, then the case's edit), nS and the learners it runs besides evalMC.

  lane   (1, 1) (63, 63) (64, 64) (65, 65) (130, 200) (16, 129) (129, 16): a full lane round exactly, a partial second one, several, both
         non-square shapes (the two staging transposes), nZ = 1 (63 lanes end their scan holding (-inf, nZ))
  tie    out of lane order (nZ = 130, row 129 - c of W2 / b2 a bit copy of row c for c in 0..64: every maximum is tied with its copy, and
         for c in 33..63 the copy -- the later index -- sits in a lower lane) and in one lane (nZ = 128, row c + 64 a copy of row c)
  equal  W2 = 0, b2 = 0, nZ = 70: z = 0 everywhere
  nan    b2 all NaN -> 0; NaN on a seeded half of the units (0 and 64 among them): a NaN never wins; b2 all -inf -> 0; +inf at 70 and 5 -> 5
  limit  (4096, 2) on the grid; nZ = 4096 (below)
  carve  expected SARSA on the grid with nS = nZ = 65 and H the smallest that forces 4, 2 and 1 rollouts per workgroup

nZ = 4096 needs nS >= 4096 rows, and on the grid (nA = 5) pi alone is then 4096 * 5 * 8 bytes = 160 KiB: with the encoder behind it the
launch is refused (the case "limit-2x4096-grid" stays in the table as that refusal; the CPU file asserts it).  CartPole's nA = 2 leaves room
(64 KiB of pi), so (2, 4096) runs there, from the trace as every CartPole case.

Shapes of the runs: R = 5 rollouts (SEEDS), 3 episodes, num_steps = 6 on the grid with the goal at (1, 2), CartPole's cap 12.
Seeds and scales were chosen on the CPU until the oracle alone meets the conditions test_latent_encoder_matrix_host.py asserts."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import latent_env_host as H  # noqa: E402
from oracle import oracle as O  # noqa: E402

SEEDS = [3, 10, 17, 24, 31]
N_EP, GRID_STEPS, GRID_GOAL, CARTPOLE_CAP = 3, 6, (1, 2), 12
GAMMA, ALPHA = 0.9, 0.2
ENVS = {"grid_coords": ("coords", 2, 5), "cartpole": ("cartpole", 4, 2)}  # env -> (HostEnv kind, dO, nA)
LANE_SHAPES = ((1, 1), (63, 63), (64, 64), (65, 65), (130, 200), (16, 129), (129, 16))
CARVE_NZ = 65


def carve_hidden(waves, nZ=CARVE_NZ):
    """the smallest H at which the grid's expected-SARSA launch (pi given, nS = nZ) holds `waves` rollouts per workgroup"""
    return next(h for h in range(1, 4097) if H.launch_shape(nZ, 5, True, True, (2, h, nZ))[0] == waves)


def _case(name, group, env, Hd, nZ, seed, w_scale=1.0, zero_bias=False, edit=None, nS=None, learners=(), refused=False):
    return dict(name=name, group=group, env=env, H=Hd, nZ=nZ, seed=seed, scale=1.0, w_scale=w_scale, zero_bias=zero_bias, edit=edit, nS=nZ if nS is None else nS,
                learners=learners, refused=refused)


BOTH = ("qlearn-eps", "expSARSA")
# (seed, the scale on W1 and W2) of the lane-round and tie cases per environment; CartPole's observations are small, so its cases run with
# zero biases
_PICK = {
    "grid_coords": {(1, 1): (1, 1.0), (63, 63): (12, 8.0), (64, 64): (104, 8.0), (65, 65): (30, 8.0), (130, 200): (12, 8.0), (16, 129): (3, 8.0),
                    (129, 16): (86, 4.0), "tie-out": (4, 8.0), "tie-lane": (4, 4.0)},
    "cartpole": {(1, 1): (1, 1.0), (63, 63): (1, 1.0), (64, 64): (1, 1.0), (65, 65): (1, 1.0), (130, 200): (1, 1.0), (16, 129): (1, 1.0),
                 (129, 16): (1, 1.0), "tie-out": (1, 1.0), "tie-lane": (1, 1.0)},
}
TIE_H = 16


def _table():
    t = []
    for env in ("grid_coords", "cartpole"):
        tag, zb = ("grid", False) if env == "grid_coords" else ("cartpole", True)
        for Hd, nZ in LANE_SHAPES:
            seed, scale = _PICK[env][(Hd, nZ)]
            t.append(_case(f"lane-{Hd}x{nZ}-{tag}", "lane", env, Hd, nZ, seed, scale, zb, learners=BOTH))
        seed, scale = _PICK[env]["tie-out"]
        t.append(_case(f"tie-out-of-lane-order-{tag}", "tie", env, TIE_H, 130, seed, scale, zb, edit="tie_out", learners=BOTH))
        seed, scale = _PICK[env]["tie-lane"]
        t.append(_case(f"tie-same-lane-{tag}", "tie", env, TIE_H, 128, seed, scale, zb, edit="tie_lane", learners=BOTH))
    g = "grid_coords"
    t.append(_case("all-equal", "equal", g, 16, 70, 2, edit="all_equal"))
    # nS = nZ + 1: the row an encoder that returned nZ itself would read exists
    t.append(_case("nan-all", "nan", g, 16, 130, 1, 4.0, edit="nan_all", nS=131))
    t.append(_case("nan-half", "nan", g, 16, 130, 1, 4.0, edit="nan_half", nS=131))
    t.append(_case("neg-inf-all", "nan", g, 16, 130, 1, 4.0, edit="neg_inf_all", nS=131))
    t.append(_case("pos-inf-70-and-5", "nan", g, 16, 130, 1, 4.0, edit="pos_inf", nS=131))
    t.append(_case("limit-4096x2-grid", "limit", g, 4096, 2, 4, 4.0))
    t.append(_case("limit-2x4096-grid", "limit", g, 2, 4096, 4, 4.0, refused=True))
    t.append(_case("limit-2x4096-cartpole", "limit", "cartpole", 2, 4096, 6, 1.0, True))
    for waves, (seed, scale) in ((4, (531, 8.0)), (2, (42, 16.0)), (1, (109, 8.0))):
        t.append(_case(f"carve-{waves}", "carve", g, carve_hidden(waves), CARVE_NZ, seed, scale, learners=BOTH))
        t[-1]["waves"] = waves
    return t


CASES = _table()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def names(groups=None, env=None, runnable=True):
    return [c["name"] for c in CASES if (groups is None or c["group"] in groups) and (env is None or c["env"] == env) and not (runnable and c["refused"])]


NAN_HALF_SEED = 9


def nan_half_units(nZ):
    """the units of the nan-half case whose bias is NaN: a seeded half, 0 and 64 among them"""
    pick = np.random.default_rng(NAN_HALF_SEED).permutation(nZ)[:nZ // 2]
    return np.unique(np.concatenate([pick, [0, 64]]))


def seeded_weights(case):
    """the case's weights before its edit"""
    _, dO, _ = ENVS[case["env"]]
    W1, b1, W2, b2 = (w.copy() for w in H.mlp_weights(dO, case["H"], case["nZ"], case["seed"], case["scale"]))
    W1 *= np.float32(case["w_scale"])  # (a power of two: exact)
    W2 *= np.float32(case["w_scale"])
    if case["zero_bias"]:
        b1[:], b2[:] = 0.0, 0.0
    return W1, b1, W2, b2


def weights(case):
    W1, b1, W2, b2 = seeded_weights(case)
    edit, nZ = case["edit"], case["nZ"]
    if edit == "tie_out":
        for c in range(65):
            W2[129 - c], b2[129 - c] = W2[c], b2[c]
    elif edit == "tie_lane":
        W2[64:], b2[64:] = W2[:64], b2[:64]
    elif edit == "all_equal":
        W2[:], b2[:] = 0.0, 0.0
    elif edit == "nan_all":
        b2[:] = np.nan
    elif edit == "nan_half":
        b2[nan_half_units(nZ)] = np.nan
    elif edit == "neg_inf_all":
        b2[:] = -np.inf
    elif edit == "pos_inf":
        b2[[70, 5]] = np.inf
    else:
        assert edit is None, edit
    return W1, b1, W2, b2


def shape(case, have_pi=True, td=False):
    """latent_env_host.launch_shape of the case: (rollouts per workgroup, LDS bytes, refused)"""
    _, dO, nA = ENVS[case["env"]]
    return H.launch_shape(case["nS"], nA, have_pi, td, (dO, case["H"], case["nZ"]))


class OracleEncoder:
    """the oracle's f32 encoder on one observation; keeps every observation it saw and the z it gave"""

    def __init__(self, w):
        self.weights, self.obs, self.z = w, [], []

    def __call__(self, obs32):
        x = np.asarray(obs32, np.float32).reshape(1, -1)
        z = int(O.mlp_encode(x, *self.weights)[0][0])
        self.obs.append(x[0].copy())
        self.z.append(z)
        return z


def oracle_z(w, obs32):
    """the oracle's z of the rows obs32 [N, dO]"""
    return O.mlp_encode(np.asarray(obs32, np.float32).reshape(len(obs32), -1), *w)[0]


def policy(nS, nA, seed=5):
    return np.random.default_rng(seed).dirichlet(np.full(nA, 1.5), nS)


def world(case, enc, seed=None):
    kind = ENVS[case["env"]][0]
    if kind == "cartpole":
        return H.LiveWorld(kind, enc, seed=seed, reseed=True, cap=CARTPOLE_CAP)
    return H.LiveWorld(kind, enc, seed=seed, reseed=True, num_steps=GRID_STEPS, goal=GRID_GOAL, num_cells=5)


def bound(case):
    return CARTPOLE_CAP if case["env"] == "cartpole" else GRID_STEPS


def host_rows(case, w, mode, pi, q0=None, tie=None, n_episodes=N_EP, seeds=SEEDS, **kw):
    """latent_env_host.run per seed on a LiveWorld behind the oracle's encoder: (the device's rows, the encoder with what it saw)"""
    nA = ENVS[case["env"]][2]
    enc, rows = OracleEncoder(w), []
    for i, s in enumerate(seeds):
        wd = world(case, enc, s)
        gen = np.random.default_rng(s)
        m = H.run(wd, case["nS"], nA, H.chooser(gen, nA), mode, pi, GAMMA, q=None if q0 is None else q0[i].copy(), tie=tie, n_episodes=n_episodes, **kw)
        m["rng_act_end"], m["rng_env_end"] = H.rng_words(gen), wd.env_words()
        rows.append(m)
    return rows, enc


def visited(case, w, seeds=SEEDS, n_episodes=N_EP):
    """(observations [N, dO], the oracle's z [N]) of the case's evalMC rollouts on the host"""
    nA = ENVS[case["env"]][2]
    _, enc = host_rows(case, w, H.EVALMC, policy(case["nS"], nA), n_episodes=n_episodes, seeds=seeds)
    return np.stack(enc.obs), np.array(enc.z)
