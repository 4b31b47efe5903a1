"""The population cases of offsim_encode_mlp_pop (tests/test_gpu_encoder_population.py on the device, tests/test_encoder_pop_host.py for what
needs none), built from the cases of tests/encoder_host.py: L weight sets on a case's observations, the grid rule restated
(csrc/offsim_hip.hip: enc_pop_grid, launch_mlp_mfma, encode_mlp_any; include/offsim.h: offsim_encode_mlp_pop), and the f64 reference of
one learner with the tolerance of encoder_host.

The grid of a population call is (g, L) with g = max(min(single, ceil(N / rows_per_wg)), ceil(single / L)): `single` the workgroups the
single call starts for N rows, rows_per_wg the rows a workgroup takes in one pass of its loop.  offsim_latent_counts: (min(ceil(N / 4096),
1024), L).

A case is built once per process and then only read."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_host as E  # noqa: E402

F32_PRODUCTS = E.F32_PRODUCTS  # the dispatcher's switch, read as encoder_host reads it
MAX_LEARNERS = 65535
LATENT_ROWS_PER_WG, LATENT_MAX_WG, LATENT_LDS_LIMIT = 4096, 1024, 64 * 1024


# ---- the grid rule ----
def rows_per_wg(path, inst):
    """rows a workgroup (4 wavefronts, or 256 lanes of the VALU kernel) takes in one pass"""
    if path in ("S", "R"):
        dO, _ = inst
        return 4 * 32 * (1 if dO == 128 else 2)  # PF = 1 where a lane's share of a row is >= 64 bytes, else 2
    return 4 * 32 if path == "G" else 256


def single_grid(path, inst, N):
    """workgroups offsim_encode_mlp starts for N >= 1 rows"""
    by_groups = ((N + 31) // 32 + 3) // 4
    if path in ("S", "R"):
        return max(1, min(256, by_groups)) * E.REG_SHAPES[inst]
    if path == "G":
        return max(1, min(1024, by_groups))
    return min(2048, (N + 255) // 256)


def pop_grid(path, inst, N, L):
    """(workgroups per learner, learners) of offsim_encode_mlp_pop"""
    single = single_grid(path, inst, N)
    need = -(-N // rows_per_wg(path, inst))
    return max(min(single, need), -(-single // L)), L


def pop_sweep_rows(path, inst, N, L):
    """rows one pass of a learner's workgroups covers"""
    return pop_grid(path, inst, N, L)[0] * rows_per_wg(path, inst)


def stride_N(path, inst, L):
    """two sweeps of a learner's full grid + 32 + 7 rows: every wavefront of every learner goes round its loop twice and some a third time"""
    full = pop_sweep_rows(path, inst, 1 << 40, L)
    N = 2 * full + 39
    assert pop_sweep_rows(path, inst, N, L) == full, (path, inst, L)
    return N


def latent_grid(N, L):
    return min(-(-N // LATENT_ROWS_PER_WG), LATENT_MAX_WG), L


def latent_lds_bytes(nZ, nY):
    return nZ * max(nY, 1) * 8


# ---- population cases ----
def with_rows(case, N):
    """the case at another number of rows (same seed)"""
    c = SimpleNamespace(**vars(case))
    c.N = N
    c.name = f"{case.name}@N{N}"
    return c


def learner_weights(case, l):
    """(W1, b1, W2, b2) of learner l: drawn as the case draws its own, from the case's seed + l (learner 0 has the case's weights)"""
    c = SimpleNamespace(**vars(case))
    c.seed = case.seed + l
    return E.make_inputs(c)[1:]


@functools.lru_cache(maxsize=None)
def _population(name, L, N):
    c = E.CASES[name] if N is None else with_rows(E.CASES[name], N)
    x = E.make_inputs(c)[0]
    ws = [learner_weights(c, l) for l in range(L)]
    for k in range(4):
        for l in range(1, L):  # every tensor of every learner differs from every other learner's: a wrong offset on any one shows
            assert all(not np.array_equal(ws[l][k], ws[m][k]) for m in range(l)), (name, k, l)
    stacked = tuple(np.ascontiguousarray(np.stack([w[k] for w in ws])) for k in range(4))
    for a in (x,) + stacked:
        a.setflags(write=False)
    return SimpleNamespace(case=c, L=L, x=x, W1=stacked[0], b1=stacked[1], W2=stacked[2], b2=stacked[3])


def population(name, L, N=None):
    """the case's observations with L stacked weight sets: x [N, dO], W1 [L, H, dO], b1 [L, H], W2 [L, nZ, H], b2 [L, nZ]"""
    return _population(name, L, N)


@functools.lru_cache(maxsize=None)
def build_learner(name, L, l):
    """encoder_host.build for learner l of population(name, L): inputs, f64 logits, B, rho_ref and both tolerances"""
    from oracle import oracle as O
    p = population(name, L)
    x, W1, b1, W2, b2 = p.x, p.W1[l], p.b1[l], p.W2[l], p.b2[l]
    ref = E.forward_f64(x, W1, b1, W2, b2)
    B = E.magnitude_f64(x, W1, b1, W2, b2)
    _, lo = O.mlp_encode(x.astype(np.float32), np.array(W1), np.array(b1), np.array(W2), np.array(b2))
    rho_ref = float((np.abs(lo.astype(np.float64) - ref) / B).max())
    base = 4.0 * max(rho_ref, 2.0 ** -24)
    for a in (ref, B, lo):
        a.setflags(write=False)
    return SimpleNamespace(case=p.case, x=x, W1=W1, b1=b1, W2=W2, b2=b2, ref=ref, B=B, oracle=lo, rho_ref=rho_ref, tol_f32=base,
                           tol_split=base + 2.0 ** -22)
