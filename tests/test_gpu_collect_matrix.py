"""Every instance of k_collect<PL, PROB, FORM, XT, VF> (csrc/collect.hpp) that collect_launch can dispatch, each pinned on host references:

  a. the network arithmetic (probs, val, final_value, v_trunc, logp) against the same network in f64, within a forward error bound
     computed in f64 and carried through the layers;
  b. the control flow (rows, terminated, truncated, reset, alive, status, the recorded observations) against the NumPy restatement
     tests/collect_host.py, fed the per-row tables of the device's own forward, in the precision the kernel compares p_new / p_log in;
  c. the PPO buffer (adv_raw, ret, adv, adv_mean, adv_std) against tests/ppo_host.py on the recorded values, both bootstrap modes.

INSTANCES lists all 56.  Instances the Python API does not reach run through the C ABI (offsim_vector_collect[_ppo]) with the ctypes
structs of _lib.py (route "abi").  EDGES names the shapes where kernels go wrong (wide, deep, bias-free, wider critic, LDS limits)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import collect_host as H  # noqa: E402
from test_gpu_collect import _env  # noqa: E402
from test_gpu_ppo import host_check  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24  # f32 unit roundoff
TINY = 2.0 ** -126  # f32's smallest normal: below it a relative bound means nothing
GAMMA, LAM = 0.99, 0.97


@pytest.fixture(scope="module")
def gpu():
    from rl_offline_simulation_amd import _lib
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    _lib.load()
    return torch.device("cuda", 0)


# ---- networks ----------------------------------------------------------------------------------------------------------------------
# name -> (depth, hidden, activation, slope, biases, scale of the last layer)
NETS = {
    "small": (2, 16, "tanh", 0.01, True, 1.0),
    "deep": (4, 24, "relu", 0.01, True, 1.0),
    "wide": (2, 200, "tanh", 0.01, True, 1.0),        # hidden > 64: the lanes' j loop takes four trips
    "leaky": (3, 33, "leaky_relu", 0.2, True, 1.0),
    "ident": (2, 20, "identity", 0.01, True, 1.0),
    "nobias": (3, 70, "tanh", 0.01, False, 1.0),      # boff = -1 in every layer
    "hot": (2, 32, "tanh", 0.01, True, 150.0),       # logits in the hundreds
    "cwide": (2, 250, "tanh", 0.01, True, 1.0),      # a critic wider than any actor here
    "cdeep": (4, 40, "leaky_relu", 0.3, True, 1.0),
    "cnobias": (2, 90, "relu", 0.01, False, 1.0),
}


def _weights(dO, out, name, seed):
    depth, hidden, _, _, bias, scale = NETS[name]
    g = torch.Generator().manual_seed(1000 + seed)
    ws, w = [], dO
    for k in range(depth):
        o = out if k == depth - 1 else hidden
        W = torch.randn(o, w, generator=g) * (1.5 / w ** 0.5)
        if k == depth - 1:
            W = W * scale
        b = torch.randn(o, generator=g) * 0.5 if bias else None
        ws.append((W.float(), None if b is None else b.float()))
        w = o
    return ws


def _actor(dO, nA, name, seed):
    from rl_offline_simulation_amd.evaluators import MLPPolicy
    _, _, act, slope, _, _ = NETS[name]
    return MLPPolicy(_weights(dO, nA, name, seed), act, slope)


def _critic(dO, name, seed):
    from rl_offline_simulation_amd.evaluators import MLPValue
    _, _, act, slope, _, _ = NETS[name]
    return MLPValue(_weights(dO, 1, name, seed + 500), act, slope)


def _f64(net, x):
    """(outputs, forward error bound) of the f32 forward (pmlp_unit: one fmaf chain over k, then + b, then the activation) against the
    same network in f64 at the inputs x [M, dO] (f64, the values the kernel reads).  Layer l: y_j = sum_k W_jk h_k + b_j.  The chain of
    in fmaf plus the bias add rounds in+1 times, so |y~ - y| <= sum_k |W_jk| dh_k + (in+1) u (sum_k |W_jk| |h_k| + |b_j|) (Higham's gamma_n,
    to first order); the activation is 1-Lipschitz (leaky_relu: max(1, slope)) and rounds once more (tanhf: at most 2 ulp = 4 u)."""
    h, dh = x, torch.zeros_like(x)
    n = len(net.weights)
    for k, (W, b) in enumerate(net.weights):
        W = W.double()
        b = torch.zeros(W.shape[0], dtype=torch.float64) if b is None else b.double()
        y = h @ W.t() + b
        dy = dh @ W.abs().t() + (W.shape[1] + 1) * U * (h.abs() @ W.abs().t() + b.abs())
        if k == n - 1:
            return y, dy
        if net.activation == "tanh":
            h = torch.tanh(y)
        elif net.activation == "relu":
            h = torch.relu(y)
        elif net.activation == "leaky_relu":
            h = torch.where(y > 0, y, y * net.slope)
        else:
            h = y
        dh = max(1.0, abs(net.slope)) * dy + 4 * U * h.abs()


def _check_probs(got, z, dz):
    """softmax in f32 (pmlp_softmax) against f64: the logits' error dz moves log p by at most 2 max dz (z_a - logsumexp is 2-Lipschitz in
    the max norm); the f32 evaluation adds, relative to p, expf (1 ulp) and the rounding of z_b - max (u |z_b - max|) on both e_a and the
    sum, nA - 1 additions and the division."""
    p = torch.softmax(z, -1)
    nA = z.shape[-1]
    R = (z - z.max(-1, keepdim=True).values).abs().max(-1, keepdim=True).values
    rel = torch.expm1(2 * dz.max(-1, keepdim=True).values) + 2 * U * R + (nA + 6) * U
    err = (got.double() - p).abs()
    assert bool((err <= p * rel + TINY).all()), float((err - p * rel).max())


def _check_logp(got, z, dz, a):
    """pmlp_logp = z_a - (max + logf(sum exp(z_b - max))) against f64 log_softmax: 2 max dz from the logits, and a few ulp of
    M = max(|z_a|, |max z| + log sum) from the f32 evaluation (the two subtractions, the add, logf), plus the sum's own relative error
    (u |z_b - max| + 1 ulp per expf, nA additions), which logf passes on as an absolute error."""
    ls = torch.log_softmax(z, -1).gather(-1, a.unsqueeze(-1))[..., 0]
    zm = z.max(-1).values
    lse = zm + torch.log(torch.exp(z - zm.unsqueeze(-1)).sum(-1))
    M = torch.maximum(z.gather(-1, a.unsqueeze(-1))[..., 0].abs(), zm.abs() + (lse - zm))
    R = (z - zm.unsqueeze(-1)).abs().max(-1).values
    bound = 2 * dz.max(-1).values + 4 * U * M + U * (R + z.shape[-1] + 4)
    err = (got.double() - ls).abs()
    assert bool((err <= bound).all()), float((err - bound).max())


def _check_value(got, net, x):
    v, dv = _f64(net, x)
    err = (got.double() - v[:, 0]).abs()
    assert bool((err <= dv[:, 0]).all()), float((err - dv[:, 0]).max())


# ---- logs --------------------------------------------------------------------------------------------------------------------------
PLOG = {"float": np.float32, "double": np.float64, "half": np.float16}
_LOGS = {}


def _log(nA, obs, dO, plog, N=3000, nS=40, seed=0):
    """synth_iid's log (5 % initial rows, 2 % terminal): obs 'state' (observations are the states) or an f32 / f16 dtype of width dO
    (a per-state embedding plus per-row noise, so every row asks the network something different)."""
    key = (nA, obs, dO, plog, N, nS, seed)
    if key not in _LOGS:
        from rl_offline_simulation_amd import synth
        e = synth.synth_iid(N, nS, nA, seed=seed, p_init=0.05)
        g = np.random.default_rng(seed + 1)
        z, zn = e["z"], e["z_next"]
        if obs == "state":
            x, xn = z, zn
        else:
            emb = g.standard_normal((nS, dO))
            x = (emb[z] + 0.3 * g.standard_normal((N, dO))).astype(obs)
            xn = (emb[zn] + 0.3 * g.standard_normal((N, dO))).astype(obs)
        _LOGS[key] = dict(obs=x, next_obs=xn, z=z, z_next=zn, a=e["actions"], r=e["rewards"], done=e["terminals"],
                          p_log=e["action_distributions"].astype(plog), t0=e["steps"] == 0)
    return _LOGS[key]


# ---- the instance table ------------------------------------------------------------------------------------------------------------
# (PL, PROB, FORM, XT, VF) and the inputs that reach it: p_log dtype = PL; the policy's probabilities are f32 where PROB is float (an MLP
# actor's always are: PROB double with an f32 p_log is then the C ABI's prob_mode OFFSIM_PROB_F64), f64 tables otherwise; obs is the
# log's observation dtype ('state': a discrete log, observations are the states, which the API hands the critic as f32); then nA, dO
# (observation width), E, T, cap (max_episode_steps), the actor's network (MLP) and the critic's (MLP), bootstrap mode, route.
# Route "abi": not reachable through VectorPSRS.collect / collect_ppo -- PROB double with an MLP actor and an f32 p_log (the API compares
# an MLP's f32 probabilities in f32 there), and a tabular actor with an f16 MLP critic (a discrete log's observations become f32).
I = lambda *a: a  # noqa: E731
INSTANCES = [
    # PL        PROB      FORM       XT       VF      obs           nA  dO  E  T    cap   actor     critic     boot         route
    # -- VF none: offsim_vector_collect (ROWS / TABULAR read no observation: XT is float)
    I("float", "float", "MLP", "float", "NONE", np.float32, 2, 4, 7, 300, None, "small", None, None, "api"),
    I("float", "float", "MLP", "half", "NONE", np.float16, 3, 5, 8, 200, 5, "deep", None, None, "api"),
    I("float", "float", "ROWS", "float", "NONE", np.float16, 16, 7, 9, 150, 1, None, None, None, "api"),
    I("float", "float", "TABULAR", "float", "NONE", "state", 2, 1, 1, 300, 5, None, None, None, "api"),
    I("float", "double", "MLP", "float", "NONE", np.float32, 3, 6, 9, 200, None, "leaky", None, None, "abi"),
    I("float", "double", "MLP", "half", "NONE", np.float16, 16, 7, 7, 150, 5, "wide", None, None, "abi"),
    I("float", "double", "ROWS", "float", "NONE", np.float32, 2, 4, 8, 300, 5, None, None, None, "api"),
    I("float", "double", "TABULAR", "float", "NONE", "state", 3, 1, 9, 200, None, None, None, None, "api"),
    I("double", "double", "MLP", "float", "NONE", np.float32, 16, 9, 8, 150, 1, "ident", None, None, "api"),
    I("double", "double", "MLP", "half", "NONE", np.float16, 2, 3, 1, 300, None, "nobias", None, None, "api"),
    I("double", "double", "ROWS", "float", "NONE", np.float32, 3, 4, 7, 200, 5, None, None, None, "api"),
    I("double", "double", "TABULAR", "float", "NONE", "state", 16, 1, 8, 150, 5, None, None, None, "api"),
    I("half", "double", "MLP", "float", "NONE", np.float32, 3, 4, 9, 200, 5, "hot", None, None, "api"),
    I("half", "double", "MLP", "half", "NONE", np.float16, 16, 5, 8, 150, None, "small", None, None, "api"),
    I("half", "double", "ROWS", "float", "NONE", np.float16, 2, 3, 7, 300, 1, None, None, None, "api"),
    I("half", "double", "TABULAR", "float", "NONE", "state", 3, 1, 1, 200, None, None, None, None, "api"),
    # -- VF MLP: the critic in-wave; XT is the critic's input type whatever the actor's form
    I("float", "float", "MLP", "float", "MLP", np.float32, 3, 4, 8, 200, 5, "small", "cwide", "spinup", "api"),
    I("float", "float", "MLP", "half", "MLP", np.float16, 2, 7, 9, 300, None, "leaky", "cdeep", "reference", "api"),
    I("float", "float", "ROWS", "float", "MLP", np.float32, 16, 6, 7, 150, 5, None, "cdeep", "spinup", "api"),
    I("float", "float", "ROWS", "half", "MLP", np.float16, 3, 5, 1, 200, 1, None, "cwide", "reference", "api"),
    I("float", "float", "TABULAR", "float", "MLP", "state", 2, 1, 8, 300, 5, None, "cnobias", "spinup", "api"),
    I("float", "float", "TABULAR", "half", "MLP", "state", 16, 1, 9, 150, None, None, "cdeep", "reference", "abi"),
    I("float", "double", "MLP", "float", "MLP", np.float32, 16, 4, 7, 150, 5, "wide", "cnobias", "spinup", "abi"),
    I("float", "double", "MLP", "half", "MLP", np.float16, 3, 3, 8, 200, 1, "nobias", "cdeep", "reference", "abi"),
    I("float", "double", "ROWS", "float", "MLP", np.float32, 2, 9, 9, 300, None, None, "small", "reference", "api"),
    I("float", "double", "ROWS", "half", "MLP", np.float16, 16, 7, 7, 150, 5, None, "cnobias", "spinup", "api"),
    I("float", "double", "TABULAR", "float", "MLP", "state", 3, 1, 1, 200, 1, None, "cwide", "spinup", "api"),
    I("float", "double", "TABULAR", "half", "MLP", "state", 2, 1, 8, 300, 5, None, "small", "spinup", "abi"),
    I("double", "double", "MLP", "float", "MLP", np.float32, 2, 4, 9, 300, 5, "deep", "cdeep", "spinup", "api"),
    I("double", "double", "MLP", "half", "MLP", np.float16, 16, 5, 7, 150, None, "hot", "cwide", "reference", "api"),
    I("double", "double", "ROWS", "float", "MLP", np.float32, 3, 6, 8, 200, 5, None, "cnobias", "reference", "api"),
    I("double", "double", "ROWS", "half", "MLP", np.float16, 2, 3, 9, 300, 5, None, "cdeep", "spinup", "api"),
    I("double", "double", "TABULAR", "float", "MLP", "state", 16, 1, 7, 150, None, None, "cdeep", "reference", "api"),
    I("double", "double", "TABULAR", "half", "MLP", "state", 3, 1, 8, 200, 5, None, "cnobias", "spinup", "abi"),
    I("half", "double", "MLP", "float", "MLP", np.float32, 3, 9, 7, 200, 1, "ident", "cnobias", "spinup", "api"),
    I("half", "double", "MLP", "half", "MLP", np.float16, 2, 5, 8, 300, 5, "wide", "small", "spinup", "api"),
    I("half", "double", "ROWS", "float", "MLP", np.float32, 16, 4, 9, 150, 5, None, "cwide", "spinup", "api"),
    I("half", "double", "ROWS", "half", "MLP", np.float16, 3, 7, 1, 200, None, None, "cdeep", "reference", "api"),
    I("half", "double", "TABULAR", "float", "MLP", "state", 2, 1, 9, 300, 5, None, "small", "reference", "api"),
    I("half", "double", "TABULAR", "half", "MLP", "state", 16, 1, 7, 150, 1, None, "cwide", "spinup", "abi"),
    # -- VF ROWS: the critic's per-row tables (ROWS / TABULAR actors read no observation: XT is float)
    I("float", "float", "MLP", "float", "ROWS", np.float32, 16, 4, 9, 150, 5, "deep", None, "spinup", "api"),
    I("float", "float", "MLP", "half", "ROWS", np.float16, 3, 3, 7, 200, None, "hot", None, "reference", "api"),
    I("float", "float", "ROWS", "float", "ROWS", np.float16, 2, 5, 8, 300, 5, None, None, "spinup", "api"),
    I("float", "float", "TABULAR", "float", "ROWS", "state", 16, 1, 7, 150, 1, None, None, "reference", "api"),
    I("float", "double", "MLP", "float", "ROWS", np.float32, 2, 6, 8, 300, 5, "nobias", None, "spinup", "abi"),
    I("float", "double", "MLP", "half", "ROWS", np.float16, 3, 9, 9, 200, 5, "leaky", None, "reference", "abi"),
    I("float", "double", "ROWS", "float", "ROWS", np.float32, 16, 4, 1, 150, None, None, None, "reference", "api"),
    I("float", "double", "TABULAR", "float", "ROWS", "state", 3, 1, 8, 200, 5, None, None, "spinup", "api"),
    I("double", "double", "MLP", "float", "ROWS", np.float32, 3, 4, 7, 200, 5, "wide", None, "spinup", "api"),
    I("double", "double", "MLP", "half", "ROWS", np.float16, 16, 7, 8, 150, 1, "ident", None, "reference", "api"),
    I("double", "double", "ROWS", "float", "ROWS", np.float16, 2, 5, 9, 300, 5, None, None, "spinup", "api"),
    I("double", "double", "TABULAR", "float", "ROWS", "state", 2, 1, 7, 300, None, None, None, "reference", "api"),
    I("half", "double", "MLP", "float", "ROWS", np.float32, 2, 4, 8, 300, None, "leaky", None, "reference", "api"),
    I("half", "double", "MLP", "half", "ROWS", np.float16, 3, 5, 9, 200, 5, "deep", None, "spinup", "api"),
    I("half", "double", "ROWS", "float", "ROWS", np.float32, 3, 6, 7, 200, 1, None, None, "spinup", "api"),
    I("half", "double", "TABULAR", "float", "ROWS", "state", 16, 1, 8, 150, 5, None, None, "reference", "api"),
]
FIELDS = "PL PROB FORM XT VF obs nA dO E T cap actor critic boot route".split()


def _id(c):
    return "-".join(str(x) for x in c[:5])


def _spec(c):
    s = dict(zip(FIELDS, c))
    if s["obs"] == "state":
        s["dO"] = 1
    return s


# ---- one run, its three checks -----------------------------------------------------------------------------------------------------
def _run(gpu, s, seed=0):
    """Builds the log, the environments (pcg64 rejection, seeds 11 k + 3), the actor and the critic of spec s; runs one collect / collect_ppo
    on the route s names; returns everything the checks need."""
    from rl_offline_simulation_amd import _lib as L
    from rl_offline_simulation_amd.evaluators import RowPolicy, RowValue
    from rl_offline_simulation_amd.evaluators.obs_policy import obs_tensor
    discrete = s["obs"] == "state"
    d = _log(s["nA"], s["obs"], s["dO"], PLOG[s["PL"]], N=s.get("N", 3000), nS=s.get("nS", 40), seed=seed)
    E, nA, dO = s["E"], s["nA"], s["dO"]
    seeds = np.arange(E) * 11 + 3
    env = _env(**d, E=E, discrete=discrete)
    env.reset_sampler(seeds)
    env.reset()
    N = len(d["z"])
    xn, x0 = obs_tensor(d["next_obs"], gpu), obs_tensor(d["obs"], gpu)  # what an in-kernel network reads (state ids: f32)
    pdt = np.float32 if s["PROB"] == "float" else np.float64
    g = np.random.default_rng(seed + 7)
    actor = net = None
    if s["FORM"] == "MLP":
        net = actor = s["actor"] if not isinstance(s["actor"], str) else _actor(dO, nA, s["actor"], seed)
        P_next, P_init = (actor.forward(x).cpu().numpy() for x in (xn, x0))
        form = "mlp"
    elif s["FORM"] == "ROWS":
        lg = g.standard_normal((2, N, nA)) * 2
        P = np.exp(lg - lg.max(-1, keepdims=True))
        P = (P / P.sum(-1, keepdims=True)).astype(pdt)
        P_next, P_init = P[0], P[1]
        actor, form = RowPolicy(P_next, P_init), "rows"
    else:
        nS = int(max(d["z"].max(), d["z_next"].max())) + 1
        pi = g.dirichlet(np.ones(nA) * 0.7, size=nS).astype(pdt)
        P_next, P_init = pi[d["z_next"]], pi[d["z"]]
        actor, form = pi, "tabular"
    critic = vnet = None
    if s["VF"] == "MLP":
        vnet = critic = s["critic"] if not isinstance(s["critic"], str) else _critic(dO, s["critic"], seed)
    elif s["VF"] == "ROWS":
        critic = RowValue(g.standard_normal(N).astype(np.float32), g.standard_normal(N).astype(np.float32))
    T, cap, boot = s["T"], s["cap"], s["boot"]
    f32 = s["PROB"] == "float"
    if s["route"] == "api":
        if critic is None:
            c, p = env.collect(actor, T, max_episode_steps=cap), None
        else:
            p = env.collect_ppo(actor, critic, T, max_episode_steps=cap, bootstrap=boot, gamma=GAMMA, lam=LAM)
            c = p.collected
    else:
        c, p = _abi(env, actor, form, f32, critic, s["XT"] == "half", T, cap, boot)
    torch.cuda.synchronize()
    # the precision the kernel compares in: f32 only where the probabilities and p_log are both f32
    P_next, P_init = (np.asarray(x, np.float32 if f32 else np.float64) for x in (P_next, P_init))
    plog = d["p_log"] if f32 else d["p_log"].astype(np.float64)
    return dict(env=env, d=d, c=c, p=p, actor=actor, net=net, vnet=vnet, critic=critic, P_next=P_next, P_init=P_init, plog=plog,
                seeds=seeds, xn=xn, x0=x0, L=L)


def _abi(env, actor, form, f32, critic, x16, T, cap, boot):
    """collect / collect_ppo through the C ABI (offsim_vector_collect[_ppo]) with prob_mode from f32 and the critic's observations as f16
    (x16): the argument structs of VectorPSRS, the choices the API does not make."""
    from rl_offline_simulation_amd import _lib as L
    from rl_offline_simulation_amd.evaluators import MLPValue
    from rl_offline_simulation_amd.evaluators.ppo_buffer import PPOBatch, _advantages
    env.env._quiesce()
    env.env._orders_for_generic()
    pol, keep, _ = env._collect_policy(actor, form)
    if critic is None:
        return env._collect_launch(pol, keep, f32, T, cap or 0, True, True), None
    E, dev = env.num_envs, env.table.device
    val = L.CollectValue()
    if isinstance(critic, MLPValue):
        xn, x0 = env._x_tables()
        if x16:
            xn, x0 = xn.half(), x0.half()
        xs = env.obs.reshape(E, -1).to(xn.dtype).contiguous()
        ws, arr = critic._device_weights(dev)
        val.form, val.n_layers, val.layers_host = L.VALUE_MLP, len(ws), C.cast(arr, C.POINTER(L.MLPLayer))
        val.activation, val.slope = {"tanh": L.ACT_TANH, "relu": L.ACT_RELU, "leaky_relu": L.ACT_LEAKY_RELU, "identity": L.ACT_IDENTITY}[
            critic.activation], critic.slope
        val.x_dtype, val.dO = (L.F16 if x16 else L.F32), critic.dO
        val.x_start, val.x_next, val.x_init = L.ptr(xs), L.ptr(xn), L.ptr(x0)
        keep += [xs, xn, x0, ws]
    else:
        vn, v0 = critic.tables(env.table.N, dev)
        val.form, val.v_next, val.v_init = L.VALUE_ROWS, L.ptr(vn), L.ptr(v0)
        keep += [vn, v0]
    value, logp = (torch.zeros((T, E), dtype=torch.float32, device=dev) for _ in range(2))
    final_value = torch.zeros((E,), dtype=torch.float32, device=dev)
    v_trunc = torch.zeros((T, E), dtype=torch.float32, device=dev) if boot == "spinup" else None
    out = L.CollectPPOOut(value=L.ptr(value), logp=L.ptr(logp), final_value=L.ptr(final_value), v_trunc=L.ptr(v_trunc))
    c = env._collect_launch(pol, keep, f32, T, cap or 0, True, True, ppo=(val, out))
    rew = c.reward.to(torch.float32)
    flags = ((c.row >= 0).to(torch.uint8) * L.COLLECT_SERVED + c.terminated.to(torch.uint8) * L.COLLECT_TERMINATED
             + c.truncated.to(torch.uint8) * L.COLLECT_TRUNCATED).to(torch.uint8)
    adv_raw, ret, adv, mean, std = _advantages(rew, value, flags, final_value, v_trunc, GAMMA, LAM, True, boot)
    return c, PPOBatch(obs=c.obs, act=c.action, rew=rew, val=value, logp=logp, adv=adv, adv_raw=adv_raw, ret=ret, valid=c.row >= 0,
                       final_value=final_value, v_trunc=v_trunc, adv_mean=mean, adv_std=std, collected=c)


def _x64(obs, xt, dO):
    """recorded observations [..., dO] as the in-kernel networks read them, widened to f64 (f16 stays f16 first: exact)"""
    x = obs.reshape(-1, dO)
    return (x.half() if xt == "half" else x.float()).double().cpu()


def check_arithmetic(r, s):
    """a. probs, logp, val, final_value, v_trunc against f64 on the recorded obs / next_obs / final_obs."""
    c, p, T, E, nA = r["c"], r["p"], s["T"], s["E"], s["nA"]
    served = (c.row >= 0).cpu()
    assert int(served.sum()) > 0
    xt = s["XT"]
    dO = s["dO"]
    x = _x64(c.obs, xt, dO).reshape(T, E, dO)[served]
    if s["FORM"] == "MLP":
        z, dz = _f64(r["net"], x)
        _check_probs(c.probs.cpu()[served], z, dz)
        # the property the control-flow check rests on: the in-kernel probabilities are MLPPolicy.forward's bit for bit
        fw = r["actor"].forward(x.to(torch.float16 if xt == "half" else torch.float32).to(c.row.device)).cpu()
        assert torch.equal(c.probs.cpu()[served], fw)
        if p is not None:
            _check_logp(p.logp.cpu()[served], z, dz, c.action.cpu().long()[served])
    if p is None:
        return
    if s["FORM"] != "MLP":  # logp = logf((float) p_new[a]): the cast and logf, a few ulp of |log p|
        pr = c.probs.cpu()[served].double().gather(-1, c.action.cpu().long()[served].unsqueeze(-1))[:, 0]
        lp = torch.log(pr)
        assert bool(((p.logp.cpu()[served].double() - lp).abs() <= 4 * U * lp.abs().clamp(min=1.0)).all())
    if s["VF"] == "MLP":
        vnet = r["vnet"]
        _check_value(p.val.cpu()[served], vnet, x)
        fw = vnet.forward(x.to(torch.float16 if xt == "half" else torch.float32).to(c.row.device)).cpu()
        assert torch.equal(p.val.cpu()[served], fw)
        _check_value(p.final_value.cpu(), vnet, _x64(c.final_obs, xt, dO))
        if p.v_trunc is not None:
            tr = (c.truncated & ~c.terminated).cpu() & served
            if bool(tr.any()):
                _check_value(p.v_trunc.cpu()[tr], vnet, _x64(c.next_obs, xt, dO).reshape(T, E, dO)[tr])
    else:  # the critic's tables, read as they are: v_init at an initial observation, v_next at next_obs (at the steps of the environments
        # whose observations check_control_flow restated)
        vn, v0 = (np.asarray(v, np.float32) for v in (r["critic"].v_next, r["critic"].v_init))
        val = p.val.cpu().numpy()
        for e, ob in r["obs_row"].items():
            assert np.array_equal(val[:len(ob), e], np.asarray([vn[v] if v >= 0 else v0[-2 - v] for v in ob], np.float32)), e
        if p.v_trunc is not None:
            tr = ((c.truncated & ~c.terminated) & (c.row >= 0)).cpu()
            assert torch.equal(p.v_trunc.cpu()[tr], torch.from_numpy(vn)[c.row.cpu().long()[tr]])
    assert bool((p.val.cpu()[~served] == 0).all()) and bool((p.logp.cpu()[~served] == 0).all())


def check_control_flow(r, s, envs=None):
    """b. rows, terminated, truncated, reset, alive, status, the recorded observations and final_obs against tests/collect_host.py."""
    L, c, d = r["L"], r["c"], r["d"]
    E, T = s["E"], s["T"]
    envs = range(E) if envs is None else envs
    row, term, trunc = c.row.cpu().numpy(), c.terminated.cpu().numpy(), c.truncated.cpu().numpy()
    rst, alive, status = c.reset.cpu().numpy(), c.alive.cpu().numpy(), c.status.cpu().numpy()
    obs, final_obs, probs = c.obs.cpu().numpy(), c.final_obs.cpu().numpy(), c.probs.cpu().numpy()
    log_obs = lambda v: d["next_obs"][v] if v >= 0 else d["obs"][-2 - v]  # noqa: E731
    code = {"running": L.ST_OK, "exhausted": L.ST_EXHAUSTED, "no_init": L.ST_NO_INIT, "keyerror": L.ST_KEYERROR}
    r["obs_row"] = {}
    for e in envs:
        o = H.collect_rows(d["z"], d["a"], d["z_next"], d["done"], r["plog"], d["t0"], r["P_next"], r["P_init"], int(r["seeds"][e]), T,
                           s["cap"] or 0)
        n = len(o["rows"])
        assert np.array_equal(row[:n, e], o["rows"]) and (row[n:, e] == -1).all(), e
        assert np.array_equal(term[:n, e], o["terminated"]) and not term[n:, e].any(), e
        assert np.array_equal(trunc[:n, e], o["truncated"]) and not trunc[n:, e].any(), e
        assert np.array_equal(rst[:n, e], o["reset"]) and not rst[n:, e].any(), e
        assert np.array_equal(alive[:n, e], ~(o["terminated"] | o["truncated"]) | o["reset"]) and not alive[n:, e].any(), e
        want = L.ST_INACTIVE if o["held"] == -1 else code[o["end"]]
        assert status[e] == want, (e, status[e], o["end"])
        # the observations, bit for bit (f16 of odd width: wave_copy_row's byte path), and p_new: the tables' rows as f32
        if n:
            assert np.stack([log_obs(v) for v in o["obs_row"]]).tobytes() == obs[:n, e].tobytes(), e
            pt = np.stack([r["P_next"][v] if v >= 0 else r["P_init"][-2 - v] for v in o["obs_row"]]).astype(np.float32)
            assert np.array_equal(probs[:n, e], pt), e
        k = n + 1 if o["end"] == "exhausted" else n  # a step that returns None was asked at the observation held
        if k > n:
            assert np.asarray(log_obs(o["held"])).tobytes() == obs[n, e].tobytes(), e
        assert not obs[k:, e].any()
        if o["held"] != -1:
            assert np.asarray(log_obs(o["held"])).tobytes() == final_obs[e].tobytes(), e
        r["obs_row"][e] = o["obs_row"]


def check_buffer(r, s):
    """c. the buffer against tests/ppo_host.py on the recorded values."""
    if r["p"] is not None:
        host_check(r["p"], GAMMA, LAM, s["boot"])


def _all_checks(r, s, envs=None):
    check_control_flow(r, s, envs)
    check_arithmetic(r, s)
    check_buffer(r, s)


def test_instance_table_is_complete():
    """The table lists every instance collect_launch dispatches, once: 4 (PL, PROB) x (4 without a critic + 6 with an MLP critic + 4 with a
    rows critic)."""
    keys = [c[:5] for c in INSTANCES]
    assert len(keys) == len(set(keys)) == 56
    plp = [("float", "float"), ("float", "double"), ("double", "double"), ("half", "double")]
    fx = {"NONE": [("MLP", "float"), ("MLP", "half"), ("ROWS", "float"), ("TABULAR", "float")],
          "ROWS": [("MLP", "float"), ("MLP", "half"), ("ROWS", "float"), ("TABULAR", "float")],
          "MLP": [(f, x) for f in ("MLP", "ROWS", "TABULAR") for x in ("float", "half")]}
    assert set(keys) == {pp + f + (vf,) for pp in plp for vf, fs in fx.items() for f in fs}
    for c in INSTANCES:
        s = _spec(c)
        assert (s["route"] == "abi") == ((s["PROB"] == "double" and s["PL"] == "float" and s["FORM"] == "MLP")
                                         or (s["FORM"] == "TABULAR" and s["XT"] == "half"))
        assert s["E"] in (1, 7, 8, 9) and s["nA"] in (2, 3, 16) and s["cap"] in (None, 1, 5) and s["T"] <= 300


@pytest.mark.parametrize("case", INSTANCES, ids=[_id(c) for c in INSTANCES])
def test_instance(gpu, case):
    s = _spec(case)
    _all_checks(_run(gpu, s), s)


# ---- the edges, each a named case through the same three checks ---------------------------------------------------------------------
NETS["cident"] = (2, 20, "identity", 0.01, True, 1.0)


def _edge(PL="float", PROB="float", FORM="MLP", XT="float", VF="MLP", obs=np.float32, nA=3, dO=4, E=8, T=200, cap=5, actor="small",
          critic="small", boot="spinup", route="api", **kw):
    s = dict(PL=PL, PROB=PROB, FORM=FORM, XT=XT, VF=VF, obs=obs, nA=nA, dO=dO, E=E, T=T, cap=cap, actor=actor, critic=critic, boot=boot,
             route=route, **kw)
    if obs == "state":
        s["dO"] = 1
    return s


EDGES = {
    "actor_hidden_200": _edge(actor="wide", nA=16, dO=9),
    "critic_hidden_250": _edge(critic="cwide", E=9, boot="reference"),
    "critic_wider_than_mlp_actor_f16": _edge(XT="half", obs=np.float16, dO=5, actor="deep", critic="cwide", cap=1),
    "rows_actor_wide_critic": _edge(FORM="ROWS", actor=None, critic="cwide", nA=2, E=7),
    "tabular_actor_wide_critic": _edge(FORM="TABULAR", obs="state", actor=None, critic="cwide", nA=16, E=9, cap=None, boot="reference"),
    "depth_4": _edge(PL="double", PROB="double", actor="deep", critic="cdeep", nA=16),
    "no_bias_actor_and_critic": _edge(PL="half", PROB="double", actor="nobias", critic="cnobias", cap=None, boot="reference"),
    "leaky_relu_slopes_0.2_0.3": _edge(actor="leaky", critic="cdeep", nA=2, E=1, T=300),
    "identity_actor_and_critic": _edge(XT="half", obs=np.float16, dO=7, actor="ident", critic="cident", nA=3, E=7),
    "f16_odd_width_3_no_critic": _edge(XT="half", obs=np.float16, dO=3, VF="NONE", critic=None, boot=None, nA=2, E=9, T=300),
    "logits_in_the_hundreds": _edge(PL="double", PROB="double", actor="hot", nA=16, E=7, cap=None, boot="reference"),
}


@pytest.mark.parametrize("name", list(EDGES))
def test_edge(gpu, name):
    s = EDGES[name]
    r = _run(gpu, s)
    _all_checks(r, s)
    if name == "logits_in_the_hundreds":  # the case is what it says
        z, _ = _f64(r["net"], _x64(r["c"].obs, "float", s["dO"]).reshape(s["T"], s["E"], -1)[(r["c"].row >= 0).cpu()])
        assert float(z.abs().max()) >= 100.0


def test_many_workgroups_4099_environments(gpu):
    """E = 4099: 513 workgroups, the last one with three environments.  The host restatement on the environments at wavefront and
    workgroup boundaries; every environment through the arithmetic and the buffer, and collect_ppo's trajectory against collect's."""
    s = _edge(E=4099, T=64, cap=5, nA=3, dO=6, actor="leaky", critic="cdeep")
    r = _run(gpu, s)
    _all_checks(r, s, envs=(0, 7, 8, 63, 64, 4095, 4098))
    twin = _env(**r["d"], E=s["E"])
    twin.reset_sampler(r["seeds"])
    twin.reset()
    c = twin.collect(r["actor"], s["T"], max_episode_steps=s["cap"])
    for f in ("row", "obs", "probs", "terminated", "truncated", "reset", "alive", "final_obs", "status"):
        assert torch.equal(getattr(r["c"], f), getattr(c, f)), f


def _lds(n_slots, nA, prob_bytes, critic_floats, w_max, waves=8):
    """collect_lds_layout for a tabular actor and an MLP critic: jump tables, pi and the critic's weights, p_new / probs per wave, two
    activation rows per wave (bytes)."""
    a16 = lambda b: (b + 15) // 16 * 16  # noqa: E731
    return waves * 65 * 32 + a16(a16(n_slots * nA * prob_bytes) + 4 * critic_floats) + waves * 16 * (8 + 4) + waves * 2 * w_max * 4


def test_tabular_and_critic_above_64k_of_lds(gpu):
    """A tabular pi of 600 states x 16 actions (f64) and a 1 -> 256 -> h -> 1 critic: the widest h whose launch fits 160 KiB of LDS runs
    (through allow_big_lds) and passes the three checks; h + 1 is refused with OFFSIM_EUNSUPPORTED before any launch."""
    from rl_offline_simulation_amd import _lib as L
    from rl_offline_simulation_amd.evaluators import MLPValue
    s = _edge(PL="double", PROB="double", FORM="TABULAR", obs="state", actor=None, nA=16, E=9, T=100, N=20000, nS=600)
    d = _log(16, "state", 1, np.float64, N=20000, nS=600)
    n_slots = _env(**d, E=1, discrete=True).table.n_slots
    floats = lambda h: 256 + 256 + 256 * h + h + h + 1  # noqa: E731
    h = max(h for h in range(1, 257) if _lds(n_slots, 16, 8, floats(h), 256) <= 160 * 1024)
    assert 64 * 1024 < _lds(n_slots, 16, 8, floats(h), 256) <= 160 * 1024 < _lds(n_slots, 16, 8, floats(h + 1), 256)
    assert floats(h + 1) <= L.COLLECT_MLP_MAX_FLOATS  # (the refusal below is the LDS limit's, not the float budget's)

    def critic(h):
        g = torch.Generator().manual_seed(h)
        return MLPValue([(torch.randn(256, 1, generator=g), torch.randn(256, generator=g) * 0.5),
                         (torch.randn(h, 256, generator=g) / 16, torch.randn(h, generator=g) * 0.5),
                         (torch.randn(1, h, generator=g) / h ** 0.5, torch.randn(1, generator=g))], "tanh")

    s["critic"] = critic(h)
    r = _run(gpu, s)
    _all_checks(r, s)
    env = r["env"]
    with pytest.raises(L.OffsimError, match="160 KiB"):
        env.collect_ppo(r["actor"], critic(h + 1), 10)


def test_actor_and_critic_fill_the_weight_budget(gpu):
    """Actor 6 -> 12 -> 3 (123 floats) and critic 6 -> 73 -> 210 -> 1 without the last bias (16261 floats): exactly
    OFFSIM_COLLECT_MLP_MAX_FLOATS runs and passes the three checks; the critic's last bias, one float more, is refused."""
    from rl_offline_simulation_amd import _lib as L
    from rl_offline_simulation_amd.evaluators import MLPPolicy, MLPValue
    g = torch.Generator().manual_seed(5)
    actor = MLPPolicy([(torch.randn(12, 6, generator=g) * 0.6, torch.randn(12, generator=g) * 0.5),
                       (torch.randn(3, 12, generator=g) * 0.5, torch.randn(3, generator=g))], "tanh")
    cw = [(torch.randn(73, 6, generator=g) * 0.6, torch.randn(73, generator=g) * 0.5),
          (torch.randn(210, 73, generator=g) * 0.15, torch.randn(210, generator=g) * 0.5), (torch.randn(1, 210, generator=g) * 0.1, None)]
    count = lambda ws: sum(W.numel() + (0 if b is None else b.numel()) for W, b in ws)  # noqa: E731
    assert count(actor.weights) + count(cw) == L.COLLECT_MLP_MAX_FLOATS
    s = _edge(nA=3, dO=6, E=9, actor=actor, critic=MLPValue(cw, "tanh"))
    r = _run(gpu, s)
    _all_checks(r, s)
    over = MLPValue(cw[:2] + [(cw[2][0], torch.zeros(1))], "tanh")
    with pytest.raises(L.OffsimError, match="OFFSIM_COLLECT_MLP_MAX_FLOATS"):
        r["env"].collect_ppo(actor, over, 10)


# ---- the standalone forwards at the shapes the in-kernel ones use -------------------------------------------------------------------
FORWARDS = [  # (depth, hidden, nA, activation, slope, observation dtype, dO)
    (4, 24, 3, "relu", 0.01, torch.float32, 6),
    (4, 40, 16, "leaky_relu", 0.3, torch.float16, 7),
    (3, 200, 3, "tanh", 0.01, torch.float32, 9),     # 200 -> 200: k_policy_mlp stages 81 + 81 + 38 output rows (a partial chunk)
    (3, 200, 16, "identity", 0.01, torch.float16, 5),
]


@pytest.mark.parametrize("depth,hidden,nA,act,slope,xdt,dO", FORWARDS)
def test_standalone_forward_against_f64(gpu, depth, hidden, nA, act, slope, xdt, dO):
    """MLPPolicy.forward / MLPValue.forward (offsim_policy_mlp / offsim_value_mlp) against f64 with the forward error bound, and the
    in-kernel forward of collect / collect_ppo at the same shape against them bit for bit."""
    from rl_offline_simulation_amd import _lib as L
    from rl_offline_simulation_amd.evaluators import MLPPolicy, MLPValue
    NETS["_fw"] = (depth, hidden, act, slope, True, 1.0)
    pol = MLPPolicy(_weights(dO, nA, "_fw", 3), act, slope)
    val = MLPValue(_weights(dO, 1, "_fw", 4), act, slope)
    g = torch.Generator().manual_seed(depth * hidden)
    x = (torch.randn(1000, dO, generator=g) * 2).to(xdt)
    rows = torch.randint(0, 1000, (777,), generator=g, dtype=torch.int32)
    xr = x.double()[rows.long()]
    z, dz = _f64(pol, xr)
    _check_probs(pol.forward(x.to(gpu), rows.to(gpu)).cpu(), z, dz)
    _check_value(val.forward(x.to(gpu), rows.to(gpu)).cpu(), val, xr)
    if sum(W.numel() + b.numel() for W, b in pol.weights + val.weights) > L.COLLECT_MLP_MAX_FLOATS:
        return  # (200 -> 200 does not fit the in-kernel networks' LDS: collect refuses it, test_gpu_collect.py pins that)
    xt = "half" if xdt == torch.float16 else "float"
    s = _edge(PL="float", PROB="float", XT=xt, obs=np.float16 if xt == "half" else np.float32, dO=dO, nA=nA, E=7, T=100, actor=pol,
              critic=val)
    r = _run(gpu, s)
    check_control_flow(r, s)
    check_arithmetic(r, s)  # includes probs == MLPPolicy.forward and val == MLPValue.forward, bit for bit


@pytest.mark.parametrize("row_bytes", [1, 2, 3, 4, 6, 8, 10, 12, 32])
def test_gather_rows_of_any_width(gpu, row_bytes):
    """offsim_gather_rows (TransitionTable's grouped layout) for rows of any width: an f16 p_log of an odd nA has rows of 6 bytes, which
    it used to refuse, so no log with f16 probabilities and 3 actions could be loaded."""
    from rl_offline_simulation_amd.table import gather_rows
    g = torch.Generator().manual_seed(row_bytes)
    src = torch.randint(0, 256, (1001, row_bytes), generator=g, dtype=torch.uint8)
    order = torch.randperm(1001, generator=g)[:777].to(torch.int32)
    assert torch.equal(gather_rows(src.to(gpu), order.to(gpu)).cpu(), src[order.long()])
    if row_bytes % 2 == 0:
        h = src.view(torch.float16)
        assert torch.equal(gather_rows(h.to(gpu), order.to(gpu)).cpu().view(torch.uint8), src[order.long()])
