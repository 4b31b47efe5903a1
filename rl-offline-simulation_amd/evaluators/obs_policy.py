"""Policies over observations for evalMC_psrs (offsim4rl/evaluators/psrs.py:241-271 with p = pi[S], S the observation, :255).

The reference indexes any `pi` by the observation, so the policy people evaluate there is the PPO actor it trains inside PSRS
(offsim4rl/agents/ppo.py:18-27: spinup's MLPCategoricalActor, probs = softmax(logits_net(obs))).  Inside evalMC the policy is only
ever asked at two kinds of observation -- next_obs of the row just accepted (psrs.py:49-51) and obs of the initial row just popped
(psrs.py:32-37) -- so a policy over observations is exactly two per-row probability tables, computed once, up front:

  P_next[g]  the policy at next_obs of GROUPED row g (the table's order, caller row table.order[g])
  P_init[k]  the policy at obs of the k-th initial row (caller row table.init_orig[k])

and the scan (offsim_eval_mc_rows_policy) takes p_new from them instead of pi[slot].  Every policy class here produces that pair on the
device (`row_tables`):

  MLPPolicy        Linear / activation stacks, forward by the HIP kernel offsim_policy_mlp, written straight in grouped order
                   (its `rows` gather index is table.order for P_next and table.init_orig for P_init: no second gather pass)
  RowPolicy        per-row probabilities the caller already has, in caller order (gathered into the two tables on the device)
  CallablePolicy   any fn(obs_tensor) -> probs, run by torch on the device in chunks (plumbing: the scan is still the HIP kernel)

PolicyPopulation is L such policies evaluated together on the same seeds: the pair stacked, [L, N, nA] and [L, N0, nA], for stacked MLPs
by one launch of offsim_policy_mlp_pop, read by the population form of the scan (offsim_eval_mc_rows_policy_pop).
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L
from ..table import gather_rows

_ACT = {"tanh": L.ACT_TANH, "relu": L.ACT_RELU, "leaky_relu": L.ACT_LEAKY_RELU, "identity": L.ACT_IDENTITY}


def obs_tensor(obs, device):
    """Observations [N, dO] as one contiguous device tensor (f16 kept, anything else f32)."""
    if isinstance(obs, torch.Tensor):
        t = obs.to(device)
    else:
        a = np.asarray(obs) if not isinstance(obs, (list, tuple)) else np.stack([np.asarray(o) for o in obs]) if len(obs) else np.zeros((0, 1))
        t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    if t.dtype not in (torch.float32, torch.float16):
        t = t.to(torch.float32)
    return t.reshape(t.shape[0], -1).contiguous()


def _sequential_layers(net, who):
    """(layers [(W, b)], activation, slope) of an nn.Sequential of Linear layers with one activation kind between them, optionally
    followed by one nn.Identity (spinup's mlp(..., output_activation=nn.Identity)); anything else raises TypeError."""
    kinds = {torch.nn.Tanh: "tanh", torch.nn.ReLU: "relu", torch.nn.LeakyReLU: "leaky_relu", torch.nn.Identity: "identity"}
    mods = list(net)
    if len(mods) >= 2 and type(mods[-1]) is torch.nn.Identity and isinstance(mods[-2], torch.nn.Linear):
        mods = mods[:-1]
    layers, acts, slope, expect_linear = [], [], 0.01, True
    for mod in mods:
        if isinstance(mod, torch.nn.Linear):
            if not expect_linear and layers:
                raise TypeError(f"{who}.from_torch: two Linear layers without an activation between them")
            layers.append((mod.weight, mod.bias))
            expect_linear = False
        elif type(mod) in kinds:
            if expect_linear:
                raise TypeError(f"{who}.from_torch: an activation must follow a Linear layer")
            acts.append(kinds[type(mod)])
            if isinstance(mod, torch.nn.LeakyReLU):
                slope = float(mod.negative_slope)
            expect_linear = True
        else:
            raise TypeError(f"{who}.from_torch: unsupported module {type(mod).__name__} (Linear, Tanh, ReLU, LeakyReLU, Identity only)")
    if not layers or expect_linear:
        raise TypeError(f"{who}.from_torch: the network must end with a Linear layer (its outputs are the logits)")
    if len(set(acts)) > 1:
        raise TypeError(f"{who}.from_torch: one activation kind between all layers, got {acts}")
    if acts and acts[0] == "leaky_relu" and len({float(x.negative_slope) for x in mods if isinstance(x, torch.nn.LeakyReLU)}) > 1:
        raise TypeError(f"{who}.from_torch: LeakyReLU layers with different slopes")
    return layers, acts[0] if acts else "identity", slope


class ObsPolicy:
    """Base: a policy over observations, turned into (P_next grouped [N, nA], P_init [N0, nA]) device tensors for a table."""

    def row_tables(self, table, obs, next_obs):
        raise NotImplementedError


class _MLPNet:
    """Linear layers with one activation kind between them, in state_dict layout as the HIP forwards read them (MLPPolicy, MLPValue)."""

    def __init__(self, weights, activation="tanh", slope=0.01):
        if activation not in _ACT:
            raise ValueError(f"{type(self).__name__}: activation must be one of {sorted(_ACT)}, got {activation!r}")
        if not 1 <= len(weights) <= L.POLICY_MLP_MAX_LAYERS:
            raise ValueError(f"{type(self).__name__}: 1 to {L.POLICY_MLP_MAX_LAYERS} Linear layers, got {len(weights)}")
        self.weights = []
        for W, b in weights:
            W = torch.as_tensor(W.detach() if isinstance(W, torch.Tensor) else np.asarray(W)).to(torch.float32).contiguous()
            b = None if b is None else torch.as_tensor(b.detach() if isinstance(b, torch.Tensor) else np.asarray(b)).to(torch.float32).contiguous()
            if W.dim() != 2 or (b is not None and b.shape != (W.shape[0],)):
                raise ValueError(f"{type(self).__name__}: every layer is (W [out, in], b [out] or None)")
            self.weights.append((W, b))
        for (W0, _), (W1, _) in zip(self.weights, self.weights[1:]):
            if W1.shape[1] != W0.shape[0]:
                raise ValueError(f"{type(self).__name__}: layer widths do not chain")
        self.activation, self.slope = activation, float(slope)
        self.nA = int(self.weights[-1][0].shape[0])
        self.dO = int(self.weights[0][0].shape[1])
        self._dev = {}

    def _device_weights(self, device):
        key = str(device)
        if key not in self._dev:
            ws = [(W.to(device), None if b is None else b.to(device)) for W, b in self.weights]
            arr = (L.MLPLayer * len(ws))()
            for i, (W, b) in enumerate(ws):
                arr[i].W, arr[i].b = L.ptr(W), L.ptr(b)
                setattr(arr[i], "in", int(W.shape[1]))
                arr[i].out = int(W.shape[0])
            self._dev[key] = (ws, arr)
        return self._dev[key]

    _value = False  # MLPValue: the entry point is offsim_value_mlp and the output [M], not offsim_policy_mlp and [M, nA]

    def forward(self, x, rows=None, out=None):
        """The HIP forward, f32 on x's device (MLPPolicy: probs [M, nA]; MLPValue: v [M]): x [n, dO] f32 / f16 device tensor, rows
        (optional) [M] int32 gather index into x."""
        if x.dim() != 2 or x.shape[1] != self.dO:
            raise ValueError(f"{type(self).__name__}: observations of width {self.dO} expected, got shape {tuple(x.shape)}")
        if x.dtype not in (torch.float32, torch.float16):
            x = x.to(torch.float32)
        x = x.contiguous()
        if rows is not None:
            rows = rows.to(device=x.device, dtype=torch.int32).contiguous()
        M = int(x.shape[0]) if rows is None else int(rows.numel())
        if out is None:
            out = torch.empty((M,) if self._value else (M, self.nA), dtype=torch.float32, device=x.device)
        ws, arr = self._device_weights(x.device)
        entry = L.load().offsim_value_mlp if self._value else L.load().offsim_policy_mlp
        L.check(entry(L.ptr(x) if x.numel() else None, L.F32 if x.dtype == torch.float32 else L.F16, int(x.shape[0]), self.dO,
                      L.ptr(rows) if rows is not None and M else None, M, arr, len(ws), _ACT[self.activation], self.slope,
                      L.ptr(out) if M else None, L.stream_ptr()))
        return out

    def refresh_host(self, device=None):
        """Copy the device weights back into self.weights (a learner that owns the device copy -- PPOLearner -- updates it in place, and
        the host copy is only brought up to date here, on demand).  device: which copy (default: the only one there is).  Synchronises."""
        if not self._dev:
            return self
        if device is None and len(self._dev) > 1:
            raise ValueError(f"{type(self).__name__}.refresh_host: copies on {sorted(self._dev)} exist, say which device to read")
        key = str(device) if device is not None else next(iter(self._dev))
        ws, _ = self._dev[key]
        self.weights = [(W.detach().cpu().clone(), None if b is None else b.detach().cpu().clone()) for W, b in ws]
        return self

    def state_dict(self, device=None):
        """The current weights as an nn.Sequential's state_dict of to_torch()'s layout: {'0.weight', '0.bias', '2.weight', ...} (CPU
        tensors, refreshed from the device copy first)."""
        self.refresh_host(device)
        out = {}
        for i, (W, b) in enumerate(self.weights):
            out[f"{2 * i}.weight"] = W.clone()
            if b is not None:
                out[f"{2 * i}.bias"] = b.clone()
        return out

    def to_torch(self, device=None):
        """An nn.Sequential of the current weights (Linear, activation, ..., Linear, Identity -- spinup's mlp() layout), on the CPU."""
        acts = {"tanh": torch.nn.Tanh, "relu": torch.nn.ReLU, "identity": torch.nn.Identity,
                "leaky_relu": lambda: torch.nn.LeakyReLU(self.slope)}
        sd = self.state_dict(device)
        mods = []
        for i, (W, b) in enumerate(self.weights):
            mods += [torch.nn.Linear(int(W.shape[1]), int(W.shape[0]), bias=b is not None),
                     acts[self.activation]() if i < len(self.weights) - 1 else torch.nn.Identity()]
        net = torch.nn.Sequential(*mods)
        net.load_state_dict(sd)
        return net


class MLPPolicy(_MLPNet, ObsPolicy):
    """probs = softmax(L_n(act(... act(L_1(obs))))) -- spinup's MLPCategoricalActor (ppo.py:18-27) -- on the HIP forward.

    weights: list of (W [out, in], b [out] or None), state_dict layout; activation: 'tanh' | 'relu' | 'leaky_relu' | 'identity' between
    layers (slope: leaky_relu's negative slope).  1-4 layers, observation width <= 128, hidden widths <= 256, <= 16 actions."""

    @classmethod
    def from_torch(cls, m):
        """An nn.Sequential of Linear and Tanh | ReLU | LeakyReLU | Identity (one activation kind, between the Linear layers), or any object
        with such a `.logits_net` (spinup's MLPCategoricalActor).  A trailing nn.Identity after the last Linear (spinup's mlp() output
        activation) is dropped.  Anything else is refused."""
        net = m.logits_net if hasattr(m, "logits_net") else m
        if not isinstance(net, torch.nn.Sequential):
            raise TypeError(f"MLPPolicy.from_torch: needs an nn.Sequential (or an object with .logits_net), got {type(m).__name__}")
        return cls(*_sequential_layers(net, "MLPPolicy"))

    def row_tables(self, table, obs, next_obs):
        xn, x0 = obs_tensor(next_obs, table.device), obs_tensor(obs, table.device)
        return self.forward(xn, table.order), self.forward(x0, table.init_orig)


class RowPolicy(ObsPolicy):
    """Per-row probabilities in caller order: p_next[i] = the policy at next_obs[i], p_init[i] = the policy at obs[i] (only the rows with
    t == 0 are read).  f32 tables with an f32 p_log run the scan's f32 mode, anything else is widened exactly to f64."""

    def __init__(self, p_next, p_init):
        self.p_next, self.p_init = p_next, p_init

    @staticmethod
    def _dev(p, device):
        t = p.to(device) if isinstance(p, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(p)).to(device)
        if t.dtype not in (torch.float32, torch.float64):
            t = t.to(torch.float64)
        return t.contiguous()

    def caller_tables(self, table):
        """(p_next, p_init) [N, nA] on the table's device, in caller row order, shapes checked, of one dtype (f32 or f64)."""
        pn, p0 = self._dev(self.p_next, table.device), self._dev(self.p_init, table.device)
        for name, p in (("p_next", pn), ("p_init", p0)):
            if p.dim() != 2 or p.shape[0] != table.N or p.shape[1] != table.nA:
                raise ValueError(f"RowPolicy: {name} must be [{table.N}, {table.nA}] (one row per logged transition), got {tuple(p.shape)}")
        if pn.dtype != p0.dtype:
            pn, p0 = pn.to(torch.float64), p0.to(torch.float64)
        return pn, p0

    def row_tables(self, table, obs=None, next_obs=None):
        pn, p0 = self.caller_tables(table)
        return gather_rows(pn, table.order), gather_rows(p0, table.init_orig)


class _StackedMLP:
    """L MLPPolicy's of one architecture, stacked per layer (W [L, out, in], b [L, out]): the host copies, and per device the stacked
    tensors with the offsim_mlp_layer array that describes learner 0 -- what PPOPopulation's own stack offers, for policies that come
    from anywhere else."""

    def __init__(self, policies):
        for p in policies:
            if not isinstance(p, MLPPolicy):
                raise ValueError(f"PolicyPopulation.from_policies: every policy must be an MLPPolicy, got {type(p).__name__}")
        first = policies[0]
        self.n, self.policies = len(policies), list(policies)
        self.activation, self.slope, self.dO, self.nA = first.activation, first.slope, first.dO, first.nA
        shape = [(tuple(W.shape), b is not None) for W, b in first.weights]
        for p in policies:
            if[(tuple(W.shape), b is not None) for W, b in p.weights] != shape or (p.activation, p.slope) != (self.activation, self.slope):
                raise ValueError("PolicyPopulation.from_policies: all policies share one architecture (layer shapes, biases, activation, slope)")
        self.host = [(torch.stack([p.weights[i][0] for p in policies]), torch.stack([p.weights[i][1] for p in policies]) if has_b else None)
                     for i, (_, has_b) in enumerate(shape)]
        self._dev = {}

    def _device_weights(self, device):
        key = str(device)
        if key not in self._dev:
            ws = [(W.to(device).contiguous(), None if b is None else b.to(device).contiguous()) for W, b in self.host]
            self._dev[key] = (ws, _stacked_layers(ws, 0))
        return self._dev[key]

    def export(self, l):
        return self.policies[l]


def _stacked_layers(ws, lo):
    """the offsim_mlp_layer array of learner `lo` of stacked tensors [(W [L, out, in], b [L, out] or None)]"""
    arr = (L.MLPLayer * len(ws))()
    for i, (W, b) in enumerate(ws):
        arr[i].W, arr[i].b = L.ptr(W[lo:]), None if b is None else L.ptr(b[lo:])
        setattr(arr[i], "in", int(W.shape[2]))
        arr[i].out = int(W.shape[1])
    return arr


class PolicyPopulation:
    """L policies over observations, evaluated together on the same seeds (BatchedPSRS.eval_mc_rows_policy_population,
    evalmc_rollouts_population): `row_tables` gives their per-row tables stacked, P_next [L, N, nA] and P_init [L, N0, nA].

      from_policies([MLPPolicy, ...])   policies of one architecture; their weights are stacked once per device and every forward is ONE
                                        launch for all of them (offsim_policy_mlp_pop)
      from_ppo(PPOPopulation)           the population's own stacked actor weights, as they are: no copy, so an evaluation after
                                        PPOPopulation.update sees the new weights
      from_rows([RowPolicy | CallablePolicy | any ObsPolicy, ...])   each policy's own row_tables, stacked
    """

    def __init__(self, stack=None, rows=None):
        if (stack is None) == (rows is None):
            raise ValueError("PolicyPopulation: use from_policies, from_ppo or from_rows")
        self._stack, self._rows = stack, rows

    @classmethod
    def from_policies(cls, policies):
        policies = list(policies)
        if not policies:
            raise ValueError("PolicyPopulation.from_policies: no policies")
        return cls(stack=_StackedMLP(policies))

    @classmethod
    def from_ppo(cls, population):
        if not hasattr(population, "_pi") or not hasattr(population._pi, "_device_weights"):
            raise TypeError(f"PolicyPopulation.from_ppo: needs a PPOPopulation, got {type(population).__name__}")
        return cls(stack=population._pi)

    @classmethod
    def from_rows(cls, policies):
        policies = list(policies)
        if not policies:
            raise ValueError("PolicyPopulation.from_rows: no policies")
        for p in policies:
            if not isinstance(p, ObsPolicy):
                raise ValueError(f"PolicyPopulation.from_rows: every policy must be a policy over observations, got {type(p).__name__}")
        return cls(rows=policies)

    def __len__(self):
        return self._stack.n if self._stack is not None else len(self._rows)

    def policy(self, l):
        """policy l on its own (from_ppo: a copy of learner l's actor with its current weights)"""
        if not 0 <= l < len(self):
            raise IndexError(f"PolicyPopulation: policy {l} of {len(self)}")
        return self._stack.export(l) if self._stack is not None else self._rows[l]

    def needs_obs(self):
        """whether row_tables reads the log's observations (everything but a population of RowPolicy's)"""
        return self._stack is not None or not all(hasattr(p, "p_next") for p in self._rows)

    def forward(self, x, rows=None, lo=0, hi=None):
        """probs [hi - lo, M, nA] of the stacked networks lo .. hi - 1 (default: all) in one launch: x [n, dO] f32 / f16 device tensor,
        rows (optional) [M] int32 gather index into x.  Every [M, nA] equals that policy's MLPPolicy.forward bit for bit."""
        st = self._stack
        if st is None:
            raise TypeError("PolicyPopulation.forward: a population of row tables has no network")
        hi = st.n if hi is None else hi
        if not 0 <= lo < hi <= st.n:
            raise IndexError(f"PolicyPopulation.forward: policies {lo}..{hi} of {st.n}")
        if x.dim() != 2 or x.shape[1] != st.dO:
            raise ValueError(f"PolicyPopulation: observations of width {st.dO} expected, got shape {tuple(x.shape)}")
        if x.dtype not in (torch.float32, torch.float16):
            x = x.to(torch.float32)
        x = x.contiguous()
        if rows is not None:
            rows = rows.to(device=x.device, dtype=torch.int32).contiguous()
        M = int(x.shape[0]) if rows is None else int(rows.numel())
        out = torch.empty((hi - lo, M, st.nA), dtype=torch.float32, device=x.device)
        ws, arr = st._device_weights(x.device)
        if lo:
            arr = _stacked_layers(ws, lo)
        L.check(L.load().offsim_policy_mlp_pop(L.ptr(x) if x.numel() else None, L.F32 if x.dtype == torch.float32 else L.F16, int(x.shape[0]), st.dO,
                                               L.ptr(rows) if rows is not None and M else None, M, arr, len(ws), _ACT[st.activation], st.slope,
                                               hi - lo, L.ptr(out) if M else None, L.stream_ptr()))
        return out

    def row_tables(self, table, obs=None, next_obs=None, lo=0, hi=None):
        """(P_next [hi - lo, N, nA] in grouped order, P_init [hi - lo, N0, nA] in init_orig order) of policies lo .. hi - 1 (default: all)
        on the table's device."""
        hi = len(self) if hi is None else hi
        if self._stack is not None:
            xn, x0 = obs_tensor(next_obs, table.device), obs_tensor(obs, table.device)
            return self.forward(xn, table.order, lo, hi), self.forward(x0, table.init_orig, lo, hi)
        pairs = [p.row_tables(table, obs, next_obs) for p in self._rows[lo:hi]]
        dt = torch.float32 if all(p.dtype == torch.float32 for pr in pairs for p in pr) else torch.float64
        return (torch.stack([pn.to(dt).reshape(table.N, table.nA) for pn, _ in pairs]),
                torch.stack([p0.to(dt).reshape(table.N0, table.nA) for _, p0 in pairs]))


class MLPValue(_MLPNet):
    """v = L_n(act(... act(L_1(obs)))) with one output unit -- spinup's MLPCritic (ppo.py:18-27: v = squeeze(v_net(obs), -1)) -- on the
    HIP forward (offsim_value_mlp), and the critic VectorPSRS.collect_ppo runs inside its kernel.  Layers, activations and limits are
    MLPPolicy's; the last layer has one output."""
    _value = True

    def __init__(self, weights, activation="tanh", slope=0.01):
        super().__init__(weights, activation, slope)
        if self.nA != 1:
            raise ValueError(f"MLPValue: the last layer must have one output, got {self.nA}")

    @classmethod
    def from_torch(cls, m):
        """An nn.Sequential as MLPPolicy.from_torch takes, ending in Linear(H, 1) (a trailing nn.Identity is dropped), or any object with
        such a `.v_net` (spinup's MLPCritic)."""
        net = m.v_net if hasattr(m, "v_net") else m
        if not isinstance(net, torch.nn.Sequential):
            raise TypeError(f"MLPValue.from_torch: needs an nn.Sequential (or an object with .v_net), got {type(m).__name__}")
        return cls(*_sequential_layers(net, "MLPValue"))


class RowValue:
    """A critic as per-row values in caller order: v_next[i] = v(next_obs[i]), v_init[i] = v(obs[i]) (only the rows with t == 0 are
    read) -- any torch critic through its tables, for VectorPSRS.collect_ppo (offsim_collect_value's ROWS form).  Read as f32."""

    def __init__(self, v_next, v_init):
        self.v_next, self.v_init = v_next, v_init

    def tables(self, N, device):
        out = []
        for name, v in (("v_next", self.v_next), ("v_init", self.v_init)):
            t = v.to(device) if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v)).to(device)
            t = t.to(torch.float32).reshape(-1).contiguous()
            if t.numel() != N:
                raise ValueError(f"RowValue: {name} must have {N} entries (one per logged transition), got {t.numel()}")
            out.append(t)
        return out


class CallablePolicy(ObsPolicy):
    """fn(obs [m, dO] device tensor) -> probs [m, nA], evaluated by torch on the device in chunks of `chunk` rows (under no_grad)."""

    def __init__(self, fn, chunk=1 << 16):
        self.fn, self.chunk = fn, int(chunk)

    def _run(self, x):
        outs = []
        with torch.no_grad():
            for b in range(0, int(x.shape[0]), self.chunk):
                p = self.fn(x[b:b + self.chunk])
                if hasattr(p, "probs") and not isinstance(p, torch.Tensor):  # a torch Distribution (Categorical)
                    p = p.probs
                outs.append(torch.as_tensor(p, device=x.device))
        if not outs:
            return None
        p = torch.cat(outs)
        return p if p.dtype in (torch.float32, torch.float64) else p.to(torch.float64)

    def row_tables(self, table, obs, next_obs):
        xn, x0 = obs_tensor(next_obs, table.device), obs_tensor(obs, table.device)
        pn = self._run(xn[table.order.to(torch.int64)])
        p0 = self._run(x0[table.init_orig.to(torch.int64)])
        empty = torch.zeros((0, table.nA), dtype=(pn if pn is not None else p0 if p0 is not None else torch.zeros(0)).dtype, device=table.device)
        pn = empty if pn is None else pn
        p0 = empty if p0 is None else p0
        if pn.dtype != p0.dtype:
            pn, p0 = pn.to(torch.float64), p0.to(torch.float64)
        return pn.reshape(-1, table.nA).contiguous(), p0.reshape(-1, table.nA).contiguous()
