"""The tabular drivers on latent states -- evalMC / qlearn / expSARSA / z_expSARSA of offsim4rl/agents/tabular.py with the tables indexed by
z = encoder(observation) -- as a plain Python loop, one rollout at a time (test infrastructure), the fixtures' reader and the LDS rule of
csrc/eval_env_latent.hpp restated.

Built from tests/true_env_host.py's environments (HostEnv "coords" / "cartpole": the dynamics in f64, the observation rounded once to f32)
and the learner of tests/td_host.py / tests/env_drivers_host.py (behaviours and ties as tabular.py writes them, the update in Python
floats: Q-learning max(Q[z']); expected SARSA sum_k Q[z'][k] * pi[z'][k] from k = 0 upwards).  The encoders: the box through the oracle's
cartpole_encode; the MLP as an f64 forward and NumPy's first arg max -- the fixtures and the GPU cases assert a top-2 logit gap that no f32
summation order can close.  Q[z] for z < 0 is NumPy's own wrap.  Outputs come back in the device's layout."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle as O  # noqa: E402
from encoder_host import forward_f64  # noqa: E402
from queue_host import (ST_OK, ST_KEYERROR, EVALMC, QLEARN, EXPSARSA, FIXED, EPS_GREEDY, SOFT_GREEDY,  # noqa: E402,F401
                        behaviour_row, mt_words, rng_words)
from true_env_host import HostEnv  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "latent_env")
N_ACTIONS = {"coords": 5, "cartpole": 2}
CARTPOLE_MLP_WEIGHT_SEED, CARTPOLE_MLP_SEEDS = 11, (0, 1, 2, 3, 4)  # the 4-8-10 encoder of the CartPole + MLP cases and their action seeds


def mlp_weights(dO, H, nZ, seed, scale=1.0):
    """a seeded dO-H-nZ encoder in state_dict layout, f32"""
    g = np.random.default_rng(seed)
    return tuple((scale * g.standard_normal(s)).astype(np.float32) for s in ((H, dO), (H,), (nZ, H), (nZ,)))


class BoxEncoder:
    def __call__(self, obs32):
        return int(O.cartpole_encode(np.asarray(obs32, np.float32).reshape(1, 4))[0])


class MlpEncoder:
    """f64 forward, first arg max; `gaps` collects the top-2 logit gap of every observation encoded"""

    def __init__(self, weights):
        self.weights, self.gaps, self.obs = weights, [], []

    def logits(self, obs32):
        return forward_f64(np.asarray(obs32, np.float32).reshape(1, -1), *self.weights)[0]

    def __call__(self, obs32):
        self.obs.append(np.asarray(obs32, np.float32).copy())
        lo = self.logits(obs32)
        top = np.sort(lo)[::-1]
        self.gaps.append(float(top[0] - top[1]) if len(top) > 1 else np.inf)
        return int(np.argmax(lo))


def clear_rows(weights, obs32):
    """tests/encoder_host.py's rule for the rows obs32 [N, dO] of one network (build / tolerance / clear_rows there, for a case of its
    table): tol = 4 * max(rho_ref, 2^-24) with rho_ref the oracle's f32 forward against f64 relative to B, the sum of absolute terms; a row
    is clear when its f64 top-2 gap exceeds 2 * tol * the larger B of those two logits -- there every in-tolerance forward has the f64 arg
    max.  Returns (clear [N] bool, the f64 arg max [N])."""
    from encoder_host import magnitude_f64
    x = np.asarray(obs32, np.float32).reshape(len(obs32), -1)
    ref, B = forward_f64(x, *weights), magnitude_f64(x, *weights)
    _, lo = O.mlp_encode(x, *weights)
    tol = 4.0 * max(float((np.abs(lo.astype(np.float64) - ref) / B).max()), 2.0 ** -24)
    order = np.argsort(-ref, axis=1, kind="stable")[:, :2]
    rows = np.arange(len(x))
    top, second = ref[rows, order[:, 0]], ref[rows, order[:, 1]]
    return (top - second) > 2.0 * tol * np.maximum(B[rows, order[:, 0]], B[rows, order[:, 1]]), np.argmax(ref, axis=1)


class LiveWorld:
    """a HostEnv behind an encoder.  reseed: episode e is HostEnv(kind, episode0 + e) -- default_rng(episode) and the reset drawn from it;
    otherwise one HostEnv(kind, seed) whose stream runs on."""

    def __init__(self, kind, enc, seed=None, reseed=True, cap=0, **kw):
        self.kind, self.enc, self.reseed, self.cap, self.kw = kind, enc, reseed, int(cap), kw
        self.env = None if reseed else HostEnv(kind, seed, **kw)
        self._fresh, self.t = not reseed, 0

    def state_row(self):
        e = self.env
        return e.s.copy() if self.kind == "cartpole" else np.array([e.x, e.y, *e.obs64()], np.float64)

    def reset(self, episode):
        if self.reseed:
            self.env = HostEnv(self.kind, episode, **self.kw)
        elif not self._fresh:
            self.env.reset()
        self._fresh, self.t = False, 0
        return self.enc(self.env.obs())

    def step(self, a):
        r, done = self.env.step(a)
        self.t += 1
        return self.enc(self.env.obs()), r, bool(done or (self.cap > 0 and self.t >= self.cap))

    def env_words(self):
        return rng_words(self.env.rng)


class TraceWorld:
    """the recorded (z, z', r, done) of a rollout served back in order: the learner replayed on a trace"""

    def __init__(self, z, z_next, r, done):
        self.z, self.z_next, self.r, self.done, self.i = z, z_next, r, done, 0

    def state_row(self):
        return np.zeros(4)

    def reset(self, episode):
        return int(self.z[self.i])

    def step(self, a):
        i = self.i
        self.i += 1
        return int(self.z_next[i]), float(self.r[i]), bool(self.done[i])


def run(world, nS, nA, draw, mode, pi, gamma, alpha=0.1, q=None, behaviour=FIXED, epsilon=0.0, alpha_ep=None, epsilon_ep=None, tie=None, episode0=0,
        n_episodes=1, trace_cap=0, ep_cap=0, snap_cap=0, snap_stride=1, rec_max=False):
    """n_episodes episodes on `world`; draw(p) -> the action (nA: none can be drawn).  q (updated in place) and a RandomState `tie` keep
    the state a second call resumes from.  tie: None (first maximum), a RandomState, or "episode".  Returns the row of every output of
    BatchedLatentEnv.eval_mc / eval_td."""
    pi = None if pi is None else np.asarray(pi, np.float64)
    gamma = float(gamma)
    o = dict(trace_pop=np.zeros(trace_cap, np.int32), td_err=np.zeros(trace_cap, np.float64), beh_arg=np.zeros(trace_cap, np.int32),
             ep_g=np.zeros(ep_cap, np.float64), ep_len=np.zeros(ep_cap + 1, np.int32), q_snap=np.zeros((snap_cap, nS, nA), np.float64),
             trace_z=np.full(trace_cap, -1, np.int32), trace_z_next=np.full(trace_cap, -1, np.int32), trace_reward=np.zeros(trace_cap),
             trace_done=np.zeros(trace_cap, np.uint8), trace_state=np.zeros((trace_cap, 4)), trace_next_state=np.zeros((trace_cap, 4)))
    tie_rs = tie if isinstance(tie, np.random.RandomState) else (np.random.RandomState(0) if tie == "episode" else None)
    ep = n_len = steps = 0
    sum_g, status = 0.0, ST_OK
    sched = lambda tab, const: float(const) if tab is None else float(tab[min(ep, len(tab) - 1)])  # noqa: E731
    while ep < n_episodes and status == ST_OK:
        if tie == "episode":
            tie_rs.seed((episode0 + ep) & 0xFFFFFFFF)  # np.random.seed(episode), before env.reset
        z = world.reset(episode0 + ep)
        G, t, done = 0.0, 0, False
        while not done:
            if mode != EVALMC and behaviour != FIXED:
                p, best = behaviour_row(behaviour, q[z], sched(epsilon_ep, epsilon), tie_rs)
                if behaviour == EPS_GREEDY and steps < trace_cap:
                    o["beh_arg"][steps] = best
            else:
                p = pi[z]
            A = draw(p)
            if steps < trace_cap:
                o["trace_pop"][steps] = A
            if A >= nA:
                status = ST_KEYERROR
                break
            before = world.state_row()
            z_, r, done = world.step(A)
            if steps < trace_cap:
                o["trace_z"][steps], o["trace_z_next"][steps], o["trace_reward"][steps], o["trace_done"][steps] = z, z_, r, done
                o["trace_state"][steps], o["trace_next_state"][steps] = before, world.state_row()
            if mode != EVALMC:
                q_sa = float(q[z, A])
                if mode == QLEARN:
                    nxt = max(float(v) for v in q[z_])
                else:
                    nxt = 0.0
                    for k in range(nA):
                        nxt = nxt + float(q[z_, k]) * float(pi[z_, k])
                td = r + gamma * nxt - q_sa
                if steps < trace_cap:
                    o["td_err"][steps] = r + gamma * max(float(v) for v in q[z_]) - q_sa if rec_max else td
                q[z, A] = q_sa + sched(alpha_ep, alpha) * td
                if snap_cap and steps % snap_stride == 0 and steps // snap_stride < snap_cap:
                    o["q_snap"][steps // snap_stride] = q
            G = G + gamma ** t * r
            t += 1
            steps += 1
            z = z_
        if status == ST_KEYERROR:
            break
        if ep_cap and n_len <= ep_cap:
            o["ep_len"][n_len] = t
        n_len += 1
        if ep < ep_cap:
            o["ep_g"][ep] = G
        sum_g += G
        ep += 1
    o.update(sum_g=sum_g, n_ep=ep, steps=steps, cand=steps, n_len=n_len, status=status)
    if q is not None:
        o["q"] = q.copy()
    if tie_rs is not None:
        o["tie_mt"] = mt_words(tie_rs)
    return o


def chooser(gen, nA):
    """draw(p) on the action stream `gen`: NumPy's own Generator.choice; a row it refuses costs the one double it would have drawn"""
    def draw(p):
        if np.isnan(p).any() or not p.sum() > 0:
            gen.random()
            return nA
        return int(gen.choice(nA, p=p))
    return draw


def replayer(actions):
    it = iter(int(a) for a in actions)
    return lambda p: next(it)


# ---- the LDS rule of the launch shape (include/offsim.h: offsim_eval_env_latent), n = nS * nA ----
def lds_bytes(waves, nS, nA, have_pi=True, td=True, mlp=None):
    n = nS * nA
    enc = wave = 0
    if mlp is not None:
        dO, H, nZ = mlp
        enc, wave = H * dO + H + nZ * H + nZ, 4 + H + nZ
    return (waves * n * 8 if td else 0) + (n * 8 if have_pi else 0) + (waves * (nA * 8 + 624 * 4) if td else 0) + 4 * enc + 4 * waves * wave


def launch_shape(nS, nA, have_pi=True, td=True, mlp=None):
    """(rollouts per workgroup, LDS bytes, refused)"""
    w = 4
    while w > 1 and lds_bytes(w, nS, nA, have_pi, td, mlp) > 65536:
        w //= 2
    b = lds_bytes(w, nS, nA, have_pi, td, mlp)
    return w, b, b > 160 * 1024 or nS * nA > 40960


def nS_for_waves(waves, nA, lo, have_pi=False, mlp=None):
    """the smallest nS >= lo whose learner launch holds `waves` rollouts per workgroup"""
    return next(s for s in range(lo, 40960 // nA) if launch_shape(s, nA, have_pi, True, mlp)[0] == waves)


# ---- the fixtures (tests/golden/make_golden_latent_env.py) ----
EPS_SCHED = lambda e: 1.0 / (1.0 + e)  # noqa: E731  (the schedule the fixtures were recorded with)
DRIVERS = {"evalMC": (EVALMC, FIXED, 0.0), "qlearn_eps": (QLEARN, EPS_GREEDY, 0.3), "qlearn_eps_sched": (QLEARN, EPS_GREEDY, None),
           "z_expSARSA": (EXPSARSA, FIXED, 0.0)}


class Fixture:
    def __init__(self, name="coords_mlp"):
        self.d = d = np.load(os.path.join(GOLDEN, name + ".npz"))
        self.runs = [str(r) for r in d["runs"]]
        self.weights = tuple(d[k] for k in ("W1", "b1", "W2", "b2"))
        self.td_off = np.concatenate([[0], np.cumsum(d["td_steps"])])

    def settings(self, i):
        drv, gx, gy, ns, seed = self.runs[i].split("|")
        return drv, (int(gx), int(gy)), int(ns), int(seed)

    def td(self, i):
        return self.d["TD_errors"][self.td_off[i]:self.td_off[i + 1]]

    def Qs(self, i):
        a, b = self.td_off[i], self.td_off[i + 1]
        nS, nA = self.d["Q"].shape[1:]
        out = np.zeros((b - a + 1, nS, nA))
        for k, (j, v) in enumerate(zip(self.d["Qs_idx"][a:b], self.d["Qs_val"][a:b])):
            out[k + 1] = out[k]
            out[k + 1].flat[j] = v
        return out

    def mt(self, i):
        return np.concatenate([self.d["mt_keys"][self.d["mt_key"][i]], [self.d["mt_pos"][i]]]).astype(np.uint32)
