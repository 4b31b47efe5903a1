"""A plain Python loop of the three environments VectorGridNavi / VectorCartPole run on the device, and of their collect and record.

The environments: the reference's MyGridNavi ("grid": the observation is the cell id) and MyGridNaviCoords ("coords")
(offsim4rl/envs/gridworld.py:14-124, 187-211) with the goal a parameter, and CartPole-v1 ("cartpole": synth.cartpole_log's equations in
f64).  Every environment has two np.random.default_rng streams: `rng` for the environment's own noise and resets, `arng` for its actions.
The action rule is the package's: the cdf of the f32 row widened to f64, normalised, then searchsorted(u, side="right").
"""
import numpy as np

SERVED, TERMINATED, TRUNCATED, RESET, ALIVE = 1, 2, 4, 8, 16
_G, _MC, _MP, _L, _F, _TAU = 9.8, 1.0, 0.1, 0.5, 10.0, 0.02
_TH_LIM, _X_LIM = 12 * 2 * np.pi / 360, 2.4
N_ACTIONS = {"grid": 5, "coords": 5, "cartpole": 2}
OBS_WIDTH = {"grid": 1, "coords": 2, "cartpole": 4}


def cartpole_step(s, a):
    """One Euler step of the f64 state s [4] under action a (synth.cartpole_log's operation order)."""
    x, xd, th, thd = (np.float64(v) for v in s)
    pm, tm = _MP * _L, _MC + _MP
    f = _F if a == 1 else -_F
    ct, st = np.cos(th), np.sin(th)
    tmp = (f + pm * thd * thd * st) / tm
    tha = (_G * st - ct * tmp) / (_L * (4.0 / 3.0 - _MP * ct * ct / tm))
    xa = tmp - pm * tha * ct / tm
    return np.array([x + _TAU * xd, xd + _TAU * xa, th + _TAU * thd, thd + _TAU * tha], np.float64)


def cartpole_done(s):
    return bool(s[0] < -_X_LIM or s[0] > _X_LIM or s[2] < -_TH_LIM or s[2] > _TH_LIM)


class HostEnv:
    def __init__(self, kind, seed, num_cells=5, num_steps=15, goal=(4, 4)):
        assert kind in N_ACTIONS
        self.kind, self.num_cells, self.num_steps, self.goal = kind, int(num_cells), int(num_steps), (int(goal[0]), int(goal[1]))
        self.rng = np.random.default_rng(seed)
        self.reset()

    def reset(self):
        self.step_count = 0
        if self.kind == "cartpole":
            self.s = self.rng.uniform(-0.05, 0.05, 4)
        else:
            self.x = self.y = 0
            self.deltas = self.rng.uniform(-0.1, 0.1, 2) if self.kind == "coords" else np.zeros(2)
        return self.obs64()

    @property
    def z(self):
        return self.x + self.num_cells * self.y

    def obs64(self):
        """The observation as the reference returns it: the cell id, or f64 values."""
        if self.kind == "cartpole":
            return self.s.copy()
        if self.kind == "grid":
            return self.z
        return np.array([self.x / 5 + 0.1 + self.deltas[0], self.y / 5 + 0.1 + self.deltas[1]], np.float64)

    def obs(self):
        """The observation as the device records it: i32 cell id, or the f64 values rounded once to f32."""
        o = self.obs64()
        return np.int32(o) if self.kind == "grid" else o.astype(np.float32)

    def state(self):
        """What the device records as state: CartPole the four f64, the grids the cell id."""
        return self.s.copy() if self.kind == "cartpole" else np.int32(self.z)

    def step(self, a):
        """(reward, done) with the old API's done"""
        if self.kind == "cartpole":
            self.s = cartpole_step(self.s, a)
            return 1.0, cartpole_done(self.s)
        if self.kind == "coords":
            self.deltas = self.rng.uniform(-0.1, 0.1, 2)
        done = self.x == self.goal[0] and self.y == self.goal[1]
        if a == 1:
            self.y = min(self.y + 1, self.num_cells - 1)
        elif a == 2:
            self.x = min(self.x + 1, self.num_cells - 1)
        elif a == 3:
            self.y = max(self.y - 1, 0)
        elif a == 4:
            self.x = max(self.x - 1, 0)
        self.step_count += 1
        if self.step_count >= self.num_steps:
            done = True
        if done:
            r = 0.0
        elif self.x == self.goal[0] and self.y == self.goal[1]:
            r, done = 1.0, True
        else:
            r = -0.1
        return r, done


def draw(p32, u):
    """Generator.choice(nA, p=p) as the package draws it; len(p) where no action can be drawn (NaN or zeros)."""
    cdf = np.cumsum(np.asarray(p32, np.float32).astype(np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        cdf = cdf / cdf[-1]
    return int(np.searchsorted(cdf, u, side="right")) if not np.isnan(cdf).any() else len(cdf)


def stream_words(g):
    """[state hi, state lo, inc hi, inc lo] of a Generator's PCG64, as the device rows hold them (int64 views)"""
    st = g.bit_generator.state["state"]
    m = (1 << 64) - 1
    return np.array([st["state"] >> 64, st["state"] & m, st["inc"] >> 64, st["inc"] & m], np.uint64).view(np.int64)


class HostVectorEnv:
    """E environments with their action streams and the open episodes' counters: VectorGridNavi / VectorCartPole on the host."""

    def __init__(self, kind, env_seeds, action_seeds=None, **kw):
        self.kind, self.nA = kind, N_ACTIONS[kind]
        self.envs = [HostEnv(kind, int(s), **kw) for s in env_seeds]
        self.arngs = [np.random.default_rng(int(s)) for s in (env_seeds if action_seeds is None else action_seeds)]
        self.ep_t = [0] * len(self.envs)

    def reset(self, mask=None):
        for k, e in enumerate(self.envs):
            if mask is None or mask[k]:
                e.reset()
                self.ep_t[k] = 0

    def collect(self, policy, T, max_episode_steps=None):
        """T steps of every environment.  policy(e, i, obs) -> the f32 probabilities at the observation `obs` of environment e at step i
        (teacher forcing: return the recorded row).  Returns step-major [T, E] arrays named as the device's records."""
        E, nA, w = len(self.envs), self.nA, OBS_WIDTH[self.kind]
        cap = 0 if max_episode_steps is None else int(max_episode_steps)
        grid = self.kind != "cartpole"
        odt, oshape = (np.int32, ()) if self.kind == "grid" else (np.float32, (w,))
        sdt, sshape = (np.int32, ()) if grid else (np.float64, (4,))
        out = dict(obs=np.zeros((T, E) + oshape, odt), next_obs=np.zeros((T, E) + oshape, odt), state=np.zeros((T, E) + sshape, sdt),
                   next_state=np.zeros((T, E) + sshape, sdt), probs=np.zeros((T, E, nA), np.float32), action=np.zeros((T, E), np.int32),
                   reward=np.zeros((T, E), np.float32), flags=np.zeros((T, E), np.uint8), ep_step=np.zeros((T, E), np.int32))
        for k, (env, g) in enumerate(zip(self.envs, self.arngs)):
            for i in range(T):
                out["obs"][i, k], out["state"][i, k] = env.obs(), env.state()
                p = np.asarray(policy(k, i, out["obs"][i, k]), np.float32)
                out["probs"][i, k] = p
                a = draw(p, g.random())
                assert a < nA, "the host loop has no stopped environments"
                r, done = env.step(a)
                out["next_obs"][i, k], out["next_state"][i, k] = env.obs(), env.state()
                out["action"][i, k], out["reward"][i, k], out["ep_step"][i, k] = a, r, self.ep_t[k]
                self.ep_t[k] += 1
                trunc = cap > 0 and self.ep_t[k] >= cap
                fl = SERVED | ALIVE | (TERMINATED if done else 0) | (TRUNCATED if trunc else 0)
                if done or trunc:
                    env.reset()
                    self.ep_t[k] = 0
                    fl |= RESET
                out["flags"][i, k] = fl
        return out

    def streams(self):
        """(env stream rows [E, 4], action stream rows [E, 4]) as the device holds them"""
        return np.stack([stream_words(e.rng) for e in self.envs]), np.stack([stream_words(g) for g in self.arngs])

    def record(self, policy, num_samples, max_episode_steps=None):
        """VectorGridNavi.record / VectorCartPole.record: one collect of ceil(N / E) steps, rows env-major, cut to N"""
        E, N = len(self.envs), int(num_samples)
        T = -(-N // E)
        c = self.collect(policy, T, max_episode_steps)

        def em(x):
            return np.ascontiguousarray(np.swapaxes(x, 0, 1)).reshape((E * T,) + x.shape[2:])[:N]

        steps = em(c["ep_step"]).astype(np.int64)
        exp = dict(episode_ids=np.cumsum(steps == 0).astype(np.int64) - 1, steps=steps, observations=em(c["obs"]),
                   actions=em(c["action"]).astype(np.int64), action_distributions=em(c["probs"]), rewards=em(c["reward"]),
                   next_observations=em(c["next_obs"]), terminals=em(c["flags"] & TERMINATED) != 0, truncateds=em(c["flags"] & TRUNCATED) != 0)
        if self.kind != "cartpole":
            exp["infos/z"], exp["infos/z_next"] = em(c["state"]).astype(np.int64), em(c["next_state"]).astype(np.int64)
        if self.kind == "grid":
            exp["observations"], exp["next_observations"] = exp["observations"].astype(np.int64), exp["next_observations"].astype(np.int64)
        return exp


# ---- CartPole on the device against the host's f64 step: the cases the error table and the GPU test share ----
# (E, T, max_episode_steps, env seed base): one environment, a partial workgroup, two workgroups and one wave; no cap, a cap that truncates
# every episode, the example's
CARTPOLE_CASES = [(1, 40, None, 10), (5, 40, 2, 20), (17, 40, 500, 30), (17, 1, None, 40), (5, 40, None, 50)]
EPS = np.finfo(np.float64).eps


def cartpole_deviation(state, action, next_state):
    """Largest |device next_state - host step(device state, device action)| over [T, E] records, in units of eps * max(1, |value|)"""
    worst = 0.0
    T, E = action.shape
    for i in range(T):
        for k in range(E):
            want = cartpole_step(state[i, k], int(action[i, k]))
            worst = max(worst, float(np.max(np.abs(next_state[i, k] - want) / (EPS * np.maximum(1.0, np.abs(want))))))
    return worst
