"""evalMC (offsim4rl/agents/tabular.py:247-270) on QueueEvaluator_impl for a policy over observations, in plain NumPy / Python, one rollout at
a time (test infrastructure), and the case list of the kernel matrix (tests/test_gpu_queue_rows_policy.py).

A restatement of documented behaviour (include/offsim.h: offsim_eval_queue_rows_policy), not of the kernel's code: the loop of
queue_host.run(mode=EVALMC) over queue_host.Sampler, with the policy row taken per ROW of the log instead of per state --

  after sm.reset() popped caller row i    p = P_init[i]   (the policy at obs of row i)
  after sm.step(A) served caller row i    p = P_next[i]   (the policy at next_obs of row i)

P_next / P_init are [N, nA] in CALLER order here (what RowPolicy takes); the device reads them gathered into grouped / init_orig order.
The draw is Generator.choice's rule written out, so that a row without a cdf entry above u (NaN, zeros) gives nA instead of raising:
c = cumsum(p as f64), cdf = c / c[-1], u = gen.random() (one draw), A = the first k with cdf[k] > u.
cur_row is reported in the device's numbering: g >= 0 the position of the last served row in grouped order (stable sort by composite
slot), -2 - k the k-th initial row in buffer order, -1 none; None when the loop ran no reset (the caller's value stays).
"""
import numpy as np

import queue_host as H


def draw(gen, row):
    c = np.cumsum(np.asarray(row).astype(np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        cdf = c / c[-1]
    hit = np.flatnonzero(cdf > gen.random())
    return int(hit[0]) if len(hit) else len(cdf)


def grouped_order(lg):
    """caller row of every grouped row: rows sorted by composite slot, buffer order within a slot"""
    return np.argsort((lg.z - lg.z_lo) * lg.nA + lg.a, kind="stable")


def run(sm, gen, P_next, P_init, gamma, n_episodes=None, trace_cap=0, ep_cap=0):
    """Runs sampler `sm` with the action stream `gen` from where they stand until the log or `n_episodes` ends.  Returns the row of every
    output of BatchedQueueEvaluator.eval_mc_rows_policy and the state left behind."""
    lg, nA = sm.log, sm.log.nA
    gamma = float(gamma)
    n_episodes = H.UNLIMITED if n_episodes is None else int(n_episodes)
    pos = np.empty(lg.N, np.int64)
    pos[grouped_order(lg)] = np.arange(lg.N)
    init_k = {int(i): k for k, i in enumerate(np.flatnonzero(lg.t0))}
    o = dict(trace_row=np.full(trace_cap, -1, np.int32), trace_pop=np.zeros(trace_cap, np.int32), ep_g=np.zeros(ep_cap, np.float64),
             ep_len=np.zeros(ep_cap + 1, np.int32), obs_row=-(1 << 31), cur_row=None, branches=set())
    ep = n_len = steps = 0
    sum_g, status, terminate = 0.0, H.ST_OK, False
    while ep < n_episodes and not terminate:
        row0 = sm.reset()
        if row0 is None:
            status, o["obs_row"], o["cur_row"] = H.ST_NO_INIT, -1, -1
            o["branches"].add("no_init")
            break
        o["obs_row"], o["cur_row"] = -2 - row0, -2 - init_k[row0]
        p = P_init[row0]
        G, t, done = 0.0, 0, False
        while not done:
            A = draw(gen, p)
            if steps < trace_cap:
                o["trace_pop"][steps] = A
            if A >= nA:
                status, terminate = H.ST_KEYERROR, True
                o["branches"].add("no_action")
                break
            try:
                row = sm.step(A)
            except KeyError:
                status, terminate = H.ST_KEYERROR, True
                o["branches"].add("never_logged")
                break
            if row is None:
                status, terminate = H.ST_EXHAUSTED, True
                o["branches"].add("exhausted")
                break
            o["obs_row"], o["cur_row"] = row, int(pos[row])
            p = P_next[row]
            if steps < trace_cap:
                o["trace_row"][steps] = row
            G = G + gamma ** t * float(lg.r64[row])
            t += 1
            steps += 1
            done = bool(lg.done[row])
        if status == H.ST_KEYERROR:
            break
        if ep_cap and n_len <= ep_cap:
            o["ep_len"][n_len] = t
        n_len += 1
        if done:
            if ep < ep_cap:
                o["ep_g"][ep] = G
            sum_g += G
            ep += 1
            o["branches"].add("episode")
        elif ep < ep_cap:
            o["ep_g"][ep] = G
    if ep >= n_episodes and status == H.ST_OK:
        o["branches"].add("episode_limit")
    o.update(sum_g=sum_g, n_ep=ep, steps=steps, cand=steps, n_len=n_len, status=status, cursor=sm.cursors(), init_cursor=sm.init_head,
             cur_slot=-1 if sm.cur is None else (sm.cur - lg.z_lo) * nA, rng=H.rng_words(gen))
    return o


# The carve of csrc/eval_queue_rows.hpp, restated: seg_off (n + 1 words), the cursors of every rollout (n words each), padded to 8 bytes,
# then one row of nA doubles per rollout; include/offsim.h: 4 rollouts per workgroup, then 2, then 1 while it exceeds 64 KiB; one rollout
# up to 160 KiB; beyond: refused (as is n_slots > 40960)
def lds_bytes(waves, n_slots, nA):
    return (((n_slots + 1) + waves * n_slots) * 4 + 7) // 8 * 8 + waves * nA * 8


def launch_shape(n_slots, nA):
    """(rollouts per workgroup, LDS bytes, refused)"""
    w = 4
    while w > 1 and lds_bytes(w, n_slots, nA) > 65536:
        w //= 2
    b = lds_bytes(w, n_slots, nA)
    return w, b, b > 160 * 1024 or n_slots > 40960


# ---------------------------------------------------------------------------------------------------------------------------------
# The case list: queue_host.make_log logs, N = 600 unless said, R = 5 (no multiple of 4: the last workgroup is partial)
# ---------------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, reaches, N=600, nZ=5, nA=5, R=5, log_seed=1, f32=False, r32=False, neg_state=False, holes=0, n_slots=None,
                 bad_rows=False, n_episodes=None, no_init=False, p_done=0.1):
        self.__dict__.update(locals())
        del self.__dict__["self"]
        self.seeds = [3 + 7 * i for i in range(R)]
        self.action_seeds = [100 + 11 * i for i in range(R)]
        self._log = self._host = self._tabs = None

    @property
    def log(self):
        if self._log is None:
            self._log = H.make_log(self.N, self.nZ, self.nA, self.log_seed, self.r32, self.neg_state, self.holes, self.n_slots, p_done=self.p_done,
                                   no_init=self.no_init)
        return self._log

    def tables(self):
        """(P_next, P_init) [N, nA] in caller order: Dirichlet rows (f32: rounded to f32, so they sum to 1 only to f32 rounding)"""
        if self._tabs is None:
            lg, g = self.log, np.random.default_rng(2000 + self.log_seed)
            pn, p0 = g.dirichlet(np.full(lg.nA, 1.5), lg.N), g.dirichlet(np.full(lg.nA, 1.5), lg.N)
            if self.bad_rows:  # a NaN row and an all-zero row among the rows that are served early
                pn[::7] = np.nan
                pn[3::7] = 0.0
            if self.f32:
                pn, p0 = pn.astype(np.float32), p0.astype(np.float32)
            self._tabs = pn, p0
        return self._tabs

    def kw(self):
        return dict(n_episodes=self.n_episodes, trace_cap=self.log.N + 1, ep_cap=self.log.N + 1)

    def host(self):
        if self._host is None:
            pn, p0 = self.tables()
            self._host = [run(H.Sampler(self.log, s), np.random.default_rng(sa), pn, p0, H.GAMMA, **self.kw())
                          for s, sa in zip(self.seeds, self.action_seeds)]
        return self._host


CASES = [
    Case("base-f64", {"episode", "exhausted"}),
    Case("base-f32", {"episode", "exhausted"}, f32=True, log_seed=2),
    Case("nA2", {"episode"}, nA=2, nZ=7, log_seed=3),
    Case("nA16-f32", {"episode"}, nA=16, nZ=3, f32=True, log_seed=4),
    Case("r32-neg-state", {"episode"}, r32=True, neg_state=True, log_seed=5),
    Case("holes", {"never_logged"}, holes=4, log_seed=6),
    Case("bad-rows", {"no_action"}, bad_rows=True, log_seed=7),
    Case("short-exhausted", {"exhausted"}, N=60, p_done=0.02, log_seed=8),
    Case("no-init", {"no_init"}, no_init=True, log_seed=9),
    Case("episodes-0", {"episode_limit"}, n_episodes=0, log_seed=10),
    Case("episodes-1", {"episode_limit", "episode"}, n_episodes=1, log_seed=11),
    # (TransitionTable keeps dense slots only while the id range stays within four times the distinct ids: a log stretched to n_slots
    # needs n_slots / 4 distinct pairs, so these two logs are longer than 600 rows)
    Case("waves2", {"episode"}, N=2000, n_slots=3500, log_seed=12),
    Case("waves1-big", {"episode"}, N=4400, n_slots=8500, log_seed=13),
]
BY_NAME = {c.name: c for c in CASES}
