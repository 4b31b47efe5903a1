"""Policy rows built so that the queue rollouts' action draw meets its cdf boundaries exactly (test infrastructure of
tests/test_draw_ties_host.py and tests/test_gpu_draw_ties.py).

The draw, restated from the documentation (include/offsim.h: offsim_eval_queue), not from the kernel:

    cdf = cumsum(p widened to f64); cdf /= cdf[-1]; u = (next64 >> 11) * 2^-53; A = cdf.searchsorted(u, side='right')

Every rollout's action stream is np.random.default_rng(seed), so the u a rollout meets at its next step is known before the step.  The
builder walks the rollouts of a case one after another ON THE EXISTING MIRRORS -- queue_host.run, queue_rows_policy_host.run,
queue_collect_host.collect, whose draw it replaces by `Steerer` -- and before each draw peeks at the next u on a copy of the generator.
The FIRST time a policy row is met (pi[z] of the tabular forms, P_init[row] / P_next[row] of the row forms) the row is rewritten in
place so that this meeting falls into the class aimed for; a later meeting of the same row is unsteered and only counted.  Rows no
rollout meets keep their Dirichlet draw.  After fixing a row the meeting is re-evaluated with the restated draw and filed under the
class it landed in (`classify`), "miss" if in none.

Classes (k: the boundary steered, A: the answer):
  tie        cdf_k == u, p_{k+1} > 0: A = k + 1 (k < nA - 2)
  last       the same at k = nA - 2: the tie hands the draw to the last action
  tie0       cdf_k == u and p_{k+1} == 0, so cdf_{k+1} == u as well: A = k + 2
  tie0-end   cdf_k == u and every later entry but the last is zero: A = nA - 1 >= k + 3
  above      cdf_k is the f64 neighbour of u above it: A = k          below: the neighbour below it: A = k + 1
  div-down   c_k > u but c_k / total <= u (total = 1 + a few ulps): A = k + 1
  div-up     c_k <= u but c_k / total > u (total = 1 - a few ulps): A = k
  f32tie     an exact tie whose entries are all f32 values (nA >= 4): A = k + 1;  f32tie0: with p_{k+1} == 0, A = k + 2
  f32dec     f32 entries, cdf_k > u in f64 while (float)cdf_k > (float)u is false: A = k
  chunk62 / chunk63 / chunk64 / chunk68   (nA = 70) a tie at that k: the answer 64 of chunk63 is the first entry of the second chunk of 64

The exact rows are sums of integers: with K = u * 2^53, prefix entries m_j * 2^-53 with sum(m_j) = K and the rest 2^53 - K behind them
give partial sums that are integers below 2^53 times 2^-53 -- exact in f64 -- and a total of exactly 1.  The f32 ties take the prefix
from the 24-bit mantissa of the f32 next to u and decompose the total t with fl(p_0 / t) == u (searched within +-2 ulps of p_0 / u)
greedily into three more f32 entries.
"""
import contextlib
import copy
import functools
from collections import Counter, namedtuple

import numpy as np

import queue_collect_host as QC
import queue_host as H
import queue_rows_policy_host as QR

INF = np.inf
CHUNK = {"chunk62": 62, "chunk63": 63, "chunk64": 64, "chunk68": 68}
F32_CLASSES = ("f32tie", "f32tie0", "f32dec")
NEED = 32  # steered meetings of every class in every case that names it


# ---------------------------------------------------------------------------------------------------------------------------------
# The draw, and the four wrong versions the built rows tell from it
# ---------------------------------------------------------------------------------------------------------------------------------
def _cdf(p):
    c = np.cumsum(np.asarray(p).astype(np.float64))
    return c, c / c[-1]


def draw(p, u):
    return int(_cdf(p)[1].searchsorted(u, side="right"))


def draw_left(p, u):
    """(a) accepts at cdf_k >= u"""
    return int(_cdf(p)[1].searchsorted(u, side="left"))


def draw_no_division(p, u):
    """(b) compares c_k with u"""
    return int(_cdf(p)[0].searchsorted(u, side="right"))


def draw_f32(p, u):
    """(c) (float)cdf_k > (float)u"""
    return int(_cdf(p)[1].astype(np.float32).searchsorted(np.float32(u), side="right"))


def draw_skip_after_tie(p, u):
    """(d) after a tie at k answers k + 1 without looking at it"""
    cdf = _cdf(p)[1]
    k = int(cdf.searchsorted(u, side="left"))
    return k + 1 if k < len(cdf) and cdf[k] == u else k


MUTANTS = {"left": draw_left, "no-division": draw_no_division, "f32": draw_f32, "skip-after-tie": draw_skip_after_tie}
CAUGHT_BY = {"left": ("tie", "last", "tie0", "tie0-end", "f32tie", "f32tie0") + tuple(CHUNK), "no-division": ("div-down", "div-up"),
             "f32": ("f32dec", "above", "below"), "skip-after-tie": ("tie0", "tie0-end", "f32tie0")}


class _Gen:
    """A Generator whose choice(nA, p=p) is fn(p, u) on its next double (what queue_host.run draws with)."""

    def __init__(self, gen, fn):
        self.gen, self.fn = gen, fn

    @property
    def bit_generator(self):
        return self.gen.bit_generator

    def choice(self, nA, p):
        return self.fn(p, self.gen)


def with_gen(fn):
    """fn(p, u) as a draw on a generator: one double consumed"""
    return lambda p, gen: fn(p, gen.random())


@contextlib.contextmanager
def draws_replaced(fn):
    """Inside, queue_rows_policy_host.run and queue_collect_host.collect draw with fn(p, gen) -> A; queue_host.run does when its
    generator is wrapped by `action_gen`."""
    old = QR.draw, QC.draw
    QR.draw = lambda gen, row: fn(row, gen)
    QC.draw = lambda p, gen: (fn(p, gen), None)
    try:
        yield lambda gen: _Gen(gen, fn)
    finally:
        QR.draw, QC.draw = old


# ---------------------------------------------------------------------------------------------------------------------------------
# Rows
# ---------------------------------------------------------------------------------------------------------------------------------
def _split(total, n, g, heavy=None):
    """n non-negative integers that sum to `total`: a random split, or (heavy: an index) one unit each and the rest on `heavy`"""
    if n == 1:
        return [total]
    if heavy is not None and total >= n:
        out = [1] * n
        out[heavy] += total - n
        return out
    cuts = sorted(int(v) for v in g.integers(0, total + 1, n - 1))
    return [b - a for a, b in zip([0] + cuts, cuts + [total])]


def _shift(x, d):
    for _ in range(abs(d)):
        x = np.nextafter(x, INF if d > 0 else -INF)
    return float(x)


def _exact_prefix(u, k, g, heavy):
    K = int(u * 2.0 ** 53)
    return [m * 2.0 ** -53 for m in _split(K, k + 1, g, heavy)], ((1 << 53) - K) * 2.0 ** -53


def _row_f64(cls, u, k, nA, g, heavy):
    """the row of class `cls` at boundary k for the uniform u, or None"""
    p = np.zeros(nA)
    if cls in ("tie", "last", "tie0", "tie0-end") or cls in CHUNK:
        p[:k + 1], rest = _exact_prefix(u, k, g, heavy)
        first = {"tie0": k + 2, "tie0-end": nA - 1}.get(cls, k + 1)
        n_rest = 1 if heavy is not None or cls in ("last", "tie0-end") else int(g.integers(1, min(3, nA - first) + 1))
        parts = _split(int(rest * 2.0 ** 53), n_rest, g)
        parts[0], parts[-1] = (parts[0], parts[-1]) if parts[0] else (parts[-1], parts[0])  # the answer's entry is not zero
        p[first:first + n_rest] = [m * 2.0 ** -53 for m in parts]
        return p
    if cls == "div-up":
        p[:k + 1], _ = _exact_prefix(u, k, g, heavy)
        totals = [_shift(1.0, -d) for d in (1, 2, 3)]
        c_k = u
    else:
        c_k = float(np.nextafter(u, -INF if cls == "below" else INF))
        if k:  # an exact prefix up to C in [c_k / 2, c_k], then c_k - C: exact, and fl(C + (c_k - C)) == c_k
            K = int(u * 2.0 ** 53)
            C = K - int(g.integers(0, K // 2 + 1))
            p[:k] = [m * 2.0 ** -53 for m in _split(C, k, g, None if heavy is None else min(heavy, k - 1))]
            p[k] = c_k - C * 2.0 ** -53
        else:
            p[0] = c_k
        totals = [_shift(1.0, d) for d in (1, 2, 3)] if cls == "div-down" else [1.0]
    for T in totals[int(g.integers(len(totals))):] + totals:
        for d in (0, -1, 1, -2, 2):
            rest = _shift(T - c_k, d)
            if rest > 0 and c_k + rest == T:
                p[k + 1] = rest
                return p
    return None


def _floor32(x):
    f = np.float32(x)
    return float(np.nextafter(f, np.float32(0))) if float(f) > x else float(f)


def _row_f32(cls, u, k, nA, g, heavy):
    target = float(np.nextafter(u, INF)) if cls == "f32dec" else u
    first = k + 2 if cls == "f32tie0" else k + 1
    near = np.float32(u)
    for p0 in (near, np.nextafter(near, np.float32(INF if float(near) < u else -INF))):
        P = float(p0)
        if not 0 < P < 1:
            continue
        for d in (0, -1, 1, -2, 2):
            t = _shift(P / target, d)
            if P / t != target or t <= P:
                continue
            e1 = _floor32(t - P)
            e2 = _floor32(t - P - e1)
            e3 = t - P - e1 - e2
            if float(np.float32(e3)) != e3:
                continue
            m, e = np.frexp(P)
            M = int(m * 2.0 ** 24)
            p = np.zeros(nA, np.float32)
            p[:k + 1] = [np.float32(v * 2.0 ** (int(e) - 24)) for v in _split(M, k + 1, g, heavy)]
            p[first:first + 3] = [e1, e2, e3]
            return p
    return None


# (feasible boundaries k, the answer at k) of every class
def _ks(cls, nA):
    if cls in CHUNK:
        return [CHUNK[cls]], lambda k: k + 1
    lo_hi = {"tie": (0, nA - 3), "last": (nA - 2, nA - 2), "tie0": (0, nA - 3), "tie0-end": (0, nA - 4), "above": (0, nA - 2), "below": (0, nA - 2),
             "div-down": (0, nA - 2), "div-up": (0, nA - 2), "f32tie": (0, nA - 4), "f32tie0": (0, nA - 5), "f32dec": (0, nA - 4)}[cls]
    ans = {"tie0": lambda k: k + 2, "tie0-end": lambda k: nA - 1, "above": lambda k: k, "div-up": lambda k: k, "f32tie0": lambda k: k + 2,
           "f32dec": lambda k: k}.get(cls, lambda k: k + 1)
    return list(range(lo_hi[0], lo_hi[1] + 1)), ans


def classify(p, u, k):
    """The classes of the list above that the meeting of row p with u holds at boundary k, by the restated arithmetic alone."""
    p = np.asarray(p)
    nA, f32 = len(p), p.dtype == np.float32
    c, cdf = _cdf(p)
    A = int(cdf.searchsorted(u, side="right"))
    out = set()
    if cdf[k] == u and A == k + 1:
        out.add("f32tie" if f32 else "last" if k == nA - 2 else "tie")
        out |= {n for n, kk in CHUNK.items() if nA == 70 and kk == k and not f32}
    if cdf[k] == u and k + 2 < nA and p[k + 1] == 0 and cdf[k + 1] == u and A == k + 2:
        out.add("f32tie0" if f32 else "tie0")
    if not f32 and cdf[k] == u and A == nA - 1 >= k + 3 and not p[k + 1:nA - 1].any():
        out.add("tie0-end")
    if f32:
        if A == k and cdf[k] > u and not np.float32(cdf[k]) > np.float32(u):
            out.add("f32dec")
        return out
    if A == k and cdf[k] == np.nextafter(u, INF) and c[-1] == 1.0:
        out.add("above")
    if A == k + 1 and cdf[k] == np.nextafter(u, -INF) and c[-1] == 1.0:
        out.add("below")
    if A == k + 1 and c[k] > u and cdf[k] <= u:
        out.add("div-down")
    if A == k and c[k] <= u and cdf[k] > u:
        out.add("div-up")
    return out


Rec = namedtuple("Rec", "rollout draw table row k aimed cls u A")


class Steerer:
    """The draw of the builder's walk: fn(p, gen) -> A.  p is the mirror's view of a row of one of `tables`; `sm` is the sampler of the
    rollout being walked (set by the builder), which says which actions still have a row to serve."""

    def __init__(self, case, tables, g):
        self.case, self.tables, self.g = case, tables, g
        self.met, self.records, self.count, self.unsteered = set(), [], Counter(), 0
        self.sm, self.rollout, self.n = None, 0, 0

    def _locate(self, p):
        at = p.__array_interface__["data"][0]
        for name, t in self.tables.items():
            lo = t.__array_interface__["data"][0]
            if lo <= at < lo + t.nbytes:
                return name, (at - lo) // t.strides[0]
        raise AssertionError("a row of none of the tables")

    def _left(self, a):
        q = self.sm.queues.get((self.sm.cur, a))
        return 0 if q is None else len(q) - self.sm.head[(self.sm.cur, a)]

    def _fix(self, p, u):
        nA, g = len(p), self.g
        alive = [a for a in range(nA) if self._left(a) > 0]
        plan = None
        for cls in sorted(self.case.classes, key=lambda c: (self.count[c], self.case.classes.index(c))):  # the class furthest behind
            ks, ans = _ks(cls, nA)
            good = [k for k in ks if ans(k) in alive]
            if good or plan is None:
                plan = cls, (good or ks)
            if good:
                break
        cls, ks = plan
        k = ks[int(g.integers(len(ks)))]
        heavy = None
        if self.case.heavy:  # nearly all of the prefix on the logged action below the boundary with the most rows left
            heavy = max(range(k + 1), key=lambda a: (self._left(a), -a))
        row = (_row_f32 if p.dtype == np.float32 else _row_f64)(cls, u, k, nA, g, heavy)
        if row is not None:
            p[:] = row
        return cls, k

    def __call__(self, p, gen):
        u = copy.deepcopy(gen).random()  # the peek
        key = self._locate(p)
        if key in self.met:
            self.unsteered += 1
        else:
            self.met.add(key)
            aimed, k = self._fix(p, u)
            landed = classify(p, u, k)
            cls = aimed if aimed in landed else min(landed & set(self.case.classes), default="miss")
            self.count[cls] += 1
            self.records.append(Rec(self.rollout, self.n, key[0], int(key[1]), k, aimed, cls, u, draw(p, u)))
        self.n += 1
        assert gen.random() == u
        return draw(p, u)


# ---------------------------------------------------------------------------------------------------------------------------------
# Logs and cases
# ---------------------------------------------------------------------------------------------------------------------------------
def make_log(nZ, nA, seed, per_pair=4, acts=None, filler=0, p_done=0.25, p_t0=0.15, r32=False):
    """Every (z, a) pair logged per_pair times -- or, with acts [nZ][...], only those actions of each state, and `filler` more actions
    below 60 once each (the table keeps dense slots only while the key range stays within four times the distinct keys) --, in shuffled
    order, with uniform next states."""
    g = np.random.default_rng(seed)
    z, a = [], []
    for s in range(nZ):
        mine = list(range(nA)) if acts is None else list(acts[s])
        for act in mine:
            z += [s] * per_pair
            a += [act] * per_pair
        if filler:
            others = [x for x in range(60) if x not in mine]
            extra = g.permutation(others)[:filler]
            z += [s] * filler
            a += [int(x) for x in extra]
    order = g.permutation(len(z))
    z, a = np.array(z)[order], np.array(a)[order]
    N = len(z)
    z_next = g.integers(0, nZ, N)
    done, t0 = g.random(N) < p_done, g.random(N) < p_t0
    t0[:3] = True
    r = g.standard_normal(N)
    return H.Log(z, a, r.astype(np.float32) if r32 else r, z_next, done, g.dirichlet(np.full(nA, 2.0), N), t0)


class Case:
    """walk: 'pi' (queue_host.run on pi [nZ, nA] f64), 'rows' (queue_rows_policy_host.run on P_next / P_init), 'collect-rows' /
    'collect-pi' (queue_collect_host.collect for T steps of R environments with the episode cap `cap`)."""

    def __init__(self, name, walk, classes, nZ, nA, R, seed, per_pair=4, dtype=np.float64, T=0, cap=8, build_seed=0):
        self.__dict__.update(locals())
        del self.__dict__["self"]
        self.heavy = nA == 70
        self.seeds = [3 + 7 * i for i in range(R)]
        self.action_seeds = [100 + 11 * i for i in range(R)]

    @functools.cached_property
    def log(self):
        if self.nA == 70:  # state z logs the answer of its boundary and one action below 60, and 17 fillers
            ks = [CHUNK[c] for c in self.classes]
            acts = [((5 * s + 3) % 60, ks[s % len(ks)] + 1) for s in range(self.nZ)]
            return make_log(self.nZ, self.nA, self.seed, self.per_pair, acts, filler=17)
        return make_log(self.nZ, self.nA, self.seed, self.per_pair, r32=self.walk.startswith("collect"))

    def kw(self):
        return dict(trace_cap=self.log.N + 1, ep_cap=self.log.N + 1)


def mirror(case, tables, fn=None):
    """The case's rollouts on the existing mirrors with `tables`: the mirrors as they are (fn None: queue_host.run draws with NumPy's
    Generator.choice), or with their draw replaced by fn(p, gen).  Returns (the mirror's output per rollout, the collect environments)."""
    lg = case.log
    with (draws_replaced(fn) if fn else contextlib.nullcontext(lambda gen: gen)) as wrap:
        outs, envs = [], []
        for i, (s, sa) in enumerate(zip(case.seeds, case.action_seeds)):
            if isinstance(fn, Steerer):
                fn.rollout, fn.n = i, 0
            if case.walk == "pi":
                sm = H.Sampler(lg, s)
                if isinstance(fn, Steerer):
                    fn.sm = sm
                outs.append(H.run(sm, wrap(np.random.default_rng(sa)), H.EVALMC, tables["pi"], H.GAMMA, **case.kw()))
            elif case.walk == "rows":
                sm = H.Sampler(lg, s)
                if isinstance(fn, Steerer):
                    fn.sm = sm
                outs.append(QR.run(sm, np.random.default_rng(sa), tables["P_next"], tables["P_init"], H.GAMMA, **case.kw()))
            else:
                env = QC.Env(lg, s, sa)
                env.reset()
                if isinstance(fn, Steerer):
                    fn.sm = env.sm
                outs.append(QC.collect(env, case.T, case.cap, **tables))
                envs.append(env)
    return outs, envs


@functools.lru_cache(maxsize=None)
def build(case):
    """dict(tables, records, count, unsteered, walk: the outputs of the walk that fixed the rows).  Deterministic; computed once."""
    lg, g = case.log, np.random.default_rng(50000 + 100 * case.seed + case.build_seed)
    rows = lambda n: g.dirichlet(np.full(lg.nA, 1.5), n).astype(case.dtype)  # noqa: E731
    tables = dict(pi=rows(lg.nZ)) if case.walk in ("pi", "collect-pi") else dict(P_next=rows(lg.N), P_init=rows(lg.N))
    st = Steerer(case, tables, g)
    outs, _ = mirror(case, tables, st)
    for t in tables.values():
        t.setflags(write=False)
    return dict(tables=tables, records=st.records, count=dict(st.count), unsteered=st.unsteered, walk=outs)


def td_mirror(case, tables, mode, L=None, gammas=(0.9, 0.97, 1.0), alphas=(0.05, 0.2, 0.5)):
    """queue_host.run of a learner with the FIXED behaviour pi on the case's rollouts: one learner (gamma, alpha of the matrix), or L
    learners that share pi and the seeds (rollout l * S + j has seed j).  Returns (the outputs per rollout, Q_init [nZ, nA]: standard
    normal * 0.1, the same table for every rollout)."""
    lg = case.log
    q0 = np.random.default_rng(7).standard_normal((lg.nZ, lg.nA)) * 0.1
    outs = []
    for l in range(L or 1):
        for s, sa in zip(case.seeds, case.action_seeds):
            outs.append(H.run(H.Sampler(lg, s), np.random.default_rng(sa), mode, tables["pi"], H.GAMMA if L is None else gammas[l],
                              alpha=H.ALPHA if L is None else alphas[l], q=q0.copy(), **case.kw()))
    return outs, q0


_T = ("tie", "tie0", "tie0-end", "last")
_N = ("above", "below", "div-down", "div-up")
CASES = [
    # pi [nZ, nA] by state: a state is steered once, so these name few classes each
    Case("pi-nA4", "pi", _T, nZ=256, nA=4, R=16, seed=1),
    Case("pi-nA3", "pi", _N, nZ=256, nA=3, R=16, seed=2, per_pair=5),
    Case("pi-nA16", "pi", ("tie", "tie0", "last"), nZ=128, nA=16, R=16, seed=3, per_pair=2),
    Case("pi-nA70-a", "pi", ("chunk62", "chunk63"), nZ=80, nA=70, R=16, seed=4, per_pair=10),
    Case("pi-nA70-b", "pi", ("chunk64", "chunk68"), nZ=80, nA=70, R=16, seed=5, per_pair=10),
    # tables by row
    Case("rows-f64-nA4", "rows", _T + _N, nZ=64, nA=4, R=5, seed=6, per_pair=12),
    Case("rows-f64-nA4-b", "rows", _N + _T, nZ=64, nA=4, R=5, seed=6, per_pair=12, build_seed=1),
    Case("rows-f64-nA3", "rows", ("tie", "last", "tie0") + _N, nZ=64, nA=3, R=5, seed=7, per_pair=16),
    Case("rows-f32-nA4", "rows", ("f32tie", "f32dec"), nZ=64, nA=4, R=5, seed=8, per_pair=12, dtype=np.float32),
    Case("rows-f32-nA16", "rows", F32_CLASSES, nZ=64, nA=16, R=5, seed=9, per_pair=3, dtype=np.float32),
    Case("rows-f32-nA16-b", "rows", F32_CLASSES[::-1], nZ=64, nA=16, R=5, seed=9, per_pair=3, dtype=np.float32, build_seed=1),
    Case("rows-f64-nA70", "rows", tuple(CHUNK), nZ=80, nA=70, R=5, seed=10, per_pair=10),
    # the collection loop (nA <= 16)
    Case("collect-rows-f64-nA4", "collect-rows", _T + _N, nZ=64, nA=4, R=9, seed=11, per_pair=12, T=120),
    Case("collect-rows-f32-nA16", "collect-rows", F32_CLASSES, nZ=64, nA=16, R=9, seed=12, per_pair=3, dtype=np.float32, T=120),
    Case("collect-pi-f64-nA4", "collect-pi", _T, nZ=256, nA=4, R=9, seed=13, T=120),
    Case("collect-pi-f64-nA3", "collect-pi", _N, nZ=256, nA=3, R=9, seed=14, per_pair=5, T=120),
    Case("collect-pi-f32-nA16", "collect-pi", F32_CLASSES, nZ=128, nA=16, R=9, seed=15, per_pair=2, dtype=np.float32, T=120),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
