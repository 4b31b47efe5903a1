"""Host-side test infrastructure: the threshold arithmetic of the compiled policy, restated from its documentation, and a builder of
logged tables in which chosen candidates meet their rejection draw at a chosen distance from the threshold.

Nothing here is kernel code.  What is restated:
  threshold   psrs.py:53-57 (`u > p_new[a] / p_log[a] / (p_new / p_log).max()`) in NumPy f64, folded to T = floor(thr * 2^53) by the
              rules of include/offsim.h (NaN or thr >= 1 -> 2^53 - 1, thr < 0 -> 0).  u = k53 * 2^-53, so "accept iff k53 <= T".
  key         [T >> 32 : 21 | done : 1 | z_next : 10 | T & 0xffffffff : 32]                              
  digest      A [T21 | done | z_next 10], B [T16 | hi 6..2 | done | hi 1..0 | z_next 8] with hi = bits 16.. of the local row,
              C [T14 | hi 8..2 | done | hi 1..0 | z_next 8] with hi = bits 8..16 of the local row        (include/offsim.h)

The builder (`build`) simulates evalMC_psrs (psrs.py:241-271) rollout after rollout with the reference's rules -- queue orders from
oracle.permutation(seed, n), draws from default_rng(seed).random() or oracle.philox_doubles -- and, the first time a row that no earlier
decision depended on meets a draw k53, chooses that row's p_log so that its threshold lands in a planned CLASS relative to k53.  A met
row is fixed from then on; later rollouts that meet it leave it alone.  The scans compare only the top 21 / 16 / 14 bits of T with the
draw's and send a narrow band to the exact 53-bit look; the classes sit on every edge of that split.  With b the format's bits,
Tb = T >> (53 - b), db = k53 >> (53 - b), delta = db - Tb:

  eq, eq-1, eq+1    delta = 0 and T == k53 (accept), k53 - 1 (reject), k53 + 1 (accept)
  far_acc, far_rej  delta = 0, |T - k53| >= 2^16, decided by the low words alone
  d-1 .. d-18       delta < 0: accepts either side of where a clear accept begins (format A: 16 units of bias, a band of 17)
  d+1, d+2          delta > 0: rejects just above the threshold
  t=1 .. t=18       Tb = n met by an ordinary draw (db >= n + 32): rejects at the bias floor, where a window entry becomes ROWS_NEVER
  thr>1             p_log < 0 in every action: thr = 2 -> T = 2^53 - 1, accept
  T=0, thr=1, nan   in the plan's SPECIAL state, whose policy row is [1, 0]: the action of probability 0 (T = 0, reject), the arg-max
                    action (thr == 1 exactly, accept), and pi[k] == p_log[k] == 0 (0 / 0: NaN, accept)
Formats B and C (labels "B:..." / "C:..."): far_acc / far_rej as d0_acc / d0_rej, d-1 and d+1 on 16 / 14 bits; ":hi" adds the payload
closest to all ones the formats allow (done = 1, z_next = 254 of 255 states), ":loc" a local row at or above 0x1ff00 (format C).

What cannot be built: the ACCEPT of a ROWS_NEVER row (T21 <= 16) needs a draw below 2^-16; no seed of a test-sized table offers one
where it is wanted, so that decision is covered from the reject side only.

A class that cannot be reached for a meeting within the bounded ulp search is SKIPPED and counted (`skipped`), never replaced.
"""
import collections

import numpy as np

TWO53 = 1 << 53
T_MAX = TWO53 - 1
FMT_BITS = {"A": 21, "B": 16, "C": 14}


# ---- documented arithmetic ----
def threshold(pi_row, p_log_row, a):
    """T of one row: the reference's f64 expression (p_log widened exactly from f16 / f32), folded by the rules of include/offsim.h."""
    p_new = np.asarray(pi_row, np.float64)
    p_log = np.asarray(p_log_row).astype(np.float64)
    with np.errstate(all="ignore"):
        M = (p_new / p_log).max()  # (ndarray.max propagates NaN)
        thr = p_new[a] / p_log[a] / M
    if thr != thr or thr >= 1.0:
        return T_MAX
    if thr < 0.0:
        return 0
    return int(np.floor(thr * 9007199254740992.0))


def key(T, done, z_next):
    return ((T >> 32) << 43) | ((1 if done else 0) << 42) | ((int(z_next) & 1023) << 32) | (T & 0xFFFFFFFF)


def digest(k, fmt, local_row=0):
    """32-bit digest of key k in stream format "A" / "B" / "C"; B and C carry the local row's bits above the loc stream's 16 / 8."""
    hi = (k >> 32) & 0xFFFFFFFF
    if fmt == "A":
        return hi
    ts, lb = (16, 16) if fmt == "B" else (18, 8)
    h = int(local_row) >> lb
    return ((hi >> ts) << ts) | (hi & 0x400) | (hi & 0xFF) | ((h & 3) << 8) | ((h >> 2) << 11)


# ---- classes ----
A_ACCEPTS = ("eq", "eq+1", "far_acc", "d-1", "d-15", "d-16", "d-17", "d-18", "thr>1")
A_REJECTS = ("eq-1", "far_rej", "d+1", "d+2", "t=1", "t=15", "t=16", "t=17", "t=18")
A_SPECIAL = ("T=0", "thr=1", "nan")
A_PAYLOAD = ("d-1", "d-15", "d-16", "d-17", "d-18")  # classes whose rows also cycle through done x z_next in {0, n_states - 1}
BC_ACCEPTS = tuple(f"{f}:{c}{p}" for c in ("d0_acc", "d-1") for f in "CB" for p in ("", ":hi"))
BC_REJECTS = tuple(f"{f}:{c}{p}" for c in ("d0_rej", "d+1") for f in "CB" for p in ("", ":hi"))
C_LOC = ("C:d0_acc:loc", "C:d0_rej:loc", "C:d-1:loc", "C:d+1:loc")
RUNS = (0, 1, 2, 0, 9, 1, 0, 3)  # rejects planned in front of each planned accept: ties arrive at candidate positions 1, 2, 3, 4 and 10
ACCEPT_KINDS = ("eq", "eq+1", "far_acc", "d0_acc", "thr>1", "thr=1", "nan")


def expected_accept(cls):
    kind = cls.split(":")[1] if cls[1:2] == ":" else cls
    return kind in ACCEPT_KINDS or kind.startswith("d-")


class Plan:
    """A deterministic schedule: every `every`-th first meeting of a row is targeted; the classes come as runs of RUNS[i] rejects
    followed by one accept, both lists rotating.  Meetings in `special_state` take the next of `special`; rows of `loc_state` with a
    local row >= `loc_min` are always targeted, with the next of `loc_classes`."""

    def __init__(self, every, accepts, rejects, bits, special_state=None, special=(), payload=(), loc_state=None, loc_min=None, loc_classes=()):
        self.every, self.accepts, self.rejects, self.bits = int(every), tuple(accepts), tuple(rejects), int(bits)
        self.special_state, self.special, self.payload = special_state, tuple(special), tuple(payload)
        self.loc_state, self.loc_min, self.loc_classes = loc_state, loc_min, tuple(loc_classes)

    def sequence(self):
        ia = ir = i = 0
        while True:
            for _ in range(RUNS[i % len(RUNS)]):
                yield self.rejects[ir % len(self.rejects)]
                ir += 1
            yield self.accepts[ia % len(self.accepts)]
            ia += 1
            i += 1


_OFFS = np.array(sorted(range(-48, 49), key=lambda j: (abs(j), j < 0)), np.int64)  # the bounded ulp search: 0, +1, -1, .. +-48
_P1_FACTORS = (1.0, 1.25, 1.6, 1.1, 1.4, 1.9)  # second free parameter: the other action's p_log, pi_o * factor


def _target(kind, k, bits):
    """(T aimed at, predicate on an int64 array of T) of a class for draw k; None where the class does not exist for this draw."""
    sh = 53 - bits
    mask, half = (1 << sh) - 1, 1 << (sh - 1)
    d, low = k >> sh, k & ((1 << sh) - 1)
    if kind == "eq":
        return k, lambda T: T == k
    if kind == "eq-1":
        return (k - 1, lambda T: T == k - 1) if low >= 1 else None
    if kind == "eq+1":
        return (k + 1, lambda T: T == k + 1) if low < mask else None
    if kind in ("far_acc", "d0_acc"):
        t = k + (mask + 1 - low) // 2
        return (t, lambda T: ((T >> sh) == d) & (T - k >= 1 << 16)) if t >> sh == d and t - k >= 1 << 17 else None
    if kind in ("far_rej", "d0_rej"):
        t = (d << sh) + low // 2
        return (t, lambda T: ((T >> sh) == d) & (k - T >= 1 << 16)) if k - t >= 1 << 17 else None
    if kind[0] == "d":
        tb = d - int(kind[1:])
        if not 32 <= tb < (1 << bits) - 1:  # (below 32 lie the floor classes)
            return None
        return (tb << sh) + ((low + half) & mask), lambda T: (T >> sh) == tb
    if kind[0] == "t":
        n = int(kind[2:])
        return ((n << sh) + half, lambda T: (T >> sh) == n) if d >= n + 32 else None
    raise ValueError(kind)


def _solve(pi_a, pi_o, t, pred):
    """(p_log of the logged action, p_log of the other action) with pred(T) true, or None: the closed form q = pi_a / (thr * c),
    c = pi_o / p1, then q stepped by ulps, the reference's expression evaluated each time (vectorised, NumPy f64)."""
    thr = (t + 0.5) / 9007199254740992.0
    for f in _P1_FACTORS:
        p1 = pi_o * f
        c = np.float64(pi_o) / np.float64(p1)
        q0 = np.float64(pi_a) / (np.float64(thr) * c)
        if not np.isfinite(q0) or q0 <= 0:
            continue
        qv = (q0.view(np.int64) + _OFFS).view(np.float64)
        x = np.float64(pi_a) / qv
        th = x / np.maximum(x, c)
        T = np.where(th >= 1.0, T_MAX, np.floor(th * 9007199254740992.0)).astype(np.int64)
        ok = np.flatnonzero(pred(T))
        if ok.size:
            return float(qv[ok[0]]), float(p1)
    return None


def draws(provider, seed, n):
    """k53 of the first n rejection draws of `seed`: u * 2^53, exact for both providers (PCG64: [0, 2^53); Philox: [1, 2^53])."""
    from oracle import oracle as O
    u = np.random.default_rng(int(seed)).random(n) if provider == "pcg64" else O.philox_doubles(int(seed), n)
    return (u * 9007199254740992.0).astype(np.int64).tolist()


Record = collections.namedtuple("Record", "seed step position row cls accept")  # step: of its rollout; position: candidate of that step, from 1


def build(log, pi, seeds, plan, provider="pcg64", gamma=0.9):
    """The sequential construction (module docstring).  `log`: dict with z, z_next, actions (nA = 2), rewards, terminals, steps and
    action_distributions [N, 2] f64 -- the BASE log, copied.  The rollouts are simulated in the order of `seeds`.  Returns
    dict(log, records, planned, skipped, trace): the built log, one Record per targeted meeting that was realised, the number of planned
    meetings, a Counter of skipped classes, and trace[seed] = the host simulation of that rollout in the shape of OraclePSRS.evalmc's result."""
    from oracle import oracle as O
    log = {k: np.array(v, copy=True) for k, v in log.items()}
    z, zn, act, term = log["z"], log["z_next"], log["actions"], log["terminals"]
    plog, rew = log["action_distributions"], log["rewards"].astype(np.float64)
    assert plog.dtype == np.float64 and plog.shape[1] == 2
    pi = np.asarray(pi, np.float64)
    N, nS = len(z), pi.shape[0]
    order = np.argsort(z, kind="stable")
    seg = np.searchsorted(z[order], np.arange(nS + 1))
    local = np.empty(N, np.int64)
    local[order] = np.arange(N) - seg[z[order]]
    init_rows = np.flatnonzero(log["steps"] == 0)
    fixed = np.zeros(N, bool)
    Tof = [0] * N
    seq, i_special, i_loc, i_pay, meetings, planned = plan.sequence(), 0, 0, 0, 0, 0
    records, skipped, traces = [], collections.Counter(), {}
    sh_of = {f: 53 - b for f, b in FMT_BITS.items()}

    def realise(g, s, k, cls):
        """Give row g the class; False where it cannot be reached."""
        nonlocal i_pay
        parts = cls.split(":") if cls[1:2] == ":" else [None, cls]
        bits = plan.bits if parts[0] is None else FMT_BITS[parts[0]]
        kind, a = parts[1], int(act[g])
        if kind in ("T=0", "thr=1", "nan"):
            assert pi[s][0] == 1.0 and pi[s][1] == 0.0
            act[g] = 1 if kind == "T=0" else 0
            plog[g] = (0.5, 0.0) if kind == "nan" else (0.5, 0.5)
            return True
        if kind == "thr>1":
            plog[g, a], plog[g, 1 - a] = -0.5, -1.0
            return threshold(pi[s], plog[g], a) == T_MAX
        tp = _target(kind, k, bits)
        sol = tp and _solve(pi[s][a], pi[s][1 - a], tp[0], tp[1])
        if not sol:
            return False
        keep = plog[g].copy()
        plog[g, a], plog[g, 1 - a] = sol
        if not bool(tp[1](np.int64(threshold(pi[s], plog[g], a)))):
            plog[g] = keep
            return False
        if len(parts) > 2:  # ":hi" / ":loc": the payload closest to all ones
            term[g], zn[g] = True, nS - 1
        elif kind in plan.payload:
            term[g], zn[g] = bool(i_pay & 2), (nS - 1) if i_pay & 1 else 0
            i_pay += 1
        return True

    for seed in seeds:
        perms = {}

        def perm(n):
            if n not in perms:
                perms[n] = O.permutation(int(seed), n)
            return perms[n]
        queues = [order[seg[s]:seg[s + 1]][perm(int(seg[s + 1] - seg[s]))].tolist() if seg[s + 1] > seg[s] else [] for s in range(nS)]
        initq = init_rows[perm(len(init_rows))].tolist() if len(init_rows) else []
        k53 = draws(provider, seed, N + 1)
        heads, ih, di, cand = [0] * nS, 0, 0, 0
        rows, popped, Gs, lengths = [], [], [], []
        terminate = False
        while not terminate and ih < len(initq):
            cur, G, t, done = int(z[initq[ih]]), 0.0, 0, False
            ih += 1
            while not done:
                q, h, npop, acc = queues[cur], heads[cur], 0, -1
                while h < len(q):
                    g = q[h]
                    h += 1
                    npop += 1
                    k = k53[di]
                    di += 1
                    if not fixed[g]:
                        fixed[g] = True
                        cls = None
                        if plan.loc_state == cur and local[g] >= plan.loc_min:
                            cls = plan.loc_classes[i_loc % len(plan.loc_classes)]
                            i_loc += 1
                        elif meetings % plan.every == 0:
                            if cur == plan.special_state:
                                cls = plan.special[i_special % len(plan.special)]
                                i_special += 1
                            else:
                                cls = next(seq)
                        meetings += 1
                        if cls is not None:
                            planned += 1
                            if realise(g, cur, k, cls):
                                records.append(Record(seed, len(rows), npop, g, cls, expected_accept(cls)))
                            else:
                                skipped[cls] += 1
                                cls = None
                        Tof[g] = threshold(pi[cur], plog[g], int(act[g]))
                        if cls is not None:
                            assert (k <= Tof[g]) == records[-1].accept, (cls, k, Tof[g])
                    if k <= Tof[g]:
                        acc = g
                        break
                heads[cur] = h
                cand += npop
                if acc < 0:
                    terminate = True
                    break
                rows.append(acc)
                popped.append(npop)
                done = bool(term[acc])
                G = G + gamma ** t * float(rew[acc])
                t += 1
                cur = int(zn[acc])
            lengths.append(t)
            if done:
                Gs.append(G)
        traces[seed] = dict(Gs=np.array(Gs, np.float64), lengths=np.array(lengths, np.int64), steps=len(rows), candidates=cand,
                            trace_rows=np.array(rows, np.int64), trace_popped=np.array(popped, np.int64))
    return dict(log=log, records=records, planned=planned, skipped=skipped, trace=traces, gamma=gamma)


def census(built):
    """Counts per class, and how many targeted meetings came at candidate positions 1, 2, >= 3 and >= 9 of their step."""
    pos = [r.position for r in built["records"]]
    return dict(classes=dict(collections.Counter(r.cls for r in built["records"])), planned=built["planned"], skipped=sum(built["skipped"].values()),
                positions={"1": sum(p == 1 for p in pos), "2": sum(p == 2 for p in pos), ">=3": sum(p >= 3 for p in pos), ">=9": sum(p >= 9 for p in pos)})


# ---- the base logs and the tables of the tests ----
def base_log(sizes, seed, p_done, p_init, back_to=None):
    """Rows of state s: sizes[s], shuffled over the buffer.  Logged actions uniform, rewards f32, base thresholds uniform in (0.1, 0.6)
    (p_log = 0.5 / thr for the logged action, 0.5 for the other: rejected windows are common, so planned ties also arrive behind
    them).  z_next uniform over the states, or (`back_to` = (state, p)) that state with probability p and a uniform other one else."""
    g = np.random.default_rng(seed)
    nS, N = len(sizes), int(np.sum(sizes))
    z = g.permutation(np.repeat(np.arange(nS, dtype=np.int64), sizes))
    if back_to is None:
        zn = g.integers(0, nS, N, dtype=np.int64)
    else:
        zn = np.where(g.random(N) < back_to[1], back_to[0], g.integers(0, nS, N, dtype=np.int64))
    a = g.integers(0, 2, N, dtype=np.int64)
    p = np.full((N, 2), 0.5)
    p[np.arange(N), a] = 0.5 / g.uniform(0.1, 0.6, N)
    t0 = g.random(N) < p_init
    t0[0] = True
    return dict(z=z, z_next=zn, observations=z, next_observations=zn, actions=a, action_distributions=p, rewards=g.random(N).astype(np.float32),
                terminals=g.random(N) < p_done, steps=np.where(t0, 0, 1).astype(np.int64))


_CACHE = {}


def table_a(every, provider="pcg64"):
    """Format A (and the window / generic kernels): six states of about 1000 rows, nA = 2, p_done 0.05; state 2 is the special one.
    Seeds 0..7: eight rollouts are two chain wavefronts of four.  The earliest rollouts of the construction meet the most unfixed rows,
    so they are built in the order 0, 4, 1, 5, ..: both wavefronts get their share of the targeted meetings."""
    name = ("a", every, provider)
    if name not in _CACHE:
        sizes = [1000, 1040, 900, 1100, 960, 1000]
        pi = np.full((6, 2), 0.5)
        pi[2] = (1.0, 0.0)
        plan = Plan(every, A_ACCEPTS, A_REJECTS, 21, special_state=2, special=A_SPECIAL, payload=A_PAYLOAD)
        b = build(base_log(sizes, 1000 + every, 0.05, 0.15), pi, [0, 4, 1, 5, 2, 6, 3, 7], plan, provider)
        _CACHE[name] = dict(b, pi=pi, seeds=list(range(8)))
    return _CACHE[name]


def table_bc(big=70_000):
    """Formats C and B: one state of `big` rows and 254 of 40 (z_next = 254 exists), four rollouts.  A state of 131072 rows adds the
    rows with a local row >= 0x1ff00, every one of them targeted (format C's high bits of the local row all set)."""
    name = ("bc", big)
    if name not in _CACHE:
        sizes = [big] + [40] * 254
        pi = np.full((255, 2), 0.5)
        loc = dict(loc_state=0, loc_min=0x1FF00, loc_classes=C_LOC) if big > 0x1FF00 else {}
        plan = Plan(8, BC_ACCEPTS, BC_REJECTS, 14, **loc)
        b = build(base_log(sizes, big, 0.05, 0.05, back_to=(0, 0.97)), pi, [0, 1, 2, 3], plan)
        _CACHE[name] = dict(b, pi=pi, seeds=[0, 1, 2, 3])
    return _CACHE[name]
