"""NumPy restatement of evalMC_psrs with a policy over observations given as per-row tables (test infrastructure).

Semantics restated from the reference's documented behaviour, not its code:
  reset_sampler(seed)  the rejection stream is default_rng(seed); the initial rows (t == 0, buffer order) are shuffled by a fresh
                       default_rng(seed); each state's queue holds its rows in buffer order, shuffled by its own fresh default_rng(seed)
                       
  reset                pops the head of the initial queue (None when empty)
  step(p_new)          pops candidates of the current state's queue (KeyError if the state has no queue, None when it runs dry) until
                       one is accepted: reject <=> u > (p_new[a] / p_log[a]) / max(p_new / p_log), u = one draw per candidate, with
                       NumPy's own promotion rules (f32 / f32 stays f32 and the draw is compared in f32)
  evalMC               the policy is asked at obs of the popped initial row (P_init[row]) and at next_obs of the accepted row
                       (P_next[row]); G = sum gamma**t r_t; lengths get every episode, Gs only the completed ones

Tables are in caller order: P_next[i] = pi[next_obs[i]], P_init[i] = pi[obs[i]].
"""
import numpy as np


def orders(z, t0, seed):
    init = [i for i in range(len(z)) if t0[i]]
    np.random.default_rng(seed=seed).shuffle(init)
    queues = {}
    for i in range(len(z)):
        queues.setdefault(int(z[i]), []).append(i)
    for k in queues:
        np.random.default_rng(seed=seed).shuffle(queues[k])
    return init, queues


def evalmc_rows(z, a, r, z_next, done, p_log, t0, P_next, P_init, seed, gamma, n_episodes=10 ** 9):
    """Returns dict(Gs, lengths, rows (accepted caller rows in step order), status 'ok' | 'keyerror', obs_row (as the device's out_obs_row:
    i >= 0 next_obs of row i, -2 - i obs of row i, -1 None))."""
    init, queues = orders(z, t0, seed)
    heads = {k: 0 for k in queues}
    rng = np.random.default_rng(seed=seed)
    ic = 0
    Gs, lengths, rows = [], [], []
    obs_row = None
    episode, terminate = 0, False
    while episode < n_episodes and not terminate:
        if ic >= len(init):
            obs_row = -1
            break
        i0 = init[ic]
        ic += 1
        s_z, p = int(z[i0]), P_init[i0]
        obs_row = -2 - i0
        G, t, d = 0, 0, False
        while not d:
            if s_z not in queues:
                return dict(Gs=np.asarray(Gs, np.float64), lengths=np.asarray(lengths, np.int64), rows=np.asarray(rows, np.int64),
                            status="keyerror", obs_row=obs_row)
            q, acc = queues[s_z], None
            while acc is None:
                if heads[s_z] >= len(q):
                    break
                j = q[heads[s_z]]
                heads[s_z] += 1
                aj = int(a[j])
                M = (p / p_log[j]).max()
                u = rng.random()
                if not (u > p[aj] / p_log[j][aj] / M):
                    acc = j
            if acc is None:
                terminate = True
                break
            rows.append(acc)
            G = G + (gamma ** t) * r[acc]
            t += 1
            s_z, p, d = int(z_next[acc]), P_next[acc], bool(done[acc])
            obs_row = acc
        lengths.append(t)
        if d:
            Gs.append(G)
            episode += 1
    return dict(Gs=np.asarray(Gs, np.float64), lengths=np.asarray(lengths, np.int64), rows=np.asarray(rows, np.int64), status="ok",
                obs_row=obs_row)


def fixture_inputs(d):
    """The arrays of a tests/golden/obs_policy/*.npz fixture as evalmc_rows takes them."""
    return dict(z=d["z"], a=d["a"], r=d["r"], z_next=d["z_next"], done=d["done"], p_log=d["p_log"], t0=d["t0"], P_next=d["P_next"],
                P_init=d["P_init"])
