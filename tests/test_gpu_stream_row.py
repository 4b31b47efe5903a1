"""The rollout's draw-stream row (include/offsim.h: offsim_rollouts.rng, rng_kind) as every kernel that replays a rollout leaves it, against the host:
  PCG64:  (PCG64(seed) advanced by n, its increment)      -- numpy.random.PCG64.advance (tests/pcg_jump_host.py)
  Philox: (seed, n0 + n, 0, 0)
with n the candidates the calls so far report for that rollout (out_popped, `cand` of offsim_evalmc_out; offsim_vector_step and
offsim_vector_collect report no count, there n is what the call added to the rollout's queue cursors: with the rejection on, every popped
candidate is one draw).  A second call goes on from the first.

The table: 6 states, 3 actions, 1500 rows in table order (no shuffle).  State HOT has ~300 rows that all log action 0; state EMPTY has no
row as a from-state (one row, the last of state 4's queue, leads to it).  R = 5 rollouts -- two blocks of 4 wavefronts, the second
partial.  The step kernels find rollout 0 in EMPTY (KeyError, no draw, row untouched), rollout 1 in HOT with p_new = 1e-12 on the logged
action (a candidate is accepted with probability < 1e-8: the whole queue is popped, more than 64 draws), rollouts 2 and 4 in ordinary
states with a Dirichlet p_new (64 rejections in a row have probability < 1e-9: 1 to 64 draws) and rollout 3 inactive (cur_slot = -1).
The scans know no inactive rollout; theirs has no initial row left (init_cursor = N0), which draws nothing either."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pcg_jump_host as H  # noqa: E402

torch = pytest.importorskip("torch")

R = 5
SEEDS = [3, 11, 2 ** 40 + 5, 17, 23]
HOT, EMPTY, N_STATES, N_ACTIONS, N_ROWS = 0, 5, 6, 3, 1500
SLOTS = [EMPTY, HOT, 1, -1, 2]
IDLE = 3  # the rollout that draws nothing in any call
PHILOX_N0 = 7  # draws the Philox rollouts have behind them when the test starts (odd: the scans pair draws from an even position)
M64 = (1 << 64) - 1
KINDS = ["pcg64", "philox"]
GAMMA = 0.9


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    from rl_offline_simulation_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


def experience():
    from rl_offline_simulation_amd import synth
    e = synth.synth_iid(N_ROWS, N_STATES - 1, N_ACTIONS, seed=77)
    e["actions"][e["z"] == HOT] = 0
    e["z_next"][np.nonzero(e["z"] == 4)[0][-1]] = EMPTY
    return e


_TABLES = {}


def table_of(gpu, plog=np.float32):
    from rl_offline_simulation_amd.table import TransitionTable
    if plog not in _TABLES:
        e = experience()
        _TABLES[plog] = TransitionTable(e["z"], e["actions"], e["rewards"], e["z_next"], e["terminals"], e["action_distributions"], e["steps"] == 0,
                                        device=gpu, plog_dtype=plog)
        lens = _TABLES[plog].segment_lengths()
        assert len(lens) == N_STATES and lens[EMPTY] == 0 and 250 < lens[HOT] < 350
    return _TABLES[plog]


def policy():
    from rl_offline_simulation_amd import synth
    return synth.dirichlet_policy(N_STATES, N_ACTIONS)


def p_new_steps(dtype):
    p = policy()[[max(s, 0) for s in SLOTS]]
    p[1] = [1e-12, 0.5, 0.5]
    return p.astype(dtype)


def make_env(table, kind, n=R, policy_for_streams=None):
    from rl_offline_simulation_amd.evaluators import BatchedPSRS
    from rl_offline_simulation_amd.evaluators.batched import SHUFFLE_NONE
    env = BatchedPSRS(table, n)
    env.reset_sampler(SEEDS[:n], shuffle=SHUFFLE_NONE, policy=policy_for_streams, rejection=kind)
    if kind == "philox":
        env.state.rng[:, 1] = PHILOX_N0
    return env


def place(state, slots):
    state.cur_slot.copy_(torch.tensor(slots, dtype=torch.int32))


def rng_rows(state):
    torch.cuda.synchronize()
    return state.rng.cpu().numpy().view(np.uint64).copy()


def cursor_sums(state):
    torch.cuda.synchronize()
    return state.cursor.to(torch.int64).sum(dim=1).cpu().numpy()


def host_rows(kind, totals, seeds=SEEDS):
    out = np.zeros((len(totals), 4), dtype=np.uint64)
    for i, (seed, n) in enumerate(zip(seeds, totals)):
        if kind == "philox":
            out[i] = [seed, PHILOX_N0 + int(n), 0, 0]
        else:
            st, inc = H.advanced(seed, int(n)), H.pcg_state(seed)[1]
            out[i] = [st >> 64, st & M64, inc >> 64, inc & M64]
    return out


def assert_rows(state, kind, totals, before):
    got = rng_rows(state)
    assert np.array_equal(got, host_rows(kind, totals, SEEDS[:len(totals)])), (kind, totals)
    assert np.array_equal(got[np.asarray(totals) == 0], before[np.asarray(totals) == 0])  # (no draw: not a word of the row is written)
    return got


def three_classes(popped):
    """The condition of the step tests: no draw, 1 .. 64 draws and more than 64 draws all occur among the four active rollouts."""
    act = [int(popped[i]) for i in range(R) if i != IDLE]
    assert any(n == 0 for n in act) and any(1 <= n <= 64 for n in act) and any(n > 64 for n in act), popped


# ---- the step kernels ----
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("plog,prob", [(np.float32, np.float64), (np.float32, np.float32), (np.float64, np.float64), (np.float16, np.float64)],
                         ids=["f32-F64", "f32-F32", "f64-F64", "f16-F64"])
def test_step_batch(plog, prob, kind, gpu):
    from rl_offline_simulation_amd import _lib as L
    table = table_of(gpu, plog)
    env = make_env(table, kind)
    place(env.state, SLOTS)
    p = p_new_steps(prob)
    row0 = rng_rows(env.state)
    assert np.array_equal(row0, host_rows(kind, [0] * R))
    env.step(p, reject_mode=L.REJECT_NEVER)  # no draw: every row bit-identical
    assert np.array_equal(rng_rows(env.state), row0)
    env.state.rewind()
    place(env.state, SLOTS)
    _, status, popped = env.step(p)
    torch.cuda.synchronize()
    n1 = popped.cpu().numpy().astype(np.int64)
    assert status.cpu().tolist() == [L.ST_KEYERROR, L.ST_EXHAUSTED, L.ST_OK, L.ST_INACTIVE, L.ST_OK]
    assert n1[1] == table.segment_lengths()[HOT]
    three_classes(n1)
    assert np.array_equal(n1, cursor_sums(env.state))
    assert_rows(env.state, kind, n1, row0)
    _, _, popped = env.step(p)
    torch.cuda.synchronize()
    n2 = popped.cpu().numpy().astype(np.int64)
    assert n2.sum() > 0
    assert_rows(env.state, kind, n1 + n2, row0)


def vector_step(env, p, mode, reject_mode):
    from rl_offline_simulation_amd import _lib as L
    L.check(L.load().offsim_vector_step(C.byref(env.table.c), C.byref(env.state.c), L.ptr(p), mode, reject_mode, None, 0, None, 0, None,
                                        L.ptr(env._row), L.ptr(env._status), L.stream_ptr()))
    torch.cuda.synchronize()
    return env._status.cpu().tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_vector_step(kind, gpu):
    from rl_offline_simulation_amd import _lib as L
    table = table_of(gpu)
    env = make_env(table, kind)
    place(env.state, SLOTS)
    p = torch.from_numpy(p_new_steps(np.float64)).to(gpu)
    row0 = rng_rows(env.state)
    vector_step(env, p, L.PROB_F64, L.REJECT_NEVER)
    assert np.array_equal(rng_rows(env.state), row0)
    env.state.rewind()
    place(env.state, SLOTS)
    status = vector_step(env, p, L.PROB_F64, L.REJECT_DEFAULT)
    n1 = cursor_sums(env.state)
    assert status[0] == L.ST_KEYERROR and status[1] == L.ST_EXHAUSTED and status[IDLE] == L.ST_INACTIVE
    three_classes(n1)
    assert_rows(env.state, kind, n1, row0)
    vector_step(env, p, L.PROB_F64, L.REJECT_DEFAULT)
    n12 = cursor_sums(env.state)
    assert n12.sum() > n1.sum()
    assert_rows(env.state, kind, n12, row0)


def exo_setup(gpu, kind):
    """PSRS_Exo's two queue families: the s-table is the test's table, the x-table queues the same rows by an exogenous state of 3 values."""
    from rl_offline_simulation_amd.table import RolloutState, TransitionTable
    ts = table_of(gpu)
    if "x" not in _TABLES:
        g = np.random.default_rng(5)
        x, x_next = g.integers(0, 3, N_ROWS), g.integers(0, 3, N_ROWS)
        _TABLES["x"] = TransitionTable(x, np.zeros(N_ROWS, np.int64), np.zeros(N_ROWS), x_next, np.zeros(N_ROWS, bool), np.ones((N_ROWS, 1), np.float32),
                                       experience()["steps"] == 0, device=gpu)
    tx = _TABLES["x"]
    env = make_env(ts, kind)
    place(env.state, SLOTS)
    rx = RolloutState(tx, R)
    place(rx, [0, 1, 2, 0, 1])
    return ts, tx, env, rx


def step_exo(ts, tx, rs, rx, p, mode, out):
    from rl_offline_simulation_amd import _lib as L
    b = out.data_ptr()
    return L.load().offsim_step_exo(C.byref(ts.c), C.byref(tx.c), C.byref(rs.c), C.byref(rx.c), L.ptr(p), mode, b, b + 4 * R, b + 8 * R, b + 12 * R,
                                    L.stream_ptr())


@pytest.mark.gpu
def test_step_exo_pcg64(gpu):
    from rl_offline_simulation_amd import _lib as L
    ts, tx, env, rx = exo_setup(gpu, "pcg64")
    p = torch.from_numpy(p_new_steps(np.float64)).to(gpu)
    out = torch.zeros((4, R), dtype=torch.int32, device=gpu)
    row0 = rng_rows(env.state)
    L.check(step_exo(ts, tx, env.state, rx, p, L.PROB_F64, out))
    torch.cuda.synchronize()
    n1 = out[3].cpu().numpy().astype(np.int64)
    assert out[2].cpu().tolist()[:2] == [L.ST_KEYERROR, L.ST_EXHAUSTED] and out[2, IDLE] == L.ST_INACTIVE
    three_classes(n1)
    assert_rows(env.state, "pcg64", n1, row0)
    L.check(step_exo(ts, tx, env.state, rx, p, L.PROB_F64, out))
    torch.cuda.synchronize()
    n2 = out[3].cpu().numpy().astype(np.int64)
    assert n2.sum() > 0
    assert_rows(env.state, "pcg64", n1 + n2, row0)


@pytest.mark.gpu
def test_step_exo_refuses_philox(gpu):
    """k_step_exo draws from PCG64 only: a Philox pair is refused, nothing is stepped."""
    from rl_offline_simulation_amd import _lib as L
    ts, tx, env, rx = exo_setup(gpu, "philox")
    p = torch.from_numpy(p_new_steps(np.float64)).to(gpu)
    out = torch.zeros((4, R), dtype=torch.int32, device=gpu)
    before = [x.clone() for x in (env.state.rng, env.state.cursor, env.state.cur_slot, rx.cursor, rx.cur_slot)]
    assert step_exo(ts, tx, env.state, rx, p, L.PROB_F64, out) == L.EUNSUPPORTED
    assert b"step_exo" in L.load().offsim_last_error() and b"PCG64" in L.load().offsim_last_error()
    torch.cuda.synchronize()
    for a, b in zip(before, (env.state.rng, env.state.cursor, env.state.cur_slot, rx.cursor, rx.cur_slot)):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("slot,p", [(HOT, [1e-12, 0.5, 0.5]), (1, [0.2, 0.3, 0.5])], ids=["hot", "plain"])
def test_step_server_one_request_then_stop(slot, p, kind, gpu):
    """One request to the resident step server, then the stop; and once more.  HOT: more than 64 draws, the advance past the jump table."""
    table = table_of(gpu)
    env = make_env(table, kind, n=1)
    place(env.state, [slot])
    row0 = rng_rows(env.state)
    total = 0
    for call in range(2):
        _, status, popped = env.step_single(np.asarray(p, dtype=np.float64))
        assert env._mb is not None  # (served by the resident wavefront)
        env._quiesce()
        assert (popped > 64) if (slot == HOT and call == 0) else (popped <= 64)
        total += popped
        assert total > 0
        assert_rows(env.state, kind, [total], row0)
        assert cursor_sums(env.state)[0] == total


# ---- the scans ----
def idle_for_scans(env):
    env.state.init_cursor[IDLE] = env.table.N0


def scan_twice(env, kind, run):
    """run(n_episodes) -> the call's out dict; two episodes first, then on to the end of the queues."""
    idle_for_scans(env)
    row0 = rng_rows(env.state)
    o = run(2)
    n1 = o["cand"].cpu().numpy()
    assert n1[IDLE] == 0 and (np.delete(n1, IDLE) > 0).all(), n1
    assert np.array_equal(n1, cursor_sums(env.state))
    assert_rows(env.state, kind, n1, row0)
    o = run(None)
    n2 = o["cand"].cpu().numpy()
    assert n2[IDLE] == 0 and n2.sum() > 0
    assert_rows(env.state, kind, n1 + n2, row0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_eval_mc(kind, gpu):
    table = table_of(gpu)
    env = make_env(table, kind)
    pi = table.policy_slots(policy())
    scan_twice(env, kind, lambda n: env.eval_mc(pi, GAMMA, n_episodes=n, fast=False))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_eval_mc_rows_policy(kind, gpu):
    table = table_of(gpu)
    env = make_env(table, kind)
    pi = torch.from_numpy(table.policy_slots(policy())).to(gpu)
    p_next, p_init = pi[table.z_next.to(torch.int64)], pi[table.init_slot.to(torch.int64)]
    scan_twice(env, kind, lambda n: env.eval_mc_rows_policy(p_next, p_init, GAMMA, n_episodes=n))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_eval_td(kind, gpu):
    from rl_offline_simulation_amd import _lib as L
    table = table_of(gpu)
    env = make_env(table, kind)
    pi = table.policy_slots(policy())
    scan_twice(env, kind, lambda n: env.eval_td(pi, GAMMA, L.TD_QLEARN, 0.1, n_episodes=n))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_eval_mc_keys(kind, gpu, monkeypatch):
    monkeypatch.setenv("OFFSIM_SCAN_ROWS", "0")
    table = table_of(gpu)
    env = make_env(table, kind)
    pi = table.policy_slots(policy())

    def run(n):
        o = env.eval_mc(pi, GAMMA, n_episodes=n)
        assert env._streams is None and "_kernel" not in o  # (offsim_eval_mc_keys)
        return o
    scan_twice(env, kind, run)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_eval_mc_streams(kind, gpu, monkeypatch):
    monkeypatch.setenv("OFFSIM_SCAN_ROWS", "1")
    table = table_of(gpu)
    pi = table.policy_slots(policy())
    env = make_env(table, kind, policy_for_streams=pi)
    assert env.scan_variant() == "k_eval_mc_rows"

    def run(n):
        o = env.eval_mc(pi, GAMMA, n_episodes=n)
        assert env._streams is not None and "_kernel" not in o  # (offsim_eval_mc_streams)
        return o
    scan_twice(env, kind, run)
    from rl_offline_simulation_amd import _lib as L
    L.check_async_faults()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_vector_collect_tabular(kind, gpu):
    """offsim_vector_collect, tabular form, T = 3: observations are the states themselves."""
    from rl_offline_simulation_amd import _lib as L
    table = table_of(gpu)
    env = make_env(table, kind)
    place(env.state, SLOTS)
    e = experience()
    pi = torch.from_numpy(table.policy_slots(policy())).to(gpu).contiguous()
    obs_init, obs_next = (torch.from_numpy(e[k].astype(np.int64)).to(gpu) for k in ("z", "z_next"))
    T = 3
    ep_t, obs_row = torch.zeros(R, dtype=torch.int32, device=gpu), torch.full((R,), -1, dtype=torch.int32, device=gpu)
    alive, obs = torch.tensor([s >= 0 for s in SLOTS], dtype=torch.uint8, device=gpu), torch.tensor(SLOTS, dtype=torch.int64, device=gpu)
    row, flags = torch.zeros((T, R), dtype=torch.int32, device=gpu), torch.zeros((T, R), dtype=torch.uint8, device=gpu)
    status = torch.zeros(R, dtype=torch.int32, device=gpu)
    pol = L.CollectPolicy(form=L.COLLECT_TABULAR, pi=L.ptr(pi))
    st = L.CollectState(ep_t=L.ptr(ep_t), obs_row=L.ptr(obs_row), alive=L.ptr(alive), obs=L.ptr(obs), obs_next=L.ptr(obs_next), obs_init=L.ptr(obs_init),
                        obs_bytes=8)
    out = L.CollectOut(row=L.ptr(row), flags=L.ptr(flags), status=L.ptr(status))
    row0 = rng_rows(env.state)
    totals = []
    for call in range(2):
        L.check(L.load().offsim_vector_collect(C.byref(table.c), C.byref(env.state.c), C.byref(pol), L.PROB_F64, L.REJECT_DEFAULT, T, 0, C.byref(st),
                                               C.byref(out), L.stream_ptr()))
        totals.append(cursor_sums(env.state))
        assert totals[-1][0] == 0 and totals[-1][IDLE] == 0  # (KeyError, inactive)
        assert_rows(env.state, kind, totals[-1], row0)
    assert status.cpu().tolist()[0] == L.ST_KEYERROR and status.cpu().tolist()[IDLE] == L.ST_INACTIVE
    assert (totals[0][[1, 2, 4]] >= 3).all() and totals[1].sum() > totals[0].sum()


# ---- a refusal that needs no device: R = 0 rollouts (and no mailbox), so that no build of the library can reach a launch from here ----
def test_prob_mode_that_is_neither_f32_nor_f64_is_refused_everywhere():
    from rl_offline_simulation_amd import _lib as L
    lib = L.load()
    fake = 0x1000  # (never dereferenced)
    t = L.Table(N=10, n_slots=3, nA=2, plog_dtype=L.F32, r_dtype=L.F32, seg_off=fake, p_log=fake, a=fake, r=fake, z_next=fake, done=fake, orig_idx=fake,
                N0=2, init_slot=fake, init_orig=fake)
    ro = L.Rollouts(R=0, rng=fake, cursor=fake, init_cursor=fake, cur_slot=fake)
    oc = L.EvalMCOut(sum_g=fake, n_ep=fake, steps=fake, cand=fake, n_len=fake, status=fake)
    pol = L.CollectPolicy(form=L.COLLECT_TABULAR, pi=fake)
    st = L.CollectState(ep_t=fake, obs_row=fake, alive=fake, obs=fake, obs_next=fake, obs_init=fake, obs_bytes=8)
    out = L.CollectOut(row=fake, flags=fake)
    val, ppo = L.CollectValue(form=L.VALUE_ROWS, v_next=fake, v_init=fake), L.CollectPPOOut(value=fake, logp=fake, final_value=fake)
    bt, bro = C.byref(t), C.byref(ro)
    calls = {
        "step_batch": lambda: lib.offsim_step_batch(bt, bro, fake, 7, L.REJECT_DEFAULT, 1, None, None, None, None),
        "vector_step": lambda: lib.offsim_vector_step(bt, bro, fake, 7, L.REJECT_DEFAULT, None, 0, None, 0, None, None, None, None),
        "step_exo": lambda: lib.offsim_step_exo(bt, bt, bro, bro, fake, 7, None, None, None, None, None),
        "step_server_start": lambda: lib.offsim_step_server_start(bt, bro, None, 7, 1, None),
        "eval_mc": lambda: lib.offsim_eval_mc(bt, bro, fake, 7, L.REJECT_DEFAULT, 0.9, None, 0, 1, C.byref(oc), None),
        "eval_mc_rows_policy": lambda: lib.offsim_eval_mc_rows_policy(bt, bro, fake, fake, 7, L.REJECT_DEFAULT, 0.9, None, 0, 1, C.byref(oc), None, None),
        "vector_collect": lambda: lib.offsim_vector_collect(bt, bro, C.byref(pol), 7, L.REJECT_DEFAULT, 0, 0, C.byref(st), C.byref(out), None),
        # (collect_ppo validates through collect's own preparation: its texts carry collect's prefix)
        "vector_collect_ppo": lambda: lib.offsim_vector_collect_ppo(bt, bro, C.byref(pol), C.byref(val), 7, L.REJECT_DEFAULT, 0, 0, C.byref(st), C.byref(out),
                                                                    C.byref(ppo), None),
    }
    for who, call in calls.items():
        assert call() == L.EINVAL, who
        msg = lib.offsim_last_error()
        assert msg.startswith(who.replace("_ppo", "").encode() + b":") and b"prob_mode" in msg, msg


@pytest.mark.gpu
def test_prob_mode_7_on_real_rollouts_steps_nothing(gpu):
    """The same refusal with a real table and R = 5 placed rollouts: OFFSIM_EINVAL, and cursors, states and rows as they were."""
    from rl_offline_simulation_amd import _lib as L
    table = table_of(gpu)
    env = make_env(table, "pcg64")
    place(env.state, SLOTS)
    p = torch.from_numpy(p_new_steps(np.float64)).to(gpu)
    before = [x.clone() for x in (env.state.rng, env.state.cursor, env.state.cur_slot)]
    lib = L.load()
    assert lib.offsim_step_batch(C.byref(table.c), C.byref(env.state.c), L.ptr(p), 7, L.REJECT_DEFAULT, 1, L.ptr(env._row), L.ptr(env._status),
                                 L.ptr(env._popped), L.stream_ptr()) == L.EINVAL
    assert lib.offsim_vector_step(C.byref(table.c), C.byref(env.state.c), L.ptr(p), 7, L.REJECT_DEFAULT, None, 0, None, 0, None, L.ptr(env._row),
                                  L.ptr(env._status), L.stream_ptr()) == L.EINVAL
    torch.cuda.synchronize()
    for a, b in zip(before, (env.state.rng, env.state.cursor, env.state.cur_slot)):
        assert torch.equal(a, b)
