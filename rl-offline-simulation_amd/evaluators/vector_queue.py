"""VectorQueueEvaluator: many QueueEvaluator environments whose learner loop runs in one launch.

The reference compares two simulators under the same learner: PSRS, to which the policy reveals its distribution (PPOAgentRevealed), and
QueueEvaluator (offsim4rl/evaluators/queue_evaluator.py:8-131), where the agent draws its own action and the simulator pops the head of
queue (z, a) (PPOAgent, offsim4rl/agents/ppo.py:258-279, on queue_evaluator.py:77-88).  VectorPSRS runs the first on the device; this
class runs the second: `num_envs` independent QueueEvaluator_impl environments over one log, environment k identical to the reference
evaluator after reset_sampler(seed_k), driven for T steps per launch by a policy over OBSERVATIONS (offsim_queue_collect,
csrc/collect_queue.hpp):

    env = VectorQueueEvaluator(dataset, num_envs=1024, num_states=162, encoder=CartpoleBoxEncoder())
    env.reset_sampler(seeds)                  # QueueEvaluator.reset_sampler(seed_k) for every environment k
    env.set_action_seeds(action_seeds)        # environment k draws its actions from default_rng(action_seeds[k]) (default: seeds)
    env.reset()
    batch = env.collect_ppo(actor, critic, 500)           # a PPOBatch: PPOLearner.update / ppo_epoch_log / PPOLearner.fit(env, ...) as they are

The action rule is the package's, as for the tabular queue drivers (DESIGN sections 22 and 24): A = Generator.choice(nA, p=p) on the
environment's own PCG64 stream with p the policy's f32 probabilities widened exactly to f64 -- not the reference agent's
np.random.choice on NumPy's global MT19937 stream.

There is no per-step step() here: BatchedQueueEvaluator.step remains the per-step path.  Mixing it with collect on the same rollout
state is out of scope (this class keeps obs / obs_row / ep_t / alive in step with its own reset and collect only).
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L
from ..spaces import is_discrete
from .queue_evaluator import BatchedQueueEvaluator
from .vector_env import _Collector


class VectorQueueEvaluator(_Collector):
    def __init__(self, dataset, num_envs, num_states=None, encoder=None, device=None, strict=False):
        # the validation of queue_evaluator.py:9-18
        if not is_discrete(dataset.observation_space) and num_states is None and encoder is None:
            raise ValueError("QueueEvaluator only supports discrete observation spaces")
        if (num_states is None or encoder is None) and (num_states != encoder):
            raise ValueError("num_states and encoder either both need to be None, or both need to be specified")
        if not is_discrete(dataset.action_space):
            raise ValueError("QueueEvaluator currently only supports discrete action spaces")
        e = dataset.experience
        if encoder is not None:
            zs, next_zs = np.asarray(encoder.encode(e["observations"])), np.asarray(encoder.encode(e["next_observations"]))
        else:
            zs, next_zs = np.asarray(e["observations"]), np.asarray(e["next_observations"])
        n = len(zs)
        t0 = (np.asarray(e["steps"]) == 0) if "steps" in e else None
        p_log = np.asarray(e["action_distributions"]).reshape(n, -1) if "action_distributions" in e else np.zeros((n, dataset.action_space.n))
        self.num_envs = int(num_envs)
        self.strict = bool(strict)  # raise KeyError((z, a)) like the reference (costs a host sync per call); otherwise such environments just stop
        self._impl = BatchedQueueEvaluator(zs, e["actions"], e["rewards"], next_zs, e["terminals"], p_log, t0, R=self.num_envs, device=device)
        if self._impl.nZ is None:
            raise L.OffsimError("the one-launch queue drivers need dense state ids (this log's ids were compacted to ranks)")
        self.table, self.env = self._impl.table, self._impl.env
        self.nZ, self.nA, self.z_lo = self._impl.nZ, self._impl.nA, self._impl.z_lo
        self.drawn_action = None
        self._init_payload(dataset, encoder is not None)

    def reset_sampler(self, seeds):
        """QueueEvaluator.reset_sampler(seed_k) for every environment; the action streams are left at the sampler seeds."""
        self._impl.reset_sampler(seeds)
        self._sbuf.zero_()  # alive and ep_t
        if self.strict:
            self.env.check_faults()

    def set_action_seeds(self, seeds):
        """Environment k draws its actions from np.random.default_rng(seeds[k])."""
        self._impl.set_action_seeds(seeds)

    def reset(self, mask=None):
        """QueueEvaluator.reset (queue_evaluator.py:113-119) for the environments in `mask` (all if None), with obs, obs_row, ep_t and alive
        kept in step.  Returns (obs [R, ...], alive [R])."""
        return self._reset_envs(mask)

    # collect / collect_ppo / collect_ppo_population are _Collector's: VectorPSRS's arguments and records, with
    #   action     the action the environment drew where a row was served (the served row's logged action, by construction), 0 elsewhere;
    #              self.drawn_action [T, E] i32 keeps the last call's raw record: the action drawn at every asked step, the unserved last
    #              one included (nA: no action could be drawn from a NaN or zero row), -1 where nothing was asked;
    #   tabular    pi [nS, nA] is indexed by the state as the reference's tabular drivers do (BatchedQueueEvaluator.state_rows);
    #   f32 / f64  a policy table is read in its own precision and widened exactly; there is no p_log to compare with.

    # ---- the simulator's part of collect / collect_ppo / collect_ppo_population (_Collector) ----
    def _launch_collect(self, pol, f32, T, cap, st, out, ppo, learners):
        """offsim_queue_collect (ppo None), offsim_queue_collect_ppo, or offsim_queue_collect_ppo_pop for `learners` learners"""
        env, t, lib = self.env, self.table, L.load()
        drawn = torch.empty((T, self.num_envs), dtype=torch.int32, device=t.device)
        if pol.form != L.COLLECT_MLP:
            pol.x_dtype = L.F32 if f32 else L.F64  # the tables' element type
        if ppo is None:
            L.check(lib.offsim_queue_collect(C.byref(t.c), C.byref(env.state.c), self.nA, C.byref(pol), T, cap, C.byref(st), C.byref(out), L.ptr(drawn),
                                             L.stream_ptr()))
        elif learners is not None:
            L.check(lib.offsim_queue_collect_ppo_pop(C.byref(t.c), C.byref(env.state.c), self.nA, C.byref(pol), C.byref(ppo[0]), learners,
                                                     self.num_envs // learners, T, cap, C.byref(st), C.byref(out), L.ptr(drawn), C.byref(ppo[1]),
                                                     L.stream_ptr()))
        else:
            L.check(lib.offsim_queue_collect_ppo(C.byref(t.c), C.byref(env.state.c), self.nA, C.byref(pol), C.byref(ppo[0]), T, cap, C.byref(st),
                                                 C.byref(out), L.ptr(drawn), C.byref(ppo[1]), L.stream_ptr()))
        self.drawn_action = drawn
        return drawn

    def _raise_keyerror(self, status, drawn):
        """KeyError((z, a)) as self.queues[z, a] raises it (queue_evaluator.py:122): the state the environment stopped in and the action it
        had drawn -- the last one asked"""
        k = int(torch.nonzero(status == L.ST_KEYERROR)[0])
        z = int(self.env.state.cur_slot[k]) // self.nA + self.z_lo
        asked = torch.nonzero(drawn[:, k] >= 0)
        raise KeyError((z, int(drawn[int(asked[-1]), k]) if len(asked) else None))

    def _policy_f32(self, dtype):
        return dtype == torch.float32

    def _tabular_policy(self, pi, f32):
        rows = self._impl.state_rows(pi)  # [nZ, nA] by state row, NaN where pi has no row (a step there: KeyError)
        return torch.from_numpy(np.ascontiguousarray(rows.astype(np.float32 if f32 else np.float64))).to(self.table.device)
