"""In-kernel clock stamps of the keyed shuffle's roles and of the hand-over between cut launches (library built with -DSHUF_PROF: the
stamps overwrite the first digests of every chain's stream, so such a build is for this script only).  The stamps of the LAST launch
survive, so the reset runs once per launch of the cut list with OFFSIM_SHUFFLE_PROF_LAUNCHES = 1, 2, ...
usage: OFFSIM_LIB=.../lib_prof.so prof_shuffle.py [N] [R] [launches = 4: the product's cut list 32768 + 8192 + 2048; cuts + 1 for another]"""
import sys, os, time, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rl_offline_simulation_amd import synth
from rl_offline_simulation_amd.table import TransitionTable
from rl_offline_simulation_amd.evaluators import BatchedPSRS
N = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
R = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
e = synth.synth_iid(N, 162, 2, seed=20221107)
t = TransitionTable(e["z"], e["actions"], e["rewards"], e["z_next"], e["terminals"], e["action_distributions"], e["steps"] == 0)
pi = t.policy_slots(synth.dirichlet_policy(162, 2))
env = BatchedPSRS(t, R)
seeds = np.arange(R, dtype=np.uint64)
L = int(sys.argv[3]) if len(sys.argv) > 3 else 4
seg = t.seg_off.cpu().numpy().astype(np.int64)
rows = torch.arange(0, R, 37, device="cuda")
prev = 0.0
for launches in range(1, L + 1):
    os.environ["OFFSIM_SHUFFLE_PROF_LAUNCHES"] = str(launches)
    for k in range(2):
        torch.cuda.synchronize(); t0 = time.time()
        env.reset_sampler(seeds, policy=pi)
        torch.cuda.synchronize(); dt = time.time() - t0
    print(f"== launches={launches}\nreset_sampler {dt:.4f} s (this launch {dt - prev:.4f} s)")
    prev = dt
    dig = env._streams["dig"]
    acc = [dig[rows, seg[s]:seg[s] + 16].cpu().numpy().astype(np.int64) & 0xffffffff for s in range(0, len(seg) - 1, 9) if seg[s + 1] - seg[s] >= 64]
    m = (np.concatenate(acc).astype(float) * 64).mean(axis=0)
    print("clocks per chain (workgroup, behind the fill):", int(m[12]))
    for w, (name, extra) in enumerate([("G0", "writing chunks out"), ("C", "waiting for room in the j ring"), ("A", "groups with a conflict"), ("G1", "writing chunks out")]):
        print(f"{name}: loop {int(m[3 * w])}, waiting for its neighbour {int(m[3 * w + 1])}, {extra} {int(m[3 * w + 2])}")
    print(f"hand-over: kernel entry to the end of the fill {int(m[13])}, SH_DONE to the workgroup's last store {int(m[14])}; G0 to its first published block {int(m[15])}", flush=True)
