"""python tools/search_cost.py [out.json] [--cpu_reps N]  (needs an MI355X; profiles/search_timing.json)
Cost of the Monte Carlo search in the physics score, in the setup of tools/minimize_cost.py: 40 poses of the 3dpf ligand (37 heavy
atoms, 5 rotatable bonds; the perturbation recipe of the test fixture) against the full typed receptor.  HIP events around the fused
calls alone, the min / median / max of REPS calls after WARM warm-up calls:
  1. ddp_pose_search, all C = 10 cycles of K = 30 iterations in one launch, at R = 1, 2, 4, 6, 8, 12 replicas (40 to 480 rows);
  2. in the same process ddp_pose_minimize at 300 iterations on the same 40 poses: the same number of line-search iterations per
     row, the yardstick;
  3. the launch-by-launch form at R = 6 (the whole advance call) and the PyTorch fp64 form on the host (--cpu_reps calls, default 3).
Then what the default search does to the energies: E after PoseMinimizer(100) and after the search, how many poses end above E = 0,
the median RMSD to the crystal pose before and after.  A lower E is not a better pose: the score is not validated."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffdock_pocket_amd import inputs as I
from diffdock_pocket_amd import launch as LA
from diffdock_pocket_amd import minimize as M
from diffdock_pocket_amd import scoring as SC
from diffdock_pocket_amd import search as SE
from diffdock_pocket_amd.sampler import modify_conformer

REPS, WARM, S, CYCLES, K = 30, 5, 40, 10, 30
argv = sys.argv[1:]
CPU_REPS = int(argv.pop(argv.index("--cpu_reps") + 1)) if "--cpu_reps" in argv else 3
argv = [a for a in argv if a != "--cpu_reps"]
GOLDEN = os.path.join(ROOT, "tests", "golden")
pdb, sdf = open(os.path.join(GOLDEN, "3dpf_protein.pdb")).read(), open(os.path.join(GOLDEN, "3dpf_ligand.sdf")).read()
g = I.build_complex_graph(pdb, sdf)
full = SC.typed_receptor(pdb, g.original_center)
dev = torch.device("cuda:0")
host_mz = M.PoseMinimizer(g, receptor=full)


def poses(S):
    gen = torch.Generator().manual_seed(2)
    tr = torch.randn(S, 3, generator=gen, dtype=torch.float64) * 0.5
    rot = torch.randn(S, 3, generator=gen, dtype=torch.float64) * 0.15
    tor = torch.randn(S, host_mz.T, generator=gen, dtype=torch.float64) * 0.3
    return modify_conformer(g["ligand"].pos.float()[None].expand(S, -1, -1).contiguous(), tr.float(), rot.float(), tor.float(),
                            host_mz.bonds, host_mz.rot_idx).contiguous()


def timed(fn, reps=REPS, warm=WARM):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b) * 1e3)
    return [round(u, 1) for u in (min(t), statistics.median(t), max(t))]


def rmsd(x, ref):
    return (x.double() - ref.double()).pow(2).sum(-1).mean(-1).sqrt()


out = {"device": torch.cuda.get_device_name(0), "reps": REPS, "warmup": WARM, "poses": S, "cycles": CYCLES, "iterations": K,
       "n_lig": host_mz.n, "n_tor": host_mz.T, "receptor_atoms_typed": int((full.radii >= 0).sum()),
       "unit": "us per call, min / median / max (HIP events around the call)"}
x = poses(S)
xd = x.to(dev)

# 1. the fused search kernel alone, one launch of S R workgroups
out["ddp_pose_search"] = {}
for R in (1, 2, 4, 6, 8, 12):
    ps = SE.PoseSearcher(g, dev, receptor=full, config=SE.SearchConfig(replicas=R, cycles=CYCLES, iterations=K))
    st = ps.start(xd)
    out["ddp_pose_search"][f"R={R} rows={S * R}"] = timed(lambda: ps._run_fused(st, 0, CYCLES, None, None))
    print("ddp_pose_search", R, out["ddp_pose_search"][f"R={R} rows={S * R}"], flush=True)

# 2. the yardstick: the fused minimiser with as many iterations as one row of the search runs
mz = M.PoseMinimizer(g, dev, receptor=full, config=M.MinimizeConfig(iterations=CYCLES * K))
t, rec = mz._tables(xd, None)
pos, step, acc = xd.clone(), torch.ones(S, dtype=torch.float64, device=dev), torch.zeros(S, dtype=torch.int32, device=dev)
e0, e1 = torch.empty(S, 4, dtype=torch.float64, device=dev), torch.empty(S, 4, dtype=torch.float64, device=dev)


def minimize_300():
    pos.copy_(xd)
    step.fill_(1.0)
    LA.pose_minimize(pos, xd, t["lig_r"], t["lig_f"], rec, t["rec_r"], t["rec_f"], mz.score_config, t["pairs"], mz._bonds_i32, mz._mask_u8, step,
                     acc, e0, e1, CYCLES * K)


out["ddp_pose_minimize_300_iterations"] = timed(minimize_300)
print("ddp_pose_minimize 300", out["ddp_pose_minimize_300_iterations"], flush=True)
out["search_R6_over_minimize_median"] = round(out["ddp_pose_search"][f"R=6 rows={S * 6}"][1] / out["ddp_pose_minimize_300_iterations"][1], 3)

# 3. the launch-by-launch form at R = 6, then the host form
ps = SE.PoseSearcher(g, dev, receptor=full, config=SE.SearchConfig())
st = ps.start(xd)
out["launch_by_launch_R6"] = timed(lambda: ps.advance(st, CYCLES, fused=False), reps=5, warm=1)
print("launch_by_launch_R6", out["launch_by_launch_R6"], flush=True)

# what the default search does to the energies
res = ps.search(xd).cpu()
m100 = M.PoseMinimizer(g, dev, receptor=full, config=M.MinimizeConfig(iterations=100)).minimize(xd).cpu()
crystal = g["ligand"].pos.float()[None]


def spread(e):
    return [round(float(v), 3) for v in (e.min(), e.median(), e.max())]


out["energy_before_min_median_max"] = spread(res.energy_before[:, 3])
out["energy_after_minimizer_100_min_median_max"] = spread(m100.energy_after[:, 3])
out["energy_after_search_replica0_cycle0_min_median_max"] = spread(res.energy_minimized[:, 3])
out["energy_after_search_min_median_max"] = spread(res.energy_after[:, 3])
out["poses_above_zero_after_minimizer_100"] = int((m100.energy_after[:, 3] > 0).sum())
out["poses_above_zero_after_search"] = int((res.energy_after[:, 3] > 0).sum())
out["median_rmsd_to_crystal_before"] = round(float(rmsd(x, crystal).median()), 3)
out["median_rmsd_to_crystal_after_minimizer_100"] = round(float(rmsd(m100.lig_pos, crystal).median()), 3)
out["median_rmsd_to_crystal_after_search"] = round(float(rmsd(res.lig_pos, crystal).median()), 3)
out["chosen_replica_histogram"] = torch.bincount(res.replica.long(), minlength=6).tolist()
out["moves_of_chosen_replica_min_median_max"] = [int(v) for v in (res.moves.min(), res.moves.median(), res.moves.max())]
dst = argv[0] if argv else "search_timing.json"


def save():
    print(json.dumps(out), flush=True)
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)


save()
torch.set_num_threads(16)
out["cpu_threads"] = torch.get_num_threads()
hs = SE.PoseSearcher(g, receptor=full, config=SE.SearchConfig())
tm = []
for _ in range(CPU_REPS):
    t0 = time.perf_counter()
    c = hs.search(x)
    tm.append((time.perf_counter() - t0) * 1e6)
    print("host form", round(tm[-1] / 1e6, 1), "s", flush=True)
if tm:
    out["host_fp64_form"] = [round(u, 1) for u in (min(tm), statistics.median(tm), max(tm))]
    out["energy_after_search_host_min_median_max"] = spread(c.energy_after[:, 3])
save()
