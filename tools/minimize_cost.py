"""python tools/minimize_cost.py [out.json]  (needs an MI355X; profiles/minimize_timing.json)
Cost of the minimisation in the physics score: PoseMinimizer.minimize of 40 poses of the 3dpf ligand (37 heavy atoms, 5 rotatable
bonds; the perturbation recipe of the test fixture) against the full typed receptor, 100 iterations - HIP events around the whole call
(the score of the poses before and after included), the min / median / max of REPS calls after WARM warm-up calls, for the fused
kernel (ddp_pose_minimize: one launch) and the launch-by-launch path in the same process; then the PyTorch fp64 form on the host."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffdock_pocket_amd import inputs as I
from diffdock_pocket_amd import minimize as M
from diffdock_pocket_amd import scoring as SC
from diffdock_pocket_amd.sampler import modify_conformer

REPS, WARM, CPU_REPS, S, ITERATIONS = 30, 5, 3, 40, 100
GOLDEN = os.path.join(ROOT, "tests", "golden")
pdb, sdf = open(os.path.join(GOLDEN, "3dpf_protein.pdb")).read(), open(os.path.join(GOLDEN, "3dpf_ligand.sdf")).read()
g = I.build_complex_graph(pdb, sdf)
full = SC.typed_receptor(pdb, g.original_center)
dev = torch.device("cuda:0")
cfg = M.MinimizeConfig(iterations=ITERATIONS)
host = M.PoseMinimizer(g, receptor=full, config=cfg)


def poses(S):
    gen = torch.Generator().manual_seed(2)
    tr = torch.randn(S, 3, generator=gen, dtype=torch.float64) * 0.5
    rot = torch.randn(S, 3, generator=gen, dtype=torch.float64) * 0.15
    tor = torch.randn(S, host.T, generator=gen, dtype=torch.float64) * 0.3
    return modify_conformer(g["ligand"].pos.float()[None].expand(S, -1, -1).contiguous(), tr.float(), rot.float(), tor.float(),
                            host.bonds, host.rot_idx).contiguous()


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b) * 1e3)
    return [round(u, 1) for u in (min(t), statistics.median(t), max(t))]


out = {"device": torch.cuda.get_device_name(0), "reps": REPS, "warmup": WARM, "poses": S, "iterations": ITERATIONS, "n_lig": host.n,
       "n_tor": host.T, "receptor_atoms_typed": int((full.radii >= 0).sum()), "unit": "us per minimize call, min / median / max"}
x = poses(S)
xd = x.to(dev)
mz = M.PoseMinimizer(g, dev, receptor=full, config=cfg)
out["fused"] = timed(lambda: mz.minimize(xd, fused=True))
print("fused", out["fused"], flush=True)
out["launch_by_launch"] = timed(lambda: mz.minimize(xd, fused=False))
print("launch_by_launch", out["launch_by_launch"], flush=True)
out["launch_by_launch_over_fused_median"] = round(out["launch_by_launch"][1] / out["fused"][1], 2)
# the kernel alone, without the two score calls and the allocations of minimize()
step, acc = torch.ones(S, dtype=torch.float64, device=dev), torch.zeros(S, dtype=torch.int32, device=dev)
out["fused_advance_only"] = timed(lambda: mz.advance(xd, xd, step, acc, ITERATIONS, fused=True))
print("fused_advance_only", out["fused_advance_only"], flush=True)
a, b = mz.minimize(xd, fused=True).cpu(), mz.minimize(xd, fused=False).cpu()
out["energy_after_fused"] = [round(float(a.energy_after[:, 3].min()), 3), round(float(a.energy_after[:, 3].max()), 3)]
out["energy_after_launch_by_launch"] = [round(float(b.energy_after[:, 3].min()), 3), round(float(b.energy_after[:, 3].max()), 3)]
out["energy_before"] = [round(float(a.energy_before[:, 3].min()), 3), round(float(a.energy_before[:, 3].max()), 3)]
torch.set_num_threads(16)
out["cpu_threads"] = torch.get_num_threads()
t = []
for _ in range(CPU_REPS):
    t0 = time.perf_counter()
    c = host.minimize(x)
    t.append((time.perf_counter() - t0) * 1e6)
out["host_fp64_form"] = [round(u, 1) for u in (min(t), statistics.median(t), max(t))]
out["energy_after_host"] = [round(float(c.energy_after[:, 3].min()), 3), round(float(c.energy_after[:, 3].max()), 3)]
print(json.dumps(out), flush=True)
dst = sys.argv[1] if len(sys.argv) > 1 else "minimize_timing.json"
with open(dst, "w") as f:
    json.dump(out, f, indent=1)
