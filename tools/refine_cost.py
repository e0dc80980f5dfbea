"""python tools/refine_cost.py [out.json]  (needs an MI355X; profiles/refine_timing.json)
Cost of the clash relief: PoseRefiner.refine of 40 poses x 50 iterations of the 3dpf ligand (37 heavy atoms, 5 rotatable bonds)
against the full receptor (2463 atoms), on the device (HIP events around the whole call: 1 + 4 x 50 launches, the two contact
passes and the result tensors; warm-up, then REPS timed calls) beside the PyTorch fp64 form of the same call on the host."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffdock_pocket_amd import inputs as I
from diffdock_pocket_amd import refine as R
from diffdock_pocket_amd.evaluation import PoseEvaluator
from diffdock_pocket_amd.sampler import modify_conformer

S, ITERS, REPS, WARM, CPU_REPS = 40, 50, 30, 5, 3
GOLDEN = os.path.join(ROOT, "tests", "golden")
pdb, sdf = open(os.path.join(GOLDEN, "3dpf_protein.pdb")).read(), open(os.path.join(GOLDEN, "3dpf_ligand.sdf")).read()
g = I.build_complex_graph(pdb, sdf)
rec = PoseEvaluator.full_receptor(pdb, g.original_center)
cfg = R.RefineConfig(iterations=ITERS)
cpu = R.PoseRefiner(g, receptor=rec, config=cfg)
gen = torch.Generator().manual_seed(2)
tr = torch.randn(S, 3, generator=gen, dtype=torch.float64) * 0.5
rot = torch.randn(S, 3, generator=gen, dtype=torch.float64) * 0.15
tor = torch.randn(S, cpu.T, generator=gen, dtype=torch.float64) * 0.3
x = modify_conformer(g["ligand"].pos.float()[None].expand(S, -1, -1).contiguous(), tr.float(), rot.float(), tor.float(), cpu.bonds,
                     cpu.rot_idx).contiguous()

dev = torch.device("cuda:0")
hip = R.PoseRefiner(g, dev, receptor=rec, config=cfg)
xd = x.to(dev)
for _ in range(WARM):
    res = hip.refine(xd)
torch.cuda.synchronize()
t_dev = []
for _ in range(REPS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = hip.refine(xd)
    b.record()
    b.synchronize()
    t_dev.append(a.elapsed_time(b))
t_cpu = []
for _ in range(CPU_REPS):
    t0 = time.perf_counter()
    res_cpu = cpu.refine(x)
    t_cpu.append((time.perf_counter() - t0) * 1e3)
q = lambda v: [round(u, 3) for u in (min(v), statistics.median(v), max(v))]      # noqa: E731
clash = lambda r: (r.energy_after[:, :2].sum(1) / r.energy_before[:, :2].sum(1)).max()      # noqa: E731
out = {"samples": S, "iterations": ITERS, "n_lig": cpu.n, "n_tor": cpu.T, "n_rec": len(rec[1]), "reps": REPS,
       "device": torch.cuda.get_device_name(0), "cpu_threads": torch.get_num_threads(),
       "device_ms_min_med_max": q(t_dev), "cpu_ms_min_med_max": q(t_cpu),
       "ratio_of_medians": round(statistics.median(t_cpu) / statistics.median(t_dev), 1),
       "worst_clash_energy_ratio_device": float(clash(res)), "worst_clash_energy_ratio_cpu": float(clash(res_cpu)),
       "clashes_before_after_device": [int(res.clashes_before.sum()), int(res.clashes_after.sum())]}
print(json.dumps(out), flush=True)
dst = sys.argv[1] if len(sys.argv) > 1 else "refine_timing.json"
with open(dst, "w") as f:
    json.dump(out, f, indent=1)
