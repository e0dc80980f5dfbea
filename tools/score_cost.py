"""python tools/score_cost.py [out.json]  (needs an MI355X; profiles/score_timing.json)
Cost of the Vinardo-form physics score: PoseScorer.score of poses of the 3dpf ligand (37 heavy atoms, 5 rotatable bonds) on the
device - 40 poses and 840 poses (40 samples x 21 trajectory frames), against the graph receptor (1139 atom nodes) and the full
receptor (2463 atoms, 1282 of them typed), with and without the gradient - HIP events around each call, the median of REPS calls after
WARM warm-up calls.  In the same run: ddp_refine_energy on the same 40 poses and the full receptor (the same launch plan: one workgroup
per sample, the receptor through a 1024-atom LDS tile), and the PyTorch fp64 form of the score on the host."""
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
from diffdock_pocket_amd import scoring as SC
from diffdock_pocket_amd.evaluation import PoseEvaluator
from diffdock_pocket_amd.sampler import modify_conformer

REPS, WARM, CPU_REPS = 200, 20, 5
GOLDEN = os.path.join(ROOT, "tests", "golden")
pdb, sdf = open(os.path.join(GOLDEN, "3dpf_protein.pdb")).read(), open(os.path.join(GOLDEN, "3dpf_ligand.sdf")).read()
g = I.build_complex_graph(pdb, sdf)
full = SC.typed_receptor(pdb, g.original_center)
dev = torch.device("cuda:0")
cpu_ref = R.PoseRefiner(g, receptor=PoseEvaluator.full_receptor(pdb, g.original_center))


def poses(S):
    gen = torch.Generator().manual_seed(2)
    tr = torch.randn(S, 3, generator=gen, dtype=torch.float64) * 0.5
    rot = torch.randn(S, 3, generator=gen, dtype=torch.float64) * 0.15
    tor = torch.randn(S, cpu_ref.T, generator=gen, dtype=torch.float64) * 0.3
    return modify_conformer(g["ligand"].pos.float()[None].expand(S, -1, -1).contiguous(), tr.float(), rot.float(), tor.float(),
                            cpu_ref.bonds, cpu_ref.rot_idx).contiguous()


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


out = {"device": torch.cuda.get_device_name(0), "reps": REPS, "warmup": WARM, "n_lig": 37, "n_tor": 5, "unit": "us, min / median / max",
       "receptor_atoms": {"graph": int(g["atom"].pos.shape[0]), "full": int(len(full.radii)), "full_typed": int((full.radii >= 0).sum())}}
x40, x840 = poses(40), poses(840)
scorers = {"graph": SC.PoseScorer(g, dev), "full": SC.PoseScorer(g, dev, receptor=full)}
for S, x in ((40, x40), (840, x840)):
    xd = x.to(dev)
    for name, sc in scorers.items():
        for grad in (False, True):
            key = f"score_{S}_poses_{name}_receptor" + ("_with_grad" if grad else "")
            out[key] = timed(lambda: sc.score(xd, with_grad=grad))
            print(key, out[key], flush=True)

# ddp_refine_energy on the same 40 poses, full receptor (all 2463 atoms, the hydrogens skipped in the loop), with its gradient
rf = R.PoseRefiner(g, dev, receptor=PoseEvaluator.full_receptor(pdb, g.original_center))
xd = x40.to(dev)
out["refine_energy_40_poses_full_receptor_with_grad"] = timed(lambda: rf.energy(xd))
print("refine_energy", out["refine_energy_40_poses_full_receptor_with_grad"], flush=True)

# the device and the host forms agree (the tests hold the bound; here only that the timed calls computed the same thing)
host = SC.PoseScorer(g, receptor=full)
want, got = host.score(x40, with_grad=True), scorers["full"].score(xd, with_grad=True).cpu()
out["max_abs_difference_total_device_vs_host"] = float((want.total - got.total).abs().max())
out["cpu_threads"] = torch.get_num_threads()
for S, x in ((40, x40), (840, x840)):
    for grad in (False, True):
        t = []
        for _ in range(CPU_REPS):
            t0 = time.perf_counter()
            host.score(x, with_grad=grad)
            t.append((time.perf_counter() - t0) * 1e6)
        out[f"host_fp64_form_{S}_poses_full_receptor" + ("_with_grad" if grad else "")] = [round(u, 1) for u in (min(t), statistics.median(t), max(t))]
print(json.dumps(out), flush=True)
dst = sys.argv[1] if len(sys.argv) > 1 else "score_timing.json"
with open(dst, "w") as f:
    json.dump(out, f, indent=1)
