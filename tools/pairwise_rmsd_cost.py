"""python tools/pairwise_rmsd_cost.py [out.json]  (needs an MI355X; profiles/pairwise_rmsd_timing.json)
All-pairs matrix: one ddp_pose_pairwise_rmsd launch against S launches of ddp_pose_rmsd with ref = pose i (the parent's way).
HIP events around each form, alternating, median of REPS after warm-up; outputs compared bit for bit at the sizes timed."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffdock_pocket_amd import launch as LA

S, N, REPS, WARM = 40, 30, 30, 8
dev = torch.device("cuda:0")
gen = torch.Generator().manual_seed(0)
pos = (torch.randn(S, N, 3, generator=gen) * 3).to(dev)
out = {"S": S, "n": N, "tile": LA.pairwise_tile(N), "reps": REPS, "device": torch.cuda.get_device_name(0), "cases": []}
for P in (1, 4096, 100000):
    t = torch.rand(P, N, generator=gen).argsort(1).to(torch.int32)
    t[0] = torch.arange(N)
    perms_t = t.T.contiguous().to(dev)
    dist = torch.empty(S, S, device=dev)
    rows = torch.empty(S, S, device=dev)
    best = torch.empty(S, S, dtype=torch.int32, device=dev)

    def new():
        LA.pose_pairwise_rmsd(pos, perms_t, out=dist)

    def old():
        for i in range(S):
            LA.pose_rmsd(pos, pos[i], perms_t, rmsd=rows[i], best=best[i])

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        return a.elapsed_time(b) * 1e3

    for _ in range(WARM):
        new(); old()
    torch.cuda.synchronize()
    tn, to = [], []
    for _ in range(REPS):
        tn.append(timed(new)); to.append(timed(old))
    iu = torch.triu_indices(S, S, 1, device=dev)
    same = bool(torch.equal(dist[iu[0], iu[1]].view(torch.int32), rows[iu[0], iu[1]].view(torch.int32)))
    q = lambda v: [round(x, 1) for x in (min(v), statistics.median(v), max(v))]
    case = {"P": P, "pairwise_us_min_med_max": q(tn), "s_launches_us_min_med_max": q(to),
            "ratio_of_medians": round(statistics.median(to) / statistics.median(tn), 2), "upper_triangle_bits_equal": same}
    print(json.dumps(case), flush=True)
    out["cases"].append(case)
dst = sys.argv[1] if len(sys.argv) > 1 else "pairwise_rmsd_timing.json"
with open(dst, "w") as f:
    json.dump(out, f, indent=1)
