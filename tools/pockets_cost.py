"""python tools/pockets_cost.py [out.json] [--once]  (needs an MI355X)
Cost of the pocket finder on the 3dpf fixture (1282 heavy atoms, a 42 x 46 x 44 grid at 1 A): pockets.find_pockets on the device, the
whole call from the PDB's atoms to the ranked pockets including the final copy (wall clock around a synchronised call; 3 warm-ups, the
median of 20), beside the tests' NumPy statement of the same definition and the package's own CPU path on the host.  --once: one
warm call and one more, for a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/pockets_cost.py --once)."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pockets_ref as REF  # noqa: E402
from diffdock_pocket_amd import pockets as P  # noqa: E402

pdb = open(os.path.join(ROOT, "tests", "golden", "3dpf_protein.pdb")).read()
pos, radii, ca = P.protein_atoms(pdb)
dev = torch.device("cuda:0")


def timed(fn, reps, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3, min(ts) * 1e3


if "--once" in sys.argv:
    for _ in range(2):
        found = P.find_pockets_atoms(pos, radii, ca, dev)
    torch.cuda.synchronize()
    print("pockets:", [(p.label, p.size, p.score) for p in found])
    sys.exit(0)

out = {"atoms": int(pos.shape[0]), "grid": list(P.make_grid(pos, P.PocketConfig())[1]), "cpu_threads": torch.get_num_threads()}
out["device_ms_median"], out["device_ms_min"] = timed(lambda: P.find_pockets_atoms(pos, radii, ca, dev), 20, 3)
out["device_from_pdb_text_ms_median"], _ = timed(lambda: P.find_pockets(pdb, dev), 20, 3)
out["numpy_reference_ms_median"], out["numpy_reference_ms_min"] = timed(lambda: REF.find_pockets(pos, radii, ca), 20, 3)
out["torch_cpu_path_ms_median"], _ = timed(lambda: P.find_pockets_atoms(pos, radii, ca, "cpu"), 5, 2)
a, b = P.find_pockets_atoms(pos, radii, ca, dev), REF.find_pockets(pos, radii, ca)[0]
out["same_table"] = [(p.label, p.size, p.score) for p in a] == [(r["label"], r["size"], r["score"]) for r in b]
print(json.dumps(out))
if len(sys.argv) > 1 and not sys.argv[1].startswith("--"):
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
