"""python tools/search_flex_cost.py [out.json]  (needs an MI355X; profiles/search_flex_timing.json, profiles/search_flex.txt)
Cost and effect of the Monte Carlo search with flexible side chains, in the setup of tools/minimize_flex_cost.py and
tools/search_cost.py: 40 poses, the ligand perturbed by the recipe of the test fixture, the side chains by chi noise N(0, 0.3 rad)
(torch.Generator().manual_seed(4)).  Two fixtures: the real 3dpf graph with every residue within 3.5 A of the pocket sphere flexible
(the case of DESIGN 4.20) and the synthetic 3dpf complex.  HIP events around the calls alone, min / median / max of REPS calls after
WARM warm-up calls, all in one process:
  1. ddp_pose_search_flex, all C = 10 cycles of K = 30 iterations in one launch, at R = 1 and 6 replicas (40 and 240 rows);
  2. the yardstick: ddp_pose_minimize_flex at C K = 300 iterations on the same 40 poses, the same number of line-search iterations
     per row;
  3. the launch-by-launch form (fused=False) at R = 6, the whole advance call.
Then what the default search (R = 6) does: E before, after the plain joint descent of replica 0 and after the search, and the clash
counts of PoseEvaluator before, after FlexPoseMinimizer(30) and after the search.  A lower E is not a better pose: the score is not
validated."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffdock_pocket_amd import inputs as I
from diffdock_pocket_amd import launch as LA
from diffdock_pocket_amd import minimize as M
from diffdock_pocket_amd import minimize_flex as MF
from diffdock_pocket_amd import search as SE
from diffdock_pocket_amd import search_flex as SF
from diffdock_pocket_amd.evaluation import PoseEvaluator
from diffdock_pocket_amd.sampler import apply_sidechain_torsions, modify_conformer
from diffdock_pocket_amd.synthetic import make_3dpf_complex

REPS, WARM, S, CYCLES, K = 30, 5, 40, 10, 30
GOLDEN = os.path.join(ROOT, "tests", "golden")
dev = torch.device("cuda:0")


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


def span(t):
    return [round(float(t.min()), 3), round(float(t.median()), 3), round(float(t.max()), 3)]


def measure(name, g):
    host = MF.FlexPoseMinimizer(g)
    r, sc = host.rigid, host.sc
    gen = torch.Generator().manual_seed(2)
    tr = torch.randn(S, 3, generator=gen, dtype=torch.float64) * 0.5
    rot = torch.randn(S, 3, generator=gen, dtype=torch.float64) * 0.15
    tor = torch.randn(S, r.T, generator=gen, dtype=torch.float64) * 0.3
    x = modify_conformer(g["ligand"].pos.float()[None].expand(S, -1, -1).contiguous(), tr.float(), rot.float(), tor.float(), r.bonds,
                         r.rot_idx).contiguous()
    chi = 0.3 * torch.randn(S, sc.n_sc, generator=torch.Generator().manual_seed(4))
    y = apply_sidechain_torsions(g["atom"].pos.float()[None].repeat(S, 1, 1), sc.edge_idx, sc.sub, sc.mapping, chi).contiguous()
    from diffdock_pocket_amd import _lib as L
    out = {"n_lig": host.n, "n_tor": r.T, "receptor_atoms": host.n_a, "moving_atoms": sc.n_mov, "side_chain_bonds": sc.n_sc,
           "lds_bytes_per_workgroup": 18496 + L.flex_state_bytes(host.n, sc.n_mov, sc.n_sc)}
    xd, yd = x.to(dev), y.to(dev)
    # 1. the fused search kernel alone
    out["ddp_pose_search_flex"] = {}
    for R in (1, 6):
        fs = SF.FlexPoseSearcher(g, dev, config=SE.SearchConfig(sidechains=True, replicas=R, cycles=CYCLES, iterations=K))
        st = fs.start(xd, yd)
        out["ddp_pose_search_flex"][f"R={R} rows={S * R}"] = timed(lambda: fs._run_fused(st, 0, CYCLES, None))
        print(name, "ddp_pose_search_flex", R, out["ddp_pose_search_flex"][f"R={R} rows={S * R}"], flush=True)
    # 2. the yardstick: the joint minimiser with as many iterations as one row of the search runs
    fx = MF.FlexPoseMinimizer(g, dev, config=M.MinimizeConfig(iterations=CYCLES * K))
    step, acc = torch.ones(S, dtype=torch.float64, device=dev), torch.zeros(S, dtype=torch.int32, device=dev)
    e0, e1 = torch.empty(S, 6, dtype=torch.float64, device=dev), torch.empty(S, 6, dtype=torch.float64, device=dev)
    pos, rec, t, rr = xd.clone(), yd.clone(), fx.scorer._dev, fx.rigid

    def minimize_300():
        pos.copy_(xd)
        rec.copy_(yd)
        step.fill_(1.0)
        LA.pose_minimize_flex(pos, xd, t["lig_r"], t["lig_f"], rec, yd, t["rec_r"], t["rec_f"], fx.score_config, t["pairs"],
                              rr._bonds_i32 if rr.T else None, rr._mask_u8 if rr.T else None, fx._sc_dev, step, acc, e0, e1, CYCLES * K)

    out["ddp_pose_minimize_flex_300_iterations"] = timed(minimize_300)
    print(name, "ddp_pose_minimize_flex 300", out["ddp_pose_minimize_flex_300_iterations"], flush=True)
    for R in (1, 6):
        out[f"search_R{R}_over_minimize_median"] = round(out["ddp_pose_search_flex"][f"R={R} rows={S * R}"][1] /
                                                         out["ddp_pose_minimize_flex_300_iterations"][1], 3)
    # 3. the launch-by-launch form at R = 6
    fs = SF.FlexPoseSearcher(g, dev, config=SE.SearchConfig(sidechains=True, replicas=6, cycles=CYCLES, iterations=K))
    st = fs.start(xd, yd)
    out["launch_by_launch_R6"] = timed(lambda: fs.advance(st, CYCLES, fused=False), reps=5, warm=1)
    print(name, "launch_by_launch_R6", out["launch_by_launch_R6"], flush=True)
    # what the default search does
    res = fs.search(xd, yd)
    m30 = MF.FlexPoseMinimizer(g, dev, config=M.MinimizeConfig(iterations=K)).minimize(xd, yd)
    ev = PoseEvaluator(g, dev)
    out["E_before"], out["E_minimized"], out["E_after"] = span(res.energy_before[:, 5]), span(res.energy_minimized[:, 5]), span(res.energy_after[:, 5])
    out["poses_above_zero_minimized"], out["poses_above_zero_after"] = int((res.energy_minimized[:, 5] > 0).sum()), int((res.energy_after[:, 5] > 0).sum())
    c0, c1, c2 = (ev.evaluate(a, b).clashes.double() for a, b in ((xd, yd), (m30.lig_pos, m30.atom_pos), (res.lig_pos, res.atom_pos)))
    out["clashes_before"], out["clashes_minimized"], out["clashes_after"] = span(c0), span(c1), span(c2)
    out["sidechain_rmsd_moved"], out["rmsd_moved"] = span(res.sidechain_rmsd_moved), span(res.rmsd_moved)
    out["chosen_replica_histogram"] = torch.bincount(res.replica.long().cpu(), minlength=6).tolist()
    print(name, {k: out[k] for k in ("E_before", "E_minimized", "E_after", "clashes_before", "clashes_minimized", "clashes_after")}, flush=True)
    return out


pdb, sdf = open(os.path.join(GOLDEN, "3dpf_protein.pdb")).read(), open(os.path.join(GOLDEN, "3dpf_ligand.sdf")).read()
out = {"device": torch.cuda.get_device_name(0), "reps": REPS, "warmup": WARM, "poses": S, "cycles": CYCLES, "iterations": K,
       "unit": "us per call, min / median / max (HIP events around the call); E and clash counts: min / median / max over the poses"}
out["real_3dpf_flexdist_3.5"] = measure("real_3dpf_flexdist_3.5", I.build_complex_graph(pdb, sdf, flexdist=3.5))
out["synthetic_3dpf"] = measure("synthetic_3dpf", make_3dpf_complex(flexible_sidechains=True))
print(json.dumps(out), flush=True)
with open(sys.argv[1] if len(sys.argv) > 1 else "search_flex_timing.json", "w") as f:
    json.dump(out, f, indent=1)
