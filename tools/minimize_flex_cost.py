"""python tools/minimize_flex_cost.py [out.json]  (needs an MI355X; profiles/minimize_flex_timing.json)
Cost and effect of the joint minimisation of ligand and flexible side chains: 40 poses x 100 iterations, the ligand perturbed by the
recipe of the test fixture, the side chains by chi noise N(0, 0.3 rad) (torch.Generator().manual_seed(4)).  HIP events around the
kernel call alone (`advance`: ddp_pose_minimize_flex against the ligand-only ddp_pose_minimize on the same inputs, each sample's own
receptor), min / median / max of REPS calls after WARM warm-up calls, in one process; then the PyTorch fp64 form on 16 host threads (first fixture only).
Two fixtures: the synthetic 3dpf complex (37 moving atoms of 1111, 17 bonds; its atom features, the elements among them, are drawn
at random, so few of its atoms are typed) and the real 3dpf graph with every residue within 3.5 A of the pocket sphere flexible
(all atoms typed).  Also E before and after for the joint and the ligand-only minimisation from the same starts, and the clash
counts of PoseEvaluator before and after."""
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
from diffdock_pocket_amd import minimize_flex as MF
from diffdock_pocket_amd.evaluation import PoseEvaluator
from diffdock_pocket_amd.sampler import apply_sidechain_torsions, modify_conformer
from diffdock_pocket_amd.synthetic import make_3dpf_complex

REPS, WARM, S, ITERATIONS = 30, 5, 40, 100
GOLDEN = os.path.join(ROOT, "tests", "golden")
dev = torch.device("cuda:0")
cfg = M.MinimizeConfig(iterations=ITERATIONS)


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


def span(t):
    return [round(float(t.min()), 3), round(float(t.median()), 3), round(float(t.max()), 3)]


def measure(name, g, cpu_calls):
    host = MF.FlexPoseMinimizer(g, config=cfg)
    r = host.rigid
    gen = torch.Generator().manual_seed(2)
    tr = torch.randn(S, 3, generator=gen, dtype=torch.float64) * 0.5
    rot = torch.randn(S, 3, generator=gen, dtype=torch.float64) * 0.15
    tor = torch.randn(S, r.T, generator=gen, dtype=torch.float64) * 0.3
    x = modify_conformer(g["ligand"].pos.float()[None].expand(S, -1, -1).contiguous(), tr.float(), rot.float(), tor.float(), r.bonds,
                         r.rot_idx).contiguous()
    sc = host.sc
    chi = 0.3 * torch.randn(S, sc.n_sc, generator=torch.Generator().manual_seed(4))
    y = apply_sidechain_torsions(g["atom"].pos.float()[None].repeat(S, 1, 1), sc.edge_idx, sc.sub, sc.mapping, chi).contiguous()
    t = host.scorer._cpu
    out = {"n_lig": host.n, "n_tor": r.T, "receptor_atoms": host.n_a, "receptor_atoms_typed": int((t["rec_r"] >= 0).sum()),
           "moving_atoms": sc.n_mov, "moving_atoms_typed": int((t["rec_r"][sc.mov] >= 0).sum()), "side_chain_bonds": sc.n_sc,
           "sc_pairs_listed": int(sc.pairs.sum())}
    xd, yd = x.to(dev), y.to(dev)
    fx, mz = MF.FlexPoseMinimizer(g, dev, config=cfg), M.PoseMinimizer(g, dev, config=cfg)
    step, acc = torch.ones(S, dtype=torch.float64, device=dev), torch.zeros(S, dtype=torch.int32, device=dev)
    out["joint_kernel"] = timed(lambda: fx.advance(xd, yd, xd, yd, step, acc, ITERATIONS))
    out["ligand_only_kernel"] = timed(lambda: mz.advance(xd, xd, step, acc, ITERATIONS, yd))
    out["joint_over_ligand_only_median"] = round(out["joint_kernel"][1] / out["ligand_only_kernel"][1], 2)
    print(name, "joint", out["joint_kernel"], "ligand only", out["ligand_only_kernel"], flush=True)
    a, b = fx.minimize(xd, yd), mz.minimize(xd, yd)
    ev = PoseEvaluator(g, dev)
    e_lig_only_joint_terms = fx.energy(b.lig_pos, yd)[0]       # the ligand-only result in the joint energy (its side chains did not move)
    out["E_before"] = span(a.energy_before[:, 5])
    out["E_after_joint"] = span(a.energy_after[:, 5])
    out["E_after_ligand_only"] = span(e_lig_only_joint_terms[:, 5])
    out["inter_plus_intra_before"] = span(b.energy_before[:, 3])
    out["inter_plus_intra_after_ligand_only"] = span(b.energy_after[:, 3])
    out["inter_plus_intra_after_joint"] = span(a.energy_after[:, 0] + a.energy_after[:, 1])
    out["sc_before"], out["sc_after_joint"] = span(a.energy_before[:, 2]), span(a.energy_after[:, 2])
    out["total_before"], out["total_after_joint"] = span(a.scores_before.total), span(a.scores_after.total)
    out["total_after_ligand_only"] = span(b.scores_after.total)
    out["accepted_joint"], out["accepted_ligand_only"] = span(a.accepted.double()), span(b.accepted.double())
    out["sidechain_rmsd_moved"] = span(a.sidechain_rmsd_moved)
    out["clashes_before"] = int(ev.evaluate(xd, yd).clashes.sum())
    out["clashes_after_joint"] = int(ev.evaluate(a.lig_pos, a.atom_pos).clashes.sum())
    out["clashes_after_ligand_only"] = int(ev.evaluate(b.lig_pos, yd).clashes.sum())
    print(name, {k: out[k] for k in ("E_before", "E_after_joint", "E_after_ligand_only", "clashes_before", "clashes_after_joint",
                                     "clashes_after_ligand_only")}, flush=True)
    if cpu_calls:
        torch.set_num_threads(16)
        out["cpu_threads"] = torch.get_num_threads()
        ts = []
        for _ in range(cpu_calls):
            t0 = time.perf_counter()
            c = host.advance(x, y, x, y, step.cpu(), acc.cpu(), ITERATIONS)
            ts.append((time.perf_counter() - t0) * 1e6)
        out["host_fp64_form"] = [round(u, 1) for u in (min(ts), statistics.median(ts), max(ts))]
        out["E_after_host"] = span(c[5][:, 5])
        print(name, "host", out["host_fp64_form"], flush=True)
    return out


pdb, sdf = open(os.path.join(GOLDEN, "3dpf_protein.pdb")).read(), open(os.path.join(GOLDEN, "3dpf_ligand.sdf")).read()
out = {"device": torch.cuda.get_device_name(0), "reps": REPS, "warmup": WARM, "poses": S, "iterations": ITERATIONS,
       "unit": "us per advance call, min / median / max"}
out["synthetic_3dpf"] = measure("synthetic_3dpf", make_3dpf_complex(flexible_sidechains=True), 1)
out["real_3dpf_flexdist_3.5"] = measure("real_3dpf_flexdist_3.5", I.build_complex_graph(pdb, sdf, flexdist=3.5), 0)
print(json.dumps(out), flush=True)
with open(sys.argv[1] if len(sys.argv) > 1 else "minimize_flex_timing.json", "w") as f:
    json.dump(out, f, indent=1)
