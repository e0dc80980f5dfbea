"""python tools/score_guidance_flex_cost.py [out.json]  (needs an MI355X; profiles/score_guidance_flex_timing.json)
Cost and effect of the side-chain part of the physics-score guidance term (score_guidance.py, SamplerConfig.score_guidance_sidechains).
Report only: there is no threshold.

 1. The launch: ddp_score_guidance_flex beside ddp_score_guidance in one process on the same 40-sample inputs (each sample's own
    receptor; the ligand perturbed by the recipe of the test fixture, the side chains by chi noise N(0, 0.3 rad)), HIP events around
    single calls, min / median / max of 200 calls after 10 warm-up calls.  Two fixtures: the synthetic flexible 3dpf complex (37 moving
    atoms, 17 bonds; few of its atoms are typed) and the real 3dpf graph with every residue within 3.5 A of the pocket flexible (all
    atoms typed).  The pair counts say what the second pass visits: moving x ligand atoms (the gather) and the listed sc_pairs.
 2. The captured flexible step of bench.py's cfg1 model (synthetic weights), 40 samples: no guidance, ligand guidance only (the parent
    commit's step), and with the side chains guided, interleaved over ROUNDS rounds in one process, device events around 20 replays.
 3. Effect: whole 20-step runs of the same model at W = 0.5 and 2, the flag off against on, one seed: the median joint E and its sc
    part (FlexPoseMinimizer.energy at restraints 0), the clash count (PoseRefiner.clashes) and the median RMSD of the moving atoms
    from the graph's own side chains.

bench.py's weights are synthetic: the figures say how the term acts on poses such a network produces and nothing about real
checkpoints; a lower E is not a better pose."""
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                       # noqa: E402
from diffdock_pocket_amd import _lib as L                          # noqa: E402
from diffdock_pocket_amd import inputs as I                        # noqa: E402
from diffdock_pocket_amd import minimize_flex as MF                # noqa: E402
from diffdock_pocket_amd import score_guidance as SG               # noqa: E402
from diffdock_pocket_amd.descent import ligand_torsions            # noqa: E402
from diffdock_pocket_amd.diffusion import get_t_schedule           # noqa: E402
from diffdock_pocket_amd.refine import PoseRefiner                 # noqa: E402
from diffdock_pocket_amd.sampler import Sampler, SamplerConfig, apply_sidechain_torsions, modify_conformer, rotate_index_lists   # noqa: E402
from diffdock_pocket_amd.synthetic import make_3dpf_complex        # noqa: E402

REPS, WARM, S, ROUNDS = 200, 10, 40, 3
GOLDEN = os.path.join(ROOT, "tests", "golden")
dev = torch.device("cuda:0")


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


def launch_cost(name, g):
    tb = SG.build_tables(g)
    sc = SG.build_sidechain_tables(g, tb)
    bonds, mask = ligand_torsions(g)
    gen = torch.Generator().manual_seed(2)
    tr, rot = torch.randn(S, 3, generator=gen, dtype=torch.float64) * 0.5, torch.randn(S, 3, generator=gen, dtype=torch.float64) * 0.15
    tor = torch.randn(S, bonds.shape[0], generator=gen, dtype=torch.float64) * 0.3
    x = modify_conformer(g["ligand"].pos.float()[None].expand(S, -1, -1).contiguous(), tr.float(), rot.float(), tor.float(), bonds,
                         rotate_index_lists(mask)).contiguous().to(dev)
    chi = 0.3 * torch.randn(S, sc.n_sc, generator=torch.Generator().manual_seed(4))
    y = apply_sidechain_torsions(g["atom"].pos.float()[None].repeat(S, 1, 1), sc.edge_idx, sc.sub, sc.mapping, chi).contiguous().to(dev)
    typed_l, typed_r = int((tb.lig_radii >= 0).sum()), int((tb.rec_radii >= 0).sum())
    out = {"n_lig": tb.n, "n_tor": int(tb.bonds.shape[0]), "receptor_atoms": int(tb.rec_radii.shape[0]), "receptor_atoms_typed": typed_r,
           "ligand_atoms_typed": typed_l, "moving_atoms": sc.n_mov, "moving_atoms_typed": int((tb.rec_radii[sc.mov] >= 0).sum()),
           "side_chain_bonds": sc.n_sc, "sc_pairs_listed": int(sc.pairs.sum()), "first_pass_pairs": tb.n * int(tb.rec_radii.shape[0]),
           "gather_pairs": sc.n_mov * tb.n}
    lig, flex = SG.ScoreGuidanceWorkspace(tb, dev), SG.ScoreGuidanceFlexWorkspace(tb, sc, dev)
    upd = [torch.zeros(S, 3, device=dev), torch.zeros(S, 3, device=dev), torch.zeros(S, lig.T, device=dev)]
    upd_sc, one = torch.zeros(S, sc.n_sc, device=dev), torch.ones(1, device=dev)
    lig.launch(x, y, upd, one)
    flex.launch(x, y, upd, one, upd_sc)                # (fills both structs; the timed calls go through the C ABI alone)
    lib, st = L.load(), torch._C._cuda_getCurrentRawStream(0)
    out["ddp_score_guidance_us"] = timed(lambda: lib.ddp_score_guidance(C.byref(lig.args), st))
    out["ddp_score_guidance_flex_us"] = timed(lambda: lib.ddp_score_guidance_flex(C.byref(flex.flex_args), st))
    out["flex_over_ligand_only_median"] = round(out["ddp_score_guidance_flex_us"][1] / out["ddp_score_guidance_us"][1], 2)
    print(name, out, flush=True)
    return out


def step_and_effect():
    model, _ = bench.build_model("cfg1", True, dev)
    g = make_3dpf_complex(seed=0, flexible_sidechains=True)
    sched = get_t_schedule(20)

    def sampler(w, sidechains):
        fields = ({"score_guidance_weight": w} if w > 0 else {}) | ({"score_guidance_sidechains": True} if sidechains else {})
        return Sampler(model, g, S, dev, SamplerConfig(inference_steps=20, flexible_sidechains=True, sigma=bench.sigma_ranges("cfg1"), **fields),
                       seed=0)

    rows = {"no_guidance": (0.0, False), "ligand_only_w0.5": (0.5, False), "with_side_chains_w0.5": (0.5, True)}
    times = {k: [] for k in rows}
    for _ in range(ROUNDS):
        for k, (w, sidechains) in rows.items():
            smp = sampler(w, sidechains)
            smp.randomize()
            for i in range(4):          # two ordinary steps, the capture, one replay
                smp.step(i, sched)
            assert bool(smp._graph)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(20):
                smp.step(4 + i % 16, sched)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(round(e0.elapsed_time(e1) / 20, 4))
            smp.check_overflow()
            smp.close()
    out = {"captured_step_ms": times}
    print("captured step", times, flush=True)
    fx, rf = MF.FlexPoseMinimizer(g, dev), PoseRefiner(g, dev)
    mov = fx.sc.mov.to(dev)
    ref = torch.as_tensor(g["atom"].pos).float().to(dev)[mov]
    effect = {}
    for w in (0.5, 2.0):
        for sidechains in (False, True):
            smp = sampler(w, sidechains)
            smp.randomize()
            lig, atoms = smp.run(sched)
            e = fx.energy(lig, atoms)[0]
            cl = rf.clashes(lig, atom_pos=atoms)
            moved = (atoms[:, mov] - ref[None]).pow(2).sum(-1).mean(-1).sqrt()
            torch.cuda.synchronize()
            key = f"w{w}_{'on' if sidechains else 'off'}"
            effect[key] = {"E_median": round(float(e[:, 5].median()), 4), "inter_median": round(float(e[:, 0].median()), 4),
                           "sc_median": round(float(e[:, 2].median()), 4), "clashes_total": int(cl.sum()),
                           "sidechain_rmsd_median": round(float(moved.median()), 4), "finite": bool(torch.isfinite(atoms).all() and torch.isfinite(lig).all())}
            print(key, effect[key], flush=True)
            smp.close()
    out["final_poses"] = effect
    return out


pdb, sdf = open(os.path.join(GOLDEN, "3dpf_protein.pdb")).read(), open(os.path.join(GOLDEN, "3dpf_ligand.sdf")).read()
out = {"device": torch.cuda.get_device_name(0), "reps": REPS, "warmup": WARM, "samples": S, "unit": "us per launch, min / median / max"}
out["synthetic_3dpf"] = launch_cost("synthetic_3dpf", make_3dpf_complex(flexible_sidechains=True))
out["real_3dpf_flexdist_3.5"] = launch_cost("real_3dpf_flexdist_3.5", I.build_complex_graph(pdb, sdf, flexdist=3.5))
out["sampler_cfg1_flex"] = step_and_effect()
print(json.dumps(out), flush=True)
with open(sys.argv[1] if len(sys.argv) > 1 else "score_guidance_flex_timing.json", "w") as f:
    json.dump(out, f, indent=1)
