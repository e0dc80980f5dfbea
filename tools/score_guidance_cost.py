"""Cost and effect of the physics-score guidance term on 3dpf at 40 samples x 20 steps, the models of bench.py (rigid row: cfg2;
flexible row: cfg1 with flexible side chains), captured step.  Report only: there is no threshold.

 1. Step time: score_guidance_weight 0 against `--time-weight` in the same process on the same model, interleaved over `--rounds`
    rounds, device events around `--steps` replayed steps after two ordinary steps, the capture and one replay; and the kernel's own
    time from back-to-back launches.  With weight 0 the sampler holds no guidance state (asserted) and the SamplerConfig is built
    without the fields, so `--weights 0 --time-only` also runs on a tree from before the term (the A/B against the parent commit:
    fresh processes of either tree, alternating).
 2. Final poses of whole 20-step runs at `--weights`, one seed per row, over the 40 poses: the median `total` of PoseScorer (graph
    receptor), the median E = inter + intra (what the term descends), the total clash count (PoseRefiner.clashes) and the median
    RMSD to the fixture's ligand pose (atom by atom, no symmetry correction).

bench.py's weights are synthetic (random initialisation, seeded): the figures say how the term acts on poses such a network produces
and nothing about real checkpoints, and a lower score is not a better pose.
Usage: python -m tools.score_guidance_cost [--steps 20] [--rounds 3] [--weights 0 0.1 0.5 2] [--out FILE]   (needs a HIP device)"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import bench                                                       # noqa: E402
from diffdock_pocket_amd import _lib as L                          # noqa: E402
from diffdock_pocket_amd.diffusion import get_t_schedule           # noqa: E402
from diffdock_pocket_amd.refine import PoseRefiner                 # noqa: E402
from diffdock_pocket_amd.sampler import Sampler, SamplerConfig     # noqa: E402
from diffdock_pocket_amd.scoring import PoseScorer                 # noqa: E402
from diffdock_pocket_amd.synthetic import make_3dpf_complex        # noqa: E402

ROWS = {"rigid": ("cfg2", False), "flex": ("cfg1", True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--weights", type=float, nargs="+", default=[0.0, 0.1, 0.5, 2.0], help="weights of the whole runs (effect)")
    ap.add_argument("--time-weight", type=float, default=0.5, help="the weight timed against 0 (0: time weight 0 alone)")
    ap.add_argument("--time-only", action="store_true", help="skip the whole runs")
    ap.add_argument("--rows", nargs="+", default=list(ROWS), choices=list(ROWS))
    ap.add_argument("--label", default="", help="printed in front of every line (which tree this is)")
    ap.add_argument("--out", default=None, help="also write the figures to this JSON file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sched = get_t_schedule(20)
    tag = f"[{a.label}] " if a.label else ""
    out = {"label": a.label, "samples": 40, "inference_steps": 20, "seed": a.seed, "weights": list(a.weights), "rows": {}}
    for row in a.rows:
        cfgname, flex = ROWS[row]
        model, _ = bench.build_model(cfgname, flex, dev)
        g = make_3dpf_complex(seed=0, flexible_sidechains=flex)

        def sampler(w):
            fields = {"score_guidance_weight": w} if w > 0 else {}
            return Sampler(model, g, 40, dev, SamplerConfig(inference_steps=20, flexible_sidechains=flex, sigma=bench.sigma_ranges(cfgname),
                                                            **fields), seed=a.seed)

        timed = (0.0,) + ((a.time_weight,) if a.time_weight > 0 else ())
        times = {w: [] for w in timed}
        kernel_us = None
        for rnd in range(a.rounds):
            for w in timed:
                smp = sampler(w)
                assert getattr(smp, "score_guidance", False) == (w > 0) and (w > 0 or not hasattr(smp, "sguid_ws"))
                smp.randomize()
                for i in range(4):          # two ordinary steps, the capture, one replay
                    smp.step(i, sched)
                assert bool(smp._graph)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(a.steps):
                    smp.step(4 + i % 16, sched)
                e1.record()
                torch.cuda.synchronize()
                times[w].append(e0.elapsed_time(e1) / a.steps)
                smp.check_overflow()
                if w > 0 and rnd == a.rounds - 1:
                    lib, ws = L.load(), smp.sguid_ws
                    st = torch._C._cuda_getCurrentRawStream(0)
                    upd = [smp.upd["tr"].clone(), smp.upd["rot"].clone(), smp.upd["tor"].clone()]      # (the sampler's own stay as they are)
                    one = torch.ones(1, device=dev)                                                    # w = 1, kept alive with upd
                    ws.launch(smp.lig_pos, smp.atom_pos if flex else None, upd, one)
                    for _ in range(10):
                        lib.ddp_score_guidance(C.byref(ws.args), st)
                    e0.record()
                    for _ in range(200):
                        lib.ddp_score_guidance(C.byref(ws.args), st)
                    e1.record()
                    torch.cuda.synchronize()
                    kernel_us = e0.elapsed_time(e1) / 200 * 1e3
                    print(f"{tag}{row}: ddp_score_guidance {kernel_us:.1f} us per launch (200 back-to-back launches, 40 samples, {ws.n} atoms, "
                          f"{ws.m} receptor atoms, T = {ws.T})")
                smp.close()
        for w, v in times.items():
            print(f"{tag}{row}: captured step, score_guidance_weight = {w}: " + ", ".join(f"{x:.3f}" for x in v) + f" ms per step (min {min(v):.3f})")
        poses = {}
        if not a.time_only:
            rf, sc = PoseRefiner(g, dev), PoseScorer(g, dev, receptor="graph")
            ref = torch.as_tensor(g["ligand"].pos).float().reshape(-1, 3).to(dev)
            for w in a.weights:
                smp = sampler(w)
                smp.randomize()
                lig, atoms = smp.run(sched)
                apos = atoms if flex else None
                s = sc.score(lig, apos)
                cl = rf.clashes(lig, atom_pos=apos)
                rmsd = (lig - ref[None]).pow(2).sum(-1).mean(-1).sqrt()
                torch.cuda.synchronize()
                poses[str(w)] = {"total_median": float(s.total.median()), "e_median": float((s.inter + s.intra).median()),
                                 "clashes_total": int(cl.sum()), "rmsd_median": float(rmsd.median()), "finite": bool(torch.isfinite(lig).all())}
                p = poses[str(w)]
                print(f"{tag}{row}: weight {w}: median total {p['total_median']:.3f}, median E {p['e_median']:.3f}, total clashes "
                      f"{p['clashes_total']}, median RMSD {p['rmsd_median']:.3f} A, finite {p['finite']}")
                smp.close()
        out["rows"][row] = {"model": cfgname, "step_ms": {str(w): v for w, v in times.items()}, "kernel_us": kernel_us, "final_poses": poses}
        del model
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
