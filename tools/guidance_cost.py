"""Cost and effect of the steric-clash guidance term on 3dpf at 40 samples x 20 steps, the models of bench.py (rigid row: cfg2;
flexible row: cfg1 with flexible side chains), captured step.  Report only: there is no threshold.

 1. Step time: clash_guidance_weight 0 against 0.5 in the same process on the same model, interleaved over `--rounds` rounds, device
    events around `--steps` replayed steps after two ordinary steps, the capture and one replay; and the kernel's own time from
    back-to-back launches.  With weight 0 the sampler holds no guidance state (asserted): its step is the launch sequence of a
    sampler without the fields.
 2. Final poses of whole 20-step runs at weights {0, 0.25, 0.5, 1, 2}, one seed per row: the total clash count (PoseRefiner.clashes) and
    the median E_cross (PoseRefiner.energy) over the 40 poses.

bench.py's weights are synthetic (random initialisation, seeded): the clash figures say how the term acts on poses such a network
produces and nothing about real checkpoints.
Usage: python -m tools.guidance_cost [--steps 20] [--rounds 3] [--out FILE]   (needs a HIP device)"""
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
from diffdock_pocket_amd.synthetic import make_3dpf_complex        # noqa: E402

ROWS = {"rigid": ("cfg2", False), "flex": ("cfg1", True)}
WEIGHTS = (0.0, 0.25, 0.5, 1.0, 2.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the figures to this JSON file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sched = get_t_schedule(20)
    out = {"samples": 40, "inference_steps": 20, "seed": a.seed, "weights": list(WEIGHTS), "rows": {}}
    for row, (cfgname, flex) in ROWS.items():
        model, _ = bench.build_model(cfgname, flex, dev)
        g = make_3dpf_complex(seed=0, flexible_sidechains=flex)

        def sampler(w):
            return Sampler(model, g, 40, dev, SamplerConfig(inference_steps=20, flexible_sidechains=flex, sigma=bench.sigma_ranges(cfgname),
                                                            clash_guidance_weight=w), seed=a.seed)

        times = {0.0: [], 0.5: []}
        kernel_us = None
        for rnd in range(a.rounds):
            for w in (0.0, 0.5):
                smp = sampler(w)
                assert smp.guidance == (w > 0) and (w > 0 or not hasattr(smp, "guid_ws"))
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
                    lib, ws = L.load(), smp.guid_ws
                    st = torch._C._cuda_getCurrentRawStream(0)
                    upd = [smp.upd["tr"].clone(), smp.upd["rot"].clone(), smp.upd["tor"].clone()]      # (the sampler's own stay as they are)
                    one = torch.ones(1, device=dev)                                                    # w = 1, kept alive with upd
                    ws.launch(smp.lig_pos, smp.atom_pos if flex else None, upd, one)
                    for _ in range(10):
                        lib.ddp_clash_guidance(C.byref(ws.args), st)
                    e0.record()
                    for _ in range(200):
                        lib.ddp_clash_guidance(C.byref(ws.args), st)
                    e1.record()
                    torch.cuda.synchronize()
                    kernel_us = e0.elapsed_time(e1) / 200 * 1e3
                    print(f"{row}: ddp_clash_guidance {kernel_us:.1f} us per launch (200 back-to-back launches, 40 samples, {ws.n} atoms, "
                          f"{ws.m} receptor atoms, T = {ws.T})")
                smp.close()
        for w, v in times.items():
            print(f"{row}: captured step, clash_guidance_weight = {w}: " + ", ".join(f"{x:.3f}" for x in v) + f" ms per step (min {min(v):.3f})")
        poses = {}
        rf = PoseRefiner(g, dev)
        for w in WEIGHTS:
            smp = sampler(w)
            smp.randomize()
            lig, atoms = smp.run(sched)
            apos = atoms if flex else None
            e, _ = rf.energy(lig, atom_pos=apos)
            cl = rf.clashes(lig, atom_pos=apos)
            torch.cuda.synchronize()
            poses[str(w)] = {"clashes_total": int(cl.sum()), "e_cross_median": float(e[:, 0].median()), "finite": bool(torch.isfinite(lig).all())}
            print(f"{row}: weight {w}: total clashes {poses[str(w)]['clashes_total']}, median E_cross {poses[str(w)]['e_cross_median']:.3f}")
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
