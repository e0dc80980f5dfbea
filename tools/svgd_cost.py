"""Cost of the SVGD term on the flagship workload: 3dpf, 40 samples, rigid receptor, the cfg2 model of bench.py, captured step.
Prints the step time with svgd_weight 0 and 0.5 (same process, same model, interleaved runs) and the three passes' own times.
Usage: python -m tools.svgd_cost [--steps 20] [--rounds 3]   (needs a HIP device)"""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import bench                                                       # noqa: E402
from diffdock_pocket_amd import _lib as L                          # noqa: E402
from diffdock_pocket_amd.diffusion import get_t_schedule           # noqa: E402
from diffdock_pocket_amd.sampler import Sampler, SamplerConfig     # noqa: E402
from diffdock_pocket_amd.synthetic import make_3dpf_complex        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model, _ = bench.build_model("cfg2", False, dev)
    g = make_3dpf_complex(seed=0, flexible_sidechains=False)
    sched = get_t_schedule(20)
    times = {0.0: [], 0.5: []}
    for rnd in range(a.rounds):
        for w in (0.0, 0.5):
            smp = Sampler(model, g, 40, dev, SamplerConfig(inference_steps=20, flexible_sidechains=False, sigma=bench.sigma_ranges("cfg2"),
                                                           svgd_weight=w), seed=0)
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
                lib, ws = L.load(), smp.svgd_ws
                st = torch._C._cuda_getCurrentRawStream(0)
                for name in ("ddp_svgd_tau", "ddp_svgd_pairs", "ddp_svgd_rows"):
                    fn = getattr(lib, name)
                    for _ in range(10):
                        fn(C.byref(ws.args), st)
                    e0.record()
                    for _ in range(200):
                        fn(C.byref(ws.args), st)
                    e1.record()
                    torch.cuda.synchronize()
                    print(f"{name}: {e0.elapsed_time(e1) / 200 * 1e3:.1f} us per launch (200 back-to-back launches, 40 samples, 37 atoms, T = {ws.T})")
            smp.close()
    for w, v in times.items():
        print(f"captured step, svgd_weight = {w}: " + ", ".join(f"{x:.3f}" for x in v) + f" ms per step (min {min(v):.3f})")


if __name__ == "__main__":
    main()
