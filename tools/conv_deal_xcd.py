"""How a conv launch's workgroups load the 8 XCDs, with the tile order of ddp_conv_deal = 0 (one contiguous range of tiles per XCD) and
with chunks of 4, 8 and 16 tiles dealt in turn.  The launches are the REAL row-stationary launches of layer 3 of one 40-sample cfg2 step
(the early launch of the receptor- / ligand-sourced convs, then the atom-sourced one), re-issued inside the forward while every buffer
of theirs is alive (as tools/overlap_ab.py does).

Needs the diagnostic library with the workgroup stamps for the per-XCD table:
    python -c "from diffdock_pocket_amd import build; build.build(defs=['DDP_DEAL_STAMPS'], tag='dealstamps')"
    DDP_HIP_LIB=diffdock_pocket_amd/libddp_hip_dealstamps.so python tools/conv_deal_xcd.py
With the product library it prints the launch times only.  Times are on the 100 MHz clock all XCDs share (10 ns per tick).  Prints one
text block (profiles/conv_deal_ab.txt).  Diagnostic; results of the launches do not depend on the order."""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
from diffdock_pocket_amd import _lib as L  # noqa: E402
from diffdock_pocket_amd import launch as K  # noqa: E402
from diffdock_pocket_amd.diffusion import get_t_schedule  # noqa: E402
from diffdock_pocket_amd.sampler import Sampler, SamplerConfig  # noqa: E402
from diffdock_pocket_amd.synthetic import make_3dpf_complex  # noqa: E402

REPS = 7
DS_WGS = 16384
CHUNKS = (0, 4, 8, 16, 0)      # (0 again at the end: what the order of the measurements is worth)


def time_one(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def xcd_table(lib, fn):
    """One stamped run of the launch -> (per XCD: workgroups, busy ticks, last end after the launch's first start), tasks per XCD."""
    L.check(lib.ddp_debug_clear_deal_stamps(), "clear stamps")
    torch.cuda.synchronize()
    fn()
    torch.cuda.synchronize()
    buf = np.zeros((DS_WGS, 8), dtype=np.uint64)
    L.check(lib.ddp_debug_read_deal_stamps(buf.ctypes.data_as(C.c_void_p), DS_WGS), "read stamps")
    ran = buf[:, 0] > 0
    ids = np.nonzero(ran)[0]
    xcc = buf[ran, 0].astype(np.int64) - 1
    task = buf[ran, 1].astype(np.int64)
    start = buf[ran, 3].astype(np.int64)
    end = buf[ran, 4:8].astype(np.int64).max(axis=1)
    t0 = start.min()
    rows = []
    for x in range(8):
        sel = xcc == x
        rows.append((int(sel.sum()), int((end[sel] - start[sel]).sum()), int((end[sel] - t0).max()) if sel.any() else 0,
                     np.bincount(task[sel], minlength=int(task.max()) + 1).tolist()))
    # workgroup ids go round-robin to the XCDs: every XCD runs ONE class of id % 8 (which one differs from launch to launch)
    by_id = all(len(set((ids[xcc == x] & 7).tolist())) <= 1 for x in range(8))
    return rows, by_id, int(end.max() - t0)


def main():
    dev = torch.device("cuda:0")
    lib = L.load()
    stamps = hasattr(lib, "ddp_debug_read_deal_stamps")
    deal = C.c_int.in_dll(lib, "ddp_conv_deal")
    model, _ = bench.build_model("cfg2", False, dev)
    cg = make_3dpf_complex(seed=0, flexible_sidechains=False)
    smp = Sampler(model, cg, 40, dev, SamplerConfig(inference_steps=20, flexible_sidechains=False, hip_graph=False), seed=0)
    smp.randomize()
    sched = get_t_schedule(20)
    for i in range(3):
        smp.step(i, sched)
    torch.cuda.synchronize()
    real_launch = K.launch_convs
    seen = []

    def launch_convs(spec, tasks, flops_spec=None, node_bytes=0.0, tag=None):
        real_launch(spec, tasks, flops_spec=flops_spec, node_bytes=node_bytes, tag=tag)
        if tag != "layer3" or not all(t._path.rows for t in tasks) or len(seen) >= 3:
            return
        torch.cuda.synchronize()
        fn = lambda: real_launch(spec, tasks, flops_spec=flops_spec, node_bytes=node_bytes, tag=tag)      # noqa: E731
        counts = [t.n_edges if t._count[1] is None else min(t.n_edges, int(t._count[1].item())) for t in tasks]
        tiles = [(n + 127) // 128 for n in counts]
        seen.append(len(tasks))
        print(f"== layer 3, rows launch {len(seen)}: {len(tasks)} tasks, edges {counts}, tiles {tiles} = {sum(tiles)}")
        before = deal.value
        try:
            for c in CHUNKS:
                deal.value = c
                med, lo, hi = time_one(fn)
                print(f"ddp_conv_deal={c:<2d} launch alone: median {med * 1e3:.1f} us of {REPS} (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
                if not stamps:
                    continue
                rows, by_id, span = xcd_table(lib, fn)
                busy = np.array([r[1] for r in rows], dtype=np.float64)
                last = np.array([r[2] for r in rows], dtype=np.float64)
                print(f"  one id % 8 class per XCD: {by_id}; launch span {span} ticks; busy ticks per XCD: max / mean = {busy.max() / busy.mean():.4f}, "
                      f"max / min = {busy.max() / busy.min():.4f}; last finish per XCD: max - min = {int(last.max() - last.min())} ticks "
                      f"({(last.max() - last.min()) / last.max() * 100:.1f} % of the span)")
                for x, (n, b, le, tk) in enumerate(rows):
                    print(f"  xcd {x}: {n:5d} workgroups, busy {b:10d} ticks, last finish {le:7d} ticks, workgroups per task {tk}")
        finally:
            deal.value = before

    K.launch_convs = launch_convs
    try:
        smp.step(3, sched)
        torch.cuda.synchronize()
    finally:
        K.launch_convs = real_launch
    smp.close()


if __name__ == "__main__":
    main()
