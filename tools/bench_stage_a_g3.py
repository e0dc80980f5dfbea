"""ddp_stage_a_gh3 alone at the layer-3 width: ms per launch (20 launches back to back, best of 3) and TB/s of G written.
  python tools/bench_stage_a_g3.py [tag]            the stage-A stacks of a 40-sample step (atom 44440 x 2, receptor 5560 x 6, ligand
                                                    1480 x 6, the 185 x 6 and 363 x 2 products), the library's own dispatch
  python tools/bench_stage_a_g3.py --forms [tag]    row lists (listed rows of capacity) and dense products around the dispatch threshold,
                                                    every shape under ddp_sa_drainwave = 0 (four symmetric waves), 1 (the shipped dispatch)
                                                    and 2 (the store wave everywhere), switched inside the process, twice each
DDP_HIP_LIB = another build of the library, DDP_SA_DRAINWAVE = 0 / 1 / 2 the kernel form of the first mode."""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from diffdock_pocket_amd import _lib as L  # noqa: E402
from diffdock_pocket_amd.packing import gh3_ld, gh_dest_table, split_h2  # noqa: E402

STACKS = (("atom", 44440, 2, 0), ("rec", 5560, 6, 0), ("lig", 1480, 6, 0), ("lig5", 185, 6, 0), ("r363", 363, 2, 0))
FORMS = (("near40", 44440, 2, 2903), ("pruned40", 44440, 2, 12000), ("list5560", 5560, 6, 1500), ("list5560b", 5560, 6, 5000),
         ("dense4096", 4096, 2, 0), ("dense8192", 8192, 2, 0))


def timeit(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / n)
    return best


def product(lib, dev, N, nb, n_list):
    """A launch of nb products of N rows (n_list > 0: a sorted row list of capacity N with a device-side length of n_list)."""
    st = torch.cuda.current_stream().cuda_stream
    k, ldx = 60, 180
    x = torch.randn(N, ldx, device=dev)
    offs = (C.c_int32 * nb)(*[120 * (i % 2) for i in range(nb)])
    ld3 = gh3_ld(180, 72)
    nc3 = ld3 // 6 * 8
    w = torch.randn(nb, k, nc3, device=dev)
    wh = split_h2(w, unified_scale=0.5)
    out = torch.empty(nb, N, ld3, device=dev)
    dest = torch.stack([gh_dest_table([32, 28, 12], 23, nc3, fmt=1)] * nb).contiguous().to(dev)
    rows = cnt = None
    if n_list:
        rows = torch.randperm(N, device=dev).sort().values.to(torch.int32).contiguous()
        cnt = torch.tensor([n_list], dtype=torch.int32, device=dev)
    keep = (x, w, wh, out, dest, rows, cnt, offs)

    def launch():
        L.check(lib.ddp_stage_a_gh3(x.data_ptr(), ldx, N, rows.data_ptr() if rows is not None else None, cnt.data_ptr() if cnt is not None else None,
                                    N, offs, nb, w.data_ptr(), wh.data_ptr(), k, nc3, out.data_ptr(), ld3, None, dest.data_ptr(), st), "ddp_stage_a_gh3")
    launch.keep = keep
    return launch, nb * (n_list or N) * ld3 * 4 / 1e9


def main():
    args = [a for a in sys.argv[1:] if a != "--forms"]
    forms = "--forms" in sys.argv[1:]
    tag = args[0] if args else "?"
    dev = torch.device("cuda:0")
    lib = L.load()
    torch.manual_seed(0)
    if not forms:
        for name, N, nb, n_list in STACKS:
            launch, gb = product(lib, dev, N, nb, n_list)
            t = timeit(launch)
            print(f"[{tag}] {name}: {N} x {nb}  {gb:.3f} GB  {t:.4f} ms  {gb / t:.2f} TB/s", flush=True)
        return
    var = C.c_int.in_dll(lib, "ddp_sa_drainwave")
    for name, N, nb, n_list in FORMS:
        launch, gb = product(lib, dev, N, nb, n_list)
        res = []
        for _ in range(2):
            for mode in (0, 1, 2):
                var.value = mode
                res.append(f"mode{mode} {timeit(launch) * 1e3:.1f} us")
        print(f"[{tag}] {name}: {n_list or N} of {N} x {nb}: " + "  ".join(res), flush=True)


if __name__ == "__main__":
    main()
